"""Shared by tests/test_resident_delta_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_resident_delta.py (hardware): a small base
state dict, a fine-tune of it, and the checks of a variant store (zipnn_amd.ResidentCheckpoint.from_state_dict(..., base=...)) against the fine-tune's own
tensors, bit for bit."""
import torch

BASES = ("dict", "store", "store+index")


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8).cpu(), b.contiguous().reshape(-1).view(torch.uint8).cpu())


def _perturb(t, frac, seed):
    """`t` with about `frac` of its BYTES changed (the recipe of test_kernels_simt._delta_pair, on a tensor)."""
    g = torch.Generator().manual_seed(seed)
    b = t.contiguous().view(torch.uint8).reshape(-1).clone()
    hit = torch.rand(b.numel(), generator=g) < frac
    b[hit] ^= torch.randint(1, 256, (int(hit.sum()),), generator=g, dtype=torch.uint8)
    return b.view(t.dtype).reshape(t.shape)


def state_dicts():
    """-> (base_sd, ft_sd) on the CPU.  bf16 [261, 512] (one 256 KiB chunk + a tail), fp32 [129, 508], fp8 [3, 65541], the two Linear layers of the hooked
    model, an int64 tensor, a tensor the base lacks, one whose shape differs in the base, one identical to the base's, one unrelated to it."""
    g = torch.Generator().manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=g) * 0.02
    base = {
        "w.bf16": rn(261, 512).to(torch.bfloat16),
        "w.fp32": rn(129, 508),
        "w.fp8": (rn(3, 65541) * 25).to(torch.float8_e4m3fn),
        "0.weight": rn(384, 512).to(torch.bfloat16), "0.bias": rn(384).to(torch.bfloat16),
        "1.weight": rn(512, 384).to(torch.bfloat16), "1.bias": rn(512).to(torch.bfloat16),
        "steps": torch.arange(40, dtype=torch.int64),
        "reshaped": rn(64, 1024).to(torch.bfloat16),
        "identical": rn(300, 512).to(torch.bfloat16),
        "unrelated": rn(256, 1024).to(torch.bfloat16),
    }
    ft = {k: _perturb(v, 0.03, 100 + i) for i, (k, v) in enumerate(base.items()) if k not in ("steps", "reshaped", "identical", "unrelated")}
    ft["steps"] = base["steps"] + 5
    ft["absent"] = rn(300, 512).to(torch.bfloat16)
    ft["reshaped"] = _perturb(base["reshaped"], 0.03, 9).reshape(128, 512)
    ft["identical"] = base["identical"].clone()
    ft["unrelated"] = torch.rand(256, 1024, generator=g).to(torch.bfloat16)       # other values altogether: tensor ^ base does not compress better than the tensor
    return base, ft


def make_base(kind, base_sd, dev):
    from zipnn_amd import ResidentCheckpoint
    if kind == "dict":
        return {k: v.to(dev).clone() for k, v in base_sd.items()}
    return ResidentCheckpoint.from_state_dict(base_sd, dev, index=(kind == "store+index"))


def model_of(sd, dev):
    m = torch.nn.Sequential(torch.nn.Linear(512, 384), torch.nn.Linear(384, 512)).to(torch.bfloat16)
    m.load_state_dict({k: sd[k] for k in ("0.weight", "0.bias", "1.weight", "1.bias")})
    return m.to(dev)


def check_variant(kind, base_sd, ft_sd, dev, forward=True):
    """The whole matrix for one kind of base; returns the variant store."""
    from zipnn_amd import ResidentCheckpoint
    base = make_base(kind, base_sd, dev)
    ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base)
    plain = ResidentCheckpoint.from_state_dict(ft_sd, dev)
    # what was delta-coded
    for n in ("w.bf16", "w.fp32", "w.fp8", "0.weight", "1.weight"):
        assert ft.info(n)["delta"] is True and ft.info(n)["compressed"], n
    for n in ("steps", "absent", "reshaped", "unrelated"):
        assert ft.info(n)["delta"] is False, n
    assert ft.info("identical")["delta"] == "same" and ft.info("identical")["resident_bytes"] == 0
    assert ft.resident_bytes < plain.resident_bytes
    assert ft.resident_bytes == sum(ft.info(n)["resident_bytes"] + (-ft.info(n)["resident_bytes"] % 256 if ft.info(n)["compressed"] else 0) for n in ft.keys())
    for n in ("w.bf16", "w.fp32", "w.fp8"):
        assert ft.info(n)["resident_bytes"] < plain.info(n)["resident_bytes"], n
    names = list(ft_sd.keys())
    # get_tensor, get_tensors(into=)
    for n in names:
        assert _bytes_equal(ft.get_tensor(n), ft_sd[n]), n
    into = torch.full((ft.scratch_bytes(names) + 64,), 0x5A, dtype=torch.uint8, device=dev)
    got = ft.get_tensors(names, into=into[:-64])
    for n in names:
        assert _bytes_equal(got[n], ft_sd[n]), n
    assert bool((into[-64:] == 0x5A).all())
    # get_slice over rows that straddle the chunk boundary (row 256 of [261, 512] bf16 starts the second chunk; rows 128/129 of the fp32 one)
    for n, idx in (("w.bf16", slice(250, 261)), ("w.bf16", slice(0, 3)), ("w.bf16", 258), ("w.fp32", slice(120, 129)), ("w.fp8", slice(0, 2)), ("w.fp8", 2),
                   ("identical", slice(250, 260)), ("absent", slice(3, 9)), ("steps", slice(1, 4))):
        s = ft.get_slice(n)
        assert _bytes_equal(s[idx], ft_sd[n][idx]), (n, idx)
    sl = ft.get_slice("w.bf16"); sl[257:259]
    assert sl.last_chunk_range == (1, 2)
    ft.status()
    # plan().run() twice
    plan = ft.plan(names)
    for _ in range(2):
        views = plan.run()
        plan.status()
        for n in names:
            assert _bytes_equal(views[n], ft_sd[n]), n
    plan.close()
    # the index: none for delta entries
    before = ft.index_bytes
    ft.build_index()
    for n in names:
        i = ft.info(n)
        assert i["index_bytes"] == 0 or i["delta"] is False, n
    assert ft.index_bytes - before == sum(-(-ft.info(n)["index_bytes"] // 256) * 256 for n in names)
    assert ft.info("absent")["index_bytes"] > 0 and ft.info("w.bf16")["index_bytes"] == 0
    for n in names:
        assert _bytes_equal(ft.get_tensor(n), ft_sd[n]), n
    got = ft.get_tensors(names)
    for n in names:
        assert _bytes_equal(got[n], ft_sd[n]), n
    # hook: the hooked forward == the plainly loaded model's
    if forward:
        x = (torch.randn(4, 512, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(dev)
        want = model_of(ft_sd, dev)(x)
        m = model_of(base_sd, dev)
        h = ft.hook(m)
        out = m(x)
        h.status()
        assert _bytes_equal(out, want)             # (bit for bit: perturbed bytes make NaNs, which compare unequal as values)
        h.remove()
        for k, p in m.state_dict().items():
            assert _bytes_equal(p, ft_sd[k]), k
    return base, ft


def check_apply_revert(kind, base_sd, ft_sd, dev, base=None, ft=None):
    """apply_ on tensors holding the base: the fine-tune's bytes for every name both have; revert_: the base's again, except what has nothing to restore from."""
    from zipnn_amd import ResidentCheckpoint
    if ft is None:
        base = make_base(kind, base_sd, dev)
        ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base)
    common = [n for n in ft_sd if n in base_sd and base_sd[n].shape == ft_sd[n].shape]
    live = {n: base_sd[n].to(dev).clone() for n in common}
    live["not.in.the.store"] = torch.ones(3, device=dev)
    changed = ft.apply_(live)
    assert sorted(changed) == sorted(n for n in common if n != "identical")
    for n in common:
        assert _bytes_equal(live[n], ft_sd[n]), n
    stay = ft.revert_(live)
    assert stay == []                              # every common name has a base counterpart of its dtype and shape
    for n in common:
        assert _bytes_equal(live[n], base_sd[n]), n
    assert bool((live["not.in.the.store"] == 1).all())
    # tensors the base cannot restore: a name it lacks, a shape it holds differently
    extra = {"absent": torch.zeros_like(ft_sd["absent"]).to(dev), "reshaped": torch.zeros_like(ft_sd["reshaped"]).to(dev)}
    assert sorted(ft.apply_(extra)) == ["absent", "reshaped"]
    for n in extra:
        assert _bytes_equal(extra[n], ft_sd[n]), n
    assert sorted(ft.revert_(extra)) == ["absent", "reshaped"]
    for n in extra:
        assert _bytes_equal(extra[n], ft_sd[n]), n      # they stay
    import pytest
    with pytest.raises(ValueError):
        ft.apply_({"w.bf16": torch.zeros(3, device=dev)})
