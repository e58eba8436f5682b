"""Shared by tests/test_resident_sparse_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_resident_sparse.py (hardware): a base
state dict, a fine-tune that replaces 2 % of the elements of some tensors, and the checks of a variant store built with sparse=True
(zipnn_amd.ResidentCheckpoint.from_state_dict(..., base=..., sparse=True)) against the fine-tune's own tensors, bit for bit."""
import numpy as np
import pytest
import torch

import patch_ref as PR
from resident_delta_util import _bytes_equal

BASES = ("dict", "store", "store+index", "chain")
M = 3 * 65536 + 5                                   # elements of the sparse tensors: three patch blocks and five elements, one and a half frame chunks of bf16
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16, "fp8": torch.float8_e4m3fn}
SMALL = 70001


def _values(g, n, dt):
    x = torch.randn(n, generator=g) * 0.02
    return (x * 25).to(dt) if dt == torch.float8_e4m3fn else x.to(dt)


def _as_int(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _replace(t, frac, g):
    """`t` with `frac` of its elements replaced by fresh values of the same distribution."""
    out = t.clone()
    idx = torch.randperm(t.numel(), generator=g)[:int(t.numel() * frac)]
    _as_int(out.reshape(-1))[idx] = _as_int(_values(g, idx.numel(), t.dtype))
    return out


def _move_all(t):
    """Every element's lowest bit flipped: tensor ^ base is one value everywhere — the delta body is next to nothing, the patch larger than the tensor."""
    return (_as_int(t) ^ 1).view(t.dtype)


def state_dicts(seed=5):
    """-> (base_sd, ft_sd) on the CPU.  Per dtype: `sp.*` (M elements, 2 % replaced), `moved.*` (every element moved), `same.*` (identical), `absent.*` (not in
    the base); the two Linear layers of the hooked model (2 % replaced); an int64 tensor."""
    g = torch.Generator().manual_seed(seed)
    base, ft = {}, {}
    for tag, dt in DTYPES.items():
        base["sp." + tag] = _values(g, M, dt)
        ft["sp." + tag] = _replace(base["sp." + tag], 0.02, g)
        base["moved." + tag] = _values(g, SMALL, dt)
        ft["moved." + tag] = _move_all(base["moved." + tag])
        base["same." + tag] = _values(g, SMALL, dt)
        ft["same." + tag] = base["same." + tag].clone()
        ft["absent." + tag] = _values(g, SMALL, dt)
    for name, shape in (("0.weight", (384, 512)), ("0.bias", (384,)), ("1.weight", (512, 384)), ("1.bias", (512,))):
        base[name] = _values(g, int(np.prod(shape)), torch.bfloat16).reshape(shape)
        ft[name] = _replace(base[name], 0.02, g)
    base["steps"] = torch.arange(40, dtype=torch.int64)
    ft["steps"] = base["steps"] + 5
    return base, ft


def further(ft_sd, seed=6):
    """A second fine-tune over the first: 2 % of the sparse tensors and of the model's weights replaced again."""
    g = torch.Generator().manual_seed(seed)
    return {k: (_replace(v, 0.02, g) if k.startswith("sp.") or k[0] in "01" else _move_all(v) if k.startswith("moved.") else v.clone()) for k, v in ft_sd.items()}


def model_of(sd, dev):
    m = torch.nn.Sequential(torch.nn.Linear(512, 384), torch.nn.Linear(384, 512)).to(torch.bfloat16)
    m.load_state_dict({k: sd[k] for k in ("0.weight", "0.bias", "1.weight", "1.bias")})
    return m.to(dev)


def changed(a, b):
    """T: the elements of a whose bytes differ from b's."""
    return int((_as_int(a.reshape(-1)) != _as_int(b.reshape(-1))).sum())


def make(kind, base_sd, ft_sd, dev, digests=True):
    """-> (what the variant is taken over, the state dict it holds, the state dict the variant must decode to)."""
    from zipnn_amd import ResidentCheckpoint
    if kind == "dict":
        return {k: v.to(dev).clone() for k, v in base_sd.items()}, base_sd, ft_sd
    base = ResidentCheckpoint.from_state_dict(base_sd, dev, index=(kind == "store+index"), digests=digests)
    if kind != "chain":
        return base, base_sd, ft_sd
    mid_sd = {k: v for k, v in ft_sd.items() if not k.startswith("absent.")}
    mid = ResidentCheckpoint.from_state_dict(mid_sd, dev, base=base, sparse=True, digests=digests)     # a variant with sparse entries as the base of another
    assert mid.info("sp.bf16")["delta"] == "sparse"
    return mid, mid_sd, further(ft_sd)


def check_kinds(ft, plain_variant, over_sd, want_sd):
    """What was chosen, and what it costs."""
    for tag, dt in DTYPES.items():
        n, E = "sp." + tag, torch.empty(0, dtype=dt).element_size()
        i = ft.info(n)
        T = changed(want_sd[n], over_sd[n])
        assert i["delta"] == "sparse" and i["patch_entries"] == T and i["compressed"], (n, i)
        assert i["resident_bytes"] == PR.patch_len(M * E, E, T), (n, i)          # the formula's L
        assert 0.018 * M < T <= 0.02 * M, (n, T)
        assert ft.info("moved." + tag)["delta"] is True and ft.info("same." + tag)["delta"] == "same" and ft.info("absent." + tag)["delta"] is False, tag
        assert ft.info("moved." + tag)["patch_entries"] is None
    assert ft.info("steps")["delta"] is False
    # with sparse=False nothing changes; with it, what is not sparse is what it was
    for n in ft.keys():
        a, b = ft.info(n), plain_variant.info(n)
        if a["delta"] != "sparse":
            assert (a["delta"], a["resident_bytes"], a["compressed"]) == (b["delta"], b["resident_bytes"], b["compressed"]), n
        else:
            assert b["delta"] is True and a["resident_bytes"] < b["resident_bytes"], n
    assert ft.resident_bytes == sum(ft.info(n)["resident_bytes"] + (-ft.info(n)["resident_bytes"] % 256 if ft.info(n)["compressed"] else 0) for n in ft.keys())
    assert ft.resident_bytes < plain_variant.resident_bytes


def check_reads(ft, want_sd, dev):
    names = list(want_sd.keys())
    for n in names:
        assert _bytes_equal(ft.get_tensor(n), want_sd[n]), n
    into = torch.full((ft.scratch_bytes(names) + 64,), 0x5A, dtype=torch.uint8, device=dev)
    got = ft.get_tensors(names, into=into[:-64])
    for n in names:
        assert _bytes_equal(got[n], want_sd[n]), n
    assert bool((into[-64:] == 0x5A).all())
    # row windows that cut frame chunks (131 072 bf16 elements, 65 536 fp32 ones, 131 072 fp8 ones) and patch blocks (65 536 elements)
    for n, idx in (("sp.bf16", slice(65530, 65540)), ("sp.bf16", slice(131070, 131075)), ("sp.bf16", slice(0, 3)), ("sp.bf16", slice(M - 13, M)), ("sp.bf16", 131072),
                   ("sp.bf16", slice(1000, 190000)), ("sp.fp32", slice(65535, 65537)), ("sp.fp32", slice(130000, 131100)), ("sp.fp16", slice(196607, 196610)),
                   ("sp.fp8", slice(131071, 131073)), ("sp.fp8", slice(65536, 65536)), ("0.weight", slice(127, 129)), ("same.bf16", slice(5, 9)), ("moved.fp8", slice(7, 70000))):
        assert _bytes_equal(ft.get_slice(n)[idx], want_sd[n][idx]), (n, idx)
    sl = ft.get_slice("sp.bf16"); sl[131070:131075]
    assert sl.last_chunk_range == (0, 2)
    ft.status()
    plan = ft.plan(names)
    for _ in range(2):
        views = plan.run()
        plan.status()
        for n in names:
            assert _bytes_equal(views[n], want_sd[n]), n
    plan.close()
    # the index skips sparse entries
    ft.build_index(deltas=True)
    for n in names:
        assert ft.info(n)["index_bytes"] == 0 or ft.info(n)["delta"] in (False, True), n
    assert not any(ft.info(n)["index_bytes"] for n in names if ft.info(n)["delta"] == "sparse") and any(ft.info(n)["index_bytes"] for n in names)
    for n in names:
        assert _bytes_equal(ft.get_tensor(n), want_sd[n]), n


def check_model(ft, over_sd, want_sd, dev, guard):
    """A hooked forward equals the plain model's; apply_ / forward / revert_ on a model that holds what the variant was taken over."""
    x = (torch.randn(4, 512, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(dev)
    want_over, want = model_of(over_sd, dev)(x), model_of(want_sd, dev)(x)
    m = model_of(over_sd, dev)
    h = ft.hook(m)
    out = m(x)
    h.status()
    assert _bytes_equal(out, want)
    h.remove()
    for guarded in ((False, True) if guard else (False,)):
        m = model_of(over_sd, dev)
        assert sorted(ft.apply_(m, guard=guarded)) == ["0.bias", "0.weight", "1.bias", "1.weight"]
        assert _bytes_equal(m(x), want)
        for k, p in m.state_dict().items():
            assert _bytes_equal(p, want_sd[k]), k
        if guarded:
            from zipnn_amd import DigestMismatch
            assert all(ft.holds(m).values())
            with pytest.raises(DigestMismatch):
                ft.apply_(m, guard=True)                                         # it holds the variant's values already
        assert ft.revert_(m, guard=guarded) == []
        assert _bytes_equal(m(x), want_over)
        for k, p in m.state_dict().items():
            assert _bytes_equal(p, over_sd[k]), k
    # live tensors of every dtype, the tensors the base cannot restore among them
    live = {n: over_sd[n].to(dev).clone() for n in want_sd if n in over_sd}
    live.update({n: torch.zeros_like(want_sd[n]).to(dev) for n in want_sd if n not in over_sd})
    ft.apply_(live)
    for n in live:
        assert _bytes_equal(live[n], want_sd[n]), n
    assert sorted(ft.revert_(live)) == sorted(n for n in want_sd if n not in over_sd)
    for n in over_sd:
        if n in live:
            assert _bytes_equal(live[n], over_sd[n]), n


def check_store(kind, base_sd, ft_sd, dev, tmp_path=None):
    from zipnn_amd import ResidentCheckpoint
    over, over_sd, want_sd = make(kind, base_sd, ft_sd, dev)
    ft = ResidentCheckpoint.from_state_dict(want_sd, dev, base=over, sparse=True, digests=True)
    today = ResidentCheckpoint.from_state_dict(want_sd, dev, base=over)
    if kind == "dict":                                                           # (the default IS sparse=False: once is enough)
        explicit = ResidentCheckpoint.from_state_dict(want_sd, dev, base=over, sparse=False)
        assert [(today.info(n)["delta"], today.info(n)["resident_bytes"]) for n in today.keys()] == [(explicit.info(n)["delta"], explicit.info(n)["resident_bytes"]) for n in explicit.keys()]
        assert today.resident_bytes == explicit.resident_bytes
    assert not any(today.info(n)["delta"] == "sparse" for n in today.keys())
    check_kinds(ft, today, over_sd, want_sd)
    check_reads(ft, want_sd, dev)
    assert all(ft.verify().values())
    check_model(ft, over_sd, want_sd, dev, guard=True)
    with pytest.raises(ValueError, match="sp.bf16"):
        ft.save_file(str(tmp_path / "sparse.znn.safetensors") if tmp_path is not None else "unwritten.znn.safetensors")
    return ft
