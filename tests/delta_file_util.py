"""Shared by tests/test_delta_file_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_delta_file.py (hardware): delta checkpoint
files — a variant store written by ResidentCheckpoint.save_file and read back by from_file(base=) / load_file(base=) — checked against the
fine-tune's own tensors, bit for bit.  The tensors are tests/resident_delta_util.state_dicts()."""
import json
import os

import pytest
import torch

import resident_delta_util as R

DELTA = ("w.bf16", "w.fp32", "w.fp8", "0.weight", "0.bias", "1.weight", "1.bias")      # what from_state_dict(base=) delta-codes of these tensors
SLICES = (("w.bf16", slice(250, 261)), ("w.bf16", slice(0, 3)), ("w.bf16", 258), ("w.fp32", slice(120, 129)), ("w.fp8", slice(0, 2)), ("w.fp8", 2),
          ("identical", slice(250, 260)), ("absent", slice(3, 9)), ("steps", slice(1, 4)))      # rows that straddle the chunk boundaries (resident_delta_util.check_variant)


def read_container(path):
    """-> (header dict in file order, data section bytes, length of the JSON header) of a safetensors file."""
    with open(path, "rb") as f:
        n = int.from_bytes(f.read(8), "little")
        hdr = json.loads(f.read(n))
        return hdr, f.read(), n


def same_file(p, q):
    """Two safetensors files are the same file: equal data sections, equal headers — the tensors in the same order at the same offsets, the same metadata —
    of equal length.  (The raw header bytes are not compared: safetensors serialises the metadata out of a hash map, so the ORDER of the metadata keys in the
    header differs between two writes of the very same content.)"""
    hp, dp, np_ = read_container(p)
    hq, dq, nq = read_container(q)
    return hp == hq and list(hp) == list(hq) and dp == dq and np_ == nq and os.path.getsize(p) == os.path.getsize(q)


def odd_state_dict(ft_sd):
    """The fine-tune plus an int8 tensor of 3 elements, named to sort first: safetensors lays the file out by dtype, then name, and pads nothing, so the
    first frame (U8 entries come last) starts at an odd byte."""
    sd = {"!odd": torch.tensor([1, -2, 3], dtype=torch.int8)}
    sd.update(ft_sd)
    return sd


def frame_offsets(path):
    """-> {name: offset of the entry in the data section} for the U8 entries that hold a frame."""
    hdr, _, _ = read_container(path)
    infos = json.loads(hdr["__metadata__"]["znn_compressed_vectors"])
    return {n: hdr[n]["data_offsets"][0] for n in infos if hdr[n]["data_offsets"][1] > hdr[n]["data_offsets"][0]}


def check_same_store(a, b):
    """b (loaded) is the store a (built): the same info() for every tensor apart from where the bytes lie, byte-equal bodies."""
    assert sorted(a.keys()) == sorted(b.keys())                     # (a file lists its tensors in safetensors' order)
    for n in a.keys():
        ia, ib = a.info(n), b.info(n)
        assert ia["delta"] == ib["delta"] and type(ia["delta"]) is type(ib["delta"]), (n, ia["delta"], ib["delta"])
        for k in ("shape", "dtype", "nbytes", "compressed", "resident_bytes"):
            assert ia[k] == ib[k], (n, k, ia[k], ib[k])
        ea, eb = a._entries[n], b._entries[n]
        if ea.compressed:
            assert (ea.P, ea.bits, ea.byts, ea.chunk) == (eb.P, eb.bits, eb.byts, eb.chunk), n
            assert torch.equal(ea.body.cpu(), eb.body.cpu()), n


def check_reads(store, sd, base_sd, dev, forward=True):
    """Every read entry point of `store` gives the tensors of `sd`, bit for bit."""
    names = list(sd.keys())
    for n in names:
        assert R._bytes_equal(store.get_tensor(n), sd[n]), n
    into = torch.full((store.scratch_bytes(names) + 64,), 0x5A, dtype=torch.uint8, device=dev)
    got = store.get_tensors(names, into=into[:-64])
    for n in names:
        assert R._bytes_equal(got[n], sd[n]), n
    assert bool((into[-64:] == 0x5A).all())
    for n, idx in SLICES:
        if n in sd:
            assert R._bytes_equal(store.get_slice(n)[idx], sd[n][idx]), (n, idx)
    store.status()
    plan = store.plan(names)
    for _ in range(2):
        views = plan.run()
        plan.status()
        for n in names:
            assert R._bytes_equal(views[n], sd[n]), n
    plan.close()
    if forward:
        x = (torch.randn(4, 512, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(dev)
        want = R.model_of(sd, dev)(x)
        m = R.model_of(base_sd, dev)
        h = store.hook(m)
        out = m(x)
        h.status()
        assert R._bytes_equal(out, want)
        h.remove()


def check_round_trip(kind, base_sd, ft_sd, dev, tmp_path, odd=False):
    """from_state_dict(base=) -> save_file -> from_file(base=): the same store, every read entry point, apply_ / revert_, a variant of the loaded variant."""
    from zipnn_amd import ResidentCheckpoint
    sd = odd_state_dict(ft_sd) if odd else ft_sd
    base = R.make_base(kind, base_sd, dev)
    ft = ResidentCheckpoint.from_state_dict(sd, dev, base=base)
    p = ft.save_file(str(tmp_path / "ft.znn.safetensors"))
    hdr, data, _ = read_container(p)
    rec = json.loads(hdr["__metadata__"]["znn_delta"])
    assert rec["version"] == 1 and rec["algo"] == "zn64-1"
    assert rec["tensors"] == dict({n: "delta" for n in DELTA}, identical="same") and sorted(rec["base_digests"]) == sorted(rec["tensors"])
    offs = frame_offsets(p)
    print("frame offsets:", offs)
    first = min(offs, key=offs.get)
    if odd:
        # U8 entries follow every other dtype, in name order: the first frame is "0.bias" — a delta frame, whose body lies a 32-byte header further —, right
        # behind the 3 int8 bytes.  The frames behind it start wherever the ones before end (their lengths are what the coder made them).
        assert first == "0.bias" and offs[first] % 2 == 1 and rec["tensors"][first] == "delta", offs
    ft2 = ResidentCheckpoint.from_file(p, dev, base=base)
    if odd:
        e = ft2._entries[first]
        assert e.delta is True and e.body.data_ptr() % 2 == 1            # (the uploaded section starts at an allocation boundary)
    check_same_store(ft, ft2)
    assert ft2.resident_bytes >= len(data) and ft2.resident_bytes - len(data) < 4096      # the data section, plus the few plain tensors that needed realigning
    check_reads(ft2, sd, base_sd, dev)
    R.check_apply_revert(kind, base_sd, ft_sd, dev, base=base, ft=ft2)
    # the index: none for delta entries, and decodes stay right
    ft2.build_index()
    assert ft2.info("absent")["index_bytes"] > 0 and ft2.info("w.bf16")["index_bytes"] == 0
    got = ft2.get_tensors(["absent", "unrelated", "w.bf16"])           # (hinted plain entries beside a delta entry)
    for n in got:
        assert R._bytes_equal(got[n], sd[n]), n
    # a variant of a variant, saved and loaded over the LOADED first variant
    sd2 = {k: R._perturb(v, 0.01, 500 + i) for i, (k, v) in enumerate(ft_sd.items()) if k.startswith("w.")}
    second = ResidentCheckpoint.from_state_dict(sd2, dev, base=ft2)
    assert all(second.info(k)["delta"] is True for k in sd2)
    p2 = second.save_file(str(tmp_path / "second.znn.safetensors"))
    second2 = ResidentCheckpoint.from_file(p2, dev, base=ft2)
    check_same_store(second, second2)
    check_reads(second2, sd2, base_sd, dev, forward=False)
    return p


def check_sizes(base_sd, ft_sd, dev, tmp_path):
    """The delta file is smaller than the plain store's file of the same tensors (the inequalities resident_delta_util.check_variant asserts for the bodies,
    in file form); the "same" tensor occupies no data bytes."""
    from zipnn_amd import ResidentCheckpoint
    base = R.make_base("store", base_sd, dev)
    d = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base).save_file(str(tmp_path / "delta.znn.safetensors"))
    p = ResidentCheckpoint.from_state_dict(ft_sd, dev).save_file(str(tmp_path / "plain.znn.safetensors"))
    raw = sum(v.numel() * v.element_size() for v in ft_sd.values())
    print("raw tensors", raw, "plain file", os.path.getsize(p), "delta file", os.path.getsize(d))
    assert os.path.getsize(d) < os.path.getsize(p) < raw
    hdr, _, _ = read_container(d)
    assert hdr["identical"]["dtype"] == "U8" and hdr["identical"]["shape"] == [0] and hdr["identical"]["data_offsets"][0] == hdr["identical"]["data_offsets"][1]
    hp, _, _ = read_container(p)
    for n in ("w.bf16", "w.fp32", "w.fp8"):
        assert hdr[n]["data_offsets"][1] - hdr[n]["data_offsets"][0] < hp[n]["data_offsets"][1] - hp[n]["data_offsets"][0], n


def check_plain_identity(ft_sd, dev, tmp_path, device):
    """A plain store's file is the file compress_safetensors_file writes from safetensors' own file of the same tensors, with and without digests, and
    from_file(p).save_file(p2) reproduces p (same_file: everything but the order of the metadata keys, which safetensors does not fix)."""
    from safetensors.torch import save_file
    from zipnn_amd import ResidentCheckpoint, safetensors_io
    src = str(tmp_path / "src.safetensors")
    save_file(ft_sd, src, {"format": "pt"})
    for dg in (False, True):
        q = safetensors_io.compress_safetensors_file(src, str(tmp_path / f"q{int(dg)}.znn.safetensors"), device=device, digests=dg)
        store = ResidentCheckpoint.from_state_dict(ft_sd, dev, digests=dg)
        p = store.save_file(str(tmp_path / f"p{int(dg)}.znn.safetensors"))
        assert same_file(p, q), dg
        assert ("znn_digests" in read_container(p)[0]["__metadata__"]) == dg
        assert "znn_delta" not in read_container(p)[0]["__metadata__"]
        again = ResidentCheckpoint.from_file(p, dev, digests=dg, index=True)          # (the index is not saved)
        p2 = again.save_file(str(tmp_path / f"p2{int(dg)}.znn.safetensors"))
        assert same_file(p2, p), dg
        p3 = safetensors_io.save_file(ft_sd, str(tmp_path / f"p3{int(dg)}.znn.safetensors"), device=dev, digests=dg)
        assert same_file(p3, p), dg
    # digests=True on a store without: computed; False on a store with: left out
    p4 = ResidentCheckpoint.from_state_dict(ft_sd, dev).save_file(str(tmp_path / "p4.znn.safetensors"), digests=True)
    assert same_file(p4, str(tmp_path / "p1.znn.safetensors"))
    p5 = ResidentCheckpoint.from_state_dict(ft_sd, dev, digests=True).save_file(str(tmp_path / "p5.znn.safetensors"), digests=False)
    assert same_file(p5, str(tmp_path / "p0.znn.safetensors"))
    got = safetensors_io.load_file(str(tmp_path / "p1.znn.safetensors"), device=device, verify=True)
    for n in ft_sd:
        assert R._bytes_equal(got[n], ft_sd[n]), n


def without_digests(store):
    """The same store (it shares the entries) as if it had been built without digests."""
    import copy
    out = copy.copy(store)
    out._digests = None
    return out


def _changed(base_sd, name):
    """base_sd with ONE byte of `name` changed."""
    out = dict(base_sd)
    b = base_sd[name].contiguous().view(torch.uint8).reshape(-1).clone()
    b[b.numel() // 2] ^= 0x01
    out[name] = b.view(base_sd[name].dtype).reshape(base_sd[name].shape)
    return out


def check_guards(base_sd, ft_sd, dev, tmp_path):
    from zipnn_amd import DigestMismatch, ResidentCheckpoint, safetensors_io
    base = R.make_base("store", base_sd, dev)
    ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base, digests=True)
    p = ft.save_file(str(tmp_path / "ft.znn.safetensors"))
    assert "znn_digests" in read_container(p)[0]["__metadata__"]
    # no base
    for call in (lambda: ResidentCheckpoint.from_file(p, dev), lambda: safetensors_io.load_file(p, device=dev)):
        with pytest.raises(ValueError, match="znn_delta") as ex:
            call()
        assert "base=" in str(ex.value) and not isinstance(ex.value, DigestMismatch)
    # a base that lacks a name / holds it in another shape
    lacking = {k: v.to(dev).clone() for k, v in base_sd.items() if k != "w.fp32"}
    with pytest.raises(ValueError, match="w.fp32") as ex:
        ResidentCheckpoint.from_file(p, dev, base=lacking)
    assert not isinstance(ex.value, DigestMismatch)
    reshaped = {k: v.to(dev).clone() for k, v in base_sd.items()}
    reshaped["1.weight"] = reshaped["1.weight"].reshape(384, 512).contiguous()
    with pytest.raises(ValueError, match="1.weight") as ex:
        ResidentCheckpoint.from_file(p, dev, base=reshaped)
    assert not isinstance(ex.value, DigestMismatch)
    # one byte of one base tensor changed: DigestMismatch naming exactly that tensor, whatever the base is — plain tensors, a store without digests (both
    # digested now), a store with recorded digests (used as they are) — and before anything is decoded
    for victim in ("w.bf16", "identical"):                                  # a delta entry's base tensor, a "same" entry's
        bad_sd = _changed(base_sd, victim)
        with_digests = ResidentCheckpoint.from_state_dict(bad_sd, dev, digests=True)
        bases = {"dict": {k: v.to(dev).clone() for k, v in bad_sd.items()}, "store": without_digests(with_digests), "store+digests": with_digests}
        dst = torch.full((ft.scratch_bytes(ft.keys()),), 0x5A, dtype=torch.uint8, device=dev)
        for kind, bad in bases.items():
            with pytest.raises(DigestMismatch) as ex:
                ResidentCheckpoint.from_file(p, dev, base=bad).get_tensors(ft.keys(), into=dst)
            assert ex.value.names == [victim], (kind, ex.value.names)
            assert bool((dst == 0x5A).all())                                # raised before anything was decoded
        with pytest.raises(DigestMismatch) as ex:
            safetensors_io.load_file(p, device=dev, base=bases["dict"])
        assert ex.value.names == [victim]
    # verify_base=False skips the check: the load goes through and decodes the wrong values, for that tensor alone …
    wrong = ResidentCheckpoint.from_file(p, dev, base=bases["dict"], verify_base=False)
    assert R._bytes_equal(wrong.get_tensor("w.fp32"), ft_sd["w.fp32"]) and not R._bytes_equal(wrong.get_tensor(victim), ft_sd[victim])
    with pytest.raises(DigestMismatch) as ex:                               # … which verify=True sees in the decoded fine-tune
        ResidentCheckpoint.from_file(p, dev, base=bases["dict"], verify_base=False, verify=True)
    assert ex.value.names == [victim]
    # the good base: verify=True passes, for each kind of base, and the guards of apply_ / revert_ work on the loaded store
    recorded = ResidentCheckpoint.from_state_dict(base_sd, dev, digests=True)
    for kind, good in (("dict", {k: v.to(dev).clone() for k, v in base_sd.items()}), ("store", base), ("store+digests", recorded)):
        ft2 = ResidentCheckpoint.from_file(p, dev, base=good, verify=True)
        assert ft2.has_digests and ft2.digests() == ft.digests(), kind
    model = R.model_of(base_sd, dev)
    before = {n: q.detach().clone() for n, q in model.named_parameters()}
    assert not any(ft2.holds(model).values())
    with pytest.raises(DigestMismatch):
        ft2.revert_(model, guard=True)                                      # the model holds the base: nothing to revert, nothing touched
    assert all(R._bytes_equal(q, before[n]) for n, q in model.named_parameters())
    ft2.apply_(model, guard=True)
    assert all(ft2.holds(model).values())
    ft2.revert_(model, guard=True)
    assert all(R._bytes_equal(q, before[n]) for n, q in model.named_parameters())
    return p, base


def check_damaged_delta_body(base_sd, ft_sd, dev, tmp_path):
    """One byte of a delta frame's body changed in the file: verify=True raises (the digest of the decoded tensor differs) or the decode is rejected; the load
    of the undamaged file right after is right."""
    from zipnn_amd import DigestMismatch, ResidentCheckpoint
    base = R.make_base("store", base_sd, dev)
    p = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base, digests=True).save_file(str(tmp_path / "good.znn.safetensors"))
    hdr, data, n = read_container(p)
    lo, hi = hdr["w.bf16"]["data_offsets"]
    raw = bytearray(open(p, "rb").read())
    assert raw[8 + n + lo + 9] == 1                                         # a delta frame
    raw[8 + n + lo + 32 + (hi - lo - 32) * 3 // 4] ^= 0x20                  # in the payload of its body
    bad = str(tmp_path / "bad.znn.safetensors")
    open(bad, "wb").write(raw)
    with pytest.raises((DigestMismatch, RuntimeError, MemoryError)) as ex:
        ResidentCheckpoint.from_file(bad, dev, base=base, verify=True)
    if isinstance(ex.value, DigestMismatch):
        assert ex.value.names == ["w.bf16"]
    ok = ResidentCheckpoint.from_file(p, dev, base=base, verify=True)
    assert R._bytes_equal(ok.get_tensor("w.bf16"), ft_sd["w.bf16"])


def check_load_file(base_sd, ft_sd, dev, tmp_path, device):
    """load_file(base=) with the base as a mapping, a store, a path to its plain file and a path to its compressed file; compress_safetensors_file(base=path)."""
    from safetensors.torch import save_file
    from zipnn_amd import ResidentCheckpoint, safetensors_io
    base_plain, ft_plain = str(tmp_path / "base.safetensors"), str(tmp_path / "ft.safetensors")
    save_file(base_sd, base_plain, {"format": "pt"})
    save_file(ft_sd, ft_plain, {"format": "pt", "note": "a fine-tune"})
    base_znn = safetensors_io.compress_safetensors_file(base_plain, device=device, digests=True)
    store = ResidentCheckpoint.from_state_dict(base_sd, dev)
    mapping = {k: v.to(dev).clone() for k, v in base_sd.items()}
    p = safetensors_io.save_file(ft_sd, str(tmp_path / "delta.znn.safetensors"), device=dev, base=store, digests=True)
    for kind, b in (("mapping", mapping), ("store", store), ("plain path", base_plain), ("compressed path", base_znn)):
        got = safetensors_io.load_file(p, device=dev, base=b, verify=True)
        assert list(got) == [k for k in read_container(p)[0] if k != "__metadata__"], kind           # (file order, as safetensors' own load_file returns it)
        for n in ft_sd:
            assert R._bytes_equal(got[n], ft_sd[n]), (kind, n)
    assert all(R._bytes_equal(mapping[k], v) for k, v in base_sd.items())  # the base is only read …
    got["identical"].zero_()                                                # … and what came back is not the base's own memory
    assert R._bytes_equal(mapping["identical"], base_sd["identical"])
    # file -> delta file, over the base's compressed file / its plain file / a store: the same delta file
    outs = [safetensors_io.compress_safetensors_file(ft_plain, str(tmp_path / f"d{i}.znn.safetensors"), device=device, base=b, digests=True)
            for i, b in enumerate((base_znn, base_plain, store))]
    for o in outs:
        assert same_file(o, outs[0])
    meta = read_container(outs[0])[0]["__metadata__"]
    assert meta["note"] == "a fine-tune" and "znn_delta" in meta and "znn_digests" in meta
    got = safetensors_io.load_file(outs[0], device=dev, base=base_znn, verify=True)
    for n in ft_sd:
        assert R._bytes_equal(got[n], ft_sd[n]), n
    # a file that is no delta file does not look at the base
    got = safetensors_io.load_file(base_znn, device=dev, base=mapping)
    assert all(R._bytes_equal(got[k], v) for k, v in base_sd.items())
    return p


def check_safe_open_refuses(path):
    """SafeOpen and the patched safe_open raise at open, naming the key and load_file(base=)."""
    import safetensors
    import safetensors.torch
    import zipnn_amd
    from zipnn_amd import zipnn as Z
    with pytest.raises(ValueError, match="znn_delta") as ex:
        zipnn_amd.SafeOpen(path, "pt", "cpu")
    assert "load_file(base=)" in str(ex.value)
    keep = (safetensors.safe_open, safetensors.torch.safe_open)
    try:
        Z._zipnn_safetensors()
        for opener in (safetensors.safe_open, safetensors.torch.safe_open):
            with pytest.raises(ValueError, match="znn_delta") as ex:
                opener(path, framework="pt", device="cpu")
            assert "load_file(base=)" in str(ex.value)
    finally:
        safetensors.safe_open, safetensors.torch.safe_open = keep
