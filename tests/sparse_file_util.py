"""Shared by tests/test_sparse_file_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_sparse_file.py (hardware): delta files with
SPARSE entries — a variant store built with sparse=True, written by save_file(sparse=True) and read back by from_file(base=) / load_file(base=) —
checked against the fine-tune's own tensors, bit for bit.  The tensors and the kinds of base are those of tests/resident_sparse_util.py."""
import json
import os

import pytest
import torch

import delta_file_util as D
import patch_ref as PR
import resident_sparse_util as S
from resident_delta_util import _bytes_equal

SPARSE = tuple("sp." + tag for tag in S.DTYPES) + ("0.weight", "0.bias", "1.weight", "1.bias")


def built(kind, base_sd, ft_sd, dev, odd=False):
    """-> (what the variant is over, its state dict, the state dict the variant decodes to, the sparse variant, the variant without sparse)."""
    from zipnn_amd import ResidentCheckpoint
    over, over_sd, want_sd = S.make(kind, base_sd, ft_sd, dev)
    if odd:
        want_sd = D.odd_state_dict(want_sd)
    ft = ResidentCheckpoint.from_state_dict(want_sd, dev, base=over, sparse=True, digests=True)
    today = ResidentCheckpoint.from_state_dict(want_sd, dev, base=over, digests=True) if not odd else None
    return over, over_sd, want_sd, ft, today


def sparse_entries(path):
    """-> (znn_delta record, {name: (lo, hi)} of the "sparse" entries, the data section)."""
    hdr, data, _ = D.read_container(path)
    rec = json.loads(hdr["__metadata__"]["znn_delta"])
    return rec, {n: tuple(hdr[n]["data_offsets"]) for n, k in rec["tensors"].items() if k == "sparse"}, data


def check_file(path, ft):
    """The file's bytes: version 2, all three kinds, every tensor that must be sparse is, each sparse entry the patch — as the built store holds it — at the
    entry's first multiple of 16 in the data section with zero bytes around it, L + 15 bytes in all.  -> Σ (L + 15)"""
    rec, ents, data = sparse_entries(path)
    hdr = D.read_container(path)[0]
    infos = json.loads(hdr["__metadata__"]["znn_compressed_vectors"])
    assert rec["version"] == 2 and rec["algo"] == "zn64-1"
    assert set(rec["tensors"].values()) == {"delta", "same", "sparse"}
    assert all(rec["tensors"].get(n) == "sparse" for n in SPARSE), rec["tensors"]
    assert sorted(rec["base_digests"]) == sorted(rec["tensors"])
    total = 0
    for n, (lo, hi) in ents.items():
        patch = bytes(ft._entries[n].patch.cpu().numpy())
        L = len(patch)
        at = (lo + 15) // 16 * 16
        assert hdr[n]["dtype"] == "U8" and hdr[n]["shape"] == [L + 15] and hi - lo == L + 15 and n in infos, n
        assert data[at:at + L] == patch and not any(data[lo:at]) and not any(data[at + L:hi]), n
        assert L == PR.patch_len(ft.info(n)["nbytes"], ft._entries[n].P, ft.info(n)["patch_entries"])
        total += L + 15
    return total


def check_same_store(a, b, path):
    """b (loaded) is the store a (built): the same info() for every tensor, byte-equal bodies and patches; b's patches are 16-byte aligned views of the one
    uploaded data section, each where the file has it."""
    D.check_same_store(a, b)
    _, ents, data = sparse_entries(path)
    blob = b._keep[0]
    assert blob.numel() == len(data)
    for n in a.keys():
        ea, eb = a._entries[n], b._entries[n]
        assert a.info(n)["patch_entries"] == b.info(n)["patch_entries"], n
        assert (ea.P, ea.bits, ea.byts, ea.chunk) == (eb.P, eb.bits, eb.byts, eb.chunk) or not ea.decoded, n
        if ea.patch is not None:
            assert torch.equal(ea.patch.cpu(), eb.patch.cpu()), n
            lo = ents[n][0]
            assert eb.patch.data_ptr() % 16 == 0 and eb.patch.data_ptr() - blob.data_ptr() == (lo + 15) // 16 * 16, n      # nothing is resident twice
    assert b.resident_bytes >= len(data) and b.resident_bytes - len(data) < 4096


def check_kinds_loaded(ft, plain_variant, over_sd, want_sd):
    """resident_sparse_util.check_kinds for a LOADED store: every per-tensor statement of it.  (Its two closing lines pin how a BUILT store packs its
    allocation — every body at a multiple of 256 —; a loaded store holds the file's data section instead, which check_same_store measures.)"""
    for tag, dt in S.DTYPES.items():
        n, E = "sp." + tag, torch.empty(0, dtype=dt).element_size()
        i = ft.info(n)
        T = S.changed(want_sd[n], over_sd[n])
        assert i["delta"] == "sparse" and i["patch_entries"] == T and i["compressed"], (n, i)
        assert i["resident_bytes"] == PR.patch_len(S.M * E, E, T), (n, i)
        assert 0.018 * S.M < T <= 0.02 * S.M, (n, T)
        assert ft.info("moved." + tag)["delta"] is True and ft.info("same." + tag)["delta"] == "same" and ft.info("absent." + tag)["delta"] is False, tag
        assert ft.info("moved." + tag)["patch_entries"] is None
    assert ft.info("steps")["delta"] is False
    for n in ft.keys():
        a, b = ft.info(n), plain_variant.info(n)
        if a["delta"] != "sparse":
            assert (a["delta"], a["resident_bytes"], a["compressed"]) == (b["delta"], b["resident_bytes"], b["compressed"]), n
        else:
            assert b["delta"] is True and a["resident_bytes"] < b["resident_bytes"], n


def check_round_trip(kind, base_sd, ft_sd, dev, tmp_path, odd=False):
    """from_state_dict(base=, sparse=True) -> save_file(sparse=True) -> from_file(base=): the same store, every entry point of DESIGN §3.10 on it, a further
    variant over it, and the file again."""
    from zipnn_amd import ResidentCheckpoint
    over, over_sd, want_sd, ft, today = built(kind, base_sd, ft_sd, dev, odd)
    with pytest.raises(ValueError, match="sp.bf16") as ex:                       # the default still refuses, and says what to pass
        ft.save_file(str(tmp_path / "refused.znn.safetensors"))
    assert "sparse=True" in str(ex.value) and not os.path.exists(tmp_path / "refused.znn.safetensors")
    p = ft.save_file(str(tmp_path / "ft.znn.safetensors"), sparse=True)
    assert sorted(os.listdir(tmp_path)) == ["ft.znn.safetensors"]                # (the temporary name is gone)
    total = check_file(p, ft)
    if odd:                                                                      # the 3 int8 bytes in front: entries start at odd offsets, patches do not
        _, ents, _ = sparse_entries(p)
        assert any(lo % 16 for lo, _ in ents.values()), ents
    ft2 = ResidentCheckpoint.from_file(p, dev, base=over, digests=True)
    check_same_store(ft, ft2, p)
    assert ft2.digests() == ft.digests()
    S.check_reads(ft2, want_sd, dev)                                             # (get_tensor(s), get_slice, plan; build_index(deltas=True) skips the patches)
    if odd:                                                                      # (the shifted layout is what this case is about: the rest runs without the three bytes)
        return p, total, over, want_sd, ft, today
    check_kinds_loaded(ft2, today, over_sd, want_sd)
    assert all(ft2.verify().values())
    S.check_model(ft2, over_sd, want_sd, dev, guard=True)                        # (hook, apply_ / revert_ with guards, holds)
    # the loaded store as the base of a further variant, and written down again
    sd3 = S.further(want_sd, seed=7)
    third = ResidentCheckpoint.from_state_dict(sd3, dev, base=ft2, sparse=True)
    assert third.info("sp.bf16")["delta"] == "sparse" and _bytes_equal(third.get_tensor("sp.bf16"), sd3["sp.bf16"]) and _bytes_equal(third.get_tensor("0.weight"), sd3["0.weight"])
    again = ft2.save_file(str(tmp_path / "again.znn.safetensors"), sparse=True)
    assert D.same_file(again, p)
    return p, total, over, want_sd, ft, today


def make_case(base_sd, ft_sd, dev, tmp_path):
    """One sparse variant over a resident base and its file, shared by the checks below (they only read them): -> (over, over_sd, want_sd, ft, today, path)."""
    over, over_sd, want_sd, ft, today = built("store", base_sd, ft_sd, dev)
    return over, over_sd, want_sd, ft, today, ft.save_file(str(tmp_path / "case.znn.safetensors"), sparse=True)


def check_sizes(case, tmp_path):
    """The sparse file is smaller than the delta file of the same pair; its sparse entries sum to Σ (L + 15).  A store without sparse entries writes the same
    bytes with sparse=True, with sparse=False and with no argument (what it wrote before there was one): version 1."""
    over, over_sd, want_sd, ft, today, p = case
    d = today.save_file(str(tmp_path / "delta.znn.safetensors"))
    total = check_file(p, ft)
    _, ents, _ = sparse_entries(p)
    assert sum(hi - lo for lo, hi in ents.values()) == total == sum(ft.info(n)["resident_bytes"] + 15 for n in ents)
    print("sparse file", os.path.getsize(p), "delta file", os.path.getsize(d), "sparse entries", total)
    assert os.path.getsize(p) < os.path.getsize(d)
    d1 = today.save_file(str(tmp_path / "delta1.znn.safetensors"), sparse=True)
    d0 = today.save_file(str(tmp_path / "delta0.znn.safetensors"), sparse=False)
    assert D.same_file(d1, d) and D.same_file(d0, d)
    rec = json.loads(D.read_container(d1)[0]["__metadata__"]["znn_delta"])
    assert rec["version"] == 1 and "sparse" not in rec["tensors"].values()


def _rewrite(path, out, edit):
    raw = bytearray(open(path, "rb").read())
    edit(raw)
    open(out, "wb").write(raw)
    return out


def check_guards(case, base_sd, dev, tmp_path):
    from zipnn_amd import DigestMismatch, ResidentCheckpoint, safetensors_io
    over, over_sd, want_sd, ft, today, p = case
    # "sparse" under version 1
    def to_v1(raw):
        assert raw.count(b'\\"version\\": 2') == 1
        raw[:] = raw.replace(b'\\"version\\": 2', b'\\"version\\": 1')
    v1 = _rewrite(p, str(tmp_path / "v1.znn.safetensors"), to_v1)
    with pytest.raises(ValueError, match="sparse"):
        ResidentCheckpoint.from_file(v1, dev, base=over)
    # no base
    for call in (lambda: ResidentCheckpoint.from_file(p, dev), lambda: safetensors_io.load_file(p, device=dev)):
        with pytest.raises(ValueError, match="znn_delta") as ex:
            call()
        assert "base=" in str(ex.value)
    # one byte of the base tensor under a patch changed: DigestMismatch naming it, before anything is decoded
    bad = {k: v.to(dev).clone() for k, v in D._changed(base_sd, "sp.fp32").items()}
    with pytest.raises(DigestMismatch) as ex:
        ResidentCheckpoint.from_file(p, dev, base=bad)
    assert ex.value.names == ["sp.fp32"]
    D.check_safe_open_refuses(p)


def check_damage(case, dev, tmp_path):
    """One byte of one sparse entry changed in the file — inside off[], a value zeroed, the slack, the padding: from_file raises a ValueError that names exactly
    that tensor.  With check_patches=False the files load; damage apply can see costs the first checked read of that tensor, and nothing else."""
    from zipnn_amd import DigestMismatch, ResidentCheckpoint
    from zipnn_amd._capi import ZnError
    over, over_sd, want_sd, ft, today, p = case
    _, ents, data = sparse_entries(p)
    start = os.path.getsize(p) - len(data)

    def place(n):
        lo, hi = ents[n]
        at = (lo + 15) // 16 * 16
        E, _, T, first, off, val = PR.parse(data[at:at + hi - lo - 15])
        a1 = PR.round16(32 + 4 * first.size)
        return start + lo, start + at, start + hi, a1, PR.round16(a1 + 2 * T), E

    def in_off(raw, n="sp.fp32"):
        lo, at, hi, a1, a2, E = place(n)
        raw[at + a1 + 2 * 5 + 1] ^= 0x80                                         # entry 5 of block 0 leaves the ascending order, up or down

    def zero_value(raw, n="sp.fp8"):
        lo, at, hi, a1, a2, E = place(n)
        assert E == 1 and raw[at + a2 + 7] != 0
        raw[at + a2 + 7] = 0

    def slack(raw, n="sp.fp16"):
        lo, at, hi, a1, a2, E = place(n)
        raw[lo if at > lo else hi - 1] = 1

    def padding(raw, n="sp.bf16"):
        lo, at, hi, a1, a2, E = place(n)
        assert a1 > 32 + 4 * 5                                                   # (M has four blocks: 12 bytes behind first[])
        raw[at + a1 - 1] = 1
    for k, (edit, victim, seen_by_apply) in enumerate(((in_off, "sp.fp32", True), (zero_value, "sp.fp8", True), (slack, "sp.fp16", False), (padding, "sp.bf16", False))):
        bad = _rewrite(p, str(tmp_path / f"bad{k}.znn.safetensors"), edit)
        with pytest.raises(ValueError) as ex:
            ResidentCheckpoint.from_file(bad, dev, base=over)
        assert not isinstance(ex.value, DigestMismatch) and repr(victim) in str(ex.value), (victim, str(ex.value))
        assert not any(repr(n) in str(ex.value) for n in ents if n != victim), str(ex.value)
        loose = ResidentCheckpoint.from_file(bad, dev, base=over, check_patches=False)
        if seen_by_apply:
            with pytest.raises(ZnError):
                loose.get_tensor(victim)
        else:
            assert _bytes_equal(loose.get_tensor(victim), want_sd[victim])
        other = "sp.bf16" if victim != "sp.bf16" else "sp.fp32"
        assert _bytes_equal(loose.get_tensor(other), want_sd[other])
    # the entry's length against the header's L: refused from the file alone, whatever check_patches says
    def longer(raw):
        lo, at, hi, a1, a2, E = place("sp.bf16")
        raw[at + 24:at + 32] = (int.from_bytes(raw[at + 24:at + 32], "little") + 16).to_bytes(8, "little")
    bad = _rewrite(p, str(tmp_path / "badlen.znn.safetensors"), longer)
    with pytest.raises(ValueError, match="sp.bf16"):
        ResidentCheckpoint.from_file(bad, dev, base=over, check_patches=False)
    ok = ResidentCheckpoint.from_file(p, dev, base=over, verify=True)
    assert _bytes_equal(ok.get_tensor("sp.fp32"), want_sd["sp.fp32"])


def check_load_file(case, base_sd, ft_sd, dev, tmp_path, device):
    """load_file(base=) over a store, a mapping and a path; compress_safetensors_file(base=, sparse=True) file to file."""
    from safetensors.torch import save_file
    from zipnn_amd import ResidentCheckpoint, safetensors_io
    base_plain, ft_plain = str(tmp_path / "base.safetensors"), str(tmp_path / "ft.safetensors")
    save_file(base_sd, base_plain, {"format": "pt"})
    save_file(ft_sd, ft_plain, {"format": "pt", "note": "a fine-tune"})
    store, p = case[0], case[5]
    mapping = {k: v.to(dev).clone() for k, v in base_sd.items()}
    rec, ents, _ = sparse_entries(p)
    assert rec["version"] == 2 and set(SPARSE) <= set(ents)
    for kind, b in (("mapping", mapping), ("store", store), ("path", base_plain)):
        got = safetensors_io.load_file(p, device=dev, base=b, verify=True)
        for n in ft_sd:
            assert _bytes_equal(got[n], ft_sd[n]), (kind, n)
    assert all(_bytes_equal(mapping[k], v) for k, v in base_sd.items())         # the base is only read
    out = safetensors_io.compress_safetensors_file(ft_plain, str(tmp_path / "f2f.znn.safetensors"), device=device, base=base_plain, digests=True, sparse=True)
    assert sparse_entries(out)[0]["tensors"] == rec["tensors"]
    meta = D.read_container(out)[0]["__metadata__"]
    assert meta["note"] == "a fine-tune" and set(SPARSE) <= set(sparse_entries(out)[1])
    got = safetensors_io.load_file(out, device=dev, base=base_plain, verify=True)
    for n in ft_sd:
        assert _bytes_equal(got[n], ft_sd[n]), n
