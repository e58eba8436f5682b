"""Shared by tests/test_resident_rebase_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_resident_rebase.py (hardware):
ResidentCheckpoint.rebased — a chain of sparse variants flattened onto its first base, and siblings over one base re-parented onto each other —
against the state dicts the stores were built from, bit for bit, and the merged patches against tests/patch_ref.py, byte for byte."""
import gc

import pytest
import torch

import patch_ref as PR
from resident_delta_util import _bytes_equal
from resident_sparse_util import _as_int, _replace, _values, changed

SPARSE = ("w.bf16", "0.weight", "w.fp8")               # 65 537 bf16 elements, 65 536 fp32 ones (a Linear's weight, for the hook), 2 * 65 536 + 3 fp8 ones
NAMES = SPARSE + ("steps", "moved")


def base_sd(seed=9):
    g = torch.Generator().manual_seed(seed)
    return {"w.bf16": _values(g, 65537, torch.bfloat16), "0.weight": _values(g, 65536, torch.float32).reshape(256, 256),
            "w.fp8": _values(g, 2 * 65536 + 3, torch.float8_e4m3fn), "steps": torch.arange(40, dtype=torch.int64),
            "moved": _values(g, 70001, torch.bfloat16)}


def step(prev, first, k, seed, back=40):
    """The next step of a run: about 1 % of the elements of the sparse tensors replaced, `back` of the elements that differ from the first step's set back to
    ITS values (their entries cancel in a merge); the int tensor counts on; `moved` changes entirely (bit k of every element flips)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n in SPARSE:
        t = _replace(prev[n], 0.01, g)
        a, f = _as_int(t.reshape(-1)), _as_int(first[n].reshape(-1))
        idx = torch.nonzero(_as_int(prev[n].reshape(-1)) != f).reshape(-1)[:back]
        a[idx] = f[idx]
        out[n] = t
    out["steps"] = prev["steps"] + 1
    out["moved"] = (_as_int(prev["moved"]) ^ (1 << k)).view(torch.bfloat16)
    return out


def chain_sds():
    b = base_sd()
    s1 = step(b, b, 0, 101, back=0)
    s2 = step(s1, b, 1, 102)
    s3 = step(s2, b, 2, 103)
    return b, s1, s2, s3


def ref_patch(t, over):
    """tests/patch_ref.py's patch of tensor `t` over tensor `over` (CPU tensors of one dtype)."""
    return PR.build(t.reshape(-1).view(torch.uint8).numpy(), over.reshape(-1).view(torch.uint8).numpy(), t.element_size())


def patch_bytes(store, name):
    return bytes(store._entries[name].patch.cpu().numpy())


def check_reads(store, want_sd, dev):
    names = list(NAMES)
    for n in names:
        assert _bytes_equal(store.get_tensor(n), want_sd[n]), n
    got = store.get_tensors(names)
    for n in names:
        assert _bytes_equal(got[n], want_sd[n]), n
    for n, idx in (("w.bf16", slice(65530, 65537)), ("w.bf16", slice(0, 3)), ("0.weight", slice(127, 129)), ("0.weight", 255), ("w.fp8", slice(65535, 131074)),
                   ("w.fp8", slice(131072, 131075)), ("moved", slice(5, 70000))):
        assert _bytes_equal(store.get_slice(n)[idx], want_sd[n][idx]), (n, idx)
    store.status()
    plan = store.plan(names)
    for _ in range(2):
        views = plan.run()
        plan.status()
        for n in names:
            assert _bytes_equal(views[n], want_sd[n]), n
    plan.close()
    x = torch.randn(4, 256, generator=torch.Generator().manual_seed(1)).to(dev)
    ref = torch.nn.Sequential(torch.nn.Linear(256, 256, bias=False))
    ref.load_state_dict({"0.weight": want_sd["0.weight"]})
    m = torch.nn.Sequential(torch.nn.Linear(256, 256, bias=False)).to(dev)
    h = store.hook(m)
    out = m(x)
    h.status()
    assert _bytes_equal(out, ref.to(dev)(x))
    h.remove()


def check_chain(dev, tmp_path):
    from zipnn_amd import ResidentCheckpoint
    b_sd, s1_sd, s2_sd, s3_sd = chain_sds()
    base = ResidentCheckpoint.from_state_dict(b_sd, dev, digests=True)
    s1 = ResidentCheckpoint.from_state_dict(s1_sd, dev, base=base, sparse=True)
    s2 = ResidentCheckpoint.from_state_dict(s2_sd, dev, base=s1, sparse=True)
    s3 = ResidentCheckpoint.from_state_dict(s3_sd, dev, base=s2, sparse=True, digests=True)
    for s in (s1, s2, s3):
        assert [s.info(n)["delta"] for n in SPARSE] == ["sparse"] * 3 and s.info("moved")["delta"] in (True, False)
    before = {n: (s3.info(n), patch_bytes(s3, n)) for n in SPARSE}
    flat = s3.rebased(base)
    assert flat.device == s3.device and flat.keys() == s3.keys()
    cancelled = 0
    for n in SPARSE:
        i, E = flat.info(n), b_sd[n].element_size()
        want = ref_patch(s3_sd[n], b_sd[n])
        T = changed(s3_sd[n], b_sd[n])
        assert i["delta"] == "sparse" and i["patch_entries"] == T == PR.parse(want)[2] and i["compressed"], (n, i)
        assert patch_bytes(flat, n) == want, n
        assert i["resident_bytes"] == len(want) and i["index_bytes"] == 0
        cancelled += sum(changed(s[n], p[n]) for s, p in ((s1_sd, b_sd), (s2_sd, s1_sd), (s3_sd, s2_sd))) - T
        assert (s3.info(n), patch_bytes(s3, n)) == before[n]                     # the source store is what it was
    assert cancelled > 0, "no entry cancelled between the steps"
    assert flat.info("steps")["delta"] is False and flat.info("moved")["delta"] in (True, False) and flat.info("moved")["patch_entries"] is None
    assert flat.digests() == s3.digests() and all(flat.verify().values())
    check_reads(flat, s3_sd, dev)
    check_reads(s3, s3_sd, dev)
    # written down and read back over the base
    p = flat.save_file(str(tmp_path / "step3.delta.znn.safetensors"), sparse=True)
    again = ResidentCheckpoint.from_file(p, dev, base=base)
    for n in NAMES:
        assert _bytes_equal(again.get_tensor(n), s3_sd[n]), n
    assert [again.info(n)["delta"] for n in SPARSE] == ["sparse"] * 3
    del again
    # a partial flattening: onto a store in the middle of the chain
    mid = s3.rebased(s1)
    for n in SPARSE:
        assert mid.info(n)["delta"] == "sparse" and patch_bytes(mid, n) == ref_patch(s3_sd[n], s1_sd[n]), n
    check_reads(mid, s3_sd, dev)
    del mid
    # … and the other way round: the base as a variant of the last step
    back = base.rebased(s3)
    for n in SPARSE:
        assert back.info(n)["delta"] == "sparse" and patch_bytes(back, n) == patch_bytes(flat, n), n
    for n in NAMES:
        assert _bytes_equal(back.get_tensor(n), b_sd[n]), n
    del back
    # the chain may go: flat keeps the base alive and nothing else
    del s1, s2, s3, before
    gc.collect()
    check_reads(flat, s3_sd, dev)
    with pytest.raises(ValueError):
        flat.rebased({n: t.to(dev) for n, t in b_sd.items()})
    with pytest.raises(ValueError):
        flat.rebased(ResidentCheckpoint(torch.device("meta"), [], 0))


def check_siblings(dev):
    from zipnn_amd import DigestMismatch, ResidentCheckpoint
    b_sd = base_sd()
    g = torch.Generator().manual_seed(77)
    a_sd = {"w.bf16": _replace(b_sd["w.bf16"], 0.01, g), "0.weight": b_sd["0.weight"].clone(), "w.fp8": _replace(b_sd["w.fp8"], 0.01, g),
            "steps": b_sd["steps"] + 1, "moved": (_as_int(b_sd["moved"]) ^ 1).view(torch.bfloat16)}
    bb_sd = {"w.bf16": _replace(a_sd["w.bf16"], 0.01, g), "0.weight": b_sd["0.weight"].clone(), "w.fp8": a_sd["w.fp8"].clone(),
             "steps": b_sd["steps"] + 2, "moved": (_as_int(b_sd["moved"]) ^ 2).view(torch.bfloat16)}
    base = ResidentCheckpoint.from_state_dict(b_sd, dev, digests=True)
    a = ResidentCheckpoint.from_state_dict(a_sd, dev, base=base, sparse=True, digests=True)
    b = ResidentCheckpoint.from_state_dict(bb_sd, dev, base=base, sparse=True, digests=True)
    assert a.info("0.weight")["delta"] == "same" and a.info("w.fp8")["delta"] == "sparse" and b.info("w.fp8")["delta"] == "sparse"
    sw = b.rebased(a)
    assert sw.info("0.weight")["delta"] == "same"                                # shared with the base, unchanged
    assert sw.info("w.fp8")["delta"] == "same" and sw.info("w.fp8")["resident_bytes"] == 0      # equal in a and b, not in the base: the two patches cancel
    assert sw.info("w.bf16")["delta"] == "sparse" and patch_bytes(sw, "w.bf16") == ref_patch(bb_sd["w.bf16"], a_sd["w.bf16"])
    assert sw.info("w.bf16")["patch_entries"] == changed(bb_sd["w.bf16"], a_sd["w.bf16"])
    check_reads(sw, bb_sd, dev)
    assert all(sw.verify().values())
    live = {n: a_sd[n].to(dev).clone() for n in NAMES}
    sw.apply_(live, guard=True)
    for n in NAMES:
        assert _bytes_equal(live[n], bb_sd[n]), n
    assert all(sw.holds(live).values())
    assert sw.revert_(live, guard=True) == []
    for n in NAMES:
        assert _bytes_equal(live[n], a_sd[n]), n
    held = {n: b_sd[n].to(dev).clone() for n in NAMES}
    with pytest.raises(DigestMismatch):
        sw.apply_(held, guard=True)                                              # they hold the base, not a
    for n in NAMES:
        assert _bytes_equal(held[n], b_sd[n]), n
    # b over the base against b over a: the re-parented store is the smaller one where the two fine-tunes are close
    assert sw.info("w.fp8")["resident_bytes"] < b.info("w.fp8")["resident_bytes"]
    del b
    gc.collect()
    check_reads(sw, bb_sd, dev)
