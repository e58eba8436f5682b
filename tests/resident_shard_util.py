"""Shared by tests/test_resident_shard_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_resident_shard.py (hardware):
ResidentCheckpoint.sharded — both shards of a two-way tensor-parallel split of a sparse variant store, against the fine-tune's own tensors
narrowed, bit for bit, and the kept patches against tests/patch_ref.py's patch of the shard pair, byte for byte."""
import gc

import pytest
import torch

import patch_ref as PR
from resident_delta_util import _bytes_equal
from resident_sparse_util import _as_int, _move_all, _replace, _values, changed

# name -> (dtype, shape, the dimension it is split along; None: absent from the spec, kept whole)
TENSORS = {"w.d0": (torch.bfloat16, (400, 350), 0), "w.d1": (torch.float32, (256, 600), 1), "w.3d": (torch.bfloat16, (6, 40, 700), 1),
           "w.half": (torch.bfloat16, (400, 350), 0), "same": (torch.bfloat16, (300, 240), 0), "moved": (torch.bfloat16, (300, 240), 1),
           "steps": (torch.int64, (40,), 0), "whole": (torch.float16, (70001,), None)}
SPARSE = ("w.d0", "w.d1", "w.3d", "whole")
WAYS = 2


def state_dicts(seed=13):
    """-> (base_sd, ft_sd) on the CPU: 2 % of the elements of the sparse tensors replaced; w.half only in the rows of the second shard; `same` identical;
    every element of `moved` moved (a delta body); an int64 tensor."""
    g = torch.Generator().manual_seed(seed)
    base, ft = {}, {}
    for name, (dt, shape, _) in TENSORS.items():
        n = 1
        for d in shape:
            n *= d
        base[name] = torch.arange(n, dtype=dt).reshape(shape) if dt == torch.int64 else _values(g, n, dt).reshape(shape)
    for name in SPARSE:
        ft[name] = _replace(base[name], 0.02, g)
    half = base["w.half"].clone()
    half[200:] = _replace(base["w.half"][200:].contiguous(), 0.02, g)
    ft.update({"w.half": half, "same": base["same"].clone(), "moved": _move_all(base["moved"]), "steps": base["steps"] + 5})
    return base, {n: ft[n] for n in TENSORS}


def further(ft_sd, seed=14):
    g = torch.Generator().manual_seed(seed)
    return {n: (_replace(t, 0.02, g) if n in SPARSE + ("w.half",) else t + 1 if n == "steps" else t.clone()) for n, t in ft_sd.items()}


def spec_of(k, names=TENSORS):
    """The k-th of WAYS equal parts of every tensor along its dimension."""
    out = {}
    for name in names:
        _, shape, dim = TENSORS[name]
        if dim is not None:
            out[name] = (dim, k * shape[dim] // WAYS, (k + 1) * shape[dim] // WAYS)
    return out


def cut(sd, spec, dev=None):
    """-> {name: the spec's narrow of sd's tensor, contiguous (on dev)}"""
    out = {n: (t.narrow(spec[n][0], spec[n][1], spec[n][2] - spec[n][1]).contiguous() if n in spec else t.clone()) for n, t in sd.items()}
    return out if dev is None else {n: t.to(dev) for n, t in out.items()}


def ref_patch(t, over):
    return PR.build(t.reshape(-1).view(torch.uint8).numpy(), over.reshape(-1).view(torch.uint8).numpy(), t.element_size())


def check_reads(store, want_sd, over_sd, dev):
    """Every entry point of a shard store against the narrowed tensors."""
    names = list(want_sd)
    assert store.keys() == names
    for n in names:
        assert _bytes_equal(store.get_tensor(n), want_sd[n]), n
        assert store.info(n)["shape"] == list(want_sd[n].shape)
    got = store.get_tensors(names)
    for n in names:
        assert _bytes_equal(got[n], want_sd[n]), n
    for n in names:
        rows = want_sd[n].shape[0]
        for idx in (slice(0, 1), slice(rows // 2 - 1, rows // 2 + 2), slice(rows - 3, rows), rows - 1):
            assert _bytes_equal(store.get_slice(n)[idx], want_sd[n][idx]), (n, idx)
    store.status()
    plan = store.plan(names)
    for _ in range(2):
        views = plan.run()
        plan.status()
        for n in names:
            assert _bytes_equal(views[n], want_sd[n]), n
    plan.close()
    live = {n: over_sd[n].to(dev).clone() for n in names}
    store.apply_(live)
    for n in names:
        assert _bytes_equal(live[n], want_sd[n]), n
    assert store.revert_(live) == []
    for n in names:
        assert _bytes_equal(live[n], over_sd[n]), n


def check_shards(dev, tmp_path, onto_kind):
    """Both shards of the two-way split, over a mapping of base shard tensors (onto_kind "dict") or over a store built from them ("store")."""
    from zipnn_amd import ResidentCheckpoint
    b_sd, ft_sd = state_dicts()
    base = ResidentCheckpoint.from_state_dict(b_sd, dev, digests=True)
    ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base, sparse=True)
    assert [ft.info(n)["delta"] for n in TENSORS] == ["sparse"] * 4 + ["same", True, False, "sparse"]
    before = {n: ft.info(n) for n in TENSORS}
    for k in range(WAYS):
        spec = spec_of(k)
        over_sd, want_sd = cut(b_sd, spec), cut(ft_sd, spec)
        onto = cut(b_sd, spec, dev)
        if onto_kind == "store":
            onto = ResidentCheckpoint.from_state_dict(onto, dev, digests=True)
        mine = ft.sharded(onto, spec)
        kinds = {n: mine.info(n)["delta"] for n in TENSORS}
        assert kinds == {"w.d0": "sparse", "w.d1": "sparse", "w.3d": "sparse", "w.half": "same" if k == 0 else "sparse", "same": "same",
                         "moved": kinds["moved"], "steps": False, "whole": "sparse"} and kinds["moved"] in (True, False), kinds
        for n in TENSORS:
            i = mine.info(n)
            if kinds[n] == "sparse":
                want = ref_patch(want_sd[n], over_sd[n])
                assert bytes(mine._entries[n].patch.cpu().numpy()) == want, n       # what patch_build gives for the shard pair
                assert i["patch_entries"] == changed(want_sd[n], over_sd[n]) == PR.parse(want)[2] and i["resident_bytes"] == len(want)
            else:
                assert i["patch_entries"] is None
            assert i["digest"] is None and i["index_bytes"] == 0
        assert mine.info("w.half")["resident_bytes"] == (0 if k == 0 else mine.info("w.half")["resident_bytes"]) and mine.info("same")["resident_bytes"] == 0
        assert bytes(mine._entries["whole"].patch.cpu().numpy()) == bytes(ft._entries["whole"].patch.cpu().numpy())
        check_reads(mine, want_sd, over_sd, dev)
        # written down once per rank, read back over the rank's shard of the base
        p = mine.save_file(str(tmp_path / f"rank{k}.{onto_kind}.delta.znn.safetensors"), sparse=True)
        again = ResidentCheckpoint.from_file(p, dev, base=onto)
        assert {n: again.info(n)["delta"] for n in TENSORS} == kinds
        for n in TENSORS:
            assert _bytes_equal(again.get_tensor(n), want_sd[n]), n
            if kinds[n] == "sparse":
                assert bytes(again._entries[n].patch.cpu().numpy()) == bytes(mine._entries[n].patch.cpu().numpy())
        del again
        assert {n: ft.info(n) for n in TENSORS} == before                          # the source store is what it was
    # the shard store keeps `onto` alive and nothing of the old store
    del ft, base
    gc.collect()
    check_reads(mine, want_sd, over_sd, dev)


def check_without_onto(dev):
    """onto=None: every tensor goes through the fallback and the result is a plain store of the shards."""
    from zipnn_amd import ResidentCheckpoint
    b_sd, ft_sd = state_dicts()
    ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=ResidentCheckpoint.from_state_dict(b_sd, dev), sparse=True)
    spec = spec_of(1)
    mine = ft.sharded(None, spec)
    want_sd = cut(ft_sd, spec)
    assert all(mine.info(n)["delta"] is False for n in TENSORS)
    for n in TENSORS:
        assert _bytes_equal(mine.get_tensor(n), want_sd[n]), n


def check_errors(dev):
    from zipnn_amd import ResidentCheckpoint
    b_sd, ft_sd = state_dicts()
    base = ResidentCheckpoint.from_state_dict(b_sd, dev)
    ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base, sparse=True)
    spec = spec_of(0)
    onto = cut(b_sd, spec, dev)
    with pytest.raises(ValueError, match="no.such"):
        ft.sharded(onto, dict(spec, **{"no.such": (0, 0, 1)}))
    for bad in ((0, 100, 401), (0, 7, 7), (2, 0, 1), (0, -1, 5)):
        with pytest.raises(ValueError, match="w.d0"):
            ft.sharded(onto, dict(spec, **{"w.d0": bad}))
    wrong = dict(onto)
    wrong["w.d1"] = cut(b_sd, spec_of(0), dev)["w.d1"][:, :-1].contiguous()      # another shape
    wrong["w.3d"] = wrong["w.3d"].to(torch.float16)                              # another dtype
    with pytest.raises(ValueError) as ei:
        ft.sharded(wrong, spec)
    assert "w.d1" in str(ei.value) and "w.3d" in str(ei.value) and "w.d0" not in str(ei.value)      # every mismatch, and only those
    with pytest.raises(ValueError, match="w.d0"):
        ft.sharded({n: t.to(dev) for n, t in b_sd.items()}, spec)                # the whole base where its shards are expected


def check_chain(dev):
    """A chain is sharded link by link, and decodes the right shards."""
    from zipnn_amd import ResidentCheckpoint
    b_sd, s1_sd = state_dicts()
    s2_sd = further(s1_sd)
    base = ResidentCheckpoint.from_state_dict(b_sd, dev)
    s1 = ResidentCheckpoint.from_state_dict(s1_sd, dev, base=base, sparse=True)
    s2 = ResidentCheckpoint.from_state_dict(s2_sd, dev, base=s1, sparse=True)
    assert [s2.info(n)["delta"] for n in SPARSE + ("w.half",)] == ["sparse"] * 5
    for k in range(WAYS):
        spec = spec_of(k)
        m1 = s1.sharded(cut(b_sd, spec, dev), spec)
        m2 = s2.sharded(m1, spec)
        want1, want2 = cut(s1_sd, spec), cut(s2_sd, spec)
        for n in SPARSE + ("w.half",):
            assert m2.info(n)["delta"] == "sparse" and bytes(m2._entries[n].patch.cpu().numpy()) == ref_patch(want2[n], want1[n]), n
        for n in TENSORS:
            assert _bytes_equal(m2.get_tensor(n), want2[n]) and _bytes_equal(m1.get_tensor(n), want1[n]), n
        got = m2.get_tensors(list(TENSORS))
        for n in TENSORS:
            assert _bytes_equal(got[n], want2[n]), n


def check_no_decode_one_select(lib, dev, monkeypatch):
    """A store of only sparse and same entries is sharded without one decode and by exactly one select call."""
    from zipnn_amd import ResidentCheckpoint
    b_sd, ft_sd = state_dicts()
    names = ("w.d0", "w.d1", "w.3d", "w.half", "same", "whole")
    b_sd, ft_sd = {n: b_sd[n] for n in names}, {n: ft_sd[n] for n in names}
    base = {n: t.to(dev) for n, t in b_sd.items()}                                # plain base tensors: building the variant decodes nothing either
    ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base, sparse=True)
    assert {ft.info(n)["delta"] for n in names} == {"sparse", "same"}
    decodes, selects = [], []
    real_decode, real_select = ResidentCheckpoint._decode, lib.patch_select_batch_dev
    monkeypatch.setattr(ResidentCheckpoint, "_decode", lambda self, work, check: decodes.append(len(work)) or real_decode(self, work, check))
    monkeypatch.setattr(lib, "patch_select_batch_dev", lambda items, stream=0: selects.append(len(list(items))) or real_select(items, stream))
    spec = spec_of(0, names)
    mine = ft.sharded(cut(b_sd, spec, dev), spec)
    assert decodes == [] and selects == [5], (decodes, selects)
    assert "zn_k_patch_select_emit" in lib.last_kernels()
    want = cut(ft_sd, spec)
    for n in names:
        assert _bytes_equal(mine.get_tensor(n), want[n]), n
