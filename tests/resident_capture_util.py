"""Shared by tests/test_resident_capture_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_resident_capture.py (hardware):
ResidentCheckpoint.from_live — live weights in an engine's own layouts captured as a variant store over a base, the qualifying tensors as "znp1"
patches built where they lie.  The live tensors are views inside sentinel-filled buffers (tests/patch_strided_util.py); the workaround the capture replaces,
from_state_dict({n: v.contiguous()}, base=base, sparse=True), is the reference for kinds and patches."""
import contextlib

import torch

import patch_strided_util as S
import resident_sparse_util as RS
from resident_delta_util import _bytes_equal

BASES = ("store", "dict")
BF, F32 = torch.bfloat16, torch.float32
# name -> (dtype, logical shape, storage elements, storage (1-D) -> the live view, what the fine-tune does to it)
LIVE = {
    "w.t": (BF, (300, 257), 300 * 257, lambda s: s.view(257, 300).t(), "few"),                                      # transposed storage; two blocks
    "w.narrow": (BF, (130, 517), 130 * 1031, lambda s: s.view(130, 1031)[:, 17:534], "few"),                         # a column slice of a fused buffer
    "w.tile": (BF, (16, 16, 10, 32), 256 * 320, lambda s: s.view(16, 10, 16, 32).permute(0, 2, 1, 3), "few"),        # a tile shuffle
    "w.plain": (BF, (70001,), 70001, lambda s: s, "few"),                                                            # contiguous
    "w.f32": (F32, (300, 257), 300 * 257, lambda s: s.view(257, 300).t(), "few"),
    "w.same": (BF, (300, 257), 300 * 257, lambda s: s.view(257, 300).t(), "none"),
    "w.dense": (BF, (300, 257), 300 * 257, lambda s: s.view(257, 300).t(), "many"),                                  # 30 % changed: at or above the ratio
    "w.int": (torch.int32, (40, 50), 2000, lambda s: s.view(50, 40).t(), "few"),
}
SPARSE = ("w.t", "w.narrow", "w.tile", "w.plain", "w.f32")


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def state_dicts(names=tuple(LIVE), seed=21):
    """-> (base_sd, new_sd) on the CPU, contiguous, in the logical shapes."""
    g = torch.Generator().manual_seed(seed)
    base, new = {}, {}
    for n in names:
        dt, shape, _, _, how = LIVE[n]
        m = _numel(shape)
        b = torch.randint(-1000, 1000, (m,), generator=g, dtype=torch.int32) if dt == torch.int32 else RS._values(g, m, dt)
        if dt == torch.int32:
            v = b.clone()
            v[::7] += 1
        else:
            v = b.clone() if how == "none" else RS._replace(b, 0.02 if how == "few" else 0.3, g)
        base[n], new[n] = b.reshape(shape), v.reshape(shape)
    return base, new


def _raw(t):
    return t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


def lives(dev, sd):
    """-> ({name: Live}, {name: the live view in the tensor's dtype}) holding sd's values"""
    lv = {n: S.Live(dev, t.element_size(), LIVE[n][2], LIVE[n][3], _raw(t)) for n, t in sd.items()}
    return lv, {n: x.view.view(LIVE[n][0]) for n, x in lv.items()}


@contextlib.contextmanager
def recorded(lib):
    """The patch size / build calls made through `lib` while the block runs -> [(method name, number of items)]"""
    names = ("patch_size_batch_dev", "patch_build_batch_dev", "patch_size_strided_batch_dev", "patch_build_strided_batch_dev")
    calls = []

    def wrap(name, fn):
        def call(items, *a, **k):
            items = list(items)
            calls.append((name, len(items)))
            return fn(items, *a, **k)
        return call
    for name in names:
        setattr(lib, name, wrap(name, getattr(lib, name)))
    try:
        yield calls
    finally:
        for name in names:
            delattr(lib, name)                                                    # (the instance attributes go; the class's methods are there again)


def make_base(kind, base_sd, dev):
    from zipnn_amd import ResidentCheckpoint
    if kind == "dict":
        return {k: v.to(dev).clone() for k, v in base_sd.items()}
    return ResidentCheckpoint.from_state_dict(base_sd, dev, index=True)


def check(kind, dev, tmp_path):
    import zipnn_amd
    from zipnn_amd import ResidentCheckpoint
    lib = zipnn_amd._capi.lib()
    tmp_path.mkdir(parents=True, exist_ok=True)
    base_sd, new_sd = state_dicts()
    base = make_base(kind, base_sd, dev)
    held, live = lives(dev, new_sd)
    assert not any(live[n].is_contiguous() for n in LIVE if n not in ("w.plain",))
    before = {n: x.bytes() for n, x in held.items()}
    with recorded(lib) as calls:
        cap = ResidentCheckpoint.from_live(live, base)
    assert all(x.bytes() == before[n] for n, x in held.items())                    # sources are only read
    ref = ResidentCheckpoint.from_state_dict({n: v.contiguous() for n, v in live.items()}, dev, base=base, sparse=True)
    kinds = {n: cap.info(n)["delta"] for n in cap.keys()}
    assert cap.keys() == list(LIVE)
    assert {n: kinds[n] for n in SPARSE} == {n: "sparse" for n in SPARSE}
    assert kinds["w.same"] == "same" and kinds["w.int"] is False
    assert kinds["w.dense"] == ref.info("w.dense")["delta"] and cap.info("w.dense")["resident_bytes"] == ref.info("w.dense")["resident_bytes"]
    # the calls: one strided size call for the seven candidates and one strided build call for the five below the ratio; the contiguous size / build calls
    # see only what fell to the chooser (w.dense: counted there, and built only if the chooser keeps its patch)
    assert [c for c in calls if "strided" in c[0]] == [("patch_size_strided_batch_dev", 7), ("patch_build_strided_batch_dev", 5)], calls
    assert all(n <= 1 for name, n in calls if "strided" not in name), calls
    for n in SPARSE:
        assert ref.info(n)["delta"] == "sparse"
        assert cap.patch(n).cpu().numpy().tobytes() == ref.patch(n).cpu().numpy().tobytes(), n
        assert cap.info(n)["patch_entries"] == ref.info(n)["patch_entries"]
    for store in (cap, ref):
        got = store.get_tensors(list(LIVE))
        for n in LIVE:
            assert _bytes_equal(got[n], new_sd[n]), n
            assert tuple(got[n].shape) == LIVE[n][1] and got[n].dtype == LIVE[n][0]
    assert _bytes_equal(cap.get_tensor("w.tile"), new_sd["w.tile"])
    # written down and read back over the same base
    path = cap.save_file(str(tmp_path / f"captured_{kind}.znn.safetensors"), sparse=True)
    back = ResidentCheckpoint.from_file(path, dev, base=base)
    assert {n: back.info(n)["delta"] for n in SPARSE} == {n: "sparse" for n in SPARSE}
    got = back.get_tensors(list(LIVE))
    assert all(_bytes_equal(got[n], new_sd[n]) for n in LIVE)
    # applied to a second replica: views that hold the base
    start = {n: base_sd[n] for n in LIVE}
    rep, target = lives(dev, start)
    assert sorted(cap.apply_(target)) == sorted(n for n in LIVE if n != "w.same")
    for n in LIVE:
        assert _bytes_equal(target[n], new_sd[n]), n
    assert all(x.outside_intact() for x in rep.values())
    cap.revert_(target)
    for n in LIVE:
        assert _bytes_equal(target[n], base_sd[n]), n
    assert all(x.outside_intact() for x in rep.values())
    # digests of the sources, as from_state_dict records them
    dig = ResidentCheckpoint.from_live(live, base, digests=True)
    assert dig.digests() == ResidentCheckpoint.from_state_dict({n: v.contiguous() for n, v in live.items()}, dev, base=base, sparse=True, digests=True).digests()
    assert dig.verify() == {n: True for n in LIVE}
    assert dig.holds(live) == {n: True for n in LIVE}
    # a ratio of 0 sends everything that changed to the chooser
    with recorded(lib) as calls:
        none = ResidentCheckpoint.from_live(live, base, ratio=0.0)
    assert ("patch_build_strided_batch_dev", 5) not in calls and all(_bytes_equal(none.get_tensor(n), new_sd[n]) for n in SPARSE)
    return {n: cap.patch(n).cpu().numpy().tobytes() for n in SPARSE}
