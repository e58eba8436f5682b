"""Shared by tests/test_resident_strided_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_resident_strided.py (hardware): a variant
store applied to NON-CONTIGUOUS live tensors (ResidentCheckpoint.apply_ / revert_ / holds / guard on strided views).  A base and a fine-tune of four
tensors of (300, 257) bf16 — one kept sparse, one as a delta, one plain, one "same" — each live in another layout inside a sentinel-filled buffer
(tests/patch_strided_util.py): the logical values are the fine-tune's after apply_, the base's after revert_, and no byte outside the views moves."""
import pytest
import torch

import patch_strided_util as S
import resident_sparse_util as RS
from resident_delta_util import _bytes_equal

SHAPE = (300, 257)
M = SHAPE[0] * SHAPE[1]
BASES = ("dict", "store")
# name -> (storage elements, storage (1-D) -> the live view of shape SHAPE)
LIVE = {
    "w.sparse": (M, lambda s: s.view(257, 300).t()),                                             # transposed storage
    "w.delta": (300 * 600, lambda s: s.view(300, 600)[:, 100:357]),                              # a dim-1 narrow of a fused buffer
    "w.plain": (M, lambda s: s.view(1, 1, 257, 300).permute(0, 3, 1, 2)[0, :, 0, :]),            # NCHW (1, 300, 1, 257) kept channels-last, seen as its (C, W) matrix
    "w.same": (M, lambda s: s.view(SHAPE)),                                                      # contiguous
}
RESHAPED = (M, lambda s: s.view(771, 100).t())                                                   # w.sparse's elements as a (100, 771) matrix, stored transposed


def state_dicts(seed=11):
    g = torch.Generator().manual_seed(seed)
    base = {n: RS._values(g, M, torch.bfloat16).reshape(SHAPE) for n in ("w.sparse", "w.delta", "w.same")}
    ft = {"w.sparse": RS._replace(base["w.sparse"], 0.02, g), "w.delta": RS._move_all(base["w.delta"]), "w.same": base["w.same"].clone(),
          "w.plain": RS._values(g, M, torch.bfloat16).reshape(SHAPE)}
    return base, ft


def _raw(t):
    return t.contiguous().view(torch.int16).reshape(-1).numpy().tobytes()


def check(kind, base_sd, ft_sd, dev):
    import zipnn_amd
    from zipnn_amd import DigestMismatch, ResidentCheckpoint
    base = {k: v.to(dev).clone() for k, v in base_sd.items()} if kind == "dict" else ResidentCheckpoint.from_state_dict(base_sd, dev, digests=True)
    ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base, sparse=True, digests=True)
    assert {n: ft.info(n)["delta"] for n in ft.keys()} == {"w.sparse": "sparse", "w.delta": True, "w.plain": False, "w.same": "same"}
    start = dict(base_sd, **{"w.plain": torch.zeros(SHAPE, dtype=torch.bfloat16)})              # (the base has no w.plain: whatever lies there is overwritten)
    lives = {n: S.Live(dev, 2, st, make, _raw(start[n])) for n, (st, make) in LIVE.items()}
    target = {n: lv.view.view(torch.bfloat16) for n, lv in lives.items()}
    assert not target["w.sparse"].is_contiguous() and not target["w.delta"].is_contiguous() and not target["w.plain"].is_contiguous()

    def holds_exactly(sd, names):
        for n in names:
            assert _bytes_equal(target[n], sd[n]), n
        assert all(lv.outside_intact() for lv in lives.values())

    holds_exactly(base_sd, base_sd)
    assert ft.holds(target) == {"w.sparse": False, "w.delta": False, "w.plain": False, "w.same": True}
    with pytest.raises(DigestMismatch):
        ft.revert_(target, guard=True)                                                            # they hold the base, not the variant
    holds_exactly(base_sd, base_sd)
    assert sorted(ft.apply_(target, guard=True)) == ["w.delta", "w.plain", "w.sparse"]
    holds_exactly(ft_sd, ft_sd)
    assert "zn_k_patch_apply_strided" in zipnn_amd._capi.lib().last_kernels()
    assert ft.holds(target) == {n: True for n in ft_sd}
    with pytest.raises(DigestMismatch):
        ft.apply_(target, guard=True)                                                             # … and the other way round
    holds_exactly(ft_sd, ft_sd)
    assert ft.revert_(target, guard=True) == ["w.plain"]                                          # nothing to restore it from: it stays
    holds_exactly(base_sd, base_sd)
    assert _bytes_equal(target["w.plain"], ft_sd["w.plain"])
    # unchecked: one status speaks for the whole run
    ft.apply_(target, check=False)
    ft.status()
    holds_exactly(ft_sd, ft_sd)
    ft.revert_(target, check=False)
    ft.status()
    holds_exactly(base_sd, base_sd)
    # the patch itself, for a live layout with ANOTHER shape than the entry's
    p = ft.patch("w.sparse")
    assert p.dtype == torch.uint8 and p.is_contiguous() and p.device == target["w.sparse"].device
    other = S.Live(dev, 2, RESHAPED[0], RESHAPED[1], _raw(base_sd["w.sparse"]))
    view = other.view.view(torch.bfloat16)
    assert tuple(view.shape) == (100, 771) and zipnn_amd.patch_apply_(view, p) is view
    assert _bytes_equal(view.reshape(SHAPE), ft_sd["w.sparse"]) and other.outside_intact()
    ft.apply_({"w.sparse": target["w.sparse"]})
    assert _raw(view.cpu()) == _raw(target["w.sparse"].cpu())                                     # … what apply_ does
    ft.revert_({"w.sparse": target["w.sparse"]})
    assert ft.patch("w.same") is None
    with pytest.raises(ValueError):
        ft.patch("w.delta")
    with pytest.raises(ValueError):
        ft.patch("w.plain")
    with pytest.raises(KeyError):
        ft.patch("w.nothing")
    # refused targets say why, before anything is touched
    with pytest.raises(ValueError, match="stride of 0"):
        ft.apply_({"w.sparse": target["w.sparse"][:1].expand(SHAPE)})
    with pytest.raises(ValueError, match="shape"):
        ft.apply_({"w.sparse": view})
    holds_exactly(base_sd, base_sd)
