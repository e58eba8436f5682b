"""CPU tests (-m "not gpu"): variant stores — zipnn_amd.ResidentCheckpoint.from_state_dict(ft_sd, base=...) holds a fine-tune as XOR deltas over a base that
is a plain {name: tensor} mapping, a resident store or a resident store with a sync index — on the emulated kernels (CPU tensors as device memory).
Every decoded tensor is compared with the fine-tune's own, bit for bit (tests/resident_delta_util.py)."""
import pytest
import torch

import resident_delta_util as R

DEV = torch.device("cpu")


@pytest.fixture(scope="module")
def sds():
    return R.state_dicts()


@pytest.mark.parametrize("kind", R.BASES)
def test_variant_store_decodes_the_fine_tune(use_simt, sds, kind):
    """get_tensor, get_tensors(into=), get_slice over rows that straddle a chunk boundary, plan().run() twice and a hooked forward of a two-Linear bf16
    Sequential all give the fine-tuned values; the variant is smaller than a plain store of the same tensors, the identical tensor holds 0 bytes, the
    unrelated one is not delta-coded; build_index() gives delta entries no index and decodes stay right."""
    base_sd, ft_sd = sds
    R.check_variant(kind, base_sd, ft_sd, DEV)


@pytest.mark.parametrize("kind", R.BASES)
def test_apply_and_revert_in_place(use_simt, sds, kind):
    """apply_ then revert_ restores the base's bytes; the names that could not be reverted are returned."""
    base_sd, ft_sd = sds
    R.check_apply_revert(kind, base_sd, ft_sd, DEV)


def test_a_module_as_base_and_a_variant_of_a_variant(use_simt, sds):
    """base= a module (its named parameters and buffers, held by reference); and a second fine-tune stored over the first variant: its decode runs the
    base's, the first delta's and its own, in that order."""
    from zipnn_amd import ResidentCheckpoint
    base_sd, ft_sd = sds
    m = R.model_of(base_sd, DEV)
    names = ["0.weight", "0.bias", "1.weight", "1.bias"]
    ft = ResidentCheckpoint.from_state_dict({k: ft_sd[k] for k in names}, DEV, base=m)
    assert all(ft.info(k)["delta"] is True for k in ("0.weight", "1.weight"))
    for k in names:
        assert R._bytes_equal(ft.get_tensor(k), ft_sd[k]), k
    changed = ft.apply_(m)                         # the base's own tensors: they now hold the fine-tune …
    assert sorted(changed) == sorted(names)
    for k, p in m.state_dict().items():
        assert R._bytes_equal(p, ft_sd[k]), k
    stay = ft.revert_(m)                           # … and the base again, except plain entries: the tensors they would be restored from are these
    assert sorted(stay) == sorted(k for k in names if ft.info(k)["delta"] is False)
    for k, p in m.state_dict().items():
        assert R._bytes_equal(p, ft_sd[k] if k in stay else base_sd[k]), k
    first = ResidentCheckpoint.from_state_dict(ft_sd, DEV, base=ResidentCheckpoint.from_state_dict(base_sd, DEV))
    ft2_sd = {k: R._perturb(v, 0.01, 500 + i) for i, (k, v) in enumerate(ft_sd.items()) if k.startswith("w.")}
    second = ResidentCheckpoint.from_state_dict(ft2_sd, DEV, base=first)
    assert all(second.info(k)["delta"] is True for k in ft2_sd)
    got = second.get_tensors(list(ft2_sd))
    for k in ft2_sd:
        assert R._bytes_equal(got[k], ft2_sd[k]), k
        assert R._bytes_equal(second.get_slice(k)[1:3], ft2_sd[k][1:3]), k
    with pytest.raises(ValueError):
        ResidentCheckpoint.from_state_dict(ft_sd, DEV, base={"w.bf16": base_sd["w.bf16"].t()})      # not contiguous


def test_status_speaks_for_every_launch_set_of_a_variant(use_simt, sds):
    """A variant over a resident base decodes in two or three launch sets; status() after plan.run() / get_slice reports damage in ANY of them — here a type
    byte of the BASE's body that is no type, which only the first set sees — and is quiet again once the body is whole."""
    from zipnn_amd import ResidentCheckpoint
    base_sd, ft_sd = sds
    names = ["w.bf16", "absent"]                   # a delta entry over the base, and a plain entry: base set, plain set, delta set
    base = ResidentCheckpoint.from_state_dict({"w.bf16": base_sd["w.bf16"]}, DEV)
    ft = ResidentCheckpoint.from_state_dict({k: ft_sd[k] for k in names}, DEV, base=base)
    assert ft.info("w.bf16")["delta"] is True and ft.info("absent")["compressed"]
    plan = ft.plan(names)
    assert len(plan._hs) == 3
    plan.run(); plan.status()
    body = base._entries["w.bf16"].body
    keep = int(body[0])
    body[0] = 7
    try:
        plan.run()
        with pytest.raises((RuntimeError, MemoryError)):
            plan.status()
        ft.get_slice("w.bf16")[0:2]
        with pytest.raises((RuntimeError, MemoryError)):
            ft.status()
    finally:
        body[0] = keep
    views = plan.run(); plan.status()
    for k in names:
        assert R._bytes_equal(views[k], ft_sd[k]), k
    plan.close()
