"""GPU tests (-m gpu): "znp1" patches applied through strided views (zn_patch_apply_strided_batch_dev) on the real libzipnn_hip.so — the cases of
tests/test_patch_strided_simt.py (tests/patch_strided_util.py) at the same shapes, against the numpy restatement applied to the logical array, and byte for byte
what the emulated build gives for the same inputs.  Hostile patches and refused layouts are refused, not trapped: no test here provokes a fault."""
import pytest
import torch

import patch_strided_util as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    yield L
    L.release_workspace()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("E", [1, 2, 4])
def test_every_layout_on_the_device_equals_the_oracle_and_the_emulated_build(lib, simt_lib, dev, E):
    got = S.check_layouts(lib, dev, E, public=True)
    torch.cuda.synchronize()
    assert got == S.check_layouts(simt_lib, torch.device("cpu"), E, public=False)


def test_one_batched_call_with_mixed_layouts_and_element_sizes_on_the_device(lib, dev):
    S.check_mixed_batch(lib, dev)
    torch.cuda.synchronize()


def test_refused_layouts_and_arguments_write_nothing_on_the_device(lib, dev):
    S.check_refusals(lib, dev, public=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("E", [1, 2, 4])
def test_hostile_patches_are_refused_on_the_device(lib, dev, E):
    S.check_hostile(lib, dev, E)
    torch.cuda.synchronize()
