"""GPU tests (-m gpu): changed-element patches ("znp1", include/zipnn_hip.h) on the real libzipnn_hip.so — the well-formed cases of
tests/test_patch_simt.py (tests/patch_util.py) at the same sizes: device-built patches equal the numpy restatement (tests/patch_ref.py) byte for byte, applies
give the tensor, then the base again, windows stay inside their canaries.  The only malformed input here is one the host refuses before any launch."""
import numpy as np
import pytest
import torch

import patch_util as U

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
def test_device_built_patches_equal_the_restatement(lib, dev, E):
    U.check_build(lib, dev, E)
    assert {"zn_k_patch_count", "zn_k_patch_scan", "zn_k_patch_emit"} <= set(lib.last_kernels().split(";"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("E,shifts", [(1, (1, 3)), (1, (5, 0)), (2, (1, 3)), (2, (0, 1)), (4, (1, 3)), (4, (2, 0))])
def test_build_at_element_aligned_addresses_that_differ_mod_16_on_the_device(lib, dev, E, shifts):
    U.check_build(lib, dev, E, shifts)
    torch.cuda.synchronize()


def test_ragged_batch_with_an_empty_and_an_identical_item_on_the_device(lib, dev):
    U.check_ragged(lib, dev)
    torch.cuda.synchronize()


def test_apply_whole_tensors_twice_over_a_base_and_the_public_functions_on_the_device(lib, dev):
    U.check_apply_whole(lib, dev)
    torch.cuda.synchronize()


@pytest.mark.parametrize("E", [1, 2, 4])
def test_apply_every_window_of_a_small_tensor_on_the_device(lib, dev, E):
    U.check_apply_windows(lib, dev, E)
    torch.cuda.synchronize()


def test_a_patch_shorter_than_its_header_is_refused_before_any_launch(lib, dev):
    src, base, patch = U.apply_pair(2)
    p = U.on_device(np.frombuffer(patch, dtype=np.uint8), dev)
    buf, view, o = U.canaried(base, dev, 2)
    with torch.cuda.device(dev):
        with pytest.raises(ValueError):
            lib.patch_apply_batch_dev([(p.data_ptr(), 31, base.size, 2, 0, base.size, view.data_ptr())])
    torch.cuda.synchronize()
    assert bytes(view.cpu().numpy()) == bytes(base) and U.canaries_intact(buf, o, base.size)
