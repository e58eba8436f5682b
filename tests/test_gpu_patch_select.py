"""GPU tests (-m gpu): select and place of "znp1" patches (include/zipnn_hip.h) on the real libzipnn_hip.so — the well-formed cases of
tests/test_patch_select_simt.py (tests/patch_select_util.py) at the same sizes: device results equal the numpy restatement (tests/patch_select_ref.py) and the
patches built from the sliced tensors (tests/patch_ref.py) byte for byte, between canaries.  No malformed patch reaches the device: the only bad calls here are
the ones the host refuses before any launch."""
import pytest
import torch

import patch_select_util as SU

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
def test_device_select_and_place_equal_the_restatement_and_the_patches_of_the_sliced_tensors(lib, dev, E):
    SU.check_select_and_place(lib, dev, E)
    torch.cuda.synchronize()


def test_ragged_batch_of_mixed_element_sizes_with_an_empty_result_on_the_device(lib, dev):
    SU.check_ragged(lib, dev)
    torch.cuda.synchronize()


def test_placed_selects_of_two_and_three_way_splits_merge_back_to_the_patch_on_the_device(lib, dev):
    SU.check_splits_merge_back(dev)
    torch.cuda.synchronize()


def test_public_select_and_place_on_2d_and_3d_shapes_on_the_device(lib, dev):
    SU.check_public(dev)
    torch.cuda.synchronize()


def test_argument_errors_are_refused_before_any_launch(lib, dev):
    with torch.cuda.device(dev):
        out, op, E, g, held, want, placed = SU.argument_errors(lib, dev)
        p = held[False]
        assert lib.patch_select_batch_dev([(p.data_ptr(), p.numel(), E) + g[1:] + (op, len(want))]) == [len(want)]
    torch.cuda.synchronize()
    o0 = op - out.data_ptr()
    host = out.cpu().numpy()
    assert bytes(host[o0:o0 + len(want)]) == want and (host[o0 + len(want):] == 0x11).all() and (host[:o0] == 0x11).all()
