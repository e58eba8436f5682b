"""GPU tests (-m gpu): the XOR-merge of "znp1" patches (include/zipnn_hip.h) on the real libzipnn_hip.so — the well-formed cases of
tests/test_patch_merge_simt.py (tests/patch_merge_util.py) at the same sizes: device merges equal the numpy restatement (tests/patch_merge_ref.py) and the patch
built from the two tensors (tests/patch_ref.py) byte for byte, between canaries.  No malformed patch reaches the device: the only bad calls here are the ones the
host refuses before any launch."""
import pytest
import torch

import patch_merge_util as MU

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
def test_device_merges_equal_the_restatement_and_the_patch_of_the_two_tensors(lib, dev, E):
    MU.check_merge(lib, dev, E)
    assert {"zn_k_patch_merge_count", "zn_k_patch_scan", "zn_k_patch_merge_emit"} <= set(lib.last_kernels().split(";"))
    torch.cuda.synchronize()


def test_ragged_batch_of_mixed_element_sizes_with_cancelling_items_on_the_device(lib, dev):
    MU.check_ragged(lib, dev)
    torch.cuda.synchronize()


def test_public_merge_takes_live_weights_from_a_to_b_and_back_on_the_device(lib, dev):
    MU.check_public(dev)
    torch.cuda.synchronize()


def test_argument_errors_are_refused_before_any_launch(lib, dev):
    with torch.cuda.device(dev):
        ok, out, want, held = MU.argument_errors(lib, dev)
        assert lib.patch_merge_batch_dev([ok]) == [len(want)]
    torch.cuda.synchronize()
    o0 = (-out.data_ptr()) % 16
    host = out.cpu().numpy()
    assert bytes(host[o0:o0 + len(want)]) == want and (host[o0 + len(want):] == 0x11).all() and (host[:o0] == 0x11).all()
