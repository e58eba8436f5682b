"""GPU tests (-m gpu): ResidentCheckpoint.rebased on the real libzipnn_hip.so — the cases of tests/test_resident_rebase_simt.py
(tests/resident_rebase_util.py) at the same sizes: a flattened chain and re-parented siblings decode the bytes of the state dicts they were built from through
every entry point, and their merged patches equal tests/patch_ref.py's byte for byte."""
import pytest
import torch

import resident_rebase_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from zipnn_amd import _capi
    assert _capi.lib().device_count() >= 1
    yield torch.device("cuda:0")
    _capi.lib().release_workspace()


def test_a_chain_of_sparse_variants_flattens_onto_its_first_base_on_the_device(dev, tmp_path):
    U.check_chain(dev, tmp_path)
    torch.cuda.synchronize()


def test_siblings_over_one_base_become_patches_over_each_other_on_the_device(dev):
    U.check_siblings(dev)
    torch.cuda.synchronize()
