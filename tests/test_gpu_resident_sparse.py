"""GPU tests (-m gpu): variant stores with sparse entries (zipnn_amd.ResidentCheckpoint.from_state_dict(..., base=..., sparse=True)) on the real
libzipnn_hip.so: the cases and checks of tests/test_resident_sparse_simt.py (tests/resident_sparse_util.py), at the same sizes, on cuda:0."""
import pytest
import torch

import resident_sparse_util as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    yield L
    L.release_workspace()


@pytest.fixture(scope="module")
def sds():
    return S.state_dicts()


@pytest.mark.parametrize("kind", S.BASES)
def test_sparse_variant_store_on_the_device(lib, sds, kind, tmp_path):
    base_sd, ft_sd = sds
    S.check_store(kind, base_sd, ft_sd, torch.device("cuda:0"), tmp_path)
    assert "zn_k_patch_apply" in lib.last_kernels()
    torch.cuda.synchronize()
