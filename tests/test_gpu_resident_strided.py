"""GPU tests (-m gpu): a variant store applied to non-contiguous live tensors (ResidentCheckpoint.apply_ / revert_ / holds / guard / patch) on the
real libzipnn_hip.so: the cases and checks of tests/test_resident_strided_simt.py (tests/resident_strided_util.py), at the same sizes, on cuda:0."""
import pytest
import torch

import resident_strided_util as S

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
def test_variant_store_on_strided_live_tensors_on_the_device(lib, sds, kind):
    S.check(kind, sds[0], sds[1], torch.device("cuda:0"))
    torch.cuda.synchronize()
