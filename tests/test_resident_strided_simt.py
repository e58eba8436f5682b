"""CPU tests (-m "not gpu"): a variant store applied to non-contiguous live tensors (ResidentCheckpoint.apply_ / revert_ / holds / guard / patch) on
the emulated kernels: a sparse entry through transposed storage, a delta entry into a dim-1 narrow of a fused buffer, a plain entry into a channels-last layout,
a "same" entry on a contiguous tensor — over a mapping of tensors and over a resident base.  The cases live in tests/resident_strided_util.py, shared with
tests/test_gpu_resident_strided.py."""
import pytest
import torch

import resident_strided_util as S


@pytest.fixture(scope="module")
def sds():
    return S.state_dicts()


@pytest.mark.parametrize("kind", S.BASES)
def test_variant_store_on_strided_live_tensors(use_simt, sds, kind):
    S.check(kind, sds[0], sds[1], torch.device("cpu"))
