"""CPU tests (-m "not gpu"): variant stores with SPARSE entries (zipnn_amd.ResidentCheckpoint.from_state_dict(..., base=..., sparse=True)) on the
emulated kernels: a fine-tune that replaces 2 % of a tensor's elements is kept as a "znp1" patch of exactly the format's length, and every read of it — get_tensor,
get_tensors, get_slice windows that cut chunks and patch blocks, plan, hook, verify, holds, apply_ / revert_ and their guards — gives the fine-tune's bytes, over
a mapping of tensors, a store with and without an index, and a variant that has sparse entries itself.  The cases live in tests/resident_sparse_util.py, shared
with tests/test_gpu_resident_sparse.py."""
import pytest
import torch

import resident_sparse_util as S

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sds():
    return S.state_dicts()


@pytest.mark.parametrize("kind", S.BASES)
def test_sparse_variant_store(use_simt, sds, kind, tmp_path):
    base_sd, ft_sd = sds
    S.check_store(kind, base_sd, ft_sd, CPU, tmp_path)
    assert "zn_k_patch_apply" in use_simt.last_kernels()
