"""CPU tests (-m "not gpu"): "znp1" patches applied through strided views (zn_patch_apply_strided_batch_dev, zipnn_amd.patch_apply_ on non-contiguous tensors;
DESIGN §3.15) on the emulated kernels of zipnn_amd/csrc/zn_patch_strided.hip, against the numpy restatement tests/patch_ref.py applied to the logical row-major
array.  The cases live in tests/patch_strided_util.py, shared with tests/test_gpu_patch_strided.py."""
import pytest
import torch

import patch_strided_util as S

CPU = torch.device("cpu")


@pytest.mark.parametrize("E", [1, 2, 4])
def test_every_layout_gives_the_oracle_s_bytes_and_touches_nothing_else(use_simt, E):
    S.check_layouts(use_simt, CPU, E, public=True)


def test_one_batched_call_with_mixed_layouts_and_element_sizes(use_simt):
    S.check_mixed_batch(use_simt, CPU)


def test_refused_layouts_and_arguments_write_nothing(use_simt):
    S.check_refusals(use_simt, CPU, public=True)
    assert use_simt._L.zn_abi_version() == 3


@pytest.mark.parametrize("E", [1, 2, 4])
def test_hostile_patches_cost_the_verdict_and_no_byte_outside_the_view(use_simt, E):
    S.check_hostile(use_simt, CPU, E)
