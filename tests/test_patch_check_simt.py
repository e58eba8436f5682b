"""CPU tests (-m "not gpu"): zn_k_patch_check / zn_patch_check_batch_dev (zipnn_amd/csrc/zn_patch.hip) on the emulated kernels — well-formed
patches of the numpy restatement pass with their T, the hostile corpus of tests/test_patch_simt.py is refused with the bit of the check each case aims at, and
four damages apply does not see are refused as well.  The cases live in tests/patch_check_util.py, shared with tests/test_gpu_patch_check.py."""
import pytest
import torch

import patch_check_util as C

CPU = torch.device("cpu")


@pytest.mark.parametrize("E", [1, 2, 4])
def test_well_formed_patches_pass_with_their_T(use_simt, E):
    C.check_well_formed(use_simt, CPU, E)


@pytest.mark.parametrize("E", [1, 2, 4])
def test_the_hostile_corpus_is_refused_by_the_check_it_aims_at(use_simt, E):
    C.check_hostile(use_simt, CPU, E)


@pytest.mark.parametrize("E", [1, 2, 4])
def test_what_apply_does_not_see_the_check_refuses(use_simt, E):
    C.check_unseen(use_simt, CPU, E)


def test_a_batch_of_five_with_one_bad_item(use_simt):
    C.check_batch_of_five(use_simt, CPU)


def test_argument_checks(use_simt):
    C.check_arguments(use_simt, CPU)
