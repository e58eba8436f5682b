"""GPU tests (-m gpu): zn_k_patch_check on the real libzipnn_hip.so — the cases of tests/test_patch_check_simt.py (tests/patch_check_util.py) at the same sizes:
well-formed patches pass with their T; the hostile corpus and the damages apply does not see cost a verdict — the kernel reads nothing outside the patch and
writes nothing but verdict words —, and the verdicts are the emulated build's, which the util holds as literals."""
import pytest
import torch

import patch_check_util as C

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
def test_well_formed_patches_pass_with_their_T_on_the_device(lib, dev, E):
    C.check_well_formed(lib, dev, E)
    torch.cuda.synchronize()


@pytest.mark.parametrize("E", [1, 2, 4])
def test_the_hostile_corpus_gets_the_emulated_builds_verdicts_on_the_device(lib, dev, E):
    C.check_hostile(lib, dev, E)
    torch.cuda.synchronize()


@pytest.mark.parametrize("E", [1, 2, 4])
def test_what_apply_does_not_see_the_check_refuses_on_the_device(lib, dev, E):
    C.check_unseen(lib, dev, E)
    torch.cuda.synchronize()


def test_a_batch_of_five_with_one_bad_item_on_the_device(lib, dev):
    C.check_batch_of_five(lib, dev)
    torch.cuda.synchronize()


def test_argument_checks_on_the_device(lib, dev):
    C.check_arguments(lib, dev)
    torch.cuda.synchronize()
