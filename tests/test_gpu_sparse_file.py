"""GPU tests (-m gpu): delta files with SPARSE entries on the real libzipnn_hip.so — the cases of tests/test_sparse_file_simt.py
(tests/sparse_file_util.py) with the same tensors: written by save_file(sparse=True), read back by from_file(base=) over each kind of base with every patch
validated whole by zn_k_patch_check before anything is decoded.  The damaged files cost a verdict and a ValueError, by construction; nothing here provokes a fault."""
import pytest
import torch

import resident_sparse_util as S
import sparse_file_util as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sds():
    return S.state_dicts()


@pytest.fixture(scope="module")
def case(sds, dev, tmp_path_factory):
    return F.make_case(sds[0], sds[1], dev, tmp_path_factory.mktemp("sparse_case"))


@pytest.mark.parametrize("kind", S.BASES)
def test_sparse_file_round_trip_on_the_device(sds, dev, kind, tmp_path):
    F.check_round_trip(kind, sds[0], sds[1], dev, tmp_path)
    from zipnn_amd import _capi
    torch.cuda.synchronize()
    assert _capi.lib().device_count() >= 1


def test_sparse_file_behind_three_odd_bytes_on_the_device(sds, dev, tmp_path):
    F.check_round_trip("dict", sds[0], sds[1], dev, tmp_path, odd=True)
    torch.cuda.synchronize()


def test_sparse_file_sizes_and_files_without_sparse_entries_on_the_device(case, tmp_path):
    F.check_sizes(case, tmp_path)


def test_sparse_file_guards_on_the_device(sds, case, dev, tmp_path):
    F.check_guards(case, sds[0], dev, tmp_path)
    torch.cuda.synchronize()


def test_damaged_patches_are_refused_by_name_at_load_on_the_device(case, dev, tmp_path):
    F.check_damage(case, dev, tmp_path)
    torch.cuda.synchronize()


def test_load_file_and_file_to_file_on_the_device(sds, case, dev, tmp_path):
    F.check_load_file(case, sds[0], sds[1], dev, tmp_path, "cuda:0")
    torch.cuda.synchronize()
