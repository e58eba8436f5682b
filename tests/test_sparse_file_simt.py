"""CPU tests (-m "not gpu"): delta files with SPARSE entries on the emulated kernels, CPU tensors as device memory — a variant store built with
sparse=True written by save_file(sparse=True) and read back by from_file(base=) over each kind of base, the file's bytes, the guards, damaged patches refused
by name at load, load_file and file-to-file compression.  The cases live in tests/sparse_file_util.py, shared with tests/test_gpu_sparse_file.py."""
import pytest
import torch

import resident_sparse_util as S
import sparse_file_util as F

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sds():
    return S.state_dicts()


@pytest.fixture(scope="module")
def case(simt_lib, sds, tmp_path_factory):
    """One sparse variant over a resident base and its file, built once on the emulated kernels for the tests that only read them."""
    import zipnn_amd._capi as capi
    keep, capi._LIB = capi._LIB, simt_lib
    try:
        return F.make_case(sds[0], sds[1], CPU, tmp_path_factory.mktemp("sparse_case"))
    finally:
        capi._LIB = keep


@pytest.mark.parametrize("kind", S.BASES)
def test_sparse_file_round_trip(use_simt, sds, kind, tmp_path):
    F.check_round_trip(kind, sds[0], sds[1], CPU, tmp_path)


def test_sparse_file_behind_three_odd_bytes(use_simt, sds, tmp_path):
    F.check_round_trip("dict", sds[0], sds[1], CPU, tmp_path, odd=True)


def test_sparse_file_sizes_and_files_without_sparse_entries(use_simt, case, tmp_path):
    F.check_sizes(case, tmp_path)


def test_sparse_file_guards(use_simt, sds, case, tmp_path):
    F.check_guards(case, sds[0], CPU, tmp_path)


def test_damaged_patches_are_refused_by_name_at_load(use_simt, case, tmp_path):
    F.check_damage(case, CPU, tmp_path)


def test_load_file_and_file_to_file(use_simt, sds, case, tmp_path):
    F.check_load_file(case, sds[0], sds[1], CPU, tmp_path, "cpu")
