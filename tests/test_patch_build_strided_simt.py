"""CPU tests (-m "not gpu"): "znp1" patches built from strided views (zn_patch_size_strided_batch_dev / zn_patch_build_strided_batch_dev, zipnn_amd.patch_build on
non-contiguous tensors) on the emulated kernels of zipnn_amd/csrc/zn_patch_strided.hip, against the numpy restatement tests/patch_ref.py on the
logical row-major bytes.  The cases live in tests/patch_build_strided_util.py, shared with tests/test_gpu_patch_build_strided.py."""
import pytest
import torch

import patch_build_strided_util as B

CPU = torch.device("cpu")


@pytest.mark.parametrize("E", [1, 2, 4])
def test_every_layout_on_either_side_gives_the_oracle_s_patch_and_changes_no_tensor(use_simt, E):
    B.check_layouts(use_simt, CPU, E)


@pytest.mark.parametrize("E", [1, 2, 4])
def test_a_transposed_source_against_a_tile_shuffled_base(use_simt, E):
    B.check_two_layouts(use_simt, CPU, E)


def test_one_batched_call_launches_the_three_strided_kernels_and_a_collapsed_batch_the_contiguous_ones(use_simt):
    B.check_mixed_batch(use_simt, CPU)


def test_a_short_capacity_writes_nothing_and_returns_every_needed_length(use_simt):
    B.check_cap(use_simt, CPU)


def test_refused_arguments_alone_and_as_the_second_item_write_nothing(use_simt):
    B.check_refusals(use_simt, CPU)
    assert use_simt._L.zn_abi_version() == 3


def test_expanded_and_overlapping_sources_are_accepted(use_simt):
    B.check_expand(use_simt, CPU)


@pytest.fixture(scope="module")
def logical_lib(tmp_path_factory):
    """A second emulated build (tests/simt/build.sh's command with another output) with -DZN_PATCH_BUILD_LOGICAL_ORDER: load order (i), the baseline."""
    import glob
    import os
    import subprocess
    from zipnn_amd._capi import ZnLib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path_factory.mktemp("simt_logical") / "libzipnn_simt_logical.so")
    files = [a for f in sorted(glob.glob(os.path.join(root, "zipnn_amd", "csrc", "*.hip"))) for a in ("-x", "c++", f)]
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-w", "-I" + os.path.join(root, "tests", "simt"), "-DZN_SIMT_EMUL=1", "-DZN_PATCH_BUILD_LOGICAL_ORDER"] + files + ["-o", so],
                   check=True, capture_output=True)
    return ZnLib(so)


def test_both_load_orders_give_identical_bytes(simt_lib, logical_lib):
    """The order in which a block's elements are loaded is free: the library's default (along memory where the fast dimension is not the last) and the
    logical order give the same patches for every case — the bitmap makes the emit order independent of it."""
    for E in (1, 2, 4):
        assert B.check_layouts(logical_lib, CPU, E) == B.check_layouts(simt_lib, CPU, E)
        assert B.check_two_layouts(logical_lib, CPU, E) == B.check_two_layouts(simt_lib, CPU, E)
    assert B.check_mixed_batch(logical_lib, CPU) == B.check_mixed_batch(simt_lib, CPU)
    assert B.check_expand(logical_lib, CPU) == B.check_expand(simt_lib, CPU)


def test_public_patch_build_reads_views_where_they_lie_and_round_trips_through_patch_apply(use_simt):
    """zipnn_amd.patch_build(view, base) launches the strided kernels (before DESIGN §3.16 the call went through a contiguous copy and recorded the contiguous ones)."""
    B.check_public(use_simt, CPU)
