"""GPU tests (-m gpu): "znp1" patches built from strided views (zn_patch_build_strided_batch_dev) on the real libzipnn_hip.so — the cases of
tests/test_patch_build_strided_simt.py (tests/patch_build_strided_util.py) at the same shapes, against the numpy restatement on the logical bytes, and byte for
byte what the emulated build gives for the same inputs.  Refused arguments are refused, not trapped: no test here provokes a fault."""
import pytest
import torch

import patch_build_strided_util as B

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
def test_every_layout_on_the_device_equals_the_oracle_and_the_emulated_build(lib, simt_lib, dev, E):
    got = B.check_layouts(lib, dev, E)
    torch.cuda.synchronize()
    assert got == B.check_layouts(simt_lib, torch.device("cpu"), E)


@pytest.mark.parametrize("E", [1, 2, 4])
def test_two_different_layouts_on_the_device(lib, simt_lib, dev, E):
    got = B.check_two_layouts(lib, dev, E)
    torch.cuda.synchronize()
    assert got == B.check_two_layouts(simt_lib, torch.device("cpu"), E)


def test_one_batched_call_and_a_collapsed_batch_on_the_device(lib, simt_lib, dev):
    got = B.check_mixed_batch(lib, dev)
    torch.cuda.synchronize()
    assert got == B.check_mixed_batch(simt_lib, torch.device("cpu"))


def test_a_short_capacity_writes_nothing_on_the_device(lib, dev):
    B.check_cap(lib, dev)
    torch.cuda.synchronize()


def test_refused_arguments_write_nothing_on_the_device(lib, dev):
    B.check_refusals(lib, dev)
    torch.cuda.synchronize()


def test_expanded_and_overlapping_sources_on_the_device(lib, simt_lib, dev):
    got = B.check_expand(lib, dev)
    torch.cuda.synchronize()
    assert got == B.check_expand(simt_lib, torch.device("cpu"))


def test_public_patch_build_on_views_of_device_memory(lib, dev):
    B.check_public(lib, dev)
    torch.cuda.synchronize()
