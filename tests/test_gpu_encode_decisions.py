"""GPU tests (-m gpu): the encoder's keep-or-store rules R1 .. R6 (tests/encode_decisions_util.py) on both sides of each edge, at every place
zipnn_amd/csrc/zn_encode_fused.hip restates them, on the real libzipnn_hip.so.  The cases and checkers are shared with tests/test_encode_decisions_simt.py:
every frame equals the oracle's, its type bytes equal the restated rule chain, both outcomes of each edge occur, and the frame decodes back."""
import pytest
import torch

import encode_decisions_util as E

pytestmark = pytest.mark.gpu
FULL = [(1, 0), (2, -1), (2, 0), (4, -1), (4, 0)]          # (planes, position of the constructed plane: -1 the last plane, 0 the first)


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    L.set_encode_onepass(1)
    yield L
    L.set_encode_onepass(1)


@pytest.mark.parametrize("mode", [2, 0], ids=["onepass", "four-kernel"])
@pytest.mark.parametrize("P,pos", FULL, ids=[f"P{P}-plane{'0' if pos == 0 else 'last'}" for P, pos in FULL])
def test_full_chunks_on_both_sides_of_every_edge_on_the_device(lib, P, pos, mode):
    """Planes of 16384 in chunks of 16384 * P: R1, R2, R4 (P = 1: n == cap) or R5 (cap > n), R1's threshold edge and R6's four thresholds, through the one-pass
    encoder (plane 0 kept: the speculation fails and the four-kernel encoder redoes the call) and through the stats + table kernels."""
    E.check_edges(lib, P, pos, mode)


@pytest.mark.parametrize("pos,mode", [(-1, 2), (0, 0)], ids=["last-onepass", "plane0-four-kernel"])
def test_full_chunks_of_two_8192_byte_planes_on_the_device(lib, pos, mode):
    E.check_edges(lib, 2, pos, mode, n=8192)


@pytest.mark.parametrize("n", E.TAILS)
def test_ragged_tail_behind_a_full_chunk_on_the_device(lib, n):
    E.check_ragged(lib, E.tail1, n, r5=n == 10001)


@pytest.mark.parametrize("n", E.ONLY)
def test_ragged_only_chunk_on_the_device(lib, n):
    E.check_ragged(lib, E.only1, n)


def test_header_and_12_byte_rules_at_9_to_23_bytes_on_the_device(lib):
    E.check_r3(lib)


@pytest.mark.parametrize("pos", [0, 1])
def test_geometry_the_fused_kernels_refuse_on_the_device(lib, pos):
    E.check_ragged(lib, E.refused2(pos), 10001, r5=True)


def test_four_planes_of_4096_through_the_ragged_workgroups_on_the_device(lib):
    E.check_ragged(lib, E.refused4(-1), 4096, r5=True)


@pytest.mark.parametrize("pos", [0, 1])
def test_ragged_tail_of_a_two_plane_tensor_on_the_device(lib, pos):
    E.check_ragged(lib, E.tail2(pos), 10001, r5=True, mode=2)


def test_threshold_compare_is_the_double_one_on_the_device(lib):
    E.check_float_double(lib)


@pytest.mark.parametrize("mode", [2, 0], ids=["onepass", "four-kernel"])
def test_largest_fused_plane_on_the_device(lib, mode):
    E.check_largest_plane(lib, mode)


@pytest.mark.parametrize("P,mode", [(1, 2), (1, 0), (2, 2), (2, 0), (4, 2), (4, 0)])
def test_delta_instances_full_chunks_on_the_device(lib, P, mode):
    E.check_edges(lib, P, -1, mode, base_seed=5)


def test_delta_instance_ragged_tail_on_the_device(lib):
    E.check_ragged(lib, E.tail1, 10001, base_seed=6)


def test_per_item_thresholds_in_one_batched_call_on_the_device(lib):
    E.check_batch_thresholds(lib, torch.device("cuda:0"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("P,mode", [(2, 2), (2, 0), (4, 2), (4, 0)])
def test_sign_rotated_layouts_on_the_device(lib, P, mode):
    E.check_rotated(lib, P, mode)
