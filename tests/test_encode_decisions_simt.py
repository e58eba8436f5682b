"""CPU tests (-m "not gpu"): the encoder's keep-or-store rules R1 .. R6 (tests/encode_decisions_util.py) on both sides of each edge, at every place
zipnn_amd/csrc/zn_encode_fused.hip restates them, on the SIMT-emulated kernels.  Shared with tests/test_gpu_encode_decisions.py, which runs the same checks on
the compiled kernels."""
import pytest
import torch

import encode_decisions_util as E

DEV = torch.device("cpu")
FULL = [(1, 0), (2, -1), (2, 0), (4, -1), (4, 0)]          # (planes, position of the constructed plane: -1 the last plane, 0 the first)


def test_constructions_reach_both_sides_with_the_oracle_alone():
    """No kernel: R2's two sides at the ten plane lengths, R3's at 14 / 15 bytes, R4's at n == cap, R5's with cap > n (pos == n - 1 raw, n - 2 kept), and the
    float / double disagreements of R6 exist.  A scan that misses fails here."""
    for n in E.R2_LENGTHS + (E.HUF_MAX,):
        L = E.r2_limit(n)
        cap = max(n, E.PLANE)
        assert E.huf_trace(E.r2_plane(n, L), cap)[0] == "R2" and E.huf_trace(E.r2_plane(n, L + 1), cap)[0] == "size", n
    assert [E.r2_limit(n) for n in E.R2_LENGTHS] == [132, 82, 36, 11, 6, 5, 5, 4, 4, 4]
    assert [E.huf_trace(E.r3_plane(n), E.PLANE)[0] for n in (9, 14, 15, 23)] == ["R3", "R3", "size", "size"]
    assert E.r4_sides() == (253, 254)
    for n, cap in ((8192, 16384), (4096, 16384), (10001, 16384), (10001, 20002), (10001, 32768), (16384, 32768), (16384, 65536)):
        k_raw, k_kept = E.r5_sides(n, cap)
        assert E.huf_trace(E.r5_plane(n, k_raw), cap) == ("R5", n - 1) and E.huf_trace(E.r5_plane(n, k_kept), cap) == ("size", n - 2)
    for n, cs, thr, _ in E.float_double_triples():
        assert E.float_rule(n, cs, thr) != E.double_rule(n, cs, thr)
    a = E.noise(4096, 1)
    for P in (2, 4):
        assert bytes(E.rotate_inv(E.rotate_fwd(a, P), P)) == bytes(a)


@pytest.mark.parametrize("mode", [2, 0], ids=["onepass", "four-kernel"])
@pytest.mark.parametrize("P,pos", FULL, ids=[f"P{P}-plane{'0' if pos == 0 else 'last'}" for P, pos in FULL])
def test_full_chunks_on_both_sides_of_every_edge(simt_lib, P, pos, mode):
    """Planes of 16384 in chunks of 16384 * P: R1, R2, R4 (P = 1: n == cap) or R5 (cap > n), R1's threshold edge and R6's four thresholds, through the one-pass
    encoder (plane 0 kept: the speculation fails and the four-kernel encoder redoes the call) and through the stats + table kernels."""
    E.check_edges(simt_lib, P, pos, mode)


@pytest.mark.parametrize("pos,mode", [(-1, 2), (0, 0)], ids=["last-onepass", "plane0-four-kernel"])
def test_full_chunks_of_two_8192_byte_planes(simt_lib, pos, mode):
    E.check_edges(simt_lib, 2, pos, mode, n=8192)


@pytest.mark.parametrize("n", E.TAILS)
def test_ragged_tail_behind_a_full_chunk(simt_lib, n):
    E.check_ragged(simt_lib, E.tail1, n, r5=n == 10001)


@pytest.mark.parametrize("n", E.ONLY)
def test_ragged_only_chunk(simt_lib, n):
    E.check_ragged(simt_lib, E.only1, n)


def test_header_and_12_byte_rules_at_9_to_23_bytes(simt_lib):
    E.check_r3(simt_lib)


@pytest.mark.parametrize("pos", [0, 1])
def test_geometry_the_fused_kernels_refuse(simt_lib, pos):
    E.check_ragged(simt_lib, E.refused2(pos), 10001, r5=True)


def test_four_planes_of_4096_through_the_ragged_workgroups(simt_lib):
    E.check_ragged(simt_lib, E.refused4(-1), 4096, r5=True)


@pytest.mark.parametrize("pos", [0, 1])
def test_ragged_tail_of_a_two_plane_tensor(simt_lib, pos):
    E.check_ragged(simt_lib, E.tail2(pos), 10001, r5=True, mode=2)


def test_threshold_compare_is_the_double_one(simt_lib):
    E.check_float_double(simt_lib)


@pytest.mark.parametrize("mode", [2, 0], ids=["onepass", "four-kernel"])
def test_largest_fused_plane(simt_lib, mode):
    E.check_largest_plane(simt_lib, mode)


@pytest.mark.parametrize("P,mode", [(1, 2), (2, 0), (4, 2)])
def test_delta_instances_full_chunks(simt_lib, P, mode):
    E.check_edges(simt_lib, P, -1, mode, base_seed=5)


def test_delta_instance_ragged_tail(simt_lib):
    E.check_ragged(simt_lib, E.tail1, 10001, base_seed=6)


def test_per_item_thresholds_in_one_batched_call(simt_lib):
    E.check_batch_thresholds(simt_lib, DEV)


@pytest.mark.parametrize("P,mode", [(2, 2), (4, 0)])
def test_sign_rotated_layouts(simt_lib, P, mode):
    E.check_rotated(simt_lib, P, mode)
