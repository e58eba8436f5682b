"""GPU tests (-m gpu): compression chunks above 256 KiB — 512 KiB, 1 MiB, 2 MiB, 4 MiB, and the limit of 2 GiB — on the real libzipnn_hip.so.  The cases and
checkers are tests/bigchunk_util.py's, shared with tests/test_bigchunk_simt.py; here every case goes through every form (the emulator's file repeats no form
on inputs its kernels cannot tell apart), and the ladder reaches 4 MiB.  No damaged bodies here: those stay on the emulator."""
import pytest
import torch

import bigchunk_util as B
import delta_inplace_util as U

pytestmark = pytest.mark.gpu

LADDER = B.ladder((19, 20, 21, 22))


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    L.set_decode_wide(1); L.set_decode_group(0); L.set_encode_onepass(1)
    yield L
    L.set_decode_wide(1); L.set_decode_group(0); L.set_encode_onepass(1)
    L.release_workspace()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("gid,cases", LADDER, ids=[g for g, _ in LADDER])
def test_ladder_encode_and_decode_on_the_device(lib, dev, decode_group, gid, cases):
    """One full chunk, and two full chunks + 300 KiB + 308 bytes, at 512 KiB .. 4 MiB in bf16, fp16 and fp32 layouts over weights-like, 1-bit-code, 11-bit-code,
    constant and random bytes, through every encode and decode form, every chunk group and every form of the small-input decoder."""
    for case in cases:
        B.check_encode(lib, dev, case)
        B.check_decode(lib, dev, case)
    B.check_groups_and_wide(lib, dev, cases[1], decode_group)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bid,case,plane", B.BOUNDARY, ids=[b for b, _, _ in B.BOUNDARY])
def test_tail_plane_straddling_the_huff0_block_limit_on_the_device(lib, dev, bid, case, plane):
    """A partial last chunk whose planes are 131071 / 131072 / 131073 bytes, behind zero or one full chunk: the encoder's `n > ZN_HUF_BLOCK_MAX` branches, the
    tail workgroups' upper edge, the serial decoder behind it."""
    B.boundary_precondition(case, plane)
    B.check_encode(lib, dev, case)
    B.check_decode(lib, dev, case)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mid,case", B.MAXBLOCK, ids=[m for m, _ in B.MAXBLOCK])
def test_fp32_at_512k_every_plane_a_largest_huff0_block_on_the_device(lib, dev, decode_group, mid, case):
    """fp32 at 512 KiB: planes of exactly 128 KiB, all four Huffman-coded with 1-bit codes (skew) or planes 1 and 3 with 11-bit codes (u11); thresholds 0.5 and
    1.0; the index is longer than its table."""
    B.maxblock_precondition(case)
    B.check_encode(lib, dev, case)
    B.check_thresholds(lib, case)
    B.check_decode(lib, dev, case, [f for f in B.DECODE_FORMS if f != "hinted"])
    B.check_hinted(lib, dev, case, expect="more")
    B.check_groups_and_wide(lib, dev, case, decode_group)
    torch.cuda.synchronize()


def test_index_of_bf16_at_1m_is_the_table_alone_on_the_device(lib, dev):
    B.check_hinted(lib, dev, ("bf16", 2 * (1 << 20) + B.TAIL, 2, 1, 10, 1 << 20), expect="table")
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", B.DELTA, ids=B.case_id)
def test_delta_compress_and_in_place_delta_decode_on_the_device(lib, dev, case):
    """The frame of a ^ b from the delta encoder; the decode into a separate destination and in place at address offsets 0, 4 and 1, every entry point of
    tests/delta_inplace_util.check_entry_points."""
    B.check_delta_compress(lib, dev, case)
    a, b, body = B.delta_case(case)
    for off in U.OFFSETS:
        U.check_entry_points(lib, case, a, b, body, off, dev)
    torch.cuda.synchronize()


def test_zipnn_api_at_big_chunks_on_the_device(lib):
    B.check_zipnn_api()


def test_streaming_chunk_below_compression_chunk_on_the_device(lib):
    B.check_streaming()


def test_fp8_header_says_1m_coder_uses_128k_on_the_device(lib):
    B.check_fp8()


def test_file_with_1m_frames_through_loader_plugin_and_resident_stores_on_the_device(lib, dev, tmp_path):
    B.check_file(tmp_path, dev)
    torch.cuda.synchronize()


def test_chunk_of_2_gib_on_the_device(lib, dev):
    B.check_chunk_2_31(lib, dev)


def test_chunk_of_4_gib_is_refused_before_anything_is_launched_on_the_device(lib, dev):
    B.check_chunk_2_32_is_refused(lib, dev)
    torch.cuda.synchronize()


def test_header_exponent_41_is_refused_on_the_device(lib):
    B.check_header_exponent_41_is_refused()


@pytest.mark.parametrize("name", B.golden_names())
def test_reference_written_big_chunk_frames_on_the_device(lib, name):
    """Frames the reference's own Python wrote at compression_chunk 512 KiB, 1 MiB and 2 MiB (tests/golden/make_golden_bigchunk.py)."""
    B.check_golden(name)
