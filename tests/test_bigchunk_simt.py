"""CPU tests (-m "not gpu"): compression chunks above 256 KiB — 512 KiB, 1 MiB, 2 MiB, and the limit of 2 GiB — on the SIMT-emulated kernels.  The cases and
checkers are tests/bigchunk_util.py's, shared with tests/test_gpu_bigchunk.py: frames equal the CPU oracle's (and the reference core's where oracle/_ref is
built), decodes equal the inputs.  The emulator runs workgroups one after another and knows no LDS capacity or launch limit: the device file runs the same cases."""
import pytest
import torch

import bigchunk_util as B
import delta_inplace_util as U
import oracle_lib as O
from test_index_simt import _hint_counters

DEV = torch.device("cpu")
LADDER = B.ladder((19, 20, 21))
# Every geometry goes through every form; the emulator decodes about a megabyte of Huffman-coded planes a second, so within ONE geometry a form is not repeated
# on inputs the kernels cannot tell apart: u11 / const / rand chunks are raw planes (or RLE) like the weights-like ones beside them, and fp32 `skew` at 512 KiB is
# what the MAXBLOCK test runs through everything.  tests/test_gpu_bigchunk.py runs every case through every form.
LIGHT = (("host", "batch"), ("dev", "unaligned"))


def _forms(gid):
    fmt, kind, e = gid.split("-")
    if (fmt, kind, e) == ("fp32", "skew", "2^19"):
        return ("host",), ("host", "dev")
    if (fmt, kind) == ("fp32", "skew"):          # (four Huffman planes in the tail: the batched, multi-range and merge forms on the weights-like case beside it)
        return B.ENCODE_FORMS, ("host", "dev", "windows", "plan", "hinted", "unaligned")
    return (B.ENCODE_FORMS, B.DECODE_FORMS) if kind in ("natural", "skew") else LIGHT


@pytest.mark.parametrize("gid,cases", LADDER, ids=[g for g, _ in LADDER])
def test_ladder_encode_and_decode(simt_lib, gid, cases):
    """One full chunk, and two full chunks + 300 KiB + 308 bytes, at 512 KiB / 1 MiB / 2 MiB in bf16, fp16 and fp32 layouts over weights-like, 1-bit-code,
    11-bit-code, constant and random bytes: host and batched encode (one-pass encoder off and forced), legacy tree descriptions; host, device, batched,
    windowed, planned, hinted, unaligned, multi-range decode and the merge of per-range bodies."""
    enc, dec = _forms(gid)
    for case in cases:
        B.check_encode(simt_lib, DEV, case, enc)
        B.check_decode(simt_lib, DEV, case, dec, hint_counters=_hint_counters)


@pytest.mark.parametrize("bid,case,plane", B.BOUNDARY, ids=[b for b, _, _ in B.BOUNDARY])
def test_tail_plane_straddling_the_huff0_block_limit(simt_lib, bid, case, plane):
    """A partial last chunk whose planes are 131071 / 131072 / 131073 bytes (only a big chunk's tail can have such planes beside others): the encoder's
    `n > ZN_HUF_BLOCK_MAX` branches, the tail workgroups' upper edge and the serial decoder behind it (the destination at +4).  Every form at 131072 behind a
    full chunk; the forms that reach those branches everywhere."""
    B.boundary_precondition(case, plane)
    every = plane == B.HUF_MAX and case[1] > case[5] and bid.split("-c")[0] != "skew-P4"       # (fp32 skew at 2 MiB with such a tail: every form in the ladder)
    B.check_encode(simt_lib, DEV, case, B.ENCODE_FORMS if every else ("host", "batch"))
    B.check_decode(simt_lib, DEV, case, B.DECODE_FORMS if every else ("host", "dev", "plan", "unaligned"), hint_counters=_hint_counters)


@pytest.mark.parametrize("mid,case", B.MAXBLOCK, ids=[m for m, _ in B.MAXBLOCK])
def test_fp32_at_512k_every_plane_a_largest_huff0_block(simt_lib, decode_group, mid, case):
    """fp32 at 512 KiB: planes of exactly 128 KiB.  skew: all four Huffman-coded (one accumulate pass per further plane at maximum length); u11: planes 1 and 3,
    11-bit codes.  Thresholds 0.5 and 1.0; the index is longer than its table.  Two full chunks: every form; with the 308-byte tail: the chunk groups and the
    small-input forms as well."""
    B.maxblock_precondition(case)
    whole, skew = case[1] % case[5] == 0, case[0] == "skew"
    B.check_encode(simt_lib, DEV, case, B.ENCODE_FORMS if whole else ("host", "batch"))
    if whole:        # (the batched, multi-range and merge forms once per geometry: on the cheaper u11 case)
        B.check_decode(simt_lib, DEV, case, ("host", "dev", "windows", "plan", "unaligned") if skew else [f for f in B.DECODE_FORMS if f != "hinted"])
        B.check_thresholds(simt_lib, case)
    else:
        B.check_decode(simt_lib, DEV, case, ("dev",) if skew else ("host", "dev", "windows", "unaligned"))
        B.check_groups_and_wide(simt_lib, DEV, case, decode_group)
    B.check_hinted(simt_lib, DEV, case, _hint_counters, expect="more")


def test_index_of_bf16_at_1m_is_the_table_alone(simt_lib):
    """Every plane of a full 1 MiB bf16 chunk is raw: no hint region, the index is its offset table."""
    B.check_hinted(simt_lib, DEV, ("bf16", 2 * (1 << 20) + B.TAIL, 2, 1, 10, 1 << 20), _hint_counters, expect="table")


GROUPS = [g for g in LADDER if g[0].split("-")[1] in ("natural", "skew") and g[0] != "fp32-skew-2^19"]      # (fp32-skew-2^19: the MAXBLOCK test's)


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_ladder_decode_groups_and_wide_forms(simt_lib, decode_group, gid, cases):
    """zn_set_decode_group 1 .. 4 and zn_set_decode_wide 0 / 2 / 3 on the two-chunks-and-a-tail case of every geometry."""
    B.check_groups_and_wide(simt_lib, DEV, cases[1], decode_group)


@pytest.mark.parametrize("case", B.DELTA, ids=B.case_id)
def test_delta_compress_and_in_place_delta_decode(simt_lib, case):
    """The frame of a ^ b from the delta encoder; the decode into a separate destination and in place at address offsets 0, 4 and 1, through
    tests/delta_inplace_util.check_entry_points."""
    B.check_delta_compress(simt_lib, DEV, case)
    a, b, body = B.delta_case(case)
    # bf16 at 1 MiB and fp16 at 512 KiB: every entry point at 0, 4 and 1; fp32 at 512 KiB (four Huffman planes of 128 KiB): every entry point at 0, the call and the
    # plan at 4 and 1; the two tail-boundary cases: the call itself
    for off in U.OFFSETS:
        entries = ("delta_dev", "windows", "plan") if case in (B.DELTA[0], B.DELTA[2]) or (case == B.DELTA[1] and off == 0) else ("delta_dev", "plan") if case == B.DELTA[1] else ("delta_dev",)
        U.check_entry_points(simt_lib, case, a, b, body, off, DEV, entries=entries)


def test_oracle_frames_equal_the_reference_cores():
    """Every case's expected frame is also what the reference's own core writes (where oracle/_ref is built)."""
    if O.ref_core() is None:
        pytest.skip("oracle/_ref not built (no reference checkout on this host)")
    B.check_reference_core([c for _, cases in LADDER for c in cases] + [c for _, c, _ in B.BOUNDARY] + [c for _, c in B.MAXBLOCK])
    d = B._gen2("bf16", 300000, 7)
    B.same(B.ref_frame(B.HDR, d, 2, 1, 10, 1 << 31), O.compress_frame(B.HDR, d, 2, 1, 10, 1 << 31), "reference core at 1 << 31")
    with pytest.raises(AssertionError):
        B.ref_frame(B.HDR, d, 2, 1, 10, 1 << 32)              # the helper's guard: the core itself is never called


def test_zipnn_api_at_big_chunks(use_simt):
    B.check_zipnn_api()


def test_streaming_chunk_below_compression_chunk(use_simt):
    B.check_streaming()


def test_fp8_header_says_1m_coder_uses_128k(use_simt):
    B.check_fp8()


def test_file_with_1m_frames_through_loader_plugin_and_resident_stores(use_simt, tmp_path):
    B.check_file(tmp_path, DEV)


def test_chunk_of_2_gib(use_simt):
    B.check_chunk_2_31(use_simt, DEV)


def test_chunk_of_4_gib_is_refused_before_anything_is_launched(simt_lib):
    B.check_chunk_2_32_is_refused(simt_lib, DEV)


def test_header_exponent_41_is_refused(use_simt):
    B.check_header_exponent_41_is_refused()


@pytest.mark.parametrize("name", B.golden_names())
def test_reference_written_big_chunk_frames(use_simt, name):
    """Frames the reference's own Python wrote at compression_chunk 512 KiB, 1 MiB and 2 MiB (tests/golden/make_golden_bigchunk.py)."""
    B.check_golden(name)
