"""CPU tests (-m "not gpu"): the in-place delta decode of include/zipnn_hip.h on the SIMT-emulated kernels — an item whose destination IS its delta base
(d_dst == d_delta; a window: d_dst == d_delta + chunk_lo * chunk) ends as decoded ^ (what it held), in every form of the decoder.  The fused kernel's delta
instance always could; the generic path (unaligned bases, partial last chunks the serial decoder takes, tableLog 12, planes the fused kernel declines)
used to decode its Huffman planes over the base before XORing with it.  Bodies: the CPU oracle's frames of tensor ^ base (tests/delta_inplace_util.py)."""
import numpy as np
import pytest
import torch

import delta_inplace_util as U
import oracle_lib as O

DEV = torch.device("cpu")


@pytest.mark.parametrize("off", U.OFFSETS, ids=lambda o: f"mod16={o}")
@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_in_place_delta_decode_every_entry_point(simt_lib, case, off):
    """zn_decompress_delta_dev, a window batch ([0,K), [1,K), [K-1,K)) and a plan run twice, destination pre-filled with the base at address 0 / 4 / 1 modulo
    16: the fine-tune's bytes == the decode into a separate destination; the plan's second run gives the base back; guard bytes untouched.  On the
    parent commit fp32 (its partial chunk) and every case at 4 and 1 give wrong bytes."""
    a, b, body = U.delta_case(case)
    U.check_entry_points(simt_lib, case, a, b, body, off, DEV)


@pytest.mark.parametrize("off", (0, 4), ids=lambda o: f"mod16={o}")
@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_aligned_in_place_calls_stay_on_the_fused_kernel(simt_lib, case, off):
    """The contract must not push aligned calls off the hot path: every full chunk by zn_k_decode_fused^delta at address 0 modulo 16, none at 4 (the generic
    kernels, zn_k_alias_rotate ahead of them where the dtype has the sign rotate)."""
    a, b, body_bytes = U.delta_case(case)
    _, nb, P, rot, bm, ch = case
    body = U.to_dev(body_bytes, DEV)
    _, dst = U.place(b, off, DEV)
    simt_lib.decompress_dev(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, dst.data_ptr(), 0, True, delta_ptr=dst.data_ptr())
    ks = simt_lib.last_kernels().split(";")
    assert ks[0].startswith("zn_k_decode_fused^delta^inplace" if P > 1 else "zn_k_decode_fused^delta") and ("^inplace" in ks[0]) == (P > 1), ks   # (one plane: the delta instance itself)
    assert simt_lib.last_fused_chunks() == (nb // ch if off == 0 else 0)
    assert ("zn_k_alias_rotate" in ks) == (rot == 1 and P > 1), ks
    assert U.got(dst) == a
    # a separate destination never launches the pre-pass
    _, bsep = U.place(b, off, DEV)
    sep = torch.empty(nb, dtype=torch.uint8)
    simt_lib.decompress_dev(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, sep.data_ptr(), 0, True, delta_ptr=bsep.data_ptr())
    assert "zn_k_alias_rotate" not in simt_lib.last_kernels() and "^inplace" not in simt_lib.last_kernels()


@pytest.mark.parametrize("off", (0, 4), ids=lambda o: f"mod16={o}")
@pytest.mark.parametrize("name", U.MORE)
def test_in_place_with_rle_raw_and_hostile_codes(simt_lib, name, off):
    """Identical tensors (every plane RLE zero), an unrelated base (raw planes), 1-bit codes with every plane Huffman-coded (two and four planes: the fused
    kernel's further passes, the serial decoder at +4), 11-bit codes, tiles denser than the stream average — aligned and at +4."""
    case, a, b, body = U.more_case(name)
    U.check_entry_points(simt_lib, case, a, b, body, off, DEV)


@pytest.mark.parametrize("off", (0, 4), ids=lambda o: f"mod16={o}")
@pytest.mark.parametrize("P", (2, 4))
def test_in_place_with_a_table_log_12_plane_behind_planes_the_fused_kernel_took(simt_lib, P, off):
    """tableLog 12 (huff0's decoders take it, the fused kernel's tables do not): chunk 0 has it in its LAST plane — aligned, the fused kernel has XORed the
    planes before it into the base when it finds out, hands the base back (the same passes once more) and leaves the chunk to the generic path; chunk 1
    has it in its first plane.  At +4 everything is the generic path's."""
    case, a, b, body = U.tl12_case(P)
    U.check_entry_points(simt_lib, case, a, b, body, off, DEV)
    assert simt_lib.last_fused_chunks() == 0


def test_in_place_batch_mixes_aliased_and_separate_items(simt_lib):
    """One zn_decompress_batch_dev call: in-place items at 0 and +4, an item with a separate base, an item without a base — each ends as its own decode."""
    specs = [(U.CASES[0], 0, "inplace"), (U.CASES[0], 4, "inplace"), (U.CASES[2], 0, "inplace"), (U.CASES[1], 0, "separate"), (U.CASES[3], 1, "inplace"),
             (U.CASES[4], 4, "inplace"), (U.CASES[1], 0, "plain")]
    items, checks, keep = [], [], []
    for case, off, how in specs:
        a, b, body_bytes = U.delta_case(case)
        _, nb, P, rot, bm, ch = case
        if how == "plain":
            body_bytes = O.compress_frame(b"", a, P, rot, bm, ch)
        body = U.to_dev(body_bytes, DEV)
        buf, dst = U.place(b if how == "inplace" else bytes(nb), off, DEV)
        base = dst if how == "inplace" else (U.place(b, off, DEV)[1] if how == "separate" else None)
        keep += [body, buf, base]
        items.append((body.data_ptr(), body.numel(), P, rot, bm, ch, nb, dst.data_ptr(), base.data_ptr() if base is not None else None))
        checks.append((buf, dst, a))
    simt_lib.decompress_batch_dev(items, 0, True)
    for i, (buf, dst, a) in enumerate(checks):
        assert U.got(dst) == a, (i, specs[i][1:])
        assert U.guards_ok(buf, dst)


def test_damaged_bodies_in_place_report_what_a_separate_destination_reports(simt_lib):
    """check=True verdicts do not depend on the aliasing: a jump table that claims more than its block holds, a cumSizes entry past the body and flipped
    payload bytes each raise (or pass) in place exactly as into a separate destination — aligned (fused kernel, then the generic path's report) and at +4 —
    and nothing outside the destination is written."""
    case = U.CASES[0]
    a, b, body_bytes = U.delta_case(case)
    _, nb, P, rot, bm, ch = case
    K = -(-nb // ch); PK = P * K
    cum = lambda body, p, c: int.from_bytes(body[PK + 8 * (p * K + c): PK + 8 * (p * K + c) + 8], "little")
    damaged = []
    d = bytearray(body_bytes)                                     # plane 1 of chunk 0: a jump table beyond the block
    blk = 9 * PK + cum(d, 0, K - 1)
    assert d[blk] < 128
    hs = 1 + d[blk]
    d[blk + hs: blk + hs + 2] = (0xFFFF).to_bytes(2, "little")
    damaged.append(bytes(d))
    d = bytearray(body_bytes)                                     # plane 0 of the partial chunk claims more bytes than the body has
    d[PK + 8 * (K - 1): PK + 8 * K] = (len(d) * 2).to_bytes(8, "little")
    damaged.append(bytes(d))
    d = bytearray(body_bytes)                                     # a type byte that is no type
    d[1] = 7
    damaged.append(bytes(d))
    r = np.random.default_rng(3)
    for _ in range(3):                                            # flipped payload bytes
        d = bytearray(body_bytes)
        for pos in r.integers(9 * PK, len(d), 8):
            d[int(pos)] ^= int(r.integers(1, 256))
        damaged.append(bytes(d))
    n_raised = 0
    for off in (0, 4):
        for db in damaged:
            body = U.to_dev(db, DEV)
            verdicts = []
            for inplace in (False, True):
                buf, dst = U.place(b, off, DEV)
                _, base = (buf, dst) if inplace else U.place(b, off, DEV)
                try:
                    simt_lib.decompress_dev(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, dst.data_ptr(), 0, True, delta_ptr=base.data_ptr())
                    verdicts.append("ok")
                except (RuntimeError, MemoryError) as e:              # (a bad type byte raises MemoryError, as the reference does)
                    verdicts.append(str(e))
                assert U.guards_ok(buf, dst)
            assert verdicts[0] == verdicts[1], (off, verdicts)
            n_raised += verdicts[1] != "ok"
    assert n_raised >= 6                                           # (the three structural damages, at both alignments, at the least)
