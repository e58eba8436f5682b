"""Shared by tests/test_bigchunk_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_bigchunk.py (hardware): compression chunks
above 256 KiB — 512 KiB .. 4 MiB, and the limit of 2 GiB — through every entry point of include/zipnn_hip.h and of the Python layer.

Above 256 KiB the geometry changes: a full chunk's plane of a two-plane tensor is longer than huff0's 128 KiB block from 512 KiB up (every plane stored raw), a
four-plane tensor's planes are exactly 128 KiB at 512 KiB (the largest block there is) and raw from 1 MiB up, and only a PARTIAL last chunk can have a plane
of 131071 / 131072 / 131073 bytes beside others.  Inputs: test_oracle.gen_bytes / test_kernels_simt._gen2.  Expected frames: the CPU oracle's
(oracle_lib.compress_frame) and, where oracle/_ref is built, the reference core's.  Expected decodes: the input bytes."""
import functools
import hashlib
import json
import os

import numpy as np
import torch

import delta_inplace_util as U
import golden_util as G
import hint_layout as HL
import oracle_lib as O
from test_kernels_simt import _gen2, _tail_planes_expected

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = bytes(range(32))
KB = 1024
HUF_MAX = 128 * KB                      # huff0's largest block: a longer plane is stored raw
SEED = 13
GUARD = 64
FILL = 0x5A
FORMATS = {"bf16": (2, 1, 10), "fp16": (2, 0, 10), "fp32": (4, 1, 220)}           # name -> (planes, bits_mode, bytes_mode)
KINDS = ("natural", "skew", "u11", "const", "rand")                               # natural: the format's own weights-like values
TAIL = 300 * KB + 308                   # the partial last chunk of the ladder: whole fp32 elements, not a multiple of 16
REF_CHUNK_LIMIT = 1 << 32               # the reference core takes the chunk size as a C int: it wraps at 2^32 and crashes the process at 2^36

# a case is the tuple of tests/delta_inplace_util.py: (kind, bytes, planes, bits_mode, bytes_mode, chunk)


def case_id(c):
    kind, nb, P, rot, bm, ch = c
    return f"{kind}-P{P}r{rot}-c{ch // KB}K-{nb}"


def ladder(exponents):
    """-> [(id, [case, case])]: per chunk 1 << e, format and kind, one full chunk and two full chunks + TAIL."""
    out = []
    for e in exponents:
        ch = 1 << e
        for fmt, (P, rot, bm) in FORMATS.items():
            for kind in KINDS:
                k = fmt if kind == "natural" else kind
                out.append((f"{fmt}-{kind}-2^{e}", [(k, ch, P, rot, bm, ch), (k, 2 * ch + TAIL, P, rot, bm, ch)]))
    return out


# a partial last chunk whose planes straddle huff0's block limit, behind zero or one full chunk
BOUNDARY_GEOMS = [("bf16", 2, 1, 10, 1 << 20), ("fp32", 4, 1, 220, 1 << 20), ("skew", 2, 1, 10, 1 << 19), ("skew", 4, 1, 220, 1 << 21)]
BOUNDARY_PLANES = (HUF_MAX - 1, HUF_MAX, HUF_MAX + 1)
BOUNDARY = [(f"{kind}-P{P}-c{ch // KB}K-full{full}-plane{pl}", (kind, full * ch + P * pl, P, rot, bm, ch), pl)
            for kind, P, rot, bm, ch in BOUNDARY_GEOMS for pl in BOUNDARY_PLANES for full in (0, 1)]

# fp32 at 512 KiB: four planes of exactly 128 KiB
MAXBLOCK = [(f"{kind}-{nb}", (kind, nb, 4, 1, 220, 1 << 19)) for kind in ("skew", "u11") for nb in (2 << 19, (2 << 19) + 308)]

# tensor ^ base of these goes through tests/delta_inplace_util.check_entry_points (the burst16 case of more_case is the one 2 * C case that file had)
DELTA = [("bf16", 2 * (1 << 20) + TAIL, 2, 1, 10, 1 << 20), ("fp32", 2 * (1 << 19) + 308, 4, 1, 220, 1 << 19), ("fp16", 2 << 19, 2, 0, 10, 1 << 19),
         ("fp32", (1 << 21) + 4 * HUF_MAX, 4, 1, 220, 1 << 21), ("bf16", (1 << 19) + 2 * (HUF_MAX + 1), 2, 1, 10, 1 << 19)]


@functools.lru_cache(maxsize=4)
def data(case):
    return _gen2(case[0], case[1], SEED)


@functools.lru_cache(maxsize=4)
def frame(case, threshold=0.95):
    """The oracle's frame of the case's data behind HDR."""
    kind, nb, P, rot, bm, ch = case
    return O.compress_frame(HDR, data(case), P, rot, bm, ch, threshold=threshold, threads=4)


def ref_frame(header, d, P, rot, bm, ch, threshold=0.95):
    """The reference core's frame (one thread).  Never above a chunk of 2^32 - 1: the core's `int origChunkSize` wraps there and segfaults further up."""
    assert ch < REF_CHUNK_LIMIT, "the reference core must not be handed a chunk of 2^32 or more"
    return O.ref_compress_frame(header, d, P, rot, bm, ch, threshold=threshold, threads=1)


def tables(case, fr=None):
    """-> (types u8[P][K], compressed sizes [P][K]) of the oracle's frame."""
    kind, nb, P, rot, bm, ch = case
    K = -(-nb // ch)
    t, cs, _ = HL.body_tables((fr or frame(case))[32:], P, K)
    return t, cs


def plane_lens(case, c):
    """Plane lengths of chunk c (the split rule: the first bytes % P planes get one byte more)."""
    kind, nb, P, rot, bm, ch = case
    t = min(ch, nb - c * ch)
    return [t // P + (1 if p < t % P else 0) for p in range(P)]


def huffman_coded(case, p, c):
    """Is plane p of chunk c a huff0 block (not raw, not RLE) in the oracle's frame?"""
    t, cs = tables(case)
    return int(t[p, c]) == 1 and 1 < int(cs[p, c]) < plane_lens(case, c)[p]


def tail_planes(case):
    return _tail_planes_expected([case], [frame(case)[32:]])


def boundary_precondition(case, plane):
    """Asserted on the ORACLE's frame before any kernel runs: with `skew` the last chunk's planes are all huff0 blocks at 131071 and 131072 bytes and all raw
    at 131073.  A case that stops meeting this has stopped testing the boundary."""
    kind, nb, P, rot, bm, ch = case
    K = -(-nb // ch)
    assert plane_lens(case, K - 1) == [plane] * P
    t, cs = tables(case)
    last = [int(x) for x in t[:, K - 1]]
    if kind == "skew":
        assert last == ([1] * P if plane <= HUF_MAX else [0] * P), (case, last)
        if plane <= HUF_MAX:
            assert all(huffman_coded(case, p, K - 1) for p in range(P))
    elif plane > HUF_MAX:
        assert last == [0] * P, (case, last)           # (weights-like values: no plane above the block limit is coded either)


def maxblock_precondition(case):
    """skew: all four 128 KiB planes of every full chunk are huff0 blocks; u11: planes 1 and 3 are."""
    kind, nb, P, rot, bm, ch = case
    assert ch // P == HUF_MAX
    for c in range(nb // ch):
        for p in (range(4) if kind == "skew" else (1, 3)):
            assert huffman_coded(case, p, c), (case, p, c)


# ---- buffers ----
def placed(data_or_n, off, dev):
    """-> (buffer of 0x5A, view whose address is `off` modulo 16): holding `data_or_n` (bytes), or that many bytes of 0x5A."""
    n = data_or_n if isinstance(data_or_n, int) else len(data_or_n)
    buf = torch.full((GUARD + 16 + n + GUARD,), FILL, dtype=torch.uint8, device=dev)
    s = GUARD + (off - (buf.data_ptr() + GUARD)) % 16
    v = buf[s:s + n]
    if not isinstance(data_or_n, int):
        v.copy_(torch.frombuffer(bytearray(data_or_n), dtype=torch.uint8))
    assert v.data_ptr() % 16 == off
    return buf, v


def guards_ok(buf, v):
    s = v.data_ptr() - buf.data_ptr()
    return bool((buf[:s] == FILL).all()) and bool((buf[s + v.numel():] == FILL).all())


def _diff(got, want):
    if len(got) != len(want):
        return ("length", len(got), len(want))
    x = np.flatnonzero(np.frombuffer(got, dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8))
    return ("bytes differ", int(x.size), "first at", int(x[0]) if x.size else None)


def same(got, want, *what):
    got, want = bytes(got), bytes(want)
    assert got == want, what + _diff(got, want)


# ---- encode ----
ENCODE_FORMS = ("host", "batch", "legacy")


def check_encode(lib, dev, case, forms=ENCODE_FORMS):
    """The frame equals the oracle's: zn_compress from host memory; zn_compress_batch_dev (codec.compress_device_batch) with the one-pass encoder off and
    forced; the legacy tree descriptions against the oracle's legacy mode."""
    from zipnn_amd import codec
    kind, nb, P, rot, bm, ch = case
    d, want = data(case), frame(case)
    if "host" in forms:
        same(lib.compress(HDR, d, P, rot, bm, ch, 0.95), want, "zn_compress", case, lib.last_kernels())
    if "batch" in forms:
        src = U.to_dev(d, dev)
        for mode in (0, 2):
            lib.set_encode_onepass(mode)
            try:
                bodies = codec.compress_device_batch(lib, [(src, P, rot, bm, ch, 0.95)])
                ks = lib.last_kernels()
            finally:
                lib.set_encode_onepass(1)
            same(U.got(bodies[0]), want[32:], "zn_compress_batch_dev, onepass", mode, case, ks)
    if "legacy" in forms:
        with O.legacy_weights():
            legacy = O.compress_frame(HDR, d, P, rot, bm, ch, threads=4)
        lib.set_legacy_tree_descriptions(True)
        try:
            got = bytes(lib.compress(HDR, d, P, rot, bm, ch, 0.95))
        finally:
            lib.set_legacy_tree_descriptions(False)
        same(got, legacy, "legacy tree descriptions", case)
        same(lib.decompress(legacy[32:], P, rot, bm, ch, nb), d, "decode of the legacy frame", case)


def check_reference_core(cases):
    """The oracle's frame is the reference core's (one thread), for every case."""
    for case in cases:
        kind, nb, P, rot, bm, ch = case
        same(ref_frame(HDR, data(case), P, rot, bm, ch), frame(case), "reference core", case)


def check_thresholds(lib, case):
    kind, nb, P, rot, bm, ch = case
    for th in (0.5, 1.0):
        want = O.compress_frame(HDR, data(case), P, rot, bm, ch, threshold=th, threads=4)
        same(lib.compress(HDR, data(case), P, rot, bm, ch, th), want, "threshold", th, case)
        same(lib.decompress(want[32:], P, rot, bm, ch, nb), data(case), "decode at threshold", th, case)


@functools.lru_cache(maxsize=2)
def delta_case(case):
    """tests/delta_inplace_util.delta_case without its unbounded cache: (tensor, base, body of tensor ^ base)."""
    return U.delta_case.__wrapped__(case)


def check_delta_compress(lib, dev, case):
    """zn_compress_delta and a batched item with a base: the oracle's frame of a ^ b."""
    from zipnn_amd import codec
    kind, nb, P, rot, bm, ch = case
    a, b, body = delta_case(case)
    same(lib.compress(HDR, a, P, rot, bm, ch, 0.95, delta=b)[32:], body, "zn_compress_delta", case, lib.last_kernels())
    bodies = codec.compress_device_batch(lib, [(U.to_dev(a, dev), P, rot, bm, ch, 0.95, U.to_dev(b, dev))])
    same(U.got(bodies[0]), body, "zn_compress_batch_dev with a base", case, lib.last_kernels())
    same(lib.decompress(body, P, rot, bm, ch, nb, delta=b), a, "zn_decompress_delta", case)


# ---- decode ----
DECODE_FORMS = ("host", "dev", "batch", "windows", "plan", "hinted", "unaligned", "multi", "merge")


def check_decode(lib, dev, case, forms=DECODE_FORMS, hint_counters=None):
    """The oracle's body decodes to the input through every form; the read-outs say which kernels took it."""
    kind, nb, P, rot, bm, ch = case
    d, body_b = data(case), frame(case)[32:]
    K = -(-nb // ch)
    st = U.stream_of(dev)
    body = U.to_dev(body_b, dev)
    win = lambda lo, hi, dst, b=body: (b.data_ptr(), b.numel(), P, rot, bm, ch, nb, lo, hi, dst)          # noqa: E731
    if "host" in forms:
        same(lib.decompress(body_b, P, rot, bm, ch, nb), d, "zn_decompress", case, lib.last_kernels())
    if "dev" in forms:
        buf, dst = placed(nb, 0, dev)
        lib.decompress_dev(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, dst.data_ptr(), st, True)
        same(U.got(dst), d, "zn_decompress_dev", case, lib.last_kernels())
        assert guards_ok(buf, dst)
        # every full chunk by the single-pass kernels (whole rows per stream, a 16-byte aligned destination: every power of two from 4 KiB up qualifies) …
        assert lib.last_fused_chunks() == nb // ch, (case, lib.last_kernels())
        # … and the partial chunk's huff0 planes of 512 .. 131072 bytes by the tail workgroups
        assert lib.last_tail_planes() == tail_planes(case), (case, lib.last_kernels())
    if "batch" in forms:
        b1, d1 = placed(nb, 0, dev)
        b2, d2 = placed(nb, 0, dev)
        lib.decompress_batch_dev([(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, d1.data_ptr()), (body.data_ptr(), body.numel(), P, rot, bm, ch, nb, d2.data_ptr())], st, True)
        same(U.got(d1), d, "zn_decompress_batch_dev, item 0", case)
        same(U.got(d2), d, "zn_decompress_batch_dev, item 1", case)
        assert guards_ok(b1, d1) and guards_ok(b2, d2)
        assert lib.last_fused_chunks() == 2 * (nb // ch) and lib.last_tail_planes() == 2 * tail_planes(case), (case, lib.last_kernels())
    if "windows" in forms:
        for lo, hi in U.windows(K):
            want = d[lo * ch:min(hi * ch, nb)]
            buf, dst = placed(len(want), 0, dev)
            lib.decompress_window_batch_dev([win(lo, hi, dst.data_ptr())], st, True)
            same(U.got(dst), want, "window", lo, hi, case, lib.last_kernels())
            assert guards_ok(buf, dst)
    if "plan" in forms:
        buf, dst = placed(nb, 0, dev)
        h = lib.plan_create([win(0, K, dst.data_ptr())])
        try:
            for run in range(2):
                dst.fill_(FILL)
                lib.plan_run(h, st, True)
                same(U.got(dst), d, "plan, run", run, case)
        finally:
            lib.plan_destroy(h)
        assert guards_ok(buf, dst)
    if "hinted" in forms:
        check_hinted(lib, dev, case, hint_counters)
    if "unaligned" in forms:
        # the body at an odd address, the destination at +4: the fused kernel takes none of it
        _, ubody = placed(body_b, 1, dev)
        buf, dst = placed(nb, 4, dev)
        lib.decompress_dev(ubody.data_ptr(), ubody.numel(), P, rot, bm, ch, nb, dst.data_ptr(), st, True)
        same(U.got(dst), d, "body at +1, destination at +4", case, lib.last_kernels())
        assert guards_ok(buf, dst)
        assert lib.last_fused_chunks() == 0, (case, lib.last_kernels())
    if "multi" in forms:
        rng = [lib.multi_range(nb, ch, 3, i) for i in range(3)]
        assert sum(ln for _, ln in rng) == nb
        outs = [placed(max(ln, 1), 0, dev) for _, ln in rng]
        lib.decompress_multi_dev(body_b, P, rot, bm, ch, nb, [0, 0, 0], [v.data_ptr() if ln else 0 for (_, v), (_, ln) in zip(outs, rng)])
        for (buf, v), (off, ln) in zip(outs, rng):
            same(U.got(v)[:ln], d[off:off + ln], "zn_decompress_multi_dev, range at", off, case)
            assert ln == 0 or guards_ok(buf, v)
        for lo, hi in U.windows(K):
            want = d[lo * ch:min(hi * ch, nb)]
            buf, dst = placed(len(want), 0, dev)
            lib.decompress_range_dev(body_b, P, rot, bm, ch, nb, lo, hi, 0, dst.data_ptr())
            same(U.got(dst), want, "zn_decompress_range_dev", lo, hi, case)
            assert guards_ok(buf, dst)
    if "merge" in forms:
        # the bodies of the three ranges, each coded on its own by the oracle, merge into the whole tensor's body
        rng = [lib.multi_range(nb, ch, 3, i) for i in range(3)]
        parts = [(O.compress_frame(b"", d[off:off + ln], P, rot, bm, ch, threads=4), -(-ln // ch)) for off, ln in rng]
        same(lib.merge_range_bodies(parts, P), body_b, "zn_merge_range_bodies", case)


def check_hinted(lib, dev, case, hint_counters=None, expect=None):
    """zn_hint_size_dev / zn_hint_build_dev, then a hinted batch and a hinted plan run twice.  The index is as long as tests/hint_layout.py says from the body's
    own tables; expect = "table": nothing but the offset table, "more": hint regions behind it.  hint_counters (the emulated build's): no hinted tile
    needed a fix-up."""
    kind, nb, P, rot, bm, ch = case
    d, body_b = data(case), frame(case)[32:]
    K = -(-nb // ch)
    st = U.stream_of(dev)
    body = U.to_dev(body_b, dev)
    item = (body.data_ptr(), body.numel(), P, rot, bm, ch, nb, 0, K, 0)
    lib.set_decode_wide(0)                  # (the small-input kernel reads no hints)
    try:
        n = lib.hint_size_dev(item, st)
        offs, table = HL.expected_table(body_b, P, ch, nb)
        assert n == int(offs[-1]), (case, n, int(offs[-1]))
        if expect == "table":
            assert n == table, (case, n, table)
        if expect == "more":
            assert n > table, (case, n, table)
        hbuf = torch.full((n + 16 + GUARD,), FILL, dtype=torch.uint8, device=dev)
        s = (-hbuf.data_ptr()) % 16
        h = hbuf[s:s + n]
        lib.hint_build_dev(item, h.data_ptr(), n, st)
        assert bool((hbuf[s + n:] == FILL).all()) and bool((hbuf[:s] == FILL).all())
        assert np.array_equal(np.frombuffer(U.got(h[:4 * (P * K + 1)]), dtype="<u4"), offs), case
        buf, dst = placed(nb, 0, dev)
        hitem = (item[:9] + (dst.data_ptr(),), h.data_ptr(), n)
        if hint_counters:
            hint_counters()
        lib.decompress_hinted_batch_dev([hitem], st, True)
        same(U.got(dst), d, "zn_decompress_hinted_batch_dev", case, lib.last_kernels())
        if hint_counters:
            hc = hint_counters()
            assert hc[1] == 0, (case, hc)
            assert (hc[0] > 0) == (n > table), (case, hc)
        plan = lib.plan_create_hinted([hitem])
        try:
            for run in range(2):
                dst.fill_(FILL)
                lib.plan_run(plan, st, True)
                same(U.got(dst), d, "hinted plan, run", run, case)
        finally:
            lib.plan_destroy(plan)
        assert guards_ok(buf, dst)
        if hint_counters:
            assert hint_counters()[1] == 0
    finally:
        lib.set_decode_wide(1)


def check_groups_and_wide(lib, dev, case, decode_group):
    """zn_set_decode_group 1 .. 4 (the fused kernel pinned) and zn_set_decode_wide 0, 2, 3."""
    kind, nb, P, rot, bm, ch = case
    d, body_b = data(case), frame(case)[32:]
    st = U.stream_of(dev)
    body = U.to_dev(body_b, dev)
    buf, dst = placed(nb, 0, dev)
    try:
        lib.set_decode_wide(0)
        for g in (1, 2, 3, 4):
            decode_group(lib, g)
            dst.fill_(FILL)
            lib.decompress_dev(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, dst.data_ptr(), st, True)
            same(U.got(dst), d, "decode group", g, case, lib.last_kernels())
            assert lib.last_fused_chunks() == nb // ch and lib.last_tail_planes() == tail_planes(case), (g, case, lib.last_kernels())
        decode_group(lib, 0)
        for mode in (0, 2, 3):
            lib.set_decode_wide(mode)
            dst.fill_(FILL)
            lib.decompress_dev(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, dst.data_ptr(), st, True)
            same(U.got(dst), d, "zn_set_decode_wide", mode, case, lib.last_kernels())
            assert lib.last_tail_planes() == tail_planes(case), (mode, case, lib.last_kernels())
    finally:
        lib.set_decode_wide(1)
    assert guards_ok(buf, dst)


# ---- the Python layer (zipnn_amd.ZipNN, the file loaders, resident stores) ----
def _tbytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def check_zipnn_api():
    """ZipNN(compression_chunk=1 << e) on bytes and on tensors: header byte 14 is e, the frame is the oracle's behind that header, and a default-constructed
    ZipNN decodes it."""
    from zipnn_amd import ZipNN
    for e, fmt in ((19, "fp32"), (20, "bf16"), (21, "fp16")):
        P, rot, bm = FORMATS[fmt]
        ch = 1 << e
        tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[fmt]
        raw = _gen2(fmt, 2 * ch + 308008, SEED + e)
        f = bytes(ZipNN(bytearray_dtype=str(tdt).replace("torch.", ""), compression_chunk=ch).compress(raw))
        assert f[14] == e
        same(f, O.compress_frame(f[:32], raw, P, rot, bm, ch, threads=4), "ZipNN on bytes", fmt, e)
        same(ZipNN().decompress(f), raw, "ZipNN() decodes it", fmt, e)
        t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(tdt).reshape(-1, 2)
        f = bytes(ZipNN(input_format="torch", compression_chunk=ch).compress(t.clone()))
        p = G.parse_frame(f)
        assert f[14] == e and p["chunk"] == ch and p["num_buf"] == P
        same(f, O.compress_frame(p["header"], raw, P, p["bits_mode"], p["bytes_mode"], ch, threads=4), "ZipNN on a tensor", fmt, e)
        back = ZipNN(input_format="torch").decompress(f)
        assert back.dtype == tdt and back.shape == t.shape
        same(_tbytes(back), raw, "ZipNN(torch) decodes it", fmt, e)


def check_streaming():
    """streaming_chunk 1 MiB below compression_chunk 2 MiB: every piece is one partial chunk; with and without the byte delta."""
    from zipnn_amd import ZipNN
    raw = _gen2("bf16", 3 * (1 << 20) + 12346, 7)
    a, b = U.delta_case.__wrapped__(("bf16", len(raw), 2, 1, 10, 1 << 21))[:2]
    for delta in (False, True):
        kw = dict(bytearray_dtype="bfloat16", compression_chunk=1 << 21, is_streaming=True, streaming_chunk=1 << 20)
        if delta:
            kw["delta_compressed_type"] = "byte"
        src = a if delta else raw
        extra = dict(delta_second_data=b) if delta else {}
        blob = bytes(ZipNN(**kw).compress(src, **extra))
        frames = G.split_frames(blob)
        assert len(frames) == 4
        coded = U.xor(a, b) if delta else raw
        for i, fr in enumerate(frames):
            p = G.parse_frame(fr)
            assert fr[14] == 21 and p["chunk"] == 1 << 21 and p["orig_len"] <= 1 << 20
            same(fr, O.compress_frame(p["header"], coded[i << 20:(i + 1) << 20], 2, 1, 10, 1 << 21), "streaming piece", i, delta)
        same(ZipNN(**kw).decompress(blob, **extra), src, "streaming round trip", delta)


def check_fp8():
    """fp8 with compression_chunk 1 MiB: the header says 20, the coder uses 128 KiB."""
    from zipnn_amd import ZipNN
    raw = (torch.randn(3 * HUF_MAX + 4321, generator=torch.Generator().manual_seed(5)) * 0.05).to(torch.float8_e4m3fn).view(torch.uint8).numpy().tobytes()
    f = bytes(ZipNN(bytearray_dtype="float8_e4m3fn", compression_chunk=1 << 20).compress(raw))
    assert f[14] == 20
    p = G.parse_frame(f)
    assert p["chunk"] == HUF_MAX and p["num_buf"] == 1
    same(f, O.compress_frame(f[:32], raw, 1, p["bits_mode"], p["bytes_mode"], HUF_MAX), "fp8 frame at 128 KiB")
    same(ZipNN().decompress(f), raw, "fp8 round trip")


def bigchunk_state():
    """A small state dict whose tensors span 1 MiB chunk boundaries: bf16 [1500, 768] (2.2 chunks), fp32 [600, 500] (1.1 chunks), fp16 [600, 1024] (1.2 chunks),
    fp16 [512, 1024] (exactly one chunk: both planes raw, the frame is longer than the tensor and the file keeps the tensor as it is, as the reference's
    producer does), an fp8 tensor and an integer one."""
    g = torch.Generator().manual_seed(41)
    rn = lambda *s: torch.randn(*s, generator=g) * 0.02                    # noqa: E731
    return {"w.bf16": rn(1500, 768).to(torch.bfloat16), "w.fp32": rn(600, 500), "w.fp16": rn(600, 1024).to(torch.float16),
            "w.fp16.raw": rn(512, 1024).to(torch.float16),
            "w.fp8": (rn(300, 1000) * 25).to(torch.float8_e4m3fn), "ids": torch.arange(100, dtype=torch.int64)}


def write_bigchunk_file(path, sd, chunk=1 << 20):
    """A `.znn.safetensors` file whose frames use `chunk` — the layout of safetensors_io.compress_safetensors_file (which takes no chunk argument), with
    digests of the source tensors."""
    from safetensors.torch import save_file
    from zipnn_amd import ZipNN, codec, safetensors_io
    from zipnn_amd.zipnn import COMPRESSED_DTYPE, build_compressed_tensor_info, set_compressed_tensors_metadata
    tensors, infos = {}, {}
    for name, t in sd.items():
        if not torch.is_floating_point(t):
            tensors[name] = t
            continue
        fr = bytes(ZipNN(input_format="torch", bytearray_dtype=t.dtype, compression_chunk=chunk).compress(t.clone()))
        assert fr[14] == chunk.bit_length() - 1
        if len(fr) >= t.numel() * t.element_size():
            tensors[name] = t
            continue
        tensors[name] = torch.frombuffer(bytearray(fr), dtype=COMPRESSED_DTYPE)
        infos[name] = build_compressed_tensor_info(t)
    metadata = {"format": "pt"}
    set_compressed_tensors_metadata(infos, metadata)
    names = list(sd.keys())
    assert sorted(infos) == ["w.bf16", "w.fp16", "w.fp32", "w.fp8"], sorted(infos)
    safetensors_io._set_digests_metadata(metadata, names, codec.digest_many([sd[n] for n in names]))
    save_file(tensors, path, metadata)
    return path


def check_file(tmp_path, dev):
    """load_file(verify=True), the plugin's get_tensor / get_slice, a resident store with index, digests and verify, and a variant store over it."""
    from zipnn_amd import ResidentCheckpoint, safetensors_io
    from zipnn_amd import zipnn as Z
    import resident_delta_util as R
    sd = bigchunk_state()
    path = write_bigchunk_file(os.path.join(str(tmp_path), "big.znn.safetensors"), sd)
    MB = 1 << 20
    loaded = safetensors_io.load_file(path, device=dev, verify=True)
    for n, t in sd.items():
        assert R._bytes_equal(loaded[n], t), n
    # bf16 [1500, 768]: 1536 bytes a row; row 682 straddles the first chunk boundary (682 * 1536 < 1 MiB < 683 * 1536), rows 1366 .. are the partial last chunk
    rows = {"w.bf16": [(slice(680, 690), (0, 2)), (slice(1400, 1450), (2, 3))], "w.fp32": [(slice(520, 530), (0, 2)), (slice(560, 600), (1, 2))]}
    assert 682 * 1536 < MB < 683 * 1536 and 1400 * 1536 > 2 * MB and 520 * 2000 < MB < 530 * 2000 and 560 * 2000 > MB
    with Z.SafeOpen(path, framework="pt", device=str(dev)) as f:
        for n, t in sd.items():
            assert R._bytes_equal(f.get_tensor(n), t), n
        for n, cases in rows.items():
            s = f.get_slice(n)
            for idx, crange in cases:
                assert R._bytes_equal(s[idx], sd[n][idx]), (n, idx)
                assert s.last_chunk_range == crange, (n, idx, s.last_chunk_range)
    store = ResidentCheckpoint.from_file(path, dev, index=True, digests=True, verify=True)
    assert store.has_digests and all(store.verify().values())
    for n, t in sd.items():
        assert R._bytes_equal(store.get_tensor(n), t), n
    for n, cases in rows.items():
        s = store.get_slice(n)
        for idx, crange in cases:
            assert R._bytes_equal(s[idx], sd[n][idx]), (n, idx)
            assert s.last_chunk_range == crange, (n, idx, s.last_chunk_range)
    # at 1 MiB the two-plane tensors' full chunks are all raw (no hint regions); the fp32 tensor's planes are 256 KiB: raw as well
    for n in ("w.bf16", "w.fp16", "w.fp32"):
        i = store.info(n)
        P = 4 if n == "w.fp32" else 2
        assert i["index_bytes"] == (HL.header_bytes(P, -(-i["nbytes"] // MB)) if n == "w.bf16" or i["index_bytes"] else 0), (n, i)      # (build_index leaves some dtypes out)
    # a variant store over it
    sd = {n: sd[n] for n in ("w.fp32", "w.fp16.raw", "w.fp8", "ids")}           # (the emulator re-codes every tensor of the variant twice: four of the six are enough)
    ft_sd = {n: (R._perturb(t, 0.03, 200 + k) if torch.is_floating_point(t) else t + 1) for k, (n, t) in enumerate(sd.items())}
    ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=store)
    for n, t in ft_sd.items():
        assert R._bytes_equal(ft.get_tensor(n), t), n
    # (a delta body is coded over a base entry with the SAME frame parameters, from_state_dict's rule: the store codes at 256 KiB, so a tensor the file holds
    #  in 1 MiB chunks stays a plain body; the fp8 one — 128 KiB on both sides — and the one the file keeps uncompressed are deltas.  apply_ / revert_ go through
    #  the base's 1 MiB bodies either way)
    assert [ft.info(n)["delta"] for n in ("w.fp32", "w.fp16.raw", "w.fp8")] == [False, True, True]
    live = {n: t.to(dev).clone() for n, t in sd.items()}
    assert sorted(ft.apply_(live)) == sorted(sd)
    for n, t in ft_sd.items():
        assert R._bytes_equal(live[n], t), n
    assert ft.revert_(live) == []
    for n, t in sd.items():
        assert R._bytes_equal(live[n], t), n


# ---- limits ----
def check_chunk_2_31(lib, dev):
    """Chunk 1 << 31, the largest there is: a 300 000-byte bf16 tensor is one partial chunk."""
    from zipnn_amd import ZipNN
    ch = 1 << 31
    d = _gen2("bf16", 300000, 7)
    want = O.compress_frame(HDR, d, 2, 1, 10, ch)
    same(lib.compress(HDR, d, 2, 1, 10, ch, 0.95), want, "zn_compress at 1 << 31")
    same(lib.decompress(want[32:], 2, 1, 10, ch, len(d)), d, "zn_decompress at 1 << 31")
    body = U.to_dev(want[32:], dev)
    buf, dst = placed(len(d), 0, dev)
    lib.decompress_dev(body.data_ptr(), body.numel(), 2, 1, 10, ch, len(d), dst.data_ptr(), U.stream_of(dev), True)
    same(U.got(dst), d, "zn_decompress_dev at 1 << 31")
    assert guards_ok(buf, dst) and lib.last_fused_chunks() == 0
    f = bytes(ZipNN(bytearray_dtype="bfloat16", compression_chunk=ch).compress(d))
    assert f[14] == 31
    same(f, O.compress_frame(f[:32], d, 2, 1, 10, ch), "ZipNN at 1 << 31")
    same(ZipNN().decompress(f), d, "ZipNN round trip at 1 << 31")
    L = lib._L
    import ctypes
    L.zn_num_chunks.restype = ctypes.c_size_t
    L.zn_num_chunks.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    for n in (0, 1, 300000, ch - 1, ch, ch + 1, 5 * ch + 7):
        K = -(-n // ch)
        assert L.zn_num_chunks(n, ch) == K
        for P in (1, 2, 4):
            assert lib.compress_bound(n, P, ch, 32) == 32 + 9 * P * K + n


def check_chunk_2_32_is_refused(lib, dev):
    """Chunk 1 << 32: ZN_E_ARG (ValueError) from compress, decompress, window, plan-create and hint-size, with nothing launched."""
    import pytest
    ch = 1 << 32
    d = _gen2("bf16", 300000, 7)
    good = O.compress_frame(HDR, d, 2, 1, 10, 1 << 31)[32:]
    body = U.to_dev(good, dev)
    buf, dst = placed(len(d), 0, dev)
    lib.decompress_dev(body.data_ptr(), body.numel(), 2, 1, 10, 1 << 31, len(d), dst.data_ptr(), U.stream_of(dev), True)
    before = lib.last_kernels()
    assert before
    item = (body.data_ptr(), body.numel(), 2, 1, 10, ch, len(d), 0, 1, dst.data_ptr())
    calls = [lambda: lib.compress(HDR, d, 2, 1, 10, ch, 0.95), lambda: lib.decompress(good, 2, 1, 10, ch, len(d)),
             lambda: lib.decompress_dev(body.data_ptr(), body.numel(), 2, 1, 10, ch, len(d), dst.data_ptr(), U.stream_of(dev), True),
             lambda: lib.compress_dev(dst.data_ptr(), len(d), 2, 1, 10, ch, 0.95, body.data_ptr(), body.numel()),
             lambda: lib.decompress_window_batch_dev([item], U.stream_of(dev), True), lambda: lib.plan_create([item]), lambda: lib.hint_size_dev(item, U.stream_of(dev))]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert lib.last_kernels() in (before, ""), (i, lib.last_kernels())
    same(U.got(dst), d, "the destination after the refused calls")
    assert guards_ok(buf, dst)


def check_header_exponent_41_is_refused():
    import pytest
    from zipnn_amd import ZipNN
    from zipnn_amd.zipnn import fast_frame_params
    f = bytearray(ZipNN(bytearray_dtype="bfloat16").compress(_gen2("bf16", 1000, 1)))
    assert fast_frame_params(memoryview(bytes(f)))[4] == 256 * KB
    f[14] = 40
    assert fast_frame_params(memoryview(bytes(f)))[4] == 1 << 40
    f[14] = 41
    with pytest.raises(ValueError):
        fast_frame_params(memoryview(bytes(f)))


# ---- frames the reference's own Python wrote at big chunks: tests/golden/make_golden_bigchunk.py ----
GOLDEN_PATH = os.path.join(HERE, "golden", "golden_bigchunk_v1.npz")


def golden_input(recipe):
    """-> (bytes of the input, bytes of the delta base or None) from an entry's seeded recipe.  gen: "gen2" = test_kernels_simt._gen2(kind, n, seed),
    "normal_fp32" = N(0, 0.02) float32 from torch's generator; base: the recipe of tests/delta_inplace_util.delta_case (3 % of the bytes perturbed)."""
    if recipe["gen"] == "gen2":
        raw = _gen2(recipe["kind"], recipe["n"], recipe["seed"])
    elif recipe["gen"] == "normal_fp32":
        raw = (torch.randn(recipe["n"] // 4, generator=torch.Generator().manual_seed(recipe["seed"])) * 0.02).numpy().tobytes()
    else:
        raise ValueError(recipe["gen"])
    base = None
    if recipe.get("base_seed") is not None:
        r = np.random.default_rng(recipe["base_seed"])
        b = np.frombuffer(raw, dtype=np.uint8).copy()
        hit = r.random(len(b)) < 0.03
        b[hit] ^= r.integers(1, 256, int(hit.sum()), dtype=np.uint8)
        base = b.tobytes()
    return raw, base


@functools.lru_cache(maxsize=1)
def golden_load():
    z = np.load(GOLDEN_PATH)
    meta = json.loads(bytes(z["meta.json"]).decode())
    return [(m, bytes(z[m["name"] + ".frame"])) for m in meta]


def golden_names():
    return [m["name"] for m, _ in golden_load()]


def check_golden(name):
    """ZipNN(**ctor) decodes the reference-written frame to the recipe's input and re-encodes the input to the same bytes; the oracle agrees frame by frame."""
    from zipnn_amd import ZipNN
    meta, blob = next((m, f) for m, f in golden_load() if m["name"] == name)
    assert G.sha(blob) == meta["frame_sha256"]
    raw, base = golden_input(meta["recipe"])
    assert len(raw) == meta["in_len"] and hashlib.sha256(raw).hexdigest() == meta["in_sha256"]
    ctor = dict(meta["ctor"])
    extra = dict(delta_second_data=base) if base is not None else {}
    coded = U.xor(raw, base) if base is not None else raw
    off = 0
    for fr in G.split_frames(blob):
        p = G.parse_frame(fr)
        assert fr[14] == meta["chunk_exponent"] and p["chunk"] == 1 << meta["chunk_exponent"]
        piece = coded[off:off + p["orig_len"]]
        off += p["orig_len"]
        same(O.decompress_body(p["body"], p["num_buf"], p["bits_mode"], p["bytes_mode"], p["chunk"], p["orig_len"], threads=2), piece, "oracle decode", name)
        same(O.compress_frame(p["header"], piece, p["num_buf"], p["bits_mode"], p["bytes_mode"], p["chunk"], threads=4), fr, "oracle re-encode", name)
    assert off == len(raw)
    back = ZipNN(**ctor).decompress(blob, **extra)
    if meta["kind"] == "torch":
        assert str(back.dtype) == "torch." + meta["dtype"] and list(back.shape) == meta["shape"]
        same(_tbytes(back), raw, "decode", name)
        src = torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(back.dtype).reshape(meta["shape"])
    else:
        same(back, raw, "decode", name)
        src = raw
    same(ZipNN(**ctor).compress(src, **extra), blob, "re-encode", name)
