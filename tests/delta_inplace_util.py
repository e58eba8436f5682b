"""Shared by tests/test_delta_inplace_simt.py (emulated kernels, CPU tensors) and tests/test_gpu_resident_delta.py (hardware): the in-place delta decode
of include/zipnn_hip.h — a destination that IS the delta base — through every entry point, and the inputs that send chunks down every path of the decoder.
Bodies are the CPU oracle's frames of tensor ^ base (one of them re-coded here with a tableLog-12 Huffman plane, checked against the oracle's decoder);
expected outputs are the tensor's bytes."""
import functools

import numpy as np
import torch

import oracle_lib as O
from test_kernels_simt import _delta_pair, _gen2

C = 256 * 1024
GUARD = 64
# (kind, bytes, planes, bits_mode, bytes_mode, chunk): the issue's cases — a tail the tail workgroups take, whole chunks, a tail the serial decoder takes,
# single-plane chunks with a 5-byte tail, two planes without the sign rotate
CASES = [("bf16", 2 * C + 1234, 2, 1, 10, C), ("bf16", 2 * C, 2, 1, 10, C), ("fp32", C + 308, 4, 1, 220, C), ("fp8", 3 * 65536 + 5, 1, 1, 10, 65536),
         ("fp16", 2 * C, 2, 0, 10, C)]
CASE_IDS = [f"{c[0]}-{c[1]}" for c in CASES]
OFFSETS = (0, 4, 1)          # base (= destination) address modulo 16


def xor(a, b):
    return (np.frombuffer(a, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes()


@functools.lru_cache(maxsize=None)
def delta_case(case, seed=31):
    """-> (tensor bytes, base bytes, body of tensor ^ base): the recipe of test_kernels_simt._delta_pair (the base with 3 % of the bytes perturbed)."""
    kind, nb, P, rot, bm, chunk = case
    a, b = _delta_pair(kind, nb, seed)
    return a, b, O.compress_frame(b"", xor(a, b), P, rot, bm, chunk)


@functools.lru_cache(maxsize=None)
def more_case(name):
    """-> (case tuple, tensor, base, body).  identical: every plane RLE zero; unrelated: raw planes; skew / u11 / burst16: the tensor ^ base is one of the hostile
    distributions of tests/test_kernels_simt.py (1-bit codes with every plane Huffman-coded, 11-bit codes, tiles denser than the stream average)."""
    if name == "identical":
        case = ("bf16", 2 * C + 1234, 2, 1, 10, C)
        b = _gen2("bf16", case[1], 3)
        coded = bytes(case[1])
    elif name == "unrelated":
        case = ("bf16", 2 * C + 1234, 2, 1, 10, C)
        b = _gen2("bf16", case[1], 3)
        coded = _gen2("rand", case[1], 4)
    elif name == "skew4":
        case = ("skew", 2 * C, 4, 1, 220, C)
        b = _gen2("fp32", case[1], 3)
        coded = _gen2("skew", case[1], 11)
    else:
        case = {"skew": ("skew", 2 * C, 2, 1, 10, C), "u11": ("u11", 2 * C, 2, 1, 10, C), "burst16": ("burst16", 4 * C, 2, 0, 10, 2 * C)}[name]
        b = _gen2("bf16", case[1], 3)
        coded = _gen2(name, case[1], 11)
    _, nb, P, rot, bm, chunk = case
    return case, xor(coded, b), b, O.compress_frame(b"", coded, P, rot, bm, chunk)


MORE = ["identical", "unrelated", "skew", "skew4", "u11", "burst16"]


# ---- a tableLog-12 Huffman block (huff0 writes at most 11; its decoders take 12): the fused kernel declines such a plane, the serial decoder takes it ----
# a complete code over the byte values 0 .. 12: values 0 .. 10 have lengths 2 .. 12, value 11 length 12 and value 12 — the last one, whose weight the tree
# description leaves out: a written weight is at most 11 — length 1
TL12_LENGTHS = list(range(2, 13)) + [12, 1]


def huf_block_tl12(plane):
    """`plane` (uint8 array over the values 0 .. 12) -> a huff0 block, four streams, whose tree description gives TL12_LENGTHS: raw 4-bit weights
    (header byte 127 + 12), the canonical code HUF_readDTableX1 derives from them (cells by rising weight, by value inside a weight)."""
    tl, n = 12, len(plane)
    weights = [tl + 1 - l for l in TL12_LENGTHS]
    hdr = bytes([127 + 12]) + bytes((weights[2 * i] << 4) | weights[2 * i + 1] for i in range(6))        # the thirteenth weight is implied
    start, code = 0, {}
    for w in range(1, tl + 1):
        for v, wv in enumerate(weights):
            if wv == w:
                code[v] = format(start >> (w - 1), "0%db" % (tl + 1 - w))
                start += 1 << (w - 1)
    assert start == 1 << tl
    seg = (n + 3) // 4
    streams = []
    for q in range(4):
        part = plane[q * seg: min((q + 1) * seg, n)]
        bits = "1" + "".join(code[int(v)] for v in part)          # (read from the top: the end mark, then the symbols in order)
        streams.append(int(bits, 2).to_bytes((len(bits) + 7) // 8, "little"))
    assert all(len(s) < 65536 for s in streams[:3])
    return hdr + b"".join(len(s).to_bytes(2, "little") for s in streams[:3]) + b"".join(streams)


def _unrotate(rotated, P):
    """chunk bytes in the rotated domain -> the bytes the frame decodes to (the decoder's rot_inv on every whole 32-bit word)."""
    u = np.frombuffer(rotated, dtype="<u4").astype(np.uint32)
    if P == 2:
        u = ((u << 8) & 0x80008000) | ((u >> 1) & 0x7F807F80) | (u & 0x007F007F)
    else:
        u = ((u << 8) & 0x80000000) | ((u >> 1) & 0x7F800000) | (u & 0x007FFFFF)
    return u.astype("<u4").tobytes()


@functools.lru_cache(maxsize=None)
def tl12_case(P):
    """-> (case tuple, tensor, base, body): two full chunks of P planes with the sign rotate, every plane Huffman-coded.  Chunk 0: the LAST plane has
    tableLog 12 — the fused kernel has decoded the planes before it when it finds out; chunk 1: the FIRST plane has — the fused kernel takes nothing.
    Checked against the oracle's decoder before anything is asked of the kernels."""
    chunk, K = C, 2
    rng = np.random.default_rng(12 + P)
    plen = chunk // P
    counts12 = [plen >> l for l in TL12_LENGTHS]
    assert sum(counts12) == plen
    blocks = [[None] * K for _ in range(P)]
    coded = b""
    for c in range(K):
        planes = []
        for p in range(P):
            if p == (P - 1 if c == 0 else 0):
                pl = rng.permutation(np.repeat(np.arange(13, dtype=np.uint8), counts12))
                blk = huf_block_tl12(pl)
                r, back = O.huf_decompress(blk, plen)
                assert r == plen and back == pl.tobytes(), "the tableLog-12 block does not decode with the oracle"
            else:
                pl = rng.choice(np.array([7, 9, 200, 31, 32, 33], dtype=np.uint8), plen, p=[0.6, 0.2, 0.1, 0.05, 0.03, 0.02])
                r, blk = O.huf_compress(pl)
                assert 1 < r < plen
            planes.append(pl)
            blocks[p][c] = blk
        rotated = np.stack(planes, axis=1).reshape(-1).tobytes()          # byte j of the chunk = byte j / P of plane j % P
        coded += _unrotate(rotated, P)
    types = bytes([1]) * (P * K)
    cum = b""
    for p in range(P):
        t = 0
        for c in range(K):
            t += len(blocks[p][c])
            cum += t.to_bytes(8, "little")
    body = types + cum + b"".join(blocks[p][c] for p in range(P) for c in range(K))
    bm = 10 if P == 2 else 220
    assert O.decompress_body(body, P, 1, bm, chunk, K * chunk) == coded
    b = _gen2("bf16" if P == 2 else "fp32", K * chunk, 5)
    return ("tl12", K * chunk, P, 1, bm, chunk), xor(coded, b), b, body


# ---- placing buffers, running the entry points ----
def place(data, off, dev):
    """-> (guarded buffer of 0xAB, view of len(data) bytes holding `data` whose address is `off` modulo 16)."""
    n = len(data)
    buf = torch.full((GUARD + 16 + n + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    s = GUARD + (off - (buf.data_ptr() + GUARD)) % 16
    v = buf[s:s + n]
    v.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    assert v.data_ptr() % 16 == off
    return buf, v


def guards_ok(buf, v):
    s = v.data_ptr() - buf.data_ptr()
    return bool((buf[:s] == 0xAB).all()) and bool((buf[s + v.numel():] == 0xAB).all())


def to_dev(data, dev):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)


def got(v):
    return v.cpu().numpy().tobytes()


def stream_of(dev):
    return torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == "cuda" else 0


def windows(K):
    return [(0, K), (1, K), (K - 1, K)] if K > 1 else [(0, K)]


def check_entry_points(lib, case, a, b, body_bytes, off, dev, entries=("delta_dev", "windows", "plan")):
    """Every entry point with the destination pre-filled with the base and d_delta == d_dst (a window: d_dst == d_delta + chunk_lo * chunk): the tensor's
    bytes, which are also what a decode into a separate destination gives; guards untouched; the plan's second run gives the base back."""
    _, nb, P, rot, bm, ch = case
    K = -(-nb // ch)
    st = stream_of(dev)
    body = to_dev(body_bytes, dev)
    # the decode this must equal: a separate destination, the base at the same alignment
    _, bsep = place(b, off, dev)
    sbuf, sep = place(bytes(nb), off, dev)
    lib.decompress_dev(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, sep.data_ptr(), st, True, delta_ptr=bsep.data_ptr())
    assert got(sep) == a and guards_ok(sbuf, sep)
    if "delta_dev" in entries:
        buf, dst = place(b, off, dev)
        lib.decompress_dev(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, dst.data_ptr(), st, True, delta_ptr=dst.data_ptr())
        ks = lib.last_kernels()
        assert got(dst) == a, ("zn_decompress_delta_dev in place", int((np.frombuffer(got(dst), dtype=np.uint8) != np.frombuffer(a, dtype=np.uint8)).sum()), ks)
        assert guards_ok(buf, dst)
    if "windows" in entries:
        for lo, hi in windows(K):
            buf, dst = place(b, off, dev)
            lib.decompress_window_batch_dev([(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, lo, hi, dst.data_ptr() + lo * ch, dst.data_ptr())], st, True)
            end = min(hi * ch, nb)
            assert got(dst) == b[:lo * ch] + a[lo * ch:end] + b[end:], ("window", lo, hi, lib.last_kernels())
            assert guards_ok(buf, dst)
    if "plan" in entries:
        buf, dst = place(b, off, dev)
        h = lib.plan_create([(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, 0, K, dst.data_ptr(), dst.data_ptr())])
        try:
            lib.plan_run(h, st, True)
            assert got(dst) == a, ("plan, first run", lib.last_kernels())
            lib.plan_run(h, st, True)
            assert got(dst) == b, ("plan, second run", lib.last_kernels())
        finally:
            lib.plan_destroy(h)
        assert guards_ok(buf, dst)
