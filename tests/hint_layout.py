"""The layout of a sync index (decode hints), restated in plain Python from the design's words — not from the kernels' text — so that the offset table
zn_k_hint_size writes can be held against something other than another run of the same source.

A body (the frame behind its 32-byte header) of P planes and K chunks is: types u8[P][K]; inclusive cumulative compressed sizes u64[P][K], plane-major;
the payload from 9 P K on, plane p's payload behind the totals of the planes before it.  The index is a table of P K + 1 u32 offsets, padded to 64 bytes,
then the hint bytes: only the FIRST Huffman-coded plane of a full chunk the fused kernel takes has a region, four huff0 streams long.

The two constants of the decoder that the region length depends on — the wave's staging ring and the cap of the sub-block size, in dwords — are read out of
zn_decode_fused.hip: a deliberate change of either changes what this module expects, and the tests that use it fail or pass on the new layout, never silently
on the old one."""
import os
import re

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zipnn_amd", "csrc", "zn_decode_fused.hip")


def _constant(name):
    with open(_SRC) as f:
        m = re.search(r"^#define\s+" + name + r"\s+(\d+)u?\b", f.read(), re.M)
    assert m, f"{name} not found in {_SRC}"
    return int(m.group(1))


RING_BYTES = _constant("ZN_F_RING_BYTES")
DCAP = _constant("ZN_F_DCAP")


def header_bytes(P, K):
    return ((P * K + 1) * 4 + 63) & ~63


def unit_symbols(P):
    """Symbols per flushed row of the fused decoder."""
    return 64 * (16 if P == 1 else 8)


def stream_bytes(slen, seg, unit):
    """Hint bytes of one huff0 stream of `slen` bytes that decodes to `seg` symbols: 64 per tile, for as many tiles as it has at the smallest sub-block
    size d (dwords per lane) the decoder can choose for it, the stream lying three bytes into a dword."""
    d = min(max(((RING_BYTES - unit - 128) * slen) // (256 * seg), 1), DCAP)
    return 64 * -(-((slen + 6) >> 2) // (64 * d))


def body_tables(body_bytes, P, K):
    """-> (types u8[P][K], compressed sizes int64[P][K], payload offsets int64[P][K])."""
    b = np.frombuffer(bytes(body_bytes[:9 * P * K]), dtype=np.uint8)
    types = b[:P * K].reshape(P, K)
    cum = b[P * K:].view("<u8").reshape(P, K).astype(np.int64)
    prev = np.concatenate([np.zeros((P, 1), dtype=np.int64), cum[:, :-1]], axis=1)
    base = 9 * P * K + np.concatenate([[0], np.cumsum(cum[:, -1])[:-1]])
    return types, cum - prev, base[:, None] + prev


def chunk_region(body_bytes, P, chunk, n, c, tables=None):
    """-> (h, region bytes): the first Huffman-coded plane of chunk c and the length of its hint region; (-1, 0) where the chunk has none."""
    K = -(-n // chunk)
    unit = unit_symbols(P)
    if min(chunk, n - c * chunk) != chunk or chunk % (4 * P * unit):
        return -1, 0
    types, csize, off = tables or body_tables(body_bytes, P, K)
    plen = chunk // P
    h = -1
    for p in range(P):
        t, cs = int(types[p, c]), int(csize[p, c])
        if t == 0 and cs >= plen:
            kind = "raw"
        elif t == 1 and cs == plen:
            kind = "raw"
        elif t == 1 and cs == 1:
            kind = "rle"
        elif t == 1 and 1 < cs < plen:
            kind = "huf"
        else:
            return -1, 0
        if kind == "huf" and h < 0:
            h = p
    if h < 0:
        return -1, 0
    cs, o = int(csize[h, c]), int(off[h, c])
    if o + cs > len(body_bytes):
        return h, 0
    h0 = body_bytes[o]
    hs = 1 + ((h0 - 126) // 2 if h0 >= 128 else h0)          # the tree description: its first byte says how long it is
    if not (hs < cs and cs - hs >= 10):
        return h, 0
    rem = cs - hs
    l1, l2, l3 = (int.from_bytes(body_bytes[o + hs + 2 * i: o + hs + 2 * i + 2], "little") for i in range(3))          # the jump table
    if not (l1 and l2 and l3 and l1 + l2 + l3 + 6 < rem):
        return h, 0
    l4 = rem - 6 - l1 - l2 - l3
    seg = plen // 4
    return h, sum(stream_bytes(l, seg, unit) for l in (l1, l2, l3, l4))


def expected_table(body_bytes, P, chunk, n):
    """-> (offsets np.uint32[P K + 1], header bytes) of the index of the body of an n-byte tensor."""
    body_bytes = bytes(body_bytes)
    K = -(-n // chunk)
    offs = np.zeros(P * K + 1, dtype=np.uint32)
    run = header_bytes(P, K)
    tables = body_tables(body_bytes, P, K) if K else None
    for c in range(K):
        h, size = chunk_region(body_bytes, P, chunk, n, c, tables)
        for p in range(P):
            offs[c * P + p] = run + (size if 0 <= h < p else 0)
        run += size
    offs[P * K] = run
    return offs, header_bytes(P, K)
