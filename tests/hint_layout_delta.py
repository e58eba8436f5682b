"""The layout of a sync index of kind ZN_HINT_DELTA ("Two kinds"), restated in plain Python from the design's words like tests/hint_layout.py
restates the PLAIN kind's: the same container — P K + 1 u32 offsets, padded to 64 bytes, then the hint bytes — in which EVERY Huffman-coded plane of a full
chunk the fused kernel takes has a region, four huff0 streams long, the planes' regions one behind the other in plane order.  Entry c P + p is where plane p's
region starts: a plane without one has an empty region (its entry equals the next)."""
import numpy as np

import hint_layout as HL


def plane_regions(body_bytes, P, chunk, n, c, tables=None):
    """-> [region bytes of plane p of chunk c for p in 0 .. P-1]; all zero where the fused kernel does not take the chunk."""
    K = -(-n // chunk)
    unit = HL.unit_symbols(P)
    none = [0] * P
    if min(chunk, n - c * chunk) != chunk or chunk % (4 * P * unit):
        return none
    types, csize, off = tables or HL.body_tables(body_bytes, P, K)
    plen = chunk // P
    seg = plen // 4
    huf = []
    for p in range(P):
        t, cs = int(types[p, c]), int(csize[p, c])
        if (t == 0 and cs >= plen) or (t == 1 and (cs == plen or cs == 1)):
            continue                                         # raw / RLE: the chunk is still the fused kernel's, the plane has no hints
        if t == 1 and 1 < cs < plen:
            huf.append(p)
        else:
            return none                                      # a plane the fused kernel does not take: neither is the chunk
    out = list(none)
    for p in huf:
        cs, o = int(csize[p, c]), int(off[p, c])
        if o + cs > len(body_bytes):
            continue
        h0 = body_bytes[o]
        hs = 1 + ((h0 - 126) // 2 if h0 >= 128 else h0)      # the tree description: its first byte says how long it is
        if not (hs < cs and cs - hs >= 10):
            continue
        rem = cs - hs
        l1, l2, l3 = (int.from_bytes(body_bytes[o + hs + 2 * i: o + hs + 2 * i + 2], "little") for i in range(3))          # the jump table
        if not (l1 and l2 and l3 and l1 + l2 + l3 + 6 < rem):
            continue
        l4 = rem - 6 - l1 - l2 - l3
        out[p] = sum(HL.stream_bytes(l, seg, unit) for l in (l1, l2, l3, l4))
    return out


def expected_table(body_bytes, P, chunk, n):
    """-> (offsets np.uint32[P K + 1], header bytes) of the DELTA index of the body of an n-byte tensor."""
    body_bytes = bytes(body_bytes)
    K = -(-n // chunk)
    offs = np.zeros(P * K + 1, dtype=np.uint32)
    run = HL.header_bytes(P, K)
    tables = HL.body_tables(body_bytes, P, K) if K else None
    for c in range(K):
        for p, size in enumerate(plane_regions(body_bytes, P, chunk, n, c, tables)):
            offs[c * P + p] = run
            run += size
    offs[P * K] = run
    return offs, HL.header_bytes(P, K)
