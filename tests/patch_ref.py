"""The patch format "znp1" (include/zipnn_hip.h) restated in numpy, from the format's definition alone: build and apply.  Test infrastructure — what the
kernels of zipnn_amd/csrc/zn_patch.hip are compared with, byte for byte (the patch of a (tensor, base) pair is unique)."""
import struct

import numpy as np

BLOCK = 65536
_UINT = {1: np.uint8, 2: np.dtype("<u2"), 4: np.dtype("<u4")}


def round16(x):
    return (x + 15) // 16 * 16


def patch_len(n, E, T):
    """L for a tensor of n bytes, E bytes per element, T differing elements."""
    nb = (n // E + BLOCK - 1) // BLOCK
    return round16(round16(32 + 4 * (nb + 1)) + 2 * T) + E * T


def _bytes(x):
    return np.frombuffer(bytes(x), dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def build(tensor, base, E, keep_empty=False):
    """-> the patch's bytes, or None when the two are identical (keep_empty: the T == 0 patch instead)."""
    a, b = _bytes(tensor), _bytes(base)
    n = a.size
    assert b.size == n and n % E == 0 and n // E < 2 ** 32
    m = n // E
    x = (a ^ b).view(_UINT[E])
    idx = np.flatnonzero(x)
    T = int(idx.size)
    if T == 0 and not keep_empty:
        return None
    nb = (m + BLOCK - 1) // BLOCK
    first = np.searchsorted(idx, np.arange(nb + 1, dtype=np.int64) * BLOCK).astype("<u4")
    a1 = round16(32 + 4 * (nb + 1))
    a2 = round16(a1 + 2 * T)
    L = a2 + E * T
    out = bytearray(L)
    out[0:8] = b"ZNP1" + bytes([E, 0, 0, 0])
    out[8:32] = struct.pack("<QQQ", n, T, L)
    out[32:32 + 4 * (nb + 1)] = first.tobytes()
    out[a1:a1 + 2 * T] = (idx % BLOCK).astype("<u2").tobytes()
    out[a2:a2 + E * T] = x[idx].astype(_UINT[E]).tobytes()
    return bytes(out)


def parse(patch):
    """-> (E, n, T, first, off, val) of a well-formed patch."""
    p = bytes(patch)
    assert p[:4] == b"ZNP1" and p[5:8] == b"\0\0\0"
    E = p[4]
    n, T, L = struct.unpack("<QQQ", p[8:32])
    assert L == len(p) == patch_len(n, E, T)
    nb = (n // E + BLOCK - 1) // BLOCK
    a1 = round16(32 + 4 * (nb + 1))
    a2 = round16(a1 + 2 * T)
    first = np.frombuffer(p, dtype="<u4", count=nb + 1, offset=32)
    off = np.frombuffer(p, dtype="<u2", count=T, offset=a1)
    val = np.frombuffer(p, dtype=_UINT[E], count=T, offset=a2)
    return E, n, T, first, off, val


def apply(dst, patch, byte_lo=0, byte_hi=None):
    """dst: the bytes [byte_lo, byte_hi) of the tensor (any array-like of bytes) -> those bytes with the window's entries XORed in (a new uint8 array)."""
    E, n, T, first, off, val = parse(patch)
    byte_hi = n if byte_hi is None else byte_hi
    out = _bytes(dst).copy()
    assert out.size == byte_hi - byte_lo and byte_lo % E == 0 and byte_hi % E == 0
    el = np.repeat(np.arange(first.size - 1, dtype=np.int64), np.diff(first.astype(np.int64))) * BLOCK + off
    keep = (el >= byte_lo // E) & (el < byte_hi // E)
    v = out.view(_UINT[E])
    v[el[keep] - byte_lo // E] ^= val[keep]
    return out
