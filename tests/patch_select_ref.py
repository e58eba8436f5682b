"""Select and place of "znp1" patches (include/zipnn_hip.h, SHARDING PATCHES) restated in numpy, from the format text alone: a patch restricted to a rectangle
of its tensor, and a rectangle's patch embedded in the whole.  Test infrastructure — what the kernels of zipnn_amd/csrc/zn_patch_select.hip are compared with,
byte for byte.  Builds on tests/patch_ref.py (parse) and shares nothing with the kernels."""
import struct

import numpy as np

import patch_ref as R

BLOCK = R.BLOCK


def _emit(E, m, idx, val, keep_empty):
    """The canonical patch of a tensor of m elements whose changed elements are idx (ascending) with XOR values val."""
    T = int(idx.size)
    if T == 0 and not keep_empty:
        return None
    nb = (m + BLOCK - 1) // BLOCK
    first = np.searchsorted(idx, np.arange(nb + 1, dtype=np.int64) * BLOCK).astype("<u4")
    a1 = R.round16(32 + 4 * (nb + 1))
    a2 = R.round16(a1 + 2 * T)
    L = a2 + E * T
    out = bytearray(L)
    out[0:8] = b"ZNP1" + bytes([E, 0, 0, 0])
    out[8:32] = struct.pack("<QQQ", m * E, T, L)
    out[32:32 + 4 * (nb + 1)] = first.tobytes()
    out[a1:a1 + 2 * T] = (idx % BLOCK).astype("<u2").tobytes()
    out[a2:a2 + E * T] = val.astype(R._UINT[E]).tobytes()
    return bytes(out)


def _entries(patch):
    E, n, T, first, off, val = R.parse(patch)
    el = np.repeat(np.arange(first.size - 1, dtype=np.int64), np.diff(first.astype(np.int64))) * BLOCK + off
    return E, n // E, el, val


def select(patch, rows, cols, r0, r1, c0, c1, keep_empty=False):
    """patch covers rows x cols elements -> the patch of the rectangle rows [r0, r1) x cols [c0, c1), or None when no entry lies inside."""
    E, m, el, val = _entries(patch)
    assert m == rows * cols and 0 <= r0 < r1 <= rows and 0 <= c0 < c1 <= cols
    row, col = el // cols, el % cols
    keep = (row >= r0) & (row < r1) & (col >= c0) & (col < c1)
    w = c1 - c0
    j = (row[keep] - r0) * w + (col[keep] - c0)
    return _emit(E, (r1 - r0) * w, j, val[keep], keep_empty)


def place(patch, rows, cols, r0, r1, c0, c1, keep_empty=False):
    """patch covers the rectangle -> the patch of the whole rows x cols tensor that changes exactly those elements, or None for a patch without entries."""
    E, m, j, val = _entries(patch)
    w = c1 - c0
    assert m == (r1 - r0) * w and 0 <= r0 < r1 <= rows and 0 <= c0 < c1 <= cols
    i = (r0 + j // w) * cols + c0 + j % w
    return _emit(E, rows * cols, i, val, keep_empty)
