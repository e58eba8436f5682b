"""The XOR-merge of two "znp1" patches (include/zipnn_hip.h) restated in numpy from the format alone: the union of the two entry lists, the values
XORed where both have an entry, the zeros dropped, re-emitted with the layout formula.  No tensor is formed.  Test infrastructure — what the kernels of
zipnn_amd/csrc/zn_patch_merge.hip are compared with, byte for byte."""
import struct

import numpy as np

import patch_ref as R


def _entries(patch):
    """-> (E, n, global element indices, values) of a well-formed patch."""
    E, n, T, first, off, val = R.parse(patch)
    el = np.repeat(np.arange(first.size - 1, dtype=np.int64), np.diff(first.astype(np.int64))) * R.BLOCK + off.astype(np.int64)
    assert el.size == T and (np.diff(el) > 0).all() and (T == 0 or el[-1] < n // E) and (val != 0).all()
    return E, n, el, val


def merge(pa, pb, keep_empty=False):
    """-> the bytes of pa (+) pb, or None when everything cancels (keep_empty: the T == 0 patch instead)."""
    E, n, ea, va = _entries(pa)
    Eb, nb_, eb, vb = _entries(pb)
    assert (E, n) == (Eb, nb_), "the two patches describe different tensors"
    el = np.union1d(ea, eb)
    v = np.zeros(el.size, dtype=R._UINT[E])
    v[np.searchsorted(el, ea)] ^= va
    v[np.searchsorted(el, eb)] ^= vb
    live = v != 0
    el, v = el[live], v[live]
    T = int(el.size)
    if T == 0 and not keep_empty:
        return None
    nb = (n // E + R.BLOCK - 1) // R.BLOCK
    first = np.searchsorted(el, np.arange(nb + 1, dtype=np.int64) * R.BLOCK).astype("<u4")
    a1 = R.round16(32 + 4 * (nb + 1))
    a2 = R.round16(a1 + 2 * T)
    L = a2 + E * T
    out = bytearray(L)
    out[0:8] = b"ZNP1" + bytes([E, 0, 0, 0])
    out[8:32] = struct.pack("<QQQ", n, T, L)
    out[32:32 + 4 * (nb + 1)] = first.tobytes()
    out[a1:a1 + 2 * T] = (el % R.BLOCK).astype("<u2").tobytes()
    out[a2:a2 + E * T] = v.astype(R._UINT[E]).tobytes()
    return bytes(out)
