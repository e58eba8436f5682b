"""Shared cases of the patch-check tests (tests/test_patch_check_simt.py on the emulated kernels, tests/test_gpu_patch_check.py on the device):
zn_patch_check_batch_dev / zipnn_amd.patch_check (include/zipnn_hip.h) over well-formed patches from tests/patch_ref.py, over the hostile corpus of
tests/test_patch_simt.py and over four damages zn_k_patch_apply does not see.  EXPECTED holds the verdicts of the EMULATED build for the whole corpus, as literals:
the device must give the same."""
import struct

import numpy as np
import pytest
import torch

import patch_ref as R
import patch_util as U
from test_patch_simt import _hostile
from zipnn_amd._capi import (PATCH_BAD_FIRST, PATCH_BAD_HEADER, PATCH_BAD_OFFSET, PATCH_BAD_PADDING, PATCH_BAD_VALUE, ZN_E_CORRUPT, ZnError)

BLOCK = R.BLOCK
ANY = PATCH_BAD_HEADER | PATCH_BAD_FIRST | PATCH_BAD_OFFSET | PATCH_BAD_VALUE | PATCH_BAD_PADDING
# the bit each case of the hostile corpus aims at (random bytes: any)
AIMS = {"truncated": PATCH_BAD_HEADER, "truncated-to-the-header": PATCH_BAD_HEADER, "wrong-E": PATCH_BAD_HEADER, "wrong-n": PATCH_BAD_HEADER,
        "wrong-n-smaller": PATCH_BAD_HEADER, "wrong-L": PATCH_BAD_HEADER, "wrong-T": PATCH_BAD_HEADER, "huge-T": PATCH_BAD_HEADER, "wrong-magic": PATCH_BAD_HEADER,
        "first-decreases": PATCH_BAD_FIRST, "first-0-nonzero": PATCH_BAD_FIRST, "first-NB-above-T": PATCH_BAD_FIRST, "first-NB-below-T": PATCH_BAD_FIRST,
        "offset-past-the-end": PATCH_BAD_OFFSET, "repeated-offset": PATCH_BAD_OFFSET, "descending-offset": PATCH_BAD_OFFSET, "zero-value": PATCH_BAD_VALUE,
        "pad-after-first": PATCH_BAD_PADDING, "pad-after-off": PATCH_BAD_PADDING, "header-bytes-5-7": PATCH_BAD_PADDING, "first-pair-of-an-unvisited-block": PATCH_BAD_FIRST}

# What the EMULATED build answered (mask per case, in corpus order; the well-formed patches' T comes from the restatement, not from here).
_MASKS = [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 4, 4, 4, 8, 1, 1, 1, 18, 18, 18, 16, 16, 16, 2]      # (the three element sizes answered alike)
EXPECTED = {1: _MASKS, 2: _MASKS, 4: _MASKS}


def exact(data, dev):
    """bytes -> a uint8 tensor that IS an allocation of exactly that length (a read behind it is a read outside the allocation), 16-byte aligned."""
    t = torch.empty(max(len(data), 1), dtype=torch.uint8, device=dev)[:len(data)]
    assert t.data_ptr() % 16 == 0
    t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8) if len(data) else torch.empty(0, dtype=torch.uint8))
    return t


def well_formed(E):
    """-> [(label, patch bytes, n, T)]: the build cases of tests/patch_util.py — every size x {T = 0, the first element, the LAST element, every element} and the
    structural ones — as the restatement builds them."""
    out = []
    for label, s, b in U.build_cases(E):
        patch = R.build(s, b, E, keep_empty=True)
        out.append((label, patch, s.size, R.parse(patch)[2]))
    return out


def _pair(E, m, T, seed):
    """-> (source, base, patch) with exactly T differing elements: the first, the last, both sides of every block edge, the rest spread evenly."""
    rng = np.random.default_rng(seed + E)
    base = U._rand(rng, m * E)
    src = base.copy()
    elems = {0, m - 1} | {e for k in range(1, (m - 1) // BLOCK + 1) for e in (k * BLOCK - 1, k * BLOCK)}
    elems |= set((np.arange(T - len(elems)) * (m // T) + 17).tolist())
    assert len(elems) == T
    U._flip(src, E, sorted(elems), rng)
    return src, base, R.build(src, base, E)


def unseen(E):
    """-> (source, base, good patch, [(label, patch bytes)]) for each of the two tensors: damages that zn_k_patch_apply does not see.  The first tensor has two
    blocks (four bytes of padding behind first[]) and a T that leaves padding behind off[]; the second has three, for a first[] pair no one-block window visits."""
    src, base, good = _pair(E, BLOCK + 40, 61, 11)
    _, n, T, first, off, val = R.parse(good)
    nb = first.size - 1
    a1 = R.round16(32 + 4 * (nb + 1))
    a2 = R.round16(a1 + 2 * T)
    assert a1 > 32 + 4 * (nb + 1) and a2 > a1 + 2 * T, "the pair must leave padding behind first[] and behind off[]"

    def edit(p, at, data):
        p = bytearray(p)
        p[at:at + len(data)] = data
        return bytes(p)
    two = [("pad-after-first", edit(good, a1 - 1, b"\x01")), ("pad-after-off", edit(good, a2 - 1, b"\x80")), ("header-bytes-5-7", edit(good, 6, b"\x01"))]
    src3, base3, good3 = _pair(E, 2 * BLOCK + 3, 70, 12)
    T3, first3 = R.parse(good3)[2], R.parse(good3)[3]
    assert first3.size == 4 and 0 < first3[1] < first3[2] < T3
    three = [("first-pair-of-an-unvisited-block", edit(good3, 32 + 4 * 2, struct.pack("<I", T3 + 1)))]
    return (src, base, good, two), (src3, base3, good3, three)


def corpus(E):
    """-> [(label, patch bytes as handed over, n)]: the hostile corpus (each patch cut to the length handed over) and the four damages apply does not see."""
    src, base, cases = _hostile(E)
    out = [(label, data[:len(data) if plen is None else plen], base.size) for label, data, plen in cases]
    for s, b, _, extra in unseen(E):
        out += [(label, data, b.size) for label, data in extra]
    return out


def run(lib, dev, items):
    """[(patch bytes, n, E)] -> (verdicts, entries) by ONE call, every patch an allocation of its own."""
    held = [exact(p, dev) for p, _, _ in items]
    return lib.patch_check_batch_dev([(t.data_ptr(), t.numel(), n, E) for t, (_, n, E) in zip(held, items)])


def check_well_formed(lib, dev, E):
    cases = well_formed(E)
    verdicts, entries = run(lib, dev, [(p, n, E) for _, p, n, _ in cases])
    for (label, p, n, T), v, t in zip(cases, verdicts, entries):
        assert (v, t) == (0, T), f"E={E} {label}: verdict {v:#x}, T {t} (want 0, {T})"
    labels = [c[0] for c in cases]
    assert {f"m{m}-{k}" for m in U.SIZES for k in ("T0", "first", "last", "all")} <= set(labels)
    # one item alone (it travels as the kernel's argument), and the public function
    label, p, n, T = cases[-1]
    assert run(lib, dev, [(p, n, E)]) == ([0], [T])
    assert "zn_k_patch_check" in lib.last_kernels()
    import zipnn_amd
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[E]
    like = torch.empty(n // E, dtype=dt, device=dev)
    assert zipnn_amd.patch_check(exact(p, dev), like) == T and zipnn_amd.patch_check(None, like) == 0


def check_hostile(lib, dev, E):
    """Every case of the corpus is refused with the bit of the check it aims at; the masks are the emulated build's (EXPECTED)."""
    import zipnn_amd
    cases = [c for c in corpus(E) if len(c[1]) >= 32]
    verdicts, entries = run(lib, dev, [(p, n, E) for _, p, n in cases])
    print(f"E={E} masks:", verdicts)
    for (label, p, n), v, t in zip(cases, verdicts, entries):
        aim = AIMS.get(label, ANY)
        assert v & aim and t == 0, f"E={E} {label}: verdict {v:#x}, aimed at {aim:#x}"
    assert verdicts == EXPECTED[E], f"E={E}: the verdicts differ from the emulated build's"
    # a patch shorter than a header never reaches a launch
    short = [c for c in corpus(E) if len(c[1]) < 32]
    assert [c[0] for c in short] == ["shorter-than-a-header"]
    with pytest.raises(ValueError):
        run(lib, dev, [(short[0][1], short[0][2], E)])
    # the public function raises ZN_E_CORRUPT and carries the mask
    label, p, n = cases[-1]
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[E]
    with pytest.raises(ZnError) as ei:
        zipnn_amd.patch_check(exact(p, dev), torch.empty(n // E, dtype=dt, device=dev))
    assert ei.value.status == ZN_E_CORRUPT and ei.value.mask == verdicts[-1]


def check_unseen(lib, dev, E):
    """The damages apply does not see: patch_apply passes — and gives the right bytes — where patch_check refuses.  (Header bytes 5-7 are the exception the format
    makes: apply reads E as the 32-bit word at offset 4, so it refuses those as a wrong E; the check names them as padding.)"""
    for src, base, good, extra in unseen(E):
        n = base.size
        for label, data in extra:
            p = exact(data, dev)
            verdicts, _ = lib.patch_check_batch_dev([(p.data_ptr(), p.numel(), n, E)])
            assert verdicts[0] == AIMS[label], (label, verdicts)
            hi = n if label != "first-pair-of-an-unvisited-block" else BLOCK * E     # (a window of block 0 alone)
            buf, view, o = U.canaried(base[:hi], dev, E)
            item = (p.data_ptr(), p.numel(), n, E, 0, hi, view.data_ptr())
            if label == "header-bytes-5-7":
                with pytest.raises(ZnError) as ei:
                    lib.patch_apply_batch_dev([item])
                assert ei.value.status == ZN_E_CORRUPT
            else:
                lib.patch_apply_batch_dev([item])
                assert bytes(view.cpu().numpy()) == bytes(src[:hi]), label
            assert U.canaries_intact(buf, o, hi), label
        g = exact(good, dev)
        assert lib.patch_check_batch_dev([(g.data_ptr(), g.numel(), n, E)])[0] == [0]


def check_batch_of_five(lib, dev):
    """Mixed element sizes in one launch, one bad item: only its word is set."""
    items = []
    for E in (2, 1, 4, 2, 1):
        label, p, n, T = well_formed(E)[-1]
        items.append([p, n, E, T])
    bad = bytearray(items[3][0])
    a2 = len(bad) - items[3][2] * items[3][3]
    bad[a2:a2 + 2] = b"\0\0"                                                     # a zero value
    items[3][0] = bytes(bad)
    verdicts, entries = run(lib, dev, [(p, n, E) for p, n, E, _ in items])
    assert verdicts == [0, 0, 0, PATCH_BAD_VALUE, 0]
    assert entries == [T if k != 3 else 0 for k, (_, _, _, T) in enumerate(items)]
    assert lib.patch_check_batch_dev([]) == ([], [])


def check_arguments(lib, dev):
    label, p, n, T = well_formed(2)[-1]
    t = exact(p, dev)
    ok = (t.data_ptr(), t.numel(), n, 2)
    assert lib.patch_check_batch_dev([ok]) == ([0], [T])
    for bad in ((0,) + ok[1:], (ok[0] + 2,) + ok[1:], (ok[0], 31) + ok[2:], ok[:3] + (3,), ok[:2] + (n - 1, 2), ok[:2] + (2 ** 33, 1)):
        with pytest.raises(ValueError):
            lib.patch_check_batch_dev([bad])
        with pytest.raises(ValueError):
            lib.patch_check_batch_dev([ok, bad])
    # a length that is not the header's L is a verdict, not an argument error; a tensor without elements has a patch too
    assert lib.patch_check_batch_dev([(ok[0], ok[1] - 16) + ok[2:]])[0] == [PATCH_BAD_HEADER]
    for E in (1, 2, 4):
        empty = R.build(np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), E, keep_empty=True)
        assert run(lib, dev, [(empty, 0, E)]) == ([0], [0])
        assert run(lib, dev, [(empty[:40] + b"\x01" + empty[41:], 0, E)])[0] == [PATCH_BAD_PADDING]
    assert lib._L.zn_abi_version() == 3
