"""Shared cases of the patch select / place tests (tests/test_patch_select_simt.py on the emulated kernels, tests/test_gpu_patch_select.py on the device):
zn_patch_select_batch_dev and zn_patch_place_batch_dev against their numpy restatement (tests/patch_select_ref.py) and against the patches tests/patch_ref.py
builds from the sliced tensors, which neither call ever sees — three byte strings that must be one.  Every case is a geometry (the tensor as rows x cols, a
rectangle of it) and two byte arrays (base, tensor); every expected value is checked on the CPU to equal patch_ref.build on the sliced arrays before it judges
the library."""
import numpy as np
import torch

import patch_ref as R
import patch_select_ref as S
import patch_util as PU

BLOCK = R.BLOCK

# (label, rows, cols, r0, r1, c0, c1)
GEOMETRIES = (
    ("1x1", 1, 1, 0, 1, 0, 1),
    ("65537x1-rows-1", 65537, 1, 1, 65537, 0, 1),
    ("3x65536-last-col", 3, 65536, 0, 3, 65535, 65536),                          # w = 1
    ("2x65537-cols-1", 2, 65537, 0, 2, 1, 65537),
    ("700x300-cols-7-45", 700, 300, 0, 700, 7, 45),                              # one output block over four input blocks
    ("700x300-cols-10-250", 700, 300, 0, 700, 10, 250),                          # three output blocks
    ("700x300-rows-1-699", 700, 300, 1, 699, 0, 300),                            # w = C
    ("700x300-rows-3-650-cols-10-250", 700, 300, 3, 650, 10, 250),
    ("700x300-whole", 700, 300, 0, 700, 0, 300),                                 # select is the identity
)


def _rand(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8)


def _odd(rng, E, k):
    return (rng.integers(0, 256, size=k * E, dtype=np.uint8).view(R._UINT[E]) | 1).astype(R._UINT[E])


def _changed(base, E, idx, rng):
    idx = np.unique(np.asarray(idx, dtype=np.int64))
    out = base.copy()
    out.view(R._UINT[E])[idx] ^= _odd(rng, E, idx.size)
    return out


def phi(g, j):
    _, rows, cols, r0, r1, c0, c1 = g
    w = c1 - c0
    return (r0 + j // w) * cols + c0 + j % w


def inside(g):
    """-> a boolean array over the tensor's elements: which lie in the rectangle"""
    _, rows, cols, r0, r1, c0, c1 = g
    mask = np.zeros((rows, cols), dtype=bool)
    mask[r0:r1, c0:c1] = True
    return mask.reshape(-1)


def cut(g, arr, E):
    """the rectangle's bytes of a tensor's bytes, contiguous"""
    _, rows, cols, r0, r1, c0, c1 = g
    return np.ascontiguousarray(arr.view(R._UINT[E]).reshape(rows, cols)[r0:r1, c0:c1]).reshape(-1).view(np.uint8)


def contents(g, E, rng):
    """-> [(label, base bytes, tensor bytes)] for one geometry"""
    _, rows, cols, r0, r1, c0, c1 = g
    m, mask = rows * cols, inside(g)
    mr = (r1 - r0) * (c1 - c0)
    base = _rand(rng, m * E)
    out = []
    # the four corners of the rectangle and the eight elements just outside them (where the tensor has them)
    near = set()
    for r in (r0, r1 - 1):
        for c in (c0, c1 - 1):
            for rr, cc in ((r, c), (r - 1 if r == r0 else r + 1, c), (r, c - 1 if c == c0 else c + 1)):
                if 0 <= rr < rows and 0 <= cc < cols:
                    near.add(rr * cols + cc)
    out.append(("corners", base, _changed(base, E, sorted(near), rng)))
    out.append(("all", base, _changed(base, E, np.arange(m), rng)))
    if not mask.all():
        outside = np.flatnonzero(~mask)
        out.append(("outside-only", base, _changed(base, E, outside[:: max(outside.size // 500, 1)], rng)))
    edge = [i for i in list(range(0, m, BLOCK)) + list(range(BLOCK - 1, m, BLOCK)) + [m - 1]]       # block offsets 0 and 65 535 of the input's blocks …
    edge += [phi(g, j) for j in list(range(0, mr, BLOCK)) + list(range(BLOCK - 1, mr, BLOCK)) + [mr - 1]]      # … and of the output's
    out.append(("block-edges", base, _changed(base, E, edge, rng)))
    if m > 2 * BLOCK:                                                            # an input block empty between two that are not
        idx = np.concatenate((rng.choice(BLOCK, size=300, replace=False), 2 * BLOCK + rng.choice(m - 2 * BLOCK, size=min(300, m - 2 * BLOCK), replace=False)))
        out.append(("empty-block", base, _changed(base, E, idx, rng)))
    out.append(("two-percent", base, _changed(base, E, rng.choice(m, size=max(m // 50, 1), replace=False), rng)))
    return out


_CASES = {}


def prepared(E):
    """-> [(label, geometry, whole patch (T may be 0), rectangle patch or None, placed-back patch or None)] for one element size, computed once: the
    restatement must agree with patch_ref.build on the sliced arrays before either judges a kernel."""
    if E not in _CASES:
        rng = np.random.default_rng(9000 * E)
        rows_ = []
        for g in GEOMETRIES:
            mask = inside(g)
            for label, base, t in contents(g, E, rng):
                whole = R.build(t, base, E, keep_empty=True)
                want = R.build(cut(g, t, E), cut(g, base, E), E)
                assert S.select(whole, *g[1:]) == want, f"E={E} {g[0]} {label}: the restated select differs from the patch of the sliced arrays"
                back = base.copy()                                               # the base with its rectangle set to the tensor's
                bv, tv = back.view(R._UINT[E]), t.view(R._UINT[E])
                bv[mask] = tv[mask]
                placed = R.build(back, base, E)
                if want is not None:
                    assert S.place(want, *g[1:]) == placed, f"E={E} {g[0]} {label}: the restated place differs from the patch of the embedded rectangle"
                    assert S.select(placed, *g[1:]) == want
                else:
                    assert placed is None
                if g[0].endswith("whole"):
                    assert want == R.build(t, base, E)
                rows_.append((f"{g[0]}/{label}", g, whole, want, placed))
        assert any(r[3] is None for r in rows_) and len({r[0] for r in rows_}) == len(rows_)
        _CASES[E] = rows_
    return _CASES[E]


def on_device(data, dev):
    return PU.on_device(np.frombuffer(data, dtype=np.uint8), dev)


def device_select(lib, dev, items, place=False):
    """items: [(patch bytes, E, rows, cols, r0, r1, c0, c1)] -> the results as bytes (None: no entry), by ONE zn_patch_select_batch_dev (place:
    zn_patch_place_batch_dev) call; capacities exactly the lengths the size call gives, each output between canaries of 0xA5; the inputs unchanged."""
    held = [on_device(it[0], dev) for it in items]
    args = [(p.data_ptr(), p.numel()) + tuple(it[1:]) for p, it in zip(held, items)]
    sizes = (lib.patch_place_size_batch_dev if place else lib.patch_select_size_batch_dev)(args)
    offs, o = [], 256
    for n in sizes:
        offs.append(o)
        o += (n + 255) // 256 * 256 + 256
    arena = torch.full((o + 16,), 0xA5, dtype=torch.uint8, device=dev)
    a0 = (-arena.data_ptr()) % 16
    lens = (lib.patch_place_batch_dev if place else lib.patch_select_batch_dev)([a + (arena.data_ptr() + a0 + off, n) for a, off, n in zip(args, offs, sizes)])
    assert lens == sizes
    host = arena.cpu().numpy()
    keep = np.ones(host.size, dtype=bool)
    for off, n in zip(offs, lens):
        keep[a0 + off: a0 + off + n] = False
    assert (host[keep] == 0xA5).all(), "a select wrote outside its output"
    for p, it in zip(held, items):
        assert bytes(p.cpu().numpy()) == it[0], "a select changed its input"
    return [bytes(host[a0 + off: a0 + off + n]) if n else None for off, n in zip(offs, lens)]


def check_select_and_place(lib, dev, E):
    rows_ = prepared(E)
    got = device_select(lib, dev, [(whole, E) + g[1:] for _, g, whole, _, _ in rows_])
    for (label, g, whole, want, _), x in zip(rows_, got):
        assert x == want, f"E={E} {label}: the device's select differs from the restatement"
        if g[0].endswith("whole") and want is not None:
            assert x == whole                                                    # the identity, byte for byte
    assert {"zn_k_patch_select_count", "zn_k_patch_scan", "zn_k_patch_select_emit"} <= set(lib.last_kernels().split(";"))
    some = [r for r in rows_ if r[3] is not None]
    got = device_select(lib, dev, [(want, E) + g[1:] for _, g, _, want, _ in some], place=True)
    for (label, g, _, want, placed), x in zip(some, got):
        assert x == placed, f"E={E} {label}: the device's place differs from the restatement"
    assert {"zn_k_patch_place_count", "zn_k_patch_scan", "zn_k_patch_place_emit"} <= set(lib.last_kernels().split(";"))
    # select(place(p)) == p, on the device's own results
    again = device_select(lib, dev, [(x, E) + g[1:] for (_, g, _, _, _), x in zip(some, got)])
    assert again == [r[3] for r in some]
    # a patch without entries places to nothing; the last case alone (it travels as the kernel's argument)
    label, g, whole, want, placed = rows_[-1]
    assert device_select(lib, dev, [(whole, E) + g[1:]]) == [want]
    assert device_select(lib, dev, [(want, E) + g[1:]], place=True) == [placed]
    empty = R.build(np.zeros(7 * 5 * E, dtype=np.uint8), np.zeros(7 * 5 * E, dtype=np.uint8), E, keep_empty=True)
    assert device_select(lib, dev, [(empty, E, 9, 11, 1, 8, 2, 7)], place=True) == [None]


def check_ragged(lib, dev):
    """Mixed element sizes and an empty result among the items in one call, in both orders, select and place."""
    rng = np.random.default_rng(31)
    items, want = [], []
    for E, g in ((2, ("a", 300, 700, 0, 300, 100, 450)), (4, ("b", 123, 100, 5, 77, 0, 100)), (1, ("c", 2, BLOCK + 1, 0, 2, 3, BLOCK)),
                 (2, ("d", 30, 10, 0, 15, 0, 10)), (4, ("e", 1, BLOCK, 0, 1, 17, 40000)), (1, ("f", 1, 1, 0, 1, 0, 1))):
        m = g[1] * g[2]
        base = _rand(rng, m * E)
        if g[0] == "d":                                                          # every change lies outside the rectangle
            t = _changed(base, E, [m - 1, m - 7], rng)
        else:
            t = _changed(base, E, rng.choice(m, size=max(m // 50, 1), replace=False), rng)
        items.append((R.build(t, base, E, keep_empty=True), E) + g[1:])
        want.append(R.build(cut(g, t, E), cut(g, base, E), E))
        assert S.select(items[-1][0], *g[1:]) == want[-1]
    assert want[3] is None and all(x is not None for x in want[:3])
    assert device_select(lib, dev, items) == want
    assert device_select(lib, dev, list(reversed(items))) == list(reversed(want))
    back = [(x if x is not None else R.build(np.zeros(15 * 10 * it[1], dtype=np.uint8), np.zeros(15 * 10 * it[1], dtype=np.uint8), it[1], keep_empty=True),) + it[1:]
            for x, it in zip(want, items)]
    placed = device_select(lib, dev, back, place=True)
    assert placed == [S.place(b[0], *b[2:]) for b in back] and placed[3] is None


_DT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _pair(E, shape, rng, dev):
    m = int(np.prod(shape))
    base = _rand(rng, m * E)
    t = _changed(base, E, rng.choice(m, size=m // 50, replace=False), rng)
    return (PU.on_device(x, dev).view(_DT[E]).view(*shape) for x in (base, t))


def check_splits_merge_back(dev):
    """patch_merge over the placed selects of a two-way and a three-way split along dim 0 and along dim 1 is the original patch."""
    import zipnn_amd
    rng = np.random.default_rng(41)
    for E in (1, 2, 4):
        shape = (700, 300)
        tb, tt = _pair(E, shape, rng, dev)
        whole = zipnn_amd.patch_build(tt, tb)
        for dim in (0, 1):
            for cuts in ((0, shape[dim] // 2 + 1, shape[dim]), (0, 7, shape[dim] - 100, shape[dim])):
                acc = None
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    part = zipnn_amd.patch_select(whole, shape, dim, lo, hi)
                    assert bytes(part.cpu().numpy()) == R.build(tt.narrow(dim, lo, hi - lo).contiguous().cpu().numpy(), tb.narrow(dim, lo, hi - lo).contiguous().cpu().numpy(), E)
                    placed = zipnn_amd.patch_place(part, shape, dim, lo, hi)
                    acc = placed if acc is None else zipnn_amd.patch_merge(acc, placed)
                assert torch.equal(acc, whole), (E, dim, cuts)


def check_public(dev):
    """patch_apply_ of a select onto the base's shard gives the tensor's shard; a 3-D shape narrowed along dim 1; what the public functions refuse."""
    import pytest
    import zipnn_amd
    rng = np.random.default_rng(51)
    for E, shape, dim, lo, hi in ((2, (700, 300), 0, 100, 350), (4, (700, 300), 1, 10, 250), (1, (5, 40, 70), 1, 3, 29), (2, (5, 40, 70), -2, 1, 40)):
        tb, tt = _pair(E, shape, rng, dev)
        whole = zipnn_amd.patch_build(tt, tb)
        sb, st = (x.narrow(dim, lo, hi - lo).contiguous() for x in (tb, tt))
        part = zipnn_amd.patch_select(whole, shape, dim, lo, hi)
        assert torch.equal(part, zipnn_amd.patch_build(st, sb)) and bytes(part.cpu().numpy()) == R.build(st.cpu().numpy(), sb.cpu().numpy(), E)
        assert zipnn_amd.patch_check(part, sb) == int((st != sb).sum())
        live = sb.clone()
        assert zipnn_amd.patch_apply_(live, part) is live and torch.equal(live, st)
        placed = zipnn_amd.patch_place(part, shape, dim, lo, hi)
        back = tb.clone()
        back.narrow(dim, lo, hi - lo).copy_(st)
        assert torch.equal(placed, zipnn_amd.patch_build(back, tb))
        assert torch.equal(zipnn_amd.patch_select(placed, shape, dim, lo, hi), part)
        shifted = torch.empty(whole.numel() + 16, dtype=torch.uint8, device=whole.device)
        o = (-shifted.data_ptr()) % 16 + 4
        shifted[o:o + whole.numel()] = whole
        assert torch.equal(zipnn_amd.patch_select(shifted[o:o + whole.numel()], shape, dim, lo, hi), part)      # (a misaligned patch is cloned)
        for bad in ((shape, dim, lo, lo), (shape, dim, lo, shape[dim] + 1), (shape, len(shape), 0, 1), (shape[:-1] + (shape[-1] + 1,), dim, lo, hi), (shape, dim, -1, hi)):
            with pytest.raises(ValueError):
                zipnn_amd.patch_select(whole, *bad)
        with pytest.raises(ValueError):
            zipnn_amd.patch_place(whole, shape, dim, lo, hi)                     # a patch of the whole tensor where the shard's is expected
        with pytest.raises(ValueError):
            zipnn_amd.patch_select(torch.zeros(48, dtype=torch.uint8, device=whole.device), shape, dim, lo, hi)
    # nothing changed inside the shard
    tb, tt = _pair(2, (64, 64), rng, dev)
    tt = tb.clone()
    tt[40, 3] ^= 5
    assert zipnn_amd.patch_select(zipnn_amd.patch_build(tt, tb), (64, 64), 0, 0, 40) is None
    assert zipnn_amd.patch_select(zipnn_amd.patch_build(tt, tb), (64, 64), 0, 40, 41) is not None


def argument_errors(lib, dev):
    """The calls the host refuses before any launch (ValueError), for select and for place: an empty rectangle, a rectangle outside the tensor, an element size
    that is not eligible, 2^32 elements or more, misaligned or null pointers, a length below 32, an output that overlaps the input.  The output is untouched."""
    import pytest
    E = 2
    label, g, whole, want, placed = [r for r in prepared(E) if r[0] == "700x300-rows-3-650-cols-10-250/two-percent"][0]
    out = torch.full((max(len(want), len(placed)) + 64,), 0x11, dtype=torch.uint8, device=dev)
    op = out.data_ptr() + (-out.data_ptr()) % 16
    held = {}
    for place, src, res in ((False, whole, want), (True, want, placed)):
        p = on_device(src, dev)
        held[place] = p
        ok = (p.data_ptr(), p.numel(), E) + g[1:] + (op, len(res))
        bad = [ok[:5] + (5, 5) + ok[7:], ok[:7] + (20, 20) + ok[9:], ok[:5] + (650, 3) + ok[7:],                      # an empty rectangle
               ok[:6] + (701,) + ok[7:], ok[:8] + (301,) + ok[9:], ok[:5] + (700, 701) + ok[7:],                      # outside the tensor
               ok[:2] + (3,) + ok[3:], ok[:2] + (8,) + ok[3:], ok[:2] + (0,) + ok[3:],                                # the element size
               ok[:3] + (1 << 16, 1 << 16) + ok[5:], ok[:3] + (1 << 33, 1) + ok[5:], ok[:3] + (1 << 40, 1 << 40) + ok[5:],      # 2^32 elements or more
               ok[:3] + (0, 300, 0, 0) + ok[7:],                                                                      # no rows at all
               (0,) + ok[1:], ok[:9] + (0, len(res)),                                                                 # null pointers
               (p.data_ptr() + 2,) + ok[1:], ok[:9] + (op + 8, len(res)),                                             # misaligned
               (p.data_ptr(), 31) + ok[2:],                                                                           # shorter than a header
               ok[:9] + (p.data_ptr(), p.numel()), ok[:9] + (p.data_ptr() + 16, len(res))]                            # the output overlaps the input
        run, size = (lib.patch_place_batch_dev, lib.patch_place_size_batch_dev) if place else (lib.patch_select_batch_dev, lib.patch_select_size_batch_dev)
        for it in bad:
            with pytest.raises(ValueError):
                run([it])
            with pytest.raises(ValueError):
                run([ok, it])
        for it in bad[:14] + bad[15:16] + bad[17:18]:                            # (the size call ignores the output)
            with pytest.raises(ValueError):
                size([it[:9]])
        assert (out == 0x11).all()
        assert run([]) == [] and size([]) == []
    return out, op, E, g, held, want, placed
