"""Shared cases of the patch-merge tests (tests/test_patch_merge_simt.py on the emulated kernels, tests/test_gpu_patch_merge.py on the device): the XOR-merge of
two "znp1" patches by zn_patch_merge_batch_dev against its numpy restatement (tests/patch_merge_ref.py) and against the patch tests/patch_ref.py builds from
the two tensors the merge never sees — three byte strings that must be one.  Every case is three byte arrays (base, A, B): the inputs are patch(A over base) and
patch(B over base), the expected result patch(B over A)."""
import numpy as np
import torch

import patch_merge_ref as M
import patch_ref as R
import patch_util as PU

BLOCK = R.BLOCK
SIZES = PU.SIZES


def _rand(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8)


def _odd(rng, E, k):
    """k random element values with the lowest bit set: never zero, and v ^ 2 is neither zero nor v."""
    return (rng.integers(0, 256, size=k * E, dtype=np.uint8).view(R._UINT[E]) | 1).astype(R._UINT[E])


def _changed(base, E, idx, vals):
    out = base.copy()
    out.view(R._UINT[E])[np.asarray(idx, dtype=np.int64)] ^= vals
    return out


def merge_cases(E, seed=0):
    """-> [(label, base bytes, A bytes, B bytes)] for one element size."""
    rng = np.random.default_rng(7000 * E + seed)
    out = []
    for m in SIZES:
        base = _rand(rng, m * E)
        ev = np.arange(m) % 2 == 0
        if m >= 2:                                                               # A and B disjoint
            out.append((f"m{m}-disjoint", base, _changed(base, E, np.flatnonzero(ev), _odd(rng, E, int(ev.sum()))),
                        _changed(base, E, np.flatnonzero(~ev), _odd(rng, E, int((~ev).sum())))))
        a = _changed(base, E, [0, m - 1] if m > 1 else [0], _odd(rng, E, 2 if m > 1 else 1))
        out.append((f"m{m}-equal", base, a, a.copy()))                           # A == B: everything cancels
        out.append((f"m{m}-empty-b", base, a, base.copy()))                      # one side an empty patch
        out.append((f"m{m}-empty-a", base, base.copy(), a))
        va = _odd(rng, E, m)                                                     # every element changed in both: the even ones equal (they cancel), the odd ones not
        vb = np.where(ev, va, va ^ np.array(2, dtype=R._UINT[E])).astype(R._UINT[E])
        out.append((f"m{m}-all", base, _changed(base, E, np.arange(m), va), _changed(base, E, np.arange(m), vb)))
    m = 2 * BLOCK + 3
    base = _rand(rng, m * E)
    edge = [0, BLOCK - 1, BLOCK, 2 * BLOCK - 1]                                  # block offsets 0 and 65 535 of blocks 0 and 1
    v = _odd(rng, E, 4)
    out.append(("edges-one-input", base, _changed(base, E, edge, v), _changed(base, E, [77], _odd(rng, E, 1))))
    out.append(("edges-both-equal", base, _changed(base, E, edge + [5], np.append(v, _odd(rng, E, 1))), _changed(base, E, edge, v)))
    out.append(("edges-both-different", base, _changed(base, E, edge, v), _changed(base, E, edge, v ^ np.array(2, dtype=R._UINT[E]))))
    out.append(("straddle", base, _changed(base, E, [BLOCK - 1, BLOCK], _odd(rng, E, 2)), _changed(base, E, [BLOCK - 1, BLOCK, BLOCK + 1], _odd(rng, E, 3))))
    blk1 = np.arange(BLOCK, 2 * BLOCK)
    few = [3, 2 * BLOCK + 1]
    full = _changed(base, E, blk1, _odd(rng, E, BLOCK))
    out.append(("block-empty-in-a-full-in-b", base, _changed(base, E, few, _odd(rng, E, 2)), full))
    out.append(("block-full-in-a-empty-in-b", base, full, _changed(base, E, few, _odd(rng, E, 2))))
    mid = BLOCK + rng.choice(BLOCK, size=500, replace=False)                     # block 1 cancels entirely between two blocks that keep entries
    vm = _odd(rng, E, 500)
    out.append(("middle-block-cancels", base, _changed(base, E, np.concatenate(([9], mid, [2 * BLOCK + 2])), np.concatenate((_odd(rng, E, 1), vm, _odd(rng, E, 1)))),
                _changed(base, E, np.concatenate((mid, [11])), np.concatenate((vm, _odd(rng, E, 1))))))
    for k in range(E):                                                           # elements that differ in one byte only, for each byte position
        idx = np.array([3, BLOCK + 1, m - 1] + list(range(1000, 1040)))
        va = (rng.integers(1, 256, size=idx.size).astype(np.uint32) << (8 * k)).astype(R._UINT[E])
        vb = va.copy()
        vb[::2] ^= np.array(1 << (8 * k), dtype=R._UINT[E])                      # every other one differs from A's in that byte alone (and may equal the base's)
        out.append((f"one-byte-{k}", base, _changed(base, E, idx, va), _changed(base, E, idx, vb)))
    out.append(("two-percent",) + two_percent(E, m, rng, base))
    return out


def two_percent(E, m, rng, base=None):
    """A changes 2 % of the elements; B changes half of those — half of them to A's values, the others to different ones — and as many new ones."""
    base = _rand(rng, m * E) if base is None else base
    k = m // 50
    perm = rng.permutation(m)
    idx_a, new_b = perm[:k], perm[k:k + k // 2]
    shared = idx_a[:k // 2]
    same, diff = shared[:shared.size // 2], shared[shared.size // 2:]
    va = _odd(rng, E, k)
    a = _changed(base, E, idx_a, va)
    b = base.copy()
    bv, av = b.view(R._UINT[E]), a.view(R._UINT[E])
    bv[same] = av[same]
    bv[diff] = av[diff] ^ np.array(2, dtype=R._UINT[E])
    bv[new_b] ^= _odd(rng, E, new_b.size)
    # what the expected merge must hold, so that the case tests what it is named for
    xa, xb = (a ^ base).view(R._UINT[E]), (b ^ base).view(R._UINT[E])
    both = (xa != 0) & (xb != 0)
    assert (both & (xa == xb)).any(), "no cancelled element"
    assert (both & (xa != xb)).any(), "no surviving coincident element"
    assert ((xa != 0) & (xb == 0)).any() and ((xa == 0) & (xb != 0)).any(), "no entries from each side alone"
    return base, a, b


def inputs(case, E):
    """(label, base, A, B) -> (patch(A over base), patch(B over base), n, E, patch(B over A) or None)"""
    _, base, a, b = case
    return R.build(a, base, E, keep_empty=True), R.build(b, base, E, keep_empty=True), base.size, E, R.build(b, a, E)


def on_device(data, dev):
    return PU.on_device(np.frombuffer(data, dtype=np.uint8), dev)


def device_merge(lib, dev, items):
    """items: [(patch a bytes, patch b bytes, n, E)] -> their merges as bytes (None: everything cancels), by ONE zn_patch_merge_batch_dev call; capacities
    exactly the lengths zn_patch_merge_size_batch_dev gives, each output between canaries of 0xA5."""
    held = [(on_device(pa, dev), on_device(pb, dev)) for pa, pb, _, _ in items]
    args = [(a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), n, E) for (a, b), (_, _, n, E) in zip(held, items)]
    sizes = lib.patch_merge_size_batch_dev(args)
    offs, o = [], 256
    for n in sizes:
        offs.append(o)
        o += (n + 255) // 256 * 256 + 256
    arena = torch.full((o + 16,), 0xA5, dtype=torch.uint8, device=dev)
    a0 = (-arena.data_ptr()) % 16
    lens = lib.patch_merge_batch_dev([it + (arena.data_ptr() + a0 + off, n) for it, off, n in zip(args, offs, sizes)])
    assert lens == sizes
    host = arena.cpu().numpy()
    keep = np.ones(host.size, dtype=bool)
    for off, n in zip(offs, lens):
        keep[a0 + off: a0 + off + n] = False
    assert (host[keep] == 0xA5).all(), "a merge wrote outside its output"
    for (a, b), (pa, pb, _, _) in zip(held, items):
        assert bytes(a.cpu().numpy()) == pa and bytes(b.cpu().numpy()) == pb, "a merge changed an input"
    return [bytes(host[a0 + off: a0 + off + n]) if n else None for off, n in zip(offs, lens)]


_CASES = {}


def prepared(E):
    """The cases of one element size with their inputs and the expected merge, computed once: the two restatements must agree before they judge a kernel."""
    if E not in _CASES:
        rows = []
        for case in merge_cases(E):
            pa, pb, n, _, want = inputs(case, E)
            assert M.merge(pa, pb) == want, f"E={E} {case[0]}: the restated merge differs from the patch built from the two tensors"
            assert M.merge(pb, pa) == want
            rows.append((case[0], pa, pb, n, want))
        labels = [r[0] for r in rows]
        assert any(r[4] is None for r in rows) and len(set(labels)) == len(labels)
        _CASES[E] = rows
    return _CASES[E]


def check_merge(lib, dev, E):
    rows = prepared(E)
    got = device_merge(lib, dev, [(pa, pb, n, E) for _, pa, pb, n, _ in rows])
    for (label, pa, pb, n, want), g in zip(rows, got):
        assert g == want, f"E={E} {label}: the device's merge differs from the restatement"
    # symmetric: (pb, pa) gives the same bytes
    got = device_merge(lib, dev, [(pb, pa, n, E) for _, pa, pb, n, _ in rows])
    for (label, pa, pb, n, want), g in zip(rows, got):
        assert g == want, f"E={E} {label}: the merge is not symmetric"
    # the last case alone (it travels as the kernel's argument)
    label, pa, pb, n, want = rows[-1]
    assert device_merge(lib, dev, [(pa, pb, n, E)]) == [want]
    assert {"zn_k_patch_merge_count", "zn_k_patch_scan", "zn_k_patch_merge_emit"} <= set(lib.last_kernels().split(";"))


def check_ragged(lib, dev):
    """Mixed element sizes and a cancelling item in one call, in both orders."""
    rng = np.random.default_rng(11)
    items, want = [], []
    for E, m in ((2, 70001), (4, 12345), (1, 2 * BLOCK + 1), (2, 300), (4, BLOCK), (1, 1)):
        if m >= 1000:
            base, a, b = two_percent(E, m, rng)
        else:                                                                    # the small items cancel
            base = _rand(rng, m * E)
            a = _changed(base, E, [0], _odd(rng, E, 1))
            b = a.copy()
        items.append((R.build(a, base, E, keep_empty=True), R.build(b, base, E, keep_empty=True), base.size, E))
        want.append(R.build(b, a, E))
        assert M.merge(items[-1][0], items[-1][1]) == want[-1]
    assert want[3] is None and want[5] is None and want[0] is not None
    assert device_merge(lib, dev, items) == want
    assert device_merge(lib, dev, list(reversed(items))) == list(reversed(want))


def check_public(dev):
    """patch_apply_(t holding A, patch_merge(pa, pb)) gives B; equal patches give None; headers that disagree are refused."""
    import pytest
    import zipnn_amd
    for E in (1, 2, 4):
        dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[E]
        base, a, b = two_percent(E, BLOCK + 40, np.random.default_rng(21 + E))
        tb, ta, tB = (PU.on_device(x, dev).view(dt) for x in (base, a, b))
        pa, pb = zipnn_amd.patch_build(ta, tb), zipnn_amd.patch_build(tB, tb)
        pm = zipnn_amd.patch_merge(pa, pb)
        assert bytes(pm.cpu().numpy()) == R.build(b, a, E) == bytes(zipnn_amd.patch_build(tB, ta).cpu().numpy())
        live = ta.clone()
        assert zipnn_amd.patch_apply_(live, pm) is live and torch.equal(live, tB)
        zipnn_amd.patch_apply_(live, pm)
        assert torch.equal(live, ta)
        assert zipnn_amd.patch_merge(pa, pa.clone()) is None
        other = zipnn_amd.patch_build(tB[:-1].clone(), tb[:-1].clone())
        with pytest.raises(ValueError):
            zipnn_amd.patch_merge(pa, other)
    z, o = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    o[0] = 1
    p1 = zipnn_amd.patch_build(PU.on_device(o, dev).view(torch.int32), PU.on_device(z, dev).view(torch.int32))
    p2 = zipnn_amd.patch_build(PU.on_device(o, dev).view(torch.int16), PU.on_device(z, dev).view(torch.int16))
    with pytest.raises(ValueError):
        zipnn_amd.patch_merge(p1, p2)                                            # the same bytes in elements of another size
    with pytest.raises(ValueError):
        zipnn_amd.patch_merge(p1, torch.zeros(48, dtype=torch.uint8, device=dev))


def argument_errors(lib, dev):
    """The calls the host refuses before any launch (ValueError): an ineligible (n, elem), a null or misaligned pointer, a length below 32, an output that
    overlaps an input.  The output buffer is untouched."""
    import pytest
    E = 2
    _, pa, pb, n, want = prepared(E)[-1]
    a, b = on_device(pa, dev), on_device(pb, dev)
    out = torch.full((len(want) + 64,), 0x11, dtype=torch.uint8, device=dev)
    o0 = (-out.data_ptr()) % 16
    op = out.data_ptr() + o0
    ok = (a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), n, E, op, len(want))
    bad = [ok[:5] + (3,) + ok[6:], ok[:4] + (n - 1, E) + ok[6:], ok[:4] + (2 ** 33, 1) + ok[6:],       # (n, elem) not eligible
           (0,) + ok[1:], ok[:2] + (0,) + ok[3:], ok[:6] + (0, len(want)),                              # null pointers
           (a.data_ptr() + 2,) + ok[1:], ok[:2] + (b.data_ptr() + 8,) + ok[3:], ok[:6] + (op + 1, len(want)),      # misaligned
           (a.data_ptr(), 31) + ok[2:], ok[:3] + (16,) + ok[4:],                                        # shorter than a header
           ok[:6] + (a.data_ptr(), a.numel()), ok[:6] + (b.data_ptr() + 16, len(want))]                 # the output overlaps an input
    for it in bad:
        with pytest.raises(ValueError):
            lib.patch_merge_batch_dev([it])
        with pytest.raises(ValueError):
            lib.patch_merge_batch_dev([ok, it])
    for it in bad[:5] + bad[6:8] + bad[9:11]:                                    # (the size call ignores the output)
        with pytest.raises(ValueError):
            lib.patch_merge_size_batch_dev([it[:6]])
    assert (out == 0x11).all()
    assert lib.patch_merge_batch_dev([]) == [] and lib.patch_merge_size_batch_dev([]) == []
    return ok, out, want, (a, b)                                                 # (the inputs stay alive with the item that names them)
