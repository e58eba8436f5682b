"""Shared cases of the patch tests (tests/test_patch_simt.py on the emulated kernels, tests/test_gpu_patch.py on the device): "znp1" patches built by
zn_patch_build_batch_dev against tests/patch_ref.py byte for byte, and applied — whole tensors, windows, in place and over a base — against its apply."""
import numpy as np
import torch

import patch_ref as R

BLOCK = R.BLOCK
SIZES = (1, 65535, 65536, 65537, 2 * 65536 + 3)


def _rand(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8)


def _flip(src, E, elems, rng, byte=None):
    """Change the given elements of src (bytes, in place): every byte (a value that differs in each), or only byte position `byte`."""
    for e in elems:
        for k in (range(E) if byte is None else (byte,)):
            src[e * E + k] ^= int(rng.integers(1, 256))


def build_cases(E, seed=0, matrix=True):
    """-> [(label, source bytes, base bytes)] — the build's cases for one element size: the sizes x T matrix (matrix=False: only its odd sizes), then the
    structural ones."""
    rng = np.random.default_rng(1000 * E + seed)
    out = []
    for m in (SIZES if matrix else (1, 65537)):
        base = _rand(rng, m * E)
        out.append((f"m{m}-T0", base.copy(), base))
        for label, el in (("first", [0]), ("last", [m - 1])):
            s = base.copy()
            _flip(s, E, el, rng)
            out.append((f"m{m}-{label}", s, base))
        s = base ^ np.uint8(0xFF)                                                # every element differs
        out.append((f"m{m}-all", s, base))
    m = 3 * BLOCK + 7
    base = _rand(rng, m * E)
    s = base.copy()
    _flip(s, E, [0, BLOCK - 1], rng)                                             # block offsets 0 and 65 535
    out.append(("offsets-0-65535", s, base))
    s = base.copy()
    _flip(s, E, [BLOCK - 1, BLOCK], rng)                                         # a pair that straddles a block edge
    out.append(("straddle", s, base))
    s = base.copy()
    _flip(s, E, [5, 77, 2 * BLOCK + 9, 3 * BLOCK + 6], rng)                      # block 1 empty between two that are not
    out.append(("empty-block", s, base))
    for k in range(E):                                                           # elements that differ in one byte only
        s = base.copy()
        _flip(s, E, [3, BLOCK + 1, m - 1] + list(range(1000, 1000 + 40)), rng, byte=k)
        out.append((f"one-byte-{k}", s, base))
    s = base.copy()
    idx = rng.choice(m, size=m // 50, replace=False)                             # 2 % at random places
    _flip(s, E, idx.tolist(), rng)
    out.append(("two-percent", s, base))
    return out


def on_device(arr, dev, shift=0):
    """numpy bytes -> a uint8 tensor on dev whose address is `shift` bytes behind a 16-byte aligned one."""
    buf = torch.empty(arr.size + 64, dtype=torch.uint8, device=dev)
    o = (-buf.data_ptr()) % 16 + shift
    t = buf[o:o + arr.size]
    t.copy_(torch.from_numpy(np.array(arr, dtype=np.uint8)).to(dev))
    assert (t.data_ptr() - shift) % 16 == 0
    return t


def device_build(lib, dev, pairs, shifts=(0, 0)):
    """pairs: [(source bytes, base bytes, E)] -> their patches as bytes (None: identical), by ONE zn_patch_build_batch_dev call; capacities exactly the lengths
    zn_patch_size_batch_dev gives, each patch between canaries."""
    srcs = [on_device(s, dev, shifts[0] * E) for s, _, E in pairs]
    bases = [on_device(b, dev, shifts[1] * E) for _, b, E in pairs]
    items = [(s.data_ptr() if s.numel() else 0, b.data_ptr() if s.numel() else 0, s.numel(), E) for s, b, (_, _, E) in zip(srcs, bases, pairs)]
    sizes = lib.patch_size_batch_dev(items)
    offs, o = [], 256
    for n in sizes:
        offs.append(o)
        o += (n + 255) // 256 * 256 + 256
    arena = torch.full((o + 16,), 0xA5, dtype=torch.uint8, device=dev)
    a0 = (-arena.data_ptr()) % 16
    lens = lib.patch_build_batch_dev([it + (arena.data_ptr() + a0 + off, n) for it, off, n in zip(items, offs, sizes)])
    assert lens == sizes
    host = arena.cpu().numpy()
    keep = np.ones(host.size, dtype=bool)
    for off, n in zip(offs, lens):
        keep[a0 + off: a0 + off + n] = False
    assert (host[keep] == 0xA5).all(), "a build wrote outside its patch"
    return [bytes(host[a0 + off: a0 + off + n]) if n else None for off, n in zip(offs, lens)]


def check_build(lib, dev, E, shifts=(0, 0)):
    cases = build_cases(E, matrix=shifts == (0, 0))
    got = device_build(lib, dev, [(s, b, E) for _, s, b in cases], shifts)
    for (label, s, b), g in zip(cases, got):
        want = R.build(s, b, E)
        assert g == want, f"E={E} {label} shifts={shifts}: the device's patch differs from the restatement"
        if want is not None:
            assert len(want) == lib.patch_len(s.size, E, R.parse(want)[2])
    # one item alone (it travels as the kernel's argument)
    label, s, b = cases[-1]
    assert device_build(lib, dev, [(s, b, E)], shifts) == [R.build(s, b, E)]


def check_ragged(lib, dev):
    """Mixed element sizes, a zero-length item and an identical item in one call."""
    rng = np.random.default_rng(5)
    pairs = []
    for E, m in ((2, 70001), (1, 0), (4, 12345), (2, 300), (1, 2 * BLOCK + 1), (4, BLOCK)):
        b = _rand(rng, m * E)
        s = b.copy()
        if m and m != 300:                                                       # (the 300-element item stays identical)
            _flip(s, E, rng.choice(m, size=max(m // 40, 1), replace=False).tolist(), rng)
        pairs.append((s, b, E))
    got = device_build(lib, dev, pairs)
    assert got == [R.build(s, b, E) for s, b, E in pairs]
    assert got[1] is None and got[3] is None and got[0] is not None
    assert device_build(lib, dev, list(reversed(pairs))) == list(reversed(got))


def apply_pair(E, m=BLOCK + 40, seed=3):
    rng = np.random.default_rng(seed + E)
    base = _rand(rng, m * E)
    src = base.copy()
    _flip(src, E, sorted(set(rng.choice(m, size=60, replace=False).tolist()) | {0, BLOCK - 1, BLOCK, m - 1}), rng)
    return src, base, R.build(src, base, E)


def canaried(arr, dev, E):
    """numpy bytes -> (buffer, view): the bytes between two 64-byte canaries of 0x5C, the view E-aligned."""
    buf = torch.full((arr.size + 128 + 16,), 0x5C, dtype=torch.uint8, device=dev)
    o = (-buf.data_ptr()) % 16 + 64
    buf[o:o + arr.size] = torch.from_numpy(np.array(arr, dtype=np.uint8)).to(dev)
    return buf, buf[o:o + arr.size], o


def canaries_intact(buf, o, n):
    h = buf.cpu().numpy()
    return bool((h[:o] == 0x5C).all() and (h[o + n:] == 0x5C).all())


def check_apply_whole(lib, dev):
    import zipnn_amd
    for E in (1, 2, 4):
        src, base, patch = apply_pair(E)
        p = on_device(np.frombuffer(patch, dtype=np.uint8), dev)
        buf, view, o = canaried(base, dev, E)
        n = base.size
        lib.patch_apply_batch_dev([(p.data_ptr(), p.numel(), n, E, 0, n, view.data_ptr())])
        assert bytes(view.cpu().numpy()) == bytes(src) == bytes(R.apply(base, patch))
        lib.patch_apply_batch_dev([(p.data_ptr(), p.numel(), n, E, 0, n, view.data_ptr())])
        assert bytes(view.cpu().numpy()) == bytes(base)                          # twice: the base again
        assert canaries_intact(buf, o, n)
        # over a base that lies elsewhere
        bt = on_device(base, dev)
        buf2, view2, o2 = canaried(np.zeros(n, dtype=np.uint8), dev, E)
        lib.patch_apply_batch_dev([(p.data_ptr(), p.numel(), n, E, 0, n, view2.data_ptr(), bt.data_ptr())])
        assert bytes(view2.cpu().numpy()) == bytes(src) and bytes(bt.cpu().numpy()) == bytes(base) and canaries_intact(buf2, o2, n)
        # a patch with no entries, and an empty window
        empty = on_device(np.frombuffer(R.build(base, base, E, keep_empty=True), dtype=np.uint8), dev)
        lib.patch_apply_batch_dev([(empty.data_ptr(), empty.numel(), n, E, 0, n, view.data_ptr()), (p.data_ptr(), p.numel(), n, E, E, E, 0)])
        assert bytes(view.cpu().numpy()) == bytes(base)
        # the public pair of functions
        dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[E]
        ts, tb = on_device(src, dev).view(dt), on_device(base, dev).view(dt)
        pt = zipnn_amd.patch_build(ts, tb)
        assert bytes(pt.cpu().numpy()) == patch and zipnn_amd.patch_build(tb, tb.clone()) is None
        live = tb.clone()
        assert zipnn_amd.patch_apply_(live, pt) is live and torch.equal(live, ts)
        zipnn_amd.patch_apply_(live, pt)
        assert torch.equal(live, tb) and zipnn_amd.patch_apply_(live, None) is live


def check_apply_windows(lib, dev, E=2):
    """Every window between a set of element bounds (mid-block, at block edges, empty ones), d_base set and NULL in turn — one batched launch, and the same
    through a patch plan run twice."""
    src, base, patch = apply_pair(E)
    m = base.size // E
    p = on_device(np.frombuffer(patch, dtype=np.uint8), dev)
    bt = on_device(base, dev)
    bounds = [0, 1, 7, BLOCK - 1, BLOCK, BLOCK + 1, m - 1, m]
    wins = [(lo * E, hi * E) for i, lo in enumerate(bounds) for hi in bounds[i:]]
    for use_plan in (False, True):
        items, held = [], []
        for k, (lo, hi) in enumerate(wins):
            with_base = k % 2 == 0
            start = np.zeros(hi - lo, dtype=np.uint8) if with_base else base[lo:hi]
            buf, view, o = canaried(start, dev, E)
            held.append((buf, view, o, lo, hi, with_base))
            items.append((p.data_ptr(), p.numel(), base.size, E, lo, hi, view.data_ptr() if hi > lo else 0) + ((bt.data_ptr(),) if with_base else ()))
        if use_plan:
            h = lib.patch_plan_create(items)
            lib.patch_plan_run(h, 0, True)
        else:
            lib.patch_apply_batch_dev(items)
        for buf, view, o, lo, hi, _ in held:
            assert bytes(view.cpu().numpy()) == bytes(src[lo:hi]) == bytes(R.apply(base[lo:hi], patch, lo, hi)), (lo, hi)
            assert canaries_intact(buf, o, hi - lo), (lo, hi)
        if use_plan:
            lib.patch_plan_run(h, 0, False)                                      # a second run: in-place items go back to the base, items over a base are the same again
            lib.decode_status()
            for buf, view, o, lo, hi, with_base in held:
                assert bytes(view.cpu().numpy()) == bytes(src[lo:hi] if with_base else base[lo:hi]) and canaries_intact(buf, o, hi - lo)
            lib.patch_plan_destroy(h)
    assert "zn_k_patch_apply" in lib.last_kernels()
