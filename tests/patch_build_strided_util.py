"""Shared cases of the strided-build tests (tests/test_patch_build_strided_simt.py on the emulated kernels, tests/test_gpu_patch_build_strided.py on the device):
"znp1" patches built from strided views of live memory (zn_patch_size_strided_batch_dev / zn_patch_build_strided_batch_dev).  The layouts, the
views inside sentinel-filled buffers (Live) and the patches' kinds are those of tests/patch_strided_util.py, unchanged; the oracle is the numpy restatement
tests/patch_ref.py on the LOGICAL row-major bytes.  Every patch is built into an allocation of exactly its length inside a sentinel-filled buffer, and after
each call the tensors' whole buffers are compared with what they held."""
import numpy as np
import torch

import patch_ref as R
import patch_strided_util as S
import patch_util as U

LAYOUTS, KINDS, Live, DT, NP, SENTINEL = S.LAYOUTS, S.KINDS, S.Live, S.DT, S.NP, S.SENTINEL
SIDES = ("source", "base", "both")                   # which side lies in the layout; the other is contiguous
STRIDED = {"zn_k_patch_count_strided", "zn_k_patch_scan", "zn_k_patch_emit_strided"}
PLAIN = {"zn_k_patch_count", "zn_k_patch_scan", "zn_k_patch_emit"}
kernels = S.kernels


def pair_bytes(E, m, kind, rng):
    """-> (new bytes, base bytes, the oracle's patch or None) for a tensor of m elements (tests/patch_strided_util.py's kinds)."""
    base, patch = S.make_patch(E, m, kind, rng)
    new = R.apply(base, patch) if m else base.copy()
    return new, base, R.build(new, base, E)


def plain(shape):
    """-> the `make` of a contiguous tensor of this shape"""
    return lambda s: s.view(tuple(shape))


def item(src, base):
    """two Lives over one logical shape -> the item of ZnLib.patch_size_strided_batch_dev"""
    m, E = src.view.numel(), src.E
    assert tuple(src.view.shape) == tuple(base.view.shape) and base.E == E
    return (src.view.data_ptr() if m else 0, base.view.data_ptr() if m else 0, m * E, E, tuple(src.view.shape), tuple(src.view.stride()), tuple(base.view.stride()))


class Out:
    """An allocation of exactly n bytes at a 16-byte aligned address inside a sentinel-filled buffer on dev."""

    def __init__(self, dev, n):
        self.buf = torch.full((n + 144,), SENTINEL, dtype=torch.uint8, device=dev)
        self.at = (-self.buf.data_ptr()) % 16 + 64
        self.n = n
        self.ptr = self.buf.data_ptr() + self.at

    def bytes(self):
        return self.buf[self.at:self.at + self.n].cpu().numpy().tobytes()

    def around_intact(self):
        h = self.buf.cpu().numpy()
        return bool((h[:self.at] == SENTINEL).all() and (h[self.at + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def build(lib, pairs):
    """pairs: [(source Live, base Live)] -> their patches as bytes (None: identical) by one size call and one build call, with everything the calls promise
    asserted: sizes_out equals the built lengths, each patch fills an allocation of exactly its length and leaves the sentinels around it, and both tensors'
    buffers are byte-identical afterwards."""
    items = [item(s, b) for s, b in pairs]
    before = [(s.bytes(), b.bytes()) for s, b in pairs]
    dev = pairs[0][0].buf.device
    sizes = lib.patch_size_strided_batch_dev(items)
    seen = kernels(lib)
    outs = [Out(dev, n) for n in sizes]
    lens = lib.patch_build_strided_batch_dev([it + (o.ptr, o.n) for it, o in zip(items, outs)])
    seen |= kernels(lib)
    assert lens == sizes
    for (s, b), (sb, bb), o in zip(pairs, before, outs):
        assert o.around_intact()
        assert s.bytes() == sb and b.bytes() == bb
    return [o.bytes() if o.n else None for o in outs], seen


def contiguous_build(lib, dev, new, base, E):
    """-> what zn_patch_build_batch_dev gives for the contiguous bytes"""
    return U.device_build(lib, dev, [(new, base, E)])[0]


def sides(dev, E, storage, make, new, base, side):
    shape = tuple(make(torch.empty(storage, dtype=DT[E])).shape)
    m = len(bytes(base)) // E
    lay = lambda data: Live(dev, E, storage, make, data)                      # noqa: E731
    flat = lambda data: Live(dev, E, m, plain(shape), data)                   # noqa: E731
    return (lay(new) if side != "base" else flat(new)), (lay(base) if side != "source" else flat(base))


def check_layouts(lib, dev, E):
    """Every layout x kind of change x side through the C calls: the oracle's bytes, which are zn_patch_build_batch_dev's for contiguous copies.
    -> {(label, kind, side): the patch's bytes}"""
    rng = np.random.default_rng(1600 + E)
    out = {}
    for label, storage, make in LAYOUTS:
        m = make(torch.empty(storage, dtype=DT[E])).numel()
        for kind in KINDS:
            new, base, want = pair_bytes(E, m, kind, rng)
            ref = contiguous_build(lib, dev, new, base, E)
            assert ref == want
            for side in SIDES:
                src, bas = sides(dev, E, storage, make, new, base, side)
                (got,), seen = build(lib, [(src, bas)])
                assert got == want, (E, label, kind, side)
                if m > 1 and label != "contiguous":
                    assert seen == (STRIDED if want is not None else STRIDED - {"zn_k_patch_emit_strided"}), (label, kind, side, seen)
                out[(label, kind, side)] = got
    return out


def check_two_layouts(lib, dev, E):
    """A transposed source against a tile-shuffled base, both seen as the logical shape (16, 16, 10, 32): 81 920 elements, two blocks."""
    rng = np.random.default_rng(1610 + E)
    storage = 256 * 320
    new, base, want = pair_bytes(E, storage, "dense", rng)
    src = Live(dev, E, storage, lambda s: s.view(320, 256).t().view(16, 16, 10, 32), new)
    bas = Live(dev, E, storage, lambda s: s.view(16, 10, 16, 32).permute(0, 2, 1, 3), base)
    (got,), seen = build(lib, [(src, bas)])
    assert got == want and seen == STRIDED
    return got


def check_mixed_batch(lib, dev):
    """One call: every layout, the element sizes and the sides in turn — exactly the three strided kernels; a batch that collapses entirely: the contiguous ones."""
    rng = np.random.default_rng(1620)
    pairs, wants = [], []
    for k, (label, storage, make) in enumerate(LAYOUTS):
        E = (1, 2, 4)[k % 3]
        m = make(torch.empty(storage, dtype=DT[E])).numel()
        new, base, want = pair_bytes(E, m, KINDS[(k + k // 3) % 3], rng)
        pairs.append(sides(dev, E, storage, make, new, base, SIDES[(k + 2 * (k // 3)) % 3]))
        wants.append(want)
    got, seen = build(lib, pairs)
    assert got == wants
    assert seen == STRIDED
    # size-1 dimensions and a zero-dim tensor collapse; so does a contiguous tensor seen through an unflattened view
    flat = []
    for E, storage, make in ((2, 70001, lambda s: s.view(1, 70001, 1)), (4, 1, lambda s: s.view(())), (1, 2160, lambda s: s.view(2, 3, 2, 3, 2, 3, 2, 5)), (2, 0, lambda s: s.view(0, 5))):
        new, base, want = pair_bytes(E, storage, "dense", rng)
        flat.append((Live(dev, E, storage, make, new), Live(dev, E, storage, make, base), want))
    got, seen = build(lib, [(s, b) for s, b, _ in flat])
    assert got == [w for _, _, w in flat]
    assert seen == PLAIN
    return got


def check_cap(lib, dev):
    """One short capacity: ZN_E_CAP, every needed length, nothing written anywhere."""
    import pytest
    from zipnn_amd._capi import ZN_E_CAP, ZnError
    rng = np.random.default_rng(1630)
    E = 2
    pairs = []
    for label, storage, make in LAYOUTS[:3]:
        new, base, _ = pair_bytes(E, make(torch.empty(storage, dtype=DT[E])).numel(), "dense", rng)
        pairs.append(sides(dev, E, storage, make, new, base, "source"))
    items = [item(s, b) for s, b in pairs]
    sizes = lib.patch_size_strided_batch_dev(items)
    assert all(sizes)
    outs = [Out(dev, n) for n in sizes]
    with pytest.raises(ZnError) as ei:
        lib.patch_build_strided_batch_dev([it + (o.ptr, o.n - (16 if k == 1 else 0)) for k, (it, o) in enumerate(zip(items, outs))])
    assert ei.value.status == ZN_E_CAP and ei.value.needed == sizes
    assert all(o.untouched() for o in outs)
    assert kernels(lib) == STRIDED - {"zn_k_patch_emit_strided"}


def check_refusals(lib, dev):
    """What the host refuses before any launch (ValueError: ZN_E_ARG), alone and as the second item of a batch; nothing is written."""
    import pytest
    E = 2
    rng = np.random.default_rng(1640)
    label, storage, make = LAYOUTS[0]                                             # transposed: logical (300, 257)
    new, base, _ = pair_bytes(E, storage, "dense", rng)
    src, bas = sides(dev, E, storage, make, new, base, "source")
    ok = item(src, bas)
    size = lib.patch_size_strided_batch_dev([ok])[0]
    out = Out(dev, size + 64)
    good = ok + (out.ptr, out.n)
    sp, bp, n, el, sizes, ss, bs = ok
    last = src.view[299, 256].data_ptr()
    span = (src.view.numel() - 1) * E                                             # the transposed view covers its storage: first to last element
    bad = [("nine dimensions", (sp, bp, 512 * E, el, (2,) * 9, (1,) * 9, (1,) * 9, out.ptr, out.n)),
           ("a product below m", (sp, bp, n, el, (300, 256), ss, bs, out.ptr, out.n)),
           ("a product above m", (sp, bp, n, el, (300, 258), ss, bs, out.ptr, out.n)),
           ("a negative source stride", (last, bp, n, el, sizes, (-1, -300), bs, out.ptr, out.n)),
           ("a negative base stride", (sp, bp, n, el, sizes, ss, (-257, 1), out.ptr, out.n)),
           ("a source that reaches 2^62 elements", (sp, bp, 2 * E, el, (2,), (1 << 62,), (1,), out.ptr, out.n)),
           ("a base that reaches 2^62 elements", (sp, bp, 2 * E, el, (2,), (1,), (1 << 62,), out.ptr, out.n)),
           ("a misaligned source", (sp + 1, bp, n, el, sizes, ss, bs, out.ptr, out.n)),
           ("a misaligned base", (sp, bp + 1, n, el, sizes, ss, bs, out.ptr, out.n)),
           ("a null source", (0, bp, n, el, sizes, ss, bs, out.ptr, out.n)),
           ("an element size of 3", (sp, bp, n, 3, sizes, ss, bs, out.ptr, out.n)),
           ("a patch that is not 16-byte aligned", (sp, bp, n, el, sizes, ss, bs, out.ptr + 8, out.n - 8)),
           ("a patch inside the source's span", (sp, bp, n, el, sizes, ss, bs, (sp + span // 2) // 16 * 16, 64)),
           ("a patch over the source's last element", (sp, bp, n, el, sizes, ss, bs, (sp + span) // 16 * 16, 64)),
           ("a patch inside the base's span", (sp, bp, n, el, sizes, ss, bs, (bp + span // 2) // 16 * 16, 64))]
    sb, bb = src.bytes(), bas.bytes()
    for why, it in bad:
        for batch in ([it], [good, it]):
            with pytest.raises(ValueError):
                lib.patch_build_strided_batch_dev(batch)
            assert out.untouched(), why
        if it[7] == out.ptr:                                                      # the size call refuses what does not concern the output
            with pytest.raises(ValueError):
                lib.patch_size_strided_batch_dev([it[:7]])
            with pytest.raises(ValueError):
                lib.patch_size_strided_batch_dev([ok, it[:7]])
    assert out.untouched() and src.bytes() == sb and bas.bytes() == bb
    assert lib.patch_build_strided_batch_dev([]) == [] and lib.patch_size_strided_batch_dev([]) == []
    assert lib.patch_build_strided_batch_dev([good]) == [size]                    # … and the good item alone is served


def check_expand(lib, dev):
    """An expand()ed source (a stride of 0) and an overlapping one are read like any other: the oracle's patch of their materialised bytes."""
    rng = np.random.default_rng(1650)
    got = []
    for E in (1, 2, 4):
        row = torch.from_numpy(rng.integers(0, 256, size=300 * E, dtype=np.uint8)).view(DT[E]).to(dev)
        buf = torch.from_numpy(rng.integers(0, 256, size=1000 * E, dtype=np.uint8)).view(DT[E]).to(dev)
        for view in (row.view(1, 300).expand(257, 300), torch.as_strided(buf, (257, 300), (2, 1))):
            base = torch.from_numpy(rng.integers(0, 256, size=257 * 300 * E, dtype=np.uint8)).view(DT[E]).view(257, 300).to(dev)
            base[::3] = view[::3]                                                 # a third of the rows is the source's
            want = R.build(view.contiguous().cpu().numpy(), base.cpu().numpy(), E)
            it = (view.data_ptr(), base.data_ptr(), 257 * 300 * E, E, (257, 300), tuple(view.stride()), tuple(base.stride()))
            size = lib.patch_size_strided_batch_dev([it])[0]
            out = Out(dev, size)
            assert lib.patch_build_strided_batch_dev([it + (out.ptr, out.n)]) == [size]
            assert out.bytes() == want and out.around_intact()
            got.append(out.bytes())
    return got


def check_public(lib, dev):
    """zipnn_amd.patch_build on views (the package's library is `lib`): the strided kernels, no copy; the round trip through patch_apply_ on the same views;
    two contiguous tensors take the contiguous launches as before."""
    import zipnn_amd
    rng = np.random.default_rng(1660)
    for E in (1, 2, 4):
        for label, storage, make in LAYOUTS:
            m = make(torch.empty(storage, dtype=DT[E])).numel()
            new, base, want = pair_bytes(E, m, "dense", rng)
            src, live = Live(dev, E, storage, make, new), Live(dev, E, storage, make, base)
            p = zipnn_amd.patch_build(src.view, live.view)
            if m > 1 and label != "contiguous":
                assert kernels(lib) == STRIDED, (label, kernels(lib))             # read where they lie: the contiguous kernels would mean a copy was made
            elif m:
                assert kernels(lib) == PLAIN
            assert (p.cpu().numpy().tobytes() if p is not None else None) == want, (E, label)
            assert zipnn_amd.patch_apply_(live.view, p) is live.view
            assert live.bytes() == src.bytes(), (E, label)                        # the view that held the base holds the new bytes; nothing around it moved
            # a new checkpoint tensor (contiguous) against the live view, and back
            live2 = Live(dev, E, storage, make, base)
            fresh = torch.from_numpy(np.array(new)).view(DT[E]).reshape(tuple(live2.view.shape)).to(dev) if m else torch.empty(tuple(live2.view.shape), dtype=DT[E], device=dev)
            p2 = zipnn_amd.patch_build(fresh, live2.view)
            assert (p2.cpu().numpy().tobytes() if p2 is not None else None) == want
            zipnn_amd.patch_apply_(live2.view, p2)
            assert live2.bytes() == src.bytes()
