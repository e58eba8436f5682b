"""Shared cases of the strided-apply tests (tests/test_patch_strided_simt.py on the emulated kernels, tests/test_gpu_patch_strided.py on the device): "znp1"
patches applied through strided views of live memory (zn_patch_apply_strided_batch_dev).  The oracle is the numpy restatement tests/patch_ref.py
applied to the LOGICAL row-major array.  Every view lies inside a larger sentinel-filled buffer at a non-zero, odd-element storage offset; after each call the
WHOLE buffer is compared: the view's elements hold the oracle's bytes and every other byte is the sentinel or what the storage held before."""
import struct

import numpy as np
import torch

import patch_ref as R
import patch_util as U

BLOCK = R.BLOCK
SENTINEL = 0x5C
OFFSET = 33                                          # elements in front of the storage: odd, so that no view starts 16-byte aligned by accident
PAD = 64
DT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
NP = {1: np.uint8, 2: np.dtype("<u2"), 4: np.dtype("<u4")}

# (label, storage elements, storage (1-D) -> the view whose logical row-major order is the tensor's): the smallest shapes that cross a block edge with a partial last block
LAYOUTS = [
    ("transposed", 257 * 300, lambda s: s.view(257, 300).t()),                                   # m = 77 100
    ("narrow", 130 * 1031, lambda s: s.view(130, 1031)[:, 17:534]),                              # m = 67 210; rows of 517 elements: not 16-byte aligned
    ("permute3", 6 * 11 * 1021, lambda s: s.view(6, 11, 1021).permute(2, 0, 1)),
    ("tile-shuffle", 256 * 320, lambda s: s.view(16, 10, 16, 32).permute(0, 2, 1, 3)),           # logical (256, 320) stored as view(16,16,10,32).permute(0,2,1,3).contiguous()
    ("eight-dims", 2160, lambda s: s.view(2, 3, 2, 3, 2, 3, 2, 5).permute(7, 6, 5, 4, 3, 2, 1, 0)),      # does not collapse
    ("zero-dim", 1, lambda s: s.view(())),
    ("size-1-dims", 257 * 300, lambda s: s.view(1, 257, 1, 300).permute(0, 3, 2, 1)),
    ("empty", 0, lambda s: s.view(0, 5)),
    ("contiguous", 70001, lambda s: s),
]
KINDS = ("edges", "dense", "empty")


class Live:
    """One view inside its sentinel-filled buffer on `dev`, holding `logical` (the tensor's bytes in row-major order)."""

    def __init__(self, dev, E, storage, make, logical):
        total = storage + OFFSET + PAD
        fill = int.from_bytes(bytes([SENTINEL]) * E, "little", signed=False)
        host = np.full(total, fill, dtype=NP[E])
        self.pos = make(torch.arange(total, dtype=torch.int64)[OFFSET:OFFSET + storage]).reshape(-1).numpy()      # logical element -> buffer element
        host[self.pos] = np.frombuffer(bytes(logical), dtype=NP[E])
        self.E, self.before = E, host
        self.buf = torch.from_numpy(host.view(np.uint8).copy()).to(dev).view(DT[E])
        self.view = make(self.buf[OFFSET:OFFSET + storage])
        assert self.view.numel() * E == len(bytes(logical))

    def item(self, p):
        """-> the item of ZnLib.patch_apply_strided_batch_dev for patch tensor p"""
        m = self.view.numel()
        return (p.data_ptr(), p.numel(), m * self.E, self.E, self.view.data_ptr() if m else 0, tuple(self.view.shape), tuple(self.view.stride()))

    def bytes(self):
        return self.buf.cpu().numpy().view(np.uint8).tobytes()

    def outside_intact(self):
        """Is every byte that is not an element of the view what it was?"""
        outside = np.ones(self.before.size, dtype=bool)
        outside[self.pos] = False
        return bool((np.frombuffer(self.bytes(), dtype=NP[self.E])[outside] == self.before[outside]).all())

    def expect(self, patches):
        """-> the buffer's bytes after these patches were applied to the logical array, by the oracle"""
        h = self.before.copy()
        logical = np.ascontiguousarray(h[self.pos]).view(np.uint8)
        for patch in patches:
            logical = R.apply(logical, patch)
        h[self.pos] = logical.view(NP[self.E])
        return h.view(np.uint8).tobytes()


def make_patch(E, m, kind, rng):
    """-> (base bytes, patch bytes) for a tensor of m elements: entries at elements 0, 65 535, 65 536 and m - 1 (those that exist), about 30 % of the elements, or none."""
    base = rng.integers(0, 256, size=m * E, dtype=np.uint8)
    src = base.copy()
    if kind == "edges":
        U._flip(src, E, sorted({e for e in (0, BLOCK - 1, BLOCK, m - 1) if 0 <= e < m}), rng)
    elif kind == "dense" and m:
        U._flip(src, E, np.flatnonzero(rng.random(m) < 0.3).tolist() or [0], rng)
    return base, R.build(src, base, E, keep_empty=True)


def kernels(lib):
    return {k for k in lib.last_kernels().split(";") if k}


def check_layouts(lib, dev, E, public):
    """Every layout x every kind of patch through the C call: the oracle's bytes, the rest of the buffer untouched, and the first bytes again after a second
    call; the dense patch through zipnn_amd.patch_apply_ as well (public: the package's library is `lib`).  -> {(label, kind): the buffer's bytes after one apply}"""
    import zipnn_amd
    rng = np.random.default_rng(700 + E)
    out = {}
    for label, storage, make in LAYOUTS:
        m = make(torch.empty(storage, dtype=DT[E])).numel()
        for kind in KINDS:
            base, patch = make_patch(E, m, kind, rng)
            live = Live(dev, E, storage, make, base)
            p = U.on_device(np.frombuffer(patch, dtype=np.uint8), dev)
            lib.patch_apply_strided_batch_dev([live.item(p)])
            got = live.bytes()
            assert got == live.expect([patch]), (E, label, kind)
            if m and kind != "empty":
                assert got != live.expect([])
            out[(label, kind)] = got
            lib.patch_apply_strided_batch_dev([live.item(p)], 0, False)          # twice: the bytes that were there; unchecked: the verdict waits in the status slot
            lib.decode_status()
            assert live.bytes() == live.expect([]), (E, label, kind)
            if public and kind == "dense":
                assert zipnn_amd.patch_apply_(live.view, p) is live.view
                assert live.bytes() == got, (E, label, "patch_apply_")
        if label == "contiguous":                                                # … which equals the contiguous call
            base, patch = make_patch(E, m, "dense", rng)
            p = U.on_device(np.frombuffer(patch, dtype=np.uint8), dev)
            one, two = Live(dev, E, storage, make, base), Live(dev, E, storage, make, base)
            lib.patch_apply_batch_dev([(p.data_ptr(), p.numel(), m * E, E, 0, m * E, one.view.data_ptr())])
            lib.patch_apply_strided_batch_dev([two.item(p)])
            assert one.bytes() == two.bytes() == one.expect([patch])
            assert kernels(lib) == {"zn_k_patch_apply"}                         # every layout of the batch collapsed: the contiguous launch
    return out


def check_mixed_batch(lib, dev):
    """One call: every layout, the element sizes in turn, all kinds of patch."""
    rng = np.random.default_rng(71)
    held, items = [], []
    for k, (label, storage, make) in enumerate(LAYOUTS):
        E = (1, 2, 4)[k % 3]
        m = make(torch.empty(storage, dtype=DT[E])).numel()
        base, patch = make_patch(E, m, KINDS[k % 2], rng)
        live = Live(dev, E, storage, make, base)
        p = U.on_device(np.frombuffer(patch, dtype=np.uint8), dev)
        held.append((label, live, patch, p))
        items.append(live.item(p))
    lib.patch_apply_strided_batch_dev(items)
    assert kernels(lib) == {"zn_k_patch_apply_strided"}                        # one launch for the batch
    for label, live, patch, _ in held:
        assert live.bytes() == live.expect([patch]), label
    lib.patch_apply_strided_batch_dev(list(reversed(items)))
    for label, live, _, _ in held:
        assert live.bytes() == live.expect([]), label


def check_refusals(lib, dev, public):
    """What the host refuses before any launch (ValueError: ZN_E_ARG), at the C call and — with the reason — at zipnn_amd.patch_apply_; nothing is written."""
    import pytest
    import zipnn_amd
    E = 2
    rng = np.random.default_rng(72)
    views = [("expand", 4, lambda s: s.view(4, 1).expand(4, 4), "stride of 0"),
             ("overlap", 16, lambda s: torch.as_strided(s, (4, 4), (2, 1), s.storage_offset()), "overlap"),
             ("nine-dims", 512, lambda s: s.view((2,) * 9).permute(8, 7, 6, 5, 4, 3, 2, 1, 0), "dimensions")]
    for label, storage, make, why in views:
        m = make(torch.empty(storage, dtype=DT[E])).numel()
        _, patch = make_patch(E, m, "dense", rng)
        p = U.on_device(np.frombuffer(patch, dtype=np.uint8), dev)
        buf = torch.full((storage + OFFSET + PAD,), 0x5C5C, dtype=DT[E], device=dev)
        view = make(buf[OFFSET:OFFSET + storage])
        with pytest.raises(ValueError):
            lib.patch_apply_strided_batch_dev([(p.data_ptr(), p.numel(), m * E, E, view.data_ptr(), tuple(view.shape), tuple(view.stride()))])
        if public:
            with pytest.raises(ValueError, match=why):
                zipnn_amd.patch_apply_(view, p)
        assert bool((buf == 0x5C5C).all()), label
    # at the C call: a product of the sizes that is not m, a negative stride, a misaligned d_dst, and the patch's own argument checks
    base, patch = make_patch(E, 300 * 257, "dense", rng)
    live = Live(dev, E, 257 * 300, LAYOUTS[0][2], base)
    p = U.on_device(np.frombuffer(patch, dtype=np.uint8), dev)
    ok = live.item(p)
    for bad in (ok[:5] + ((300, 256), ok[6]), ok[:5] + ((300, 258), ok[6]), ok[:4] + (live.view[299, 256].data_ptr(), ok[5], (-1, -300)), ok[:4] + (ok[4] + 1,) + ok[5:],
                ok[:4] + (0,) + ok[5:], ok[:3] + (3,) + ok[4:], (0,) + ok[1:], (ok[0] + 2,) + ok[1:], (ok[0], 31) + ok[2:], ok[:5] + ((300, 257), (0, 1))):
        with pytest.raises(ValueError):
            lib.patch_apply_strided_batch_dev([bad])
        with pytest.raises(ValueError):
            lib.patch_apply_strided_batch_dev([ok, bad])                         # … and a refused item refuses the batch before the launch
    assert live.bytes() == live.expect([])
    lib.patch_apply_strided_batch_dev([])                                        # count == 0


def hostile(E):
    """-> (base bytes, [(label, patch bytes)]): tests/patch_util.py's well-formed patch (BLOCK + 40 elements) damaged in the ways apply must refuse."""
    _, base, good = U.apply_pair(E)
    _, n, T, first, off, _ = R.parse(good)
    nb = first.size - 1
    a1 = R.round16(32 + 4 * (nb + 1))
    a2 = R.round16(a1 + 2 * T)

    def edit(at, data):
        p = bytearray(good)
        p[at:at + len(data)] = data
        return bytes(p)
    return base, [("wrong-n", edit(8, struct.pack("<Q", n + E))),
                  ("offset-past-the-end", edit(a1 + 2 * (T - 1), struct.pack("<H", 65535))),
                  ("repeated-offset", edit(a1 + 2 * 5, struct.pack("<H", int(off[4])))),
                  ("descending-offset", edit(a1 + 2 * 5, struct.pack("<H", int(off[4]) - 1 if off[4] else 0))),
                  ("zero-value", edit(a2 + E * 7, bytes(E))),
                  ("first-decreases", edit(32 + 4, struct.pack("<I", int(first[2]) + 1)))]


def check_hostile(lib, dev, E):
    """Hostile patches through a transposed view: checked, the call raises; unchecked, the verdict waits in the status slot; never a byte outside the view's
    elements.  Each patch lies in an allocation of exactly its length."""
    import pytest
    from zipnn_amd._capi import ZN_E_CORRUPT, ZnError
    base, cases = hostile(E)
    m = base.size // E
    assert m % 8 == 0

    def make(s):
        return s.view(m // 8, 8).t()
    for label, data in cases:
        p = torch.empty(len(data) + 16, dtype=torch.uint8, device=dev)
        a0 = (-p.data_ptr()) % 16
        p = p[a0:a0 + len(data)]
        p.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        live = Live(dev, E, m, make, base)
        with pytest.raises(ZnError) as ei:
            lib.patch_apply_strided_batch_dev([live.item(p)])
        assert ei.value.status == ZN_E_CORRUPT, label
        assert live.outside_intact(), label                                      # the view's own elements are undefined after a corrupt patch; nothing else moved
        lib.patch_apply_strided_batch_dev([live.item(p)], 0, False)
        with pytest.raises(ZnError):
            lib.decode_status()
        assert live.outside_intact(), label
