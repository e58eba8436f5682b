"""CPU tests (-m "not gpu"): changed-element patches ("znp1", include/zipnn_hip.h) on the emulated kernels of zipnn_amd/csrc/zn_patch.hip —
builds against the numpy restatement of the format (tests/patch_ref.py) byte for byte, applies against its apply, and — on this build only — hostile patches:
each costs the verdict and never a byte outside the destination.  The well-formed cases live in tests/patch_util.py, shared with tests/test_gpu_patch.py."""
import struct

import numpy as np
import pytest
import torch

import patch_ref as R
import patch_util as U
from zipnn_amd._capi import ZN_E_CORRUPT, ZnError

CPU = torch.device("cpu")


@pytest.mark.parametrize("E", [1, 2, 4])
def test_build_equals_the_restatement(use_simt, E):
    U.check_build(use_simt, CPU, E)
    assert {"zn_k_patch_count", "zn_k_patch_scan", "zn_k_patch_emit"} <= set(use_simt.last_kernels().split(";"))


@pytest.mark.parametrize("E,shifts", [(1, (1, 3)), (1, (5, 0)), (2, (1, 3)), (2, (0, 1)), (4, (1, 3)), (4, (2, 0))])
def test_build_at_element_aligned_addresses_that_differ_mod_16(use_simt, E, shifts):
    U.check_build(use_simt, CPU, E, shifts)


def test_ragged_batch_with_an_empty_and_an_identical_item(use_simt):
    U.check_ragged(use_simt, CPU)


def test_sizes_capacity_and_argument_checks(use_simt):
    lib = use_simt
    src, base, patch = U.apply_pair(2)
    s, b = U.on_device(src, CPU), U.on_device(base, CPU)
    it = (s.data_ptr(), b.data_ptr(), s.numel(), 2)
    assert lib.patch_size_batch_dev([it]) == [len(patch)] and lib.patch_size_batch_dev([]) == []
    assert len(patch) == R.patch_len(src.size, 2, R.parse(patch)[2]) == lib.patch_len(src.size, 2, R.parse(patch)[2])
    out = torch.full((len(patch) + 64,), 0x11, dtype=torch.uint8)
    with pytest.raises(ZnError) as ei:                                           # a capacity one byte short: ZN_E_CAP, nothing written
        lib.patch_build_batch_dev([it + (out.data_ptr(), len(patch) - 1)])
    assert ei.value.status == -3 and (out == 0x11).all()
    for bad in ((s.data_ptr(), b.data_ptr(), s.numel(), 3), (s.data_ptr(), b.data_ptr(), s.numel() - 1, 2), (0, b.data_ptr(), 16, 2), (s.data_ptr() + 1, b.data_ptr(), 16, 2),
                (s.data_ptr(), b.data_ptr(), 2 ** 33, 1)):
        with pytest.raises(ValueError):
            lib.patch_size_batch_dev([bad])
    with pytest.raises(ValueError):
        lib.patch_build_batch_dev([it + (out.data_ptr() + 1, len(patch))])        # an unaligned patch buffer
    assert lib.patch_len(10, 4, 1) == 0 and lib.patch_len(8, 4, 3) == 0
    assert lib._L.zn_abi_version() == 3


def test_apply_whole_tensors_twice_over_a_base_and_the_public_functions(use_simt):
    U.check_apply_whole(use_simt, CPU)


@pytest.mark.parametrize("E", [1, 2, 4])
def test_apply_every_window_of_a_small_tensor(use_simt, E):
    U.check_apply_windows(use_simt, CPU, E)


def _hostile(E=2):
    """-> (source, base, [(label, patch bytes, patch_len handed over)]): one well-formed patch damaged in every way the header names, and random bytes."""
    src, base, good = U.apply_pair(E)
    _, n, T, first, off, val = R.parse(good)
    nb = first.size - 1
    a1 = R.round16(32 + 4 * (nb + 1))
    a2 = R.round16(a1 + 2 * T)

    def edit(at, data):
        p = bytearray(good)
        p[at:at + len(data)] = data
        return bytes(p)
    out = [("truncated", good, len(good) - 16), ("truncated-to-the-header", good, 32), ("shorter-than-a-header", good, 16),
           ("wrong-E", edit(4, bytes([4 if E != 4 else 2])), None), ("wrong-n", edit(8, struct.pack("<Q", n + E)), None),
           ("wrong-n-smaller", edit(8, struct.pack("<Q", n - E)), None), ("wrong-L", edit(24, struct.pack("<Q", len(good) + 16)), None),
           ("wrong-T", edit(16, struct.pack("<Q", T + 1)), None), ("huge-T", edit(16, struct.pack("<Q", 2 ** 63)), None),
           ("wrong-magic", edit(0, b"ZNP2"), None),
           ("first-decreases", edit(32 + 4, struct.pack("<I", int(first[2]) + 1)), None),
           ("first-0-nonzero", edit(32, struct.pack("<I", 1)), None),
           ("first-NB-above-T", edit(32 + 4 * nb, struct.pack("<I", T + 1)), None),
           ("first-NB-below-T", edit(32 + 4 * nb, struct.pack("<I", T - 1)), None),
           ("offset-past-the-end", edit(a1 + 2 * (T - 1), struct.pack("<H", 65535)), None),
           ("repeated-offset", edit(a1 + 2 * 5, struct.pack("<H", int(off[4]))), None),
           ("descending-offset", edit(a1 + 2 * 5, struct.pack("<H", int(off[4]) - 1 if off[4] else 0)), None),
           ("zero-value", edit(a2 + E * 7, bytes(E)), None)]
    rng = np.random.default_rng(99)
    for i in range(6):
        r = bytearray(rng.integers(0, 256, size=len(good), dtype=np.uint8).tobytes())
        if i >= 3:                                                               # … behind a header that is right
            r[:32] = good[:32]
        out.append((f"random-{i}", bytes(r), None))
    return src, base, out


@pytest.mark.parametrize("E", [1, 2, 4])
def test_hostile_patches_cost_the_verdict_and_nothing_else(use_simt, E):
    lib = use_simt
    src, base, cases = _hostile(E)
    n = base.size
    for label, data, plen in cases:
        plen = len(data) if plen is None else plen
        # the patch in an allocation of exactly its length: a read outside it is a read outside the allocation
        p = torch.empty(plen + 16, dtype=torch.uint8)
        a0 = (-p.data_ptr()) % 16
        p = p[a0:a0 + plen]
        p.copy_(torch.frombuffer(bytearray(data[:plen]), dtype=torch.uint8))
        for lo, hi, with_base in ((0, n, False), (0, n, True), (E * 100, n - E * 3, False)):
            buf, view, o = U.canaried(base[lo:hi], CPU, E)
            bt = torch.from_numpy(base.copy())
            item = (p.data_ptr(), plen, n, E, lo, hi, view.data_ptr()) + ((bt.data_ptr(),) if with_base else ())
            with pytest.raises((ZnError, ValueError)) as ei:
                lib.patch_apply_batch_dev([item])
            if isinstance(ei.value, ZnError):
                assert ei.value.status == ZN_E_CORRUPT, label
            assert U.canaries_intact(buf, o, hi - lo), label
        # unchecked, the verdict waits in the call's status slot — and joins a chain
        buf, view, o = U.canaried(base, CPU, E)
        item = (p.data_ptr(), plen, n, E, 0, n, view.data_ptr())
        if plen >= 32:
            lib.patch_apply_batch_dev([item], 0, False)
            with pytest.raises(ZnError):
                lib.decode_status()
    # a good patch behind a bad one in a chain: the status speaks for both; a good call alone clears it
    good = U.on_device(np.frombuffer(U.apply_pair(E)[2], dtype=np.uint8), CPU)
    label, data, _ = cases[-1]
    bad = U.on_device(np.frombuffer(data, dtype=np.uint8), CPU)
    buf, view, o = U.canaried(base, CPU, E)
    lib.patch_apply_batch_dev([(bad.data_ptr(), bad.numel(), n, E, 0, n, view.data_ptr())], 0, False)
    lib.decode_status_chain(True)
    try:
        lib.patch_apply_batch_dev([(good.data_ptr(), good.numel(), n, E, 0, n, view.data_ptr())], 0, False)
    finally:
        lib.decode_status_chain(False)
    with pytest.raises(ZnError):
        lib.decode_status()
    assert U.canaries_intact(buf, o, n)
    view.copy_(torch.from_numpy(base))
    lib.patch_apply_batch_dev([(good.data_ptr(), good.numel(), n, E, 0, n, view.data_ptr())], 0, False)
    lib.decode_status()
    assert bytes(view.numpy()) == bytes(src)


def test_apply_argument_checks(use_simt):
    lib = use_simt
    src, base, patch = U.apply_pair(2)
    p = U.on_device(np.frombuffer(patch, dtype=np.uint8), CPU)
    buf, view, o = U.canaried(base, CPU, 2)
    n = base.size
    ok = (p.data_ptr(), p.numel(), n, 2, 0, n, view.data_ptr())
    for bad in (ok[:3] + (3,) + ok[4:], ok[:4] + (1, n) + ok[6:], ok[:4] + (0, n + 2) + ok[6:], ok[:4] + (8, 4) + ok[6:], ok[:6] + (view.data_ptr() + 1,),
                ok[:6] + (0,), (0,) + ok[1:], (p.data_ptr() + 2,) + ok[1:], (p.data_ptr(), 31) + ok[2:]):
        with pytest.raises(ValueError):
            lib.patch_apply_batch_dev([bad])
        with pytest.raises(ValueError):
            lib.patch_plan_create([ok, bad])
    assert bytes(view.numpy()) == bytes(base) and U.canaries_intact(buf, o, n)
    lib.patch_apply_batch_dev([])                                                # count == 0
