"""CPU tests (-m "not gpu"): select and place of "znp1" patches (include/zipnn_hip.h) on the emulated kernels of
zipnn_amd/csrc/zn_patch_select.hip — against the numpy restatement (tests/patch_select_ref.py) and against the patches built from the sliced tensors
(tests/patch_ref.py), byte for byte, and — on this build only — hostile inputs: each costs the verdict and never a byte outside the output.  The well-formed
cases live in tests/patch_select_util.py, shared with tests/test_gpu_patch_select.py."""
import numpy as np
import pytest
import torch

import patch_check_util as C
import patch_select_util as SU
import patch_util as U
from test_patch_simt import _hostile
from zipnn_amd._capi import (PATCH_BAD_FIRST, PATCH_BAD_HEADER, PATCH_BAD_OFFSET, PATCH_BAD_VALUE, ZN_E_CORRUPT, ZnError)

CPU = torch.device("cpu")


@pytest.mark.parametrize("E", [1, 2, 4])
def test_select_and_place_equal_the_restatement_and_the_patches_of_the_sliced_tensors(use_simt, E):
    SU.check_select_and_place(use_simt, CPU, E)


def test_ragged_batch_of_mixed_element_sizes_with_an_empty_result(use_simt):
    SU.check_ragged(use_simt, CPU)


def test_placed_selects_of_two_and_three_way_splits_merge_back_to_the_patch(use_simt):
    SU.check_splits_merge_back(CPU)


def test_public_select_and_place_on_2d_and_3d_shapes(use_simt):
    SU.check_public(CPU)


def test_capacity_and_argument_checks(use_simt):
    lib = use_simt
    out, op, E, g, held, want, placed = SU.argument_errors(lib, CPU)
    o0 = op - out.data_ptr()
    for place, res in ((False, want), (True, placed)):
        p = held[place]
        run, size = (lib.patch_place_batch_dev, lib.patch_place_size_batch_dev) if place else (lib.patch_select_batch_dev, lib.patch_select_size_batch_dev)
        it = (p.data_ptr(), p.numel(), E) + g[1:]
        assert size([it]) == [len(res)]
        # capacities short in one item of two: ZN_E_CAP, nothing written, every needed length returned
        arr, n = lib._patch_select_items([it + (op, len(res) - 1), it + (op + len(out) // 2 // 16 * 16, 0)])
        fn = lib._L.zn_patch_place_batch_dev if place else lib._L.zn_patch_select_batch_dev
        assert fn(arr, n, None) == -3 and [arr[0].out_len, arr[1].out_len] == [len(res)] * 2 and (out == 0x11).all()
        with pytest.raises(ZnError) as ei:
            run([it + (op, len(res) - 1)])
        assert ei.value.status == -3 and (out == 0x11).all()
        assert run([it + (op, len(res))]) == [len(res)]
        assert bytes(out[o0:o0 + len(res)].numpy()) == res and (out[o0 + len(res):] == 0x11).all() and (out[:o0] == 0x11).all()
        out.fill_(0x11)
    assert lib._L.zn_abi_version() == 3


@pytest.mark.parametrize("E", [1, 2, 4])
def test_hostile_inputs_cost_the_verdict_and_nothing_else(use_simt, E):
    lib = use_simt
    src, base, cases = _hostile(E)
    m = base.size // E
    # (what, place, rows, cols, r0, r1, c0, c1): the input covers m elements in each
    whole = ("select-whole", False, 1, m, 0, 1, 0, m)
    place = ("place", True, m + 5, 3, 2, m + 2, 1, 2)
    sub = ("select-sub", False, 1, m, 0, 1, 100, m - 3)
    kinds = {label.split("-")[0] for label, _, _ in cases}
    assert {"wrong", "first", "offset", "descending", "repeated", "zero", "random"} <= kinds
    seen = 0
    for label, data, plen in cases:
        plen = len(data) if plen is None else plen
        if plen < 32:
            continue                                                             # (never reaches a launch: test_capacity_and_argument_checks)
        # the damaged patch in an allocation of exactly its length: a read outside it is a read outside the allocation
        p = C.exact(data[:plen], CPU)
        verdict = lib.patch_check_batch_dev([(p.data_ptr(), plen, base.size, E)])[0][0]
        must = bool(verdict & (PATCH_BAD_HEADER | PATCH_BAD_FIRST | PATCH_BAD_OFFSET | PATCH_BAD_VALUE))
        assert must or label.startswith("random"), label                         # (every named damage is one zn_patch_check rejects for header, first, offset or value)
        for what, pl, *rect in (whole, place, sub):
            run, size = (lib.patch_place_batch_dev, lib.patch_place_size_batch_dev) if pl else (lib.patch_select_batch_dev, lib.patch_select_size_batch_dev)
            item = (p.data_ptr(), plen, E) + tuple(rect)
            cap = 2 * len(data) + 4096                                           # (a result has no more entries than its input, and at most four blocks here)
            answers = []
            try:
                size([item])
                answers.append(0)
            except ZnError as e:
                answers.append(e.status)
            buf, view, o = U.canaried(np.zeros(cap, dtype=np.uint8), CPU, 1)
            view = view[(-view.data_ptr()) % 16:]
            try:
                run([item + (view.data_ptr(), view.numel())])
                answers.append(0)
            except ZnError as e:
                answers.append(e.status)
            assert U.canaries_intact(buf, o, cap), (label, what)
            assert set(answers) <= {0, ZN_E_CORRUPT}, (label, what, answers)
            if what != "select-sub":                                             # (damage in a block a proper sub-rectangle does not visit is legitimately not seen)
                assert answers == ([ZN_E_CORRUPT] * 2 if must else [0, 0]) or (not must and verdict), (label, what, answers, verdict)
            seen += 1
    assert seen >= 60
    # a bad item spoils the call it is in, and only that call
    good = C.exact(U.apply_pair(E)[2], CPU)
    item = (good.data_ptr(), good.numel(), E) + tuple(sub[2:])
    with pytest.raises(ZnError):
        lib.patch_select_size_batch_dev([item, (p.data_ptr(), p.numel(), E) + tuple(whole[2:]), item])
    sizes = lib.patch_select_size_batch_dev([item, item])
    assert sizes[0] == sizes[1] > 0
