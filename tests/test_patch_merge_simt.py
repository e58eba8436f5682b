"""CPU tests (-m "not gpu"): the XOR-merge of "znp1" patches (include/zipnn_hip.h) on the emulated kernels of zipnn_amd/csrc/zn_patch_merge.hip —
merges against the numpy restatement (tests/patch_merge_ref.py) and against the patch built from the two tensors (tests/patch_ref.py), byte for byte, and — on
this build only — hostile inputs: each costs the verdict and never a byte outside the output.  The well-formed cases live in tests/patch_merge_util.py, shared
with tests/test_gpu_patch_merge.py."""
import numpy as np
import pytest
import torch

import patch_check_util as C
import patch_merge_util as MU
import patch_util as U
from test_patch_simt import _hostile
from zipnn_amd._capi import ZN_E_CORRUPT, ZnError

CPU = torch.device("cpu")


@pytest.mark.parametrize("E", [1, 2, 4])
def test_merge_equals_the_restatement_and_the_patch_of_the_two_tensors(use_simt, E):
    MU.check_merge(use_simt, CPU, E)
    assert {"zn_k_patch_merge_count", "zn_k_patch_scan", "zn_k_patch_merge_emit"} <= set(use_simt.last_kernels().split(";"))


def test_ragged_batch_of_mixed_element_sizes_with_cancelling_items(use_simt):
    MU.check_ragged(use_simt, CPU)


def test_public_merge_takes_live_weights_from_a_to_b_and_back(use_simt):
    MU.check_public(CPU)


def test_capacity_and_argument_checks(use_simt):
    lib = use_simt
    ok, out, want, held = MU.argument_errors(lib, CPU)
    assert lib.patch_merge_size_batch_dev([ok[:6]]) == [len(want)]
    with pytest.raises(ZnError) as ei:                                           # a capacity one byte short: ZN_E_CAP, nothing written
        lib.patch_merge_batch_dev([ok[:7] + (len(want) - 1,)])
    assert ei.value.status == -3 and (out == 0x11).all()
    assert lib.patch_merge_batch_dev([ok]) == [len(want)]
    o0 = (-out.data_ptr()) % 16
    assert bytes(out[o0:o0 + len(want)].numpy()) == want and (out[o0 + len(want):] == 0x11).all() and (out[:o0] == 0x11).all()
    assert lib._L.zn_abi_version() == 3


@pytest.mark.parametrize("E", [1, 2, 4])
def test_hostile_inputs_cost_the_verdict_and_nothing_else(use_simt, E):
    lib = use_simt
    src, base, cases = _hostile(E)
    n = base.size
    good_bytes = U.apply_pair(E)[2]
    good = C.exact(good_bytes, CPU)
    kinds = {label.split("-")[0] for label, _, _ in cases}
    assert {"wrong", "first", "offset", "descending", "repeated", "zero", "random"} <= kinds
    seen = 0
    for label, data, plen in cases:
        plen = len(data) if plen is None else plen
        if plen < 32:
            continue                                                             # (never reaches a launch: test_capacity_and_argument_checks)
        # the damaged patch in an allocation of exactly its length: a read outside it is a read outside the allocation
        p = C.exact(data[:plen], CPU)
        for a, b in ((p, good), (good, p)):
            item = (a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), n, E)
            with pytest.raises(ZnError) as ei:
                lib.patch_merge_size_batch_dev([item])
            assert ei.value.status == ZN_E_CORRUPT, label
            buf, view, o = U.canaried(np.zeros(2 * len(good_bytes) + len(data), dtype=np.uint8), CPU, 1)
            view = view[(-view.data_ptr()) % 16:]
            with pytest.raises(ZnError) as ei:
                lib.patch_merge_batch_dev([item + (view.data_ptr(), view.numel())])
            assert ei.value.status == ZN_E_CORRUPT, label
            assert U.canaries_intact(buf, o, 2 * len(good_bytes) + len(data)), label
            seen += 1
    assert seen >= 40
    # a bad item spoils the call it is in, and only that call
    item = (good.data_ptr(), good.numel(), good.data_ptr(), good.numel(), n, E)
    with pytest.raises(ZnError):
        lib.patch_merge_size_batch_dev([item, (p.data_ptr(), p.numel(), good.data_ptr(), good.numel(), n, E), item])
    assert lib.patch_merge_size_batch_dev([item, item]) == [0, 0]
