"""GPU tests (-m gpu): the in-place delta decode of include/zipnn_hip.h (a destination that IS the delta base) and variant stores
(zipnn_amd.ResidentCheckpoint.from_state_dict(..., base=...)) on the real libzipnn_hip.so.  The cases, bodies and checks are those of
tests/test_delta_inplace_simt.py and tests/test_resident_delta_simt.py (tests/delta_inplace_util.py, tests/resident_delta_util.py).  No damaged bodies
here: those stay on the emulator."""
import pytest
import torch

import delta_inplace_util as U
import resident_delta_util as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    yield L
    L.release_workspace()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sds():
    return R.state_dicts()


@pytest.mark.parametrize("off", (0, 4), ids=lambda o: f"mod16={o}")
@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_in_place_delta_decode_every_entry_point_on_the_device(lib, dev, case, off):
    """zn_decompress_delta_dev, a window batch and a plan run twice with the destination pre-filled with the base, aligned (the fused kernel's delta
    instance) and at +4 (the generic kernels behind zn_k_alias_rotate): the fine-tune's bytes, the base back on the plan's second run, guards untouched."""
    a, b, body = U.delta_case(case)
    U.check_entry_points(lib, case, a, b, body, off, dev)
    torch.cuda.synchronize()


@pytest.mark.parametrize("off", (0, 4), ids=lambda o: f"mod16={o}")
@pytest.mark.parametrize("name", ["identical", "unrelated", "skew", "skew4", "u11", "burst16", "tl12-2", "tl12-4"])
def test_in_place_with_rle_raw_hostile_and_table_log_12_planes_on_the_device(lib, dev, name, off):
    """Every plane RLE zero, raw planes, every plane Huffman-coded with 1-bit codes (the fused kernel's further passes over its own output), 11-bit codes,
    tiles denser than the stream average in chunks of 2 * C (burst16), and a
    tableLog-12 plane behind planes the fused kernel has already XORed into the base (it hands the base back and leaves the chunk to the generic path)."""
    case, a, b, body = U.tl12_case(int(name[-1])) if name.startswith("tl12") else U.more_case(name)
    U.check_entry_points(lib, case, a, b, body, off, dev)
    torch.cuda.synchronize()


def test_aligned_in_place_call_stays_on_the_fused_delta_instance(lib, dev):
    """The contract does not push aligned calls off the hot path: every full chunk of an aligned in-place call by zn_k_decode_fused^delta."""
    for case in U.CASES:
        a, b, body_bytes = U.delta_case(case)
        _, nb, P, rot, bm, ch = case
        body = U.to_dev(body_bytes, dev)
        _, dst = U.place(b, 0, dev)
        lib.decompress_dev(body.data_ptr(), body.numel(), P, rot, bm, ch, nb, dst.data_ptr(), U.stream_of(dev), True, delta_ptr=dst.data_ptr())
        first = lib.last_kernels().split(";")[0]
        assert first.startswith("zn_k_decode_fused^delta") and ("^inplace" in first) == (P > 1), lib.last_kernels()      # (the in-place instance says so; one plane: the delta instance)
        assert lib.last_fused_chunks() == nb // ch, (case, lib.last_kernels())
        assert U.got(dst) == a


@pytest.mark.parametrize("kind", R.BASES)
def test_variant_store_on_the_device(lib, dev, sds, kind):
    """The store matrix on cuda:0: get_tensor, get_tensors(into=), get_slice across a chunk boundary, plan().run() twice, hook, sizes, the index."""
    base_sd, ft_sd = sds
    R.check_variant(kind, base_sd, ft_sd, dev)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", R.BASES)
def test_apply_forward_revert_cycle_on_the_device(lib, dev, sds, kind):
    """apply_ on a model that holds the base, forward, revert_: the fine-tune's output bit for bit, then the base's weights and output again."""
    from zipnn_amd import ResidentCheckpoint
    base_sd, ft_sd = sds
    base = R.make_base(kind, base_sd, dev)
    ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base)
    R.check_apply_revert(kind, base_sd, ft_sd, dev, base=base, ft=ft)
    x = (torch.randn(4, 512, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(dev)
    m = R.model_of(base_sd, dev)
    want_base, want_ft = R.model_of(base_sd, dev)(x), R.model_of(ft_sd, dev)(x)
    ft.apply_(m)
    assert R._bytes_equal(m(x), want_ft)
    for k, p in m.state_dict().items():
        assert R._bytes_equal(p, ft_sd[k]), k
    assert ft.revert_(m) == []
    assert R._bytes_equal(m(x), want_base)
    for k, p in m.state_dict().items():
        assert R._bytes_equal(p, base_sd[k]), k
    torch.cuda.synchronize()
