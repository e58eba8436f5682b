"""GPU tests (-m gpu): sync indexes of kind ZN_HINT_DELTA (include/zipnn_hip.h) on the real libzipnn_hip.so — the matrix of
tests/test_index_delta_simt.py at the same sizes.  Bodies are the CPU oracle's frames of tensor ^ base and the expected bytes are the tensor's; the device build
has no counters, so what is asserted is the name of the launch (zn_last_kernels: the hinted delta instances ran) and byte equality — with the index the emulated
library builds for the same body, where the point is that the device builds the same one.  Small calls take the wide kernel, which reads no hints: the fused form
is forced for these tests."""
import numpy as np
import pytest
import torch

import hint_layout_delta as HLD
import index_delta_util as D

pytestmark = pytest.mark.gpu
C2 = D.C2


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    L.set_decode_wide(0)
    yield L
    L.set_decode_wide(1); L.set_decode_group(0)
    L.release_workspace()


def _dev():
    return torch.device("cuda:0")


def _on_dev(case, shift=0):
    a, b, body, spec = case
    return a, b, D.to_dev(body, _dev(), shift), D.to_dev(b, _dev()), spec


def _launches(inplace, P, tail=False):
    return ["zn_k_decode_hinted^delta" + ("^inplace" if inplace and P > 1 else "") + ("+tail" if tail else "")]


@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp32", "fp8"])
def test_delta_index_on_the_device_is_the_emulated_one_and_decodes(lib, simt_lib, kind):
    """Every plane Huffman-coded: the device builds, byte for byte, the DELTA index the kernels' sources build on the CPU for the same body at the same address
    modulo 4 (table and hint bytes: the same sub-block sizes, the same starts), and decodes from it to the fine-tune's bytes — separate destination, in place."""
    a, b, body, base, spec = _on_dev(D.pair_case(kind))
    h, n = D.build(lib, body, spec)
    host = D.to_dev(D.pair_case(kind)[2], torch.device("cpu"))
    assert host.data_ptr() % 4 == body.data_ptr() % 4 == 0
    he, ne = D.build(simt_lib, host, spec)
    assert ne == n and torch.equal(h.cpu(), he)
    want, hdr = HLD.expected_table(D.got(host), spec[0], spec[3], spec[4])
    assert bool((h[:4 * len(want)].cpu().numpy().view("<u4") == want).all()) and int(want[-1]) == n > hdr
    for inplace in (False, True):
        assert D.decode(lib, body, spec, base, h, inplace=inplace) == a
        assert D.hinted_launches(lib) == _launches(inplace, spec[0]), lib.last_kernels()
        assert D.decode(lib, body, spec, base, None, inplace=inplace) == a
        assert "hinted" not in lib.last_kernels()


@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp8"])
def test_dense_delta_body_on_the_device(lib, simt_lib, kind):
    """tensor ^ base as dense as plain weights (4-dword sub-blocks: the register-resident form of the delta instances, the capped dense codes)."""
    a, b, body, base, spec = _on_dev(D.dense_case(kind))
    h, n = D.build(lib, body, spec)
    he, ne = D.build(simt_lib, D.to_dev(D.dense_case(kind)[2], torch.device("cpu")), spec)
    assert ne == n and torch.equal(h.cpu(), he)
    for inplace in (False, True):
        assert D.decode(lib, body, spec, base, h, inplace=inplace) == a
        assert D.hinted_launches(lib) == _launches(inplace, spec[0]), lib.last_kernels()


@pytest.mark.parametrize("group", [1, 2, 3, 4])
def test_mixed_chunk_kinds_in_every_group_size_on_the_device(lib, decode_group, group):
    """All planes Huffman-coded, first plane raw and a later one Huffman-coded, raw, RLE, first Huffman-coded and later raw, a partial last chunk."""
    a, b, body, base, spec = _on_dev(D.kinds_case(D.CHUNK_KINDS, extra=1000))
    decode_group(lib, 0)
    h, n = D.build(lib, body, spec)
    decode_group(lib, group)
    for inplace in (False, True):
        assert D.decode(lib, body, spec, base, h, inplace=inplace) == a
        assert D.hinted_launches(lib) == _launches(inplace, 2, tail=True), lib.last_kernels()


@pytest.mark.parametrize("kind", ["bf16", "fp32", "fp8"])
def test_windows_partial_last_chunk_and_in_place_on_the_device(lib, kind):
    for extra in (0, 1000):
        a, b, body, base, spec = _on_dev(D.pair_case(kind, 4, extra))
        K = -(-len(a) // C2)
        h, _ = D.build(lib, body, spec)
        for lo, hi in ((1, 3), (0, K), (K - 1, K)):
            for inplace in (False, True):
                got = D.decode(lib, body, spec, base, h, lo=lo, hi=hi, inplace=inplace)
                assert got == D.want_window(a, b, spec, lo, hi, inplace), (extra, lo, hi, inplace, lib.last_kernels())
                if (lo + 1) * C2 <= len(a):
                    assert "zn_k_decode_hinted^delta" in lib.last_kernels(), (extra, lo, hi, inplace, lib.last_kernels())


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_delta_index_built_where_the_body_lies_on_the_device(lib, simt_lib, shift):
    """The body 1, 2, 3 bytes into a device buffer: the index is the emulated one of the same shift — and not the one of shift 0."""
    a, b, body, base, spec = _on_dev(D.pair_case("bf16"), shift)
    assert body.data_ptr() % 4 == shift
    h, n = D.build(lib, body, spec)
    cpu = torch.device("cpu")
    he, _ = D.build(simt_lib, D.to_dev(D.pair_case("bf16")[2], cpu, shift), spec)
    h0, _ = D.build(simt_lib, D.to_dev(D.pair_case("bf16")[2], cpu, 0), spec)
    assert torch.equal(h.cpu(), he) and not torch.equal(h.cpu(), h0)
    assert D.decode(lib, body, spec, base, h) == a
    assert D.hinted_launches(lib) == _launches(False, 2), lib.last_kernels()


def test_hinted_plan_run_twice_in_place_gives_the_base_back_on_the_device(lib):
    for kind in ("bf16", "fp8"):
        a, b, body, base, spec = _on_dev(D.pair_case(kind))
        h, _ = D.build(lib, body, spec)
        assert D.decode(lib, body, spec, base, h, inplace=True, plan_runs=1) == a
        assert D.hinted_launches(lib) == _launches(True, spec[0]), lib.last_kernels()
        assert D.decode(lib, body, spec, base, h, inplace=True, plan_runs=2) == b
        assert D.decode(lib, body, spec, base, h, inplace=True, plan_runs=3) == a


@pytest.mark.parametrize("P", [2, 4])
def test_in_place_undo_with_hints_on_the_device(lib, P):
    """tests/delta_inplace_util.tl12_case: the fused kernel gives chunk 0 up after its first passes and hands the base back by running them again, from the
    same hints; the same bytes with and without the index."""
    from delta_inplace_util import tl12_case
    case, a, b, body_bytes = tl12_case(P)
    spec = (case[2], case[3], case[4], case[5], case[1])
    body, base = D.to_dev(body_bytes, _dev()), D.to_dev(b, _dev())
    h, n = D.build(lib, body, spec)
    hinted = D.decode(lib, body, spec, base, h, inplace=True)
    assert D.hinted_launches(lib) == ["zn_k_decode_hinted^delta^inplace"], lib.last_kernels()
    plain = D.decode(lib, body, spec, base, None, inplace=True)
    assert "hinted" not in lib.last_kernels()
    assert hinted == plain == a
    assert D.decode(lib, body, spec, base, h) == a


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_wrong_delta_hints_change_nothing_on_the_device(lib, kind):
    """Random, zero, 0xFF hint bytes, a scrambled table, another body's index, a PLAIN index as DELTA, a DELTA index as PLAIN beside no base."""
    dev = _dev()
    a, b, body, base, spec = _on_dev(D.pair_case(kind))
    a2, b2, body2, base2, spec2 = _on_dev(D.pair_case(kind, seed=10))
    h, n = D.build(lib, body, spec)
    hdr = D.header_bytes(spec)
    g = torch.Generator(device=dev); g.manual_seed(5)
    rnd = h.clone(); rnd[hdr:] = torch.randint(0, 256, (n - hdr,), generator=g, device=dev, dtype=torch.uint8)
    zero = h.clone(); zero[hdr:] = 0
    ff = h.clone(); ff[hdr:] = 0xFF
    scr = torch.randint(0, 256, (n,), generator=g, device=dev, dtype=torch.uint8)
    allff = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
    n2 = lib.hint_size_dev(D.item(body2, spec2), D.stream_of(dev), D.DELTA)
    other = torch.zeros(max(n, n2), dtype=torch.uint8, device=dev)
    lib.hint_build_dev(D.item(body2, spec2), other.data_ptr(), other.numel(), D.stream_of(dev), D.DELTA)
    pl = torch.zeros(n, dtype=torch.uint8, device=dev)
    lib.hint_build_dev(D.item(body, spec), pl.data_ptr(), pl.numel(), D.stream_of(dev), D.PLAIN)
    for hints in (rnd, zero, ff, scr, allff, other, pl):
        for inplace in (False, True):
            assert D.decode(lib, body, spec, base, hints, inplace=inplace) == a
            assert D.hinted_launches(lib) == _launches(inplace, spec[0]), lib.last_kernels()
    coded = D.xor(a, b)
    assert D.decode(lib, body, spec, None, h, kind=D.PLAIN) == coded
    assert D.hinted_launches(lib) == ["zn_k_decode_hinted"], lib.last_kernels()
    assert D.decode(lib, body, spec, None, h, kind=D.DELTA) == coded and "hinted" not in lib.last_kernels()
    assert D.decode(lib, body, spec, base, pl, kind=D.PLAIN) == a and "hinted" not in lib.last_kernels()


def test_delta_index_table_across_sizing_blocks_on_the_device(lib):
    kind, chunk, chunks, extra = "bf16", 4096, 257, 100
    a, b, body, base, spec = _on_dev(D.pair_case(kind, chunks, extra, seed=31, chunk=chunk))
    K = -(-len(a) // chunk)
    h, n = D.build(lib, body, spec)
    want, hdr = HLD.expected_table(D.got(body), spec[0], chunk, len(a))
    got = h[:4 * len(want)].cpu().numpy().view("<u4")
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0 and int(want[-1]) == n, (bad[:4], n)
    for lo, hi in ((0, K), (254, K), (K - 1, K)):
        assert D.decode(lib, body, spec, base, h, lo=lo, hi=hi) == a[lo * chunk: min(hi * chunk, len(a))], (lo, hi)
        if (lo + 1) * chunk <= len(a):
            assert "zn_k_decode_hinted^delta" in lib.last_kernels()


@pytest.mark.parametrize("base_kind", ["dict", "store+index"])
def test_variant_store_with_delta_index_on_the_device(lib, base_kind, tmp_path):
    import resident_delta_util as U
    from delta_file_util import same_file
    from zipnn_amd.resident import ResidentCheckpoint
    dev = _dev()
    base, ft, base_sd, ft_sd = D.variant_store(base_kind, dev)
    before = ft.save_file(str(tmp_path / "before.znn.safetensors"))
    D.check_store_with_delta_index(base_kind, base, ft, base_sd, ft_sd, dev, lib, wide_after=0)
    assert same_file(ft.save_file(str(tmp_path / "after.znn.safetensors")), before)
    held = ft.resident_bytes - ft.index_bytes
    ft.drop_index()
    assert ft.index_bytes == 0 and ft.resident_bytes == held and all(ft.info(n)["index_bytes"] == 0 for n in ft.keys())
    assert U._bytes_equal(ft.get_tensor("w.bf16"), ft_sd["w.bf16"])
    ft2 = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base, index="deltas")
    assert ft2.info("w.bf16")["index_bytes"] > 0 and ft2.info("absent")["index_bytes"] > 0
    ft4 = ResidentCheckpoint.from_file(str(tmp_path / "after.znn.safetensors"), dev, base=base, index="deltas")
    assert ft4.info("w.bf16")["index_bytes"] > 0
    lib.set_decode_wide(0)
    assert U._bytes_equal(ft4.get_tensor("w.bf16"), ft_sd["w.bf16"]) and "zn_k_decode_hinted^delta" in lib.last_kernels()


def test_guarded_apply_forward_revert_cycle_reads_the_delta_index(lib):
    """A two-layer MLP holding the base's weights: apply_(guard=True) turns them into the fine-tune's in place — from the index —, the forward pass equals the
    plainly loaded fine-tune's bit for bit, revert_(guard=True) hands the base back."""
    import resident_delta_util as U
    from zipnn_amd.resident import ResidentCheckpoint
    dev = _dev()
    base_sd, ft_sd = U.state_dicts()
    keys = ("0.weight", "0.bias", "1.weight", "1.bias")
    bsd, fsd = {k: base_sd[k] for k in keys}, {k: ft_sd[k] for k in keys}
    base = ResidentCheckpoint.from_state_dict(bsd, dev, index=True, digests=True)
    ft = ResidentCheckpoint.from_state_dict(fsd, dev, base=base, index="deltas", digests=True)
    assert ft.info("0.weight")["delta"] is True and ft.info("0.weight")["index_bytes"] > 0
    m = U.model_of(base_sd, dev)
    x = (torch.randn(4, 512, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(dev)
    want = U.model_of(ft_sd, dev)(x)
    lib.set_decode_wide(0)
    for _ in range(2):
        changed = ft.apply_(m, guard=True)
        assert sorted(changed) == sorted(keys)
        assert any(k.startswith("zn_k_decode_hinted^delta") for k in D.hinted_launches(lib)), lib.last_kernels()
        assert U._bytes_equal(m(x), want)
        assert ft.revert_(m, guard=True) == []
        for k, p in m.state_dict().items():
            assert U._bytes_equal(p, base_sd[k]), k
