"""GPU tests (-m gpu): the batched codec at checkpoint scale — hundreds to thousands of tensors in one zn_decompress_batch_dev /
zn_compress_batch_dev call, most of them ragged (a partial last chunk: norms, biases, router weights).  The decode launch changes shape with the
number of ragged tensors in it (merge workgroups per tensor, tail slots, tail scratch, the rest-instance limit, chunk groups, two streams); every
case checks each body against the CPU oracle, each decoded tensor against its source, and asserts the path it was written for (zn_last_kernels,
zn_last_tail_planes against the count the oracle's frames give)."""
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from test_kernels_simt import _delta_pair, _gen2, _oracle_bodies, _ragged_batch, _ragged_count, _tail_planes_expected

pytestmark = pytest.mark.gpu
HDR = bytes(range(32))
KB = 1024
REST = "zn_k_decode_fused^rest+tail+merge"
GENERIC = "zn_k_decode_fused+tail;zn_k_decode_planes;zn_k_merge_planes"
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    yield L
    _CACHE.clear()
    L.release_workspace()


def _merge_per(ntt):
    """zn_launch_decode_fused's rule, restated: 32 merge workgroups per ragged tensor, halved while merge_per * ntt > 4096."""
    m = 32
    while m > 1 and m * ntt > 4096:
        m //= 2
    return m


def _kinds_present(specs):
    return [P for P in (1, 2, 4) if any(s[2] == P and s[1] for s in specs)]


def _chunks(specs, P, full_only=False):
    return sum((nb // ch) if full_only else -(-nb // ch) for (_k, nb, p, _r, _b, ch) in specs if p == P)


def _stage(lib, bufs, dev, odd=False):
    """Host byte strings -> slices of ONE uploaded device blob, at 256-byte aligned offsets — or at odd ones (odd=True), as a file's data section puts them."""
    from zipnn_amd import codec
    offs, o = [], (1 if odd else 0)
    for b in bufs:
        offs.append(o)
        o += len(b)
        o = (o + 1 if o % 2 == 0 else o + 2) if odd else (o + 255) // 256 * 256
    host = codec.new_bytearray(max(o, 1))
    mv = memoryview(host)
    for b, off in zip(bufs, offs):
        mv[off:off + len(b)] = b
    blob = codec.to_device(lib, host, dev)
    return [blob[off:off + len(b)] for b, off in zip(bufs, offs)]


def _assert_same(outs, srcs, specs):
    """Every decoded tensor == its source (one comparison on the device; the first mismatch named)."""
    if sum(o.numel() for o in outs) == 0:
        return
    if torch.equal(torch.cat([o.reshape(-1) for o in outs]), torch.cat([s.reshape(-1) for s in srcs])):
        return
    bad = next(i for i, (o, s) in enumerate(zip(outs, srcs)) if not torch.equal(o, s))
    pytest.fail(f"tensor {bad} of {len(outs)} decoded wrong: {specs[bad]}")


def _compress_and_check(lib, specs, srcs, bodies, deltas=None):
    """zn_compress_batch_dev over device slices: every body == the oracle's; -> the device bodies."""
    from zipnn_amd import codec
    items = [(s, P, rot, bm, ch, 0.95) + ((deltas[i],) if deltas is not None else ()) for i, (s, (_k, _n, P, rot, bm, ch)) in enumerate(zip(srcs, specs))]
    arena, offs, lens = codec.compress_device_batch(lib, items, return_arena=True)
    host = arena.cpu().numpy()
    for i, (o, n, want) in enumerate(zip(offs, lens, bodies)):
        assert n == len(want) and host[o:o + n].tobytes() == want, (i, specs[i])
    return [arena[o:o + n] for o, n in zip(offs, lens)]


def _decode(lib, specs, bodies_dev, check=True, deltas=None):
    from zipnn_amd import codec
    return codec.decompress_device_batch(lib, [(b, P, rot, bm, ch, nb) + ((deltas[i],) if deltas is not None else ())
                                               for i, (b, (_k, nb, P, rot, bm, ch)) in enumerate(zip(bodies_dev, specs))], check=check)


def _batch(n2, seed=None):
    """Case 1's batches: exactly n2 two-plane ragged tensors of 8 KiB chunks, fewer one- and four-plane ones (other merge_per), whole and empty
    tensors between them; the oracle's bodies.  Kept for the module (a few tens of MB at n2 = 4 097)."""
    key = (n2, seed)
    if key not in _CACHE:
        specs, datas = _ragged_batch(n2, seed if seed is not None else n2, chunk=8192, n1=min(n2 // 4 + 3, 120), n4=n2 // 8 + 5, full_max=2)
        _CACHE[key] = specs, datas, _oracle_bodies(specs, datas)
    return _CACHE[key]


@pytest.mark.parametrize("n2", [128, 129, 257, 1025, 4097])
def test_merge_workgroups_per_ragged_tensor_at_every_halving(lib, n2, request):
    """n2 ragged two-plane tensors in one call: merge_per = 32, 16, 8, 2, 1 workgroups per partial chunk in the rest instance of
    zn_k_decode_fused (zn_tail_merge_wg: tensor m / merge_per, words sub = m % merge_per of nsub = merge_per).  The one- and four-plane
    tensors of the same call keep other counts.  Encoded by one batched call first: every body == the oracle's."""
    request.addfinalizer(lib.release_workspace)          # (4 097 tails reserve about 1 GiB of tail scratch)
    dev = torch.device("cuda:0")
    specs, datas, bodies = _batch(n2)
    assert _ragged_count(specs, 2) == n2 and _merge_per(n2) == {128: 32, 129: 16, 257: 8, 1025: 2, 4097: 1}[n2]
    assert _merge_per(_ragged_count(specs, 4)) != _merge_per(n2) or n2 == 128
    assert _chunks(specs, 1) < 512                       # (not the two-stream form: that is the test below)
    srcs = _stage(lib, datas, dev)
    got = _compress_and_check(lib, specs, srcs, bodies)
    assert "zn_k_encode_emit+tail" in lib.last_kernels()
    outs = _decode(lib, specs, got)
    assert lib.last_kernels() == ";".join([REST] * 3)
    assert lib.last_tail_planes() == _tail_planes_expected(specs, bodies) > n2 // 4
    _assert_same(outs, srcs, specs)


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("n2", [129, 257])
def test_wide_kernel_carries_the_merge_at_16_and_8_per_tensor(lib, n2, mode, request):
    """The small-input kernel (zn_set_decode_wide 2 / 3: its 16- / 8-wave form) with tail workgroups in front and merge_per = 16 / 8 merge workgroups
    per ragged tensor at the end of ITS launch; the fused kernel behind it has neither."""
    request.addfinalizer(lambda: lib.set_decode_wide(1))
    dev = torch.device("cuda:0")
    specs, datas, bodies = _batch(n2)
    srcs = _stage(lib, datas, dev)
    lib.set_decode_wide(mode)
    outs = _decode(lib, specs, _stage(lib, bodies, dev))
    form = "zn_k_decode_wide" if mode == 2 else "zn_k_decode_wide^2"
    assert lib.last_kernels() == ";".join([form + "+tail+merge;zn_k_decode_fused^rest"] * 3)
    assert lib.last_tail_planes() == _tail_planes_expected(specs, bodies)
    _assert_same(outs, srcs, specs)


def _fill_slots(limit, seed):
    """bf16 / fp32 tensors (sign rotate: what the automatic rule gives the wide kernel) of one full chunk + a tail each, as many as keep
    full chunks + 4 P + 32 slots per ragged tensor within `limit`."""
    specs, used, i = [], 0, 0
    while True:
        P = (2, 4)[i % 2]
        need = 1 + 4 * P + 32
        if used + need > limit:
            break
        ch = 256 * KB
        specs.append(("bf16" if P == 2 else "fp32", ch + 600 * P + 4 * int(np.random.default_rng(seed + i).integers(0, 20000)), P, 1, 10 if P == 2 else 220, ch))
        used += need; i += 1
    return specs, used


def test_wide_kernel_automatic_mode_with_many_tails(lib, request):
    """Automatic mode: a bf16 / fp32 batch whose full chunks + tail and merge workgroups fit the CUs once takes the 16-wave form, one that fits
    them twice the 8-wave form — the slot count the host rule adds per ragged tensor, at the CU count the device reports."""
    request.addfinalizer(lambda: lib.set_decode_wide(1))
    lib.set_decode_wide(1)
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for limit, form, seed in ((cus, "zn_k_decode_wide", 1), (2 * cus, "zn_k_decode_wide^2", 2)):
        specs, used = _fill_slots(limit, 100 * seed)
        assert used > limit // 2 and len(specs) >= 2
        datas = [_gen2(k, nb, 300 + 10 * seed + i) for i, (k, nb, *_r) in enumerate(specs)]
        bodies = _oracle_bodies(specs, datas, threads=4)
        srcs = _stage(lib, datas, dev)
        outs = _decode(lib, specs, _stage(lib, bodies, dev))
        assert lib.last_kernels() == ";".join([form + "+tail+merge;zn_k_decode_fused^rest"] * 2)
        assert lib.last_tail_planes() == _tail_planes_expected(specs, bodies)
        _assert_same(outs, srcs, specs)


def _residue_batch(seed, n=216, chunk=8192):
    """n tensors whose chunk counts (full + partial) run through 1 .. 12 with and without a tail — every residue mod 2, 3 and 4 —,
    of every plane count and distribution."""
    kinds = [("bf16", 2, 1), ("fp16", 2, 0), ("fp32", 4, 1), ("fp8", 1, 0), ("skew", 2, 0), ("rand", 2, 1), ("const", 1, 0), ("skew", 4, 0)]
    r = np.random.default_rng(seed)
    specs = []
    for i in range(n):
        kind, P, rot = kinds[i % len(kinds)]
        full = (i // 2) % 12
        tail = 0 if i % 2 else int(r.integers(1, chunk)) // P * P + (i % 3 == 0)
        if full == 0 and tail == 0:
            full = 1
        specs.append((kind, full * chunk + tail, P, rot, 220 if P == 4 else 10, chunk))
    return specs, [_gen2(k, nb, seed + i) for i, (k, nb, *_r) in enumerate(specs)]


@pytest.mark.parametrize("group", [1, 2, 3, 4])
def test_forced_chunk_groups_over_many_segments(lib, group, decode_group):
    """zn_set_decode_group 1..4 on a 216-tensor batch whose chunk counts cover every residue mod 2, 3, 4, tails included: a workgroup's group of
    chunks starts and ends inside and across segments (wg0 per segment), the partial chunk of a group is skipped for the tail workgroups."""
    dev = torch.device("cuda:0")
    specs, datas = _residue_batch(7)
    bodies = _oracle_bodies(specs, datas)
    srcs = _stage(lib, datas, dev)
    decode_group(lib, group)
    outs = _decode(lib, specs, _stage(lib, bodies, dev))
    assert lib.last_kernels() == ";".join([REST] * 3)
    assert lib.last_tail_planes() == _tail_planes_expected(specs, bodies)
    _assert_same(outs, srcs, specs)


def test_automatic_chunk_group_above_one_on_a_ragged_batch(lib):
    """More than 1 024 full two-plane chunks over 260 ragged tensors: the automatic rule (zn_decode_group_for, at this device's CU count) picks a
    group above one by itself."""
    dev = torch.device("cuda:0")
    specs, datas = _ragged_batch(260, 11, chunk=8192, n1=40, n4=20, full_max=18, tail_max=6000)
    kq = _chunks(specs, 2, full_only=True)
    assert kq > 1024 and lib.decode_group_for(kq) > 1
    bodies = _oracle_bodies(specs, datas)
    srcs = _stage(lib, datas, dev)
    outs = _decode(lib, specs, _stage(lib, bodies, dev))
    assert lib.last_kernels() == ";".join([REST] * 3)
    assert lib.last_tail_planes() == _tail_planes_expected(specs, bodies)
    _assert_same(outs, srcs, specs)


def test_above_the_rest_instance_limit_with_170_tails(lib, request):
    """One plane count with more than ZN_REST_TAIL_MAX_CHUNKS (24 576) chunks of 16 KiB over 170 ragged tensors (about 400 MB): the plain instance
    with its tail workgroups, then the generic plane and merge kernels take the 170 partial chunks.  Encoded by one batched call first."""
    request.addfinalizer(lib.release_workspace)
    dev = torch.device("cuda:0")
    specs, datas = _ragged_batch(170, 13, chunk=16 * KB, full_min=120, full_max=200, whole_every=40,
                                 kinds={2: [("bf16", 1), ("fp16", 0), ("rand", 1), ("const", 1), ("skew", 0), ("bf16", 1)]})
    assert _chunks(specs, 2) > 24576 and _kinds_present(specs) == [2]
    bodies = _oracle_bodies(specs, datas, threads=16)
    srcs = _stage(lib, datas, dev)
    del datas
    got = _compress_and_check(lib, specs, srcs, bodies)
    outs = _decode(lib, specs, got)
    assert lib.last_kernels() == GENERIC
    assert lib.last_tail_planes() == _tail_planes_expected(specs, bodies) > 100
    _assert_same(outs, srcs, specs)


@pytest.mark.parametrize("full_max,form", [(3, REST), (14, GENERIC)], ids=["rest-1024", "generic"])
def test_misaligned_destinations_and_bodies(lib, full_max, form):
    """Bodies at odd offsets of one uploaded blob (a file's data section); outputs packed at running offsets by decompress_device_batch(into=…)
    and, through the C entry, with odd gaps between them.  At most 1 024 chunks the rest instance decodes the misaligned tensors with the
    generic code; above that the generic kernels take the call.  The bytes between and behind the tensors stay as they were (0x5A)."""
    from zipnn_amd import codec
    dev = torch.device("cuda:0")
    specs, datas = _ragged_batch(150, 17 + full_max, chunk=8192, n1=25, n4=20, full_max=full_max)
    total_chunks = sum(-(-nb // ch) for (_k, nb, _p, _r, _b, ch) in specs)
    assert (total_chunks <= 1024) == (form == REST)
    bodies = _oracle_bodies(specs, datas)
    srcs = _stage(lib, datas, dev)
    bd = _stage(lib, bodies, dev, odd=True)
    assert all(b.data_ptr() % 2 for b in bd if b.numel())
    items = [(b, P, rot, bm, ch, nb) for b, (_k, nb, P, rot, bm, ch) in zip(bd, specs)]
    n = sum(len(d) for d in datas)
    buf = torch.full((n + 4099,), 0x5A, dtype=torch.uint8, device=dev)
    codec.decompress_device_batch(lib, items, into=buf)
    assert lib.last_kernels() == ";".join([form] * 3)
    assert lib.last_tail_planes() == _tail_planes_expected(specs, bodies)
    assert torch.equal(buf[:n], torch.cat(srcs)) and bool((buf[n:] == 0x5A).all())
    # odd gaps between the outputs: nothing is written outside a tensor
    offs, o = [], 3
    for d in datas:
        offs.append(o); o += len(d) + 1 + 2 * (len(offs) % 3)
    buf = torch.full((o + 4096,), 0x5A, dtype=torch.uint8, device=dev)
    lib.decompress_batch_dev([(b.data_ptr(), b.numel(), P, rot, bm, ch, nb, buf.data_ptr() + off if nb else 0, None)
                              for b, off, (_k, nb, P, rot, bm, ch) in zip(bd, offs, specs)], torch.cuda.current_stream().cuda_stream, True)
    assert lib.last_kernels() == ";".join([form] * 3)
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=dev)
    for off, d in zip(offs, datas):
        mask[off:off + len(d)] = False
    assert bool((buf[mask] == 0x5A).all())
    _assert_same([buf[off:off + len(d)] for off, d in zip(offs, datas)], srcs, specs)


def test_delta_batch_with_many_tails(lib):
    """160 ragged two-plane tensors (and one- / four-plane ones) against base tensors: the XOR fused into the encoder (bodies == the oracle's
    frames of tensor ^ base) and into the decoder (zn_k_decode_fused^delta+tail, then the generic kernels finish the partial chunks)."""
    dev = torch.device("cuda:0")
    specs, _d = _ragged_batch(160, 19, chunk=8192, n1=30, n4=25, full_max=3)
    pairs = [_delta_pair(k, nb, 900 + i) for i, (k, nb, *_r) in enumerate(specs)]
    datas = [a for a, _b in pairs]
    xors = [(np.frombuffer(a, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes() for a, b in pairs]
    bodies = _oracle_bodies(specs, xors)
    srcs = _stage(lib, datas, dev)
    bases = _stage(lib, [b for _a, b in pairs], dev)
    got = _compress_and_check(lib, specs, srcs, bodies, deltas=bases)
    assert "^delta" in lib.last_kernels()
    outs = _decode(lib, specs, got, deltas=bases)
    k = lib.last_kernels()
    assert k.count("zn_k_decode_fused^delta+tail") == 3 and k.count("zn_k_merge_planes") == 3, k
    assert lib.last_tail_planes() == _tail_planes_expected(specs, bodies) > 200
    _assert_same(outs, srcs, specs)


def test_workspace_reuse_from_4097_to_129_tails_and_back(lib, request):
    """4 097 ragged tensors, then 129, then the 4 097 again, each checked (check = 1) and unchecked (check = 0 + zn_decode_status): the tail-sync
    words and tail flags a bigger call left in the workspace must not let a smaller call's merge run early, nor the reverse."""
    request.addfinalizer(lib.release_workspace)
    dev = torch.device("cuda:0")
    runs = []
    for n2 in (4097, 129):
        specs, datas, bodies = _batch(n2)
        runs.append((specs, _stage(lib, datas, dev), _stage(lib, bodies, dev), _tail_planes_expected(specs, bodies)))
    for specs, srcs, bd, tp in (runs[0], runs[1], runs[0]):
        for check in (True, False):
            outs = _decode(lib, specs, bd, check=check)
            if not check:
                lib.decode_status()
            assert lib.last_kernels() == ";".join([REST] * 3)
            assert lib.last_tail_planes() == tp
            _assert_same(outs, srcs, specs)


def test_llama_shaped_batch_with_many_ragged_tensors_on_two_streams(lib):
    """A Llama-shaped checkpoint (two layers: embeddings, linears, norms in bf16; an fp8 copy of the linears) plus 200 ragged bf16 biases / norms and
    150 ragged fp8 ones: both kinds have >= 512 chunks and > 128 ragged tensors, so the two kinds' launches run on two streams, each with merge
    workgroups of 16 per tensor.  Compressed by one batched call (every frame == the oracle's), decoded checked and unchecked."""
    import bench
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(8)
    C = 256 * KB
    flats, specs = [], []
    for name, shape, linear in bench.llama8b_shapes(layers=2):
        x = (torch.randn(shape, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        flats.append(x.reshape(-1).view(torch.uint8)); specs.append(("bf16", flats[-1].numel(), 2, 1, 10, C))
        if linear:
            flats.append(x.to(torch.float8_e4m3fn).reshape(-1).view(torch.uint8)); specs.append(("fp8", flats[-1].numel(), 1, 0, 10, 128 * KB))
    r = np.random.default_rng(9)
    for i in range(200):
        n = int(r.choice([4096, 1024, 2816, 14336, 896, 3584])) + int(r.integers(0, 3))
        flats.append((torch.randn(n, generator=g, device=dev) * 0.05).to(torch.bfloat16).view(torch.uint8)); specs.append(("bf16", 2 * n, 2, 1, 10, C))
    for i in range(150):
        n = int(r.choice([4096, 1024, 14336, 131072 + 4096])) + int(r.integers(0, 7))
        flats.append((torch.randn(n, generator=g, device=dev) * 0.5).to(torch.float8_e4m3fn).view(torch.uint8)); specs.append(("fp8", n, 1, 0, 10, 128 * KB))
    assert _chunks(specs, 1) >= 512 and _chunks(specs, 2) >= 512 and _ragged_count(specs, 1) > 128 and _ragged_count(specs, 2) > 128
    datas = [f.cpu().numpy() for f in flats]
    bodies = [O.compress_frame(HDR, d, P, rot, bm, ch, threads=16)[32:] for d, (_k, _n, P, rot, bm, ch) in zip(datas, specs)]
    del datas
    got = _compress_and_check(lib, specs, flats, bodies)
    tp = _tail_planes_expected(specs, bodies)
    for check in (True, False):
        outs = _decode(lib, specs, got, check=check)
        if not check:
            lib.decode_status()
        assert lib.last_kernels() == "(two streams);" + ";".join([REST] * 2)
        assert lib.last_tail_planes() == tp
        _assert_same(outs, flats, specs)
        del outs


def test_onepass_encoder_over_420_ragged_bf16_tensors(lib, request):
    """420 bf16 tensors, 6 300 full chunks in all, most of them ragged: the one-pass encoder's look-back runs across tensor boundaries and the partial
    chunks ride in its launches as ptails — forced (zn_set_encode_onepass 2) and in automatic mode (which may back off after a misspeculation, so the
    kernel is asserted only where it is forced); bodies == the oracle's both times, and the batch decodes back."""
    request.addfinalizer(lambda: lib.set_encode_onepass(1))
    dev = torch.device("cuda:0")
    specs, datas = _ragged_batch(420, 23, chunk=16 * KB, full_max=30, whole_every=0, kinds={2: [("bf16", 1)]})     # (16 KiB: the fused encoders take full chunks from there)
    assert _chunks(specs, 2, full_only=True) >= 6144 and _ragged_count(specs, 2) == 420
    bodies = _oracle_bodies(specs, datas)
    srcs = _stage(lib, datas, dev)
    lib.set_encode_onepass(2)
    got = _compress_and_check(lib, specs, srcs, bodies)
    assert "zn_k_encode_onepass" in lib.last_kernels()
    lib.set_encode_onepass(1)
    got = _compress_and_check(lib, specs, srcs, bodies)
    outs = _decode(lib, specs, got)
    _assert_same(outs, srcs, specs)


def test_checkpoint_of_300_mostly_ragged_tensors_end_to_end(lib, tmp_path):
    """A synthetic safetensors file of ~300 tensors — GPT-2 / Qwen-like biases and norms (ragged), a few matrices, in bf16 / fp16 / fp32 —
    through compress_safetensors_file(device="cuda:0"), load_file(device="cuda:0") and the plugin's safe_open(...).get_tensor: every tensor
    bit-exact, every frame's body == the oracle's."""
    from safetensors import safe_open
    from safetensors.torch import save_file
    from zipnn_amd import ZipNN, safetensors_io, zipnn_safetensors
    g = torch.Generator().manual_seed(29)
    tensors = {}
    for i in range(26):
        dt = (torch.bfloat16, torch.float16, torch.float32)[i % 3]
        p = f"model.layers.{i}."
        for n, shape in (("q_proj.bias", (896,)), ("k_proj.bias", (128,)), ("v_proj.bias", (128,)), ("input_layernorm.weight", (896,)),
                         ("post_attention_layernorm.weight", (896,)), ("attn.c_attn.bias", (2304,)), ("mlp.c_fc.bias", (3072,)),
                         ("mlp.c_proj.bias", (768 + i,)), ("ln_1.bias", (768,)), ("ln_2.weight", (768,)), ("router.weight", (8, 769 + 3 * i))):
            tensors[p + n] = (torch.randn(shape, generator=g) * 0.05).to(dt)
        if i % 4 == 0:
            tensors[p + "mlp.down_proj.weight"] = (torch.randn(300 + i, 1111, generator=g) * 0.02).to(dt)
    tensors["wte.weight"] = (torch.randn(5003, 768, generator=g) * 0.02).to(torch.bfloat16)
    tensors["position_ids"] = torch.arange(1024)
    assert 280 <= len(tensors) <= 320
    src = os.path.join(tmp_path, "m.safetensors")
    save_file(tensors, src, {"format": "pt"})
    znn = safetensors_io.compress_safetensors_file(src, device="cuda:0")
    assert "zn_k_encode" in lib.last_kernels()
    n_frames = 0
    with safe_open(znn, "pt", "cpu") as f:
        meta = f.metadata()
        for k, v in tensors.items():
            if not torch.is_floating_point(v):
                continue
            stored = f.get_tensor(k)
            if stored.dtype != torch.uint8:            # stored as it is (did not shrink)
                continue
            hdr, P, rot, bm, ch = ZipNN(input_format="torch", bytearray_dtype=v.dtype).torch_frame_plan(v)
            fr = stored.numpy().tobytes()
            assert fr[len(hdr):] == O.compress_frame(hdr, v.contiguous().view(torch.uint8).numpy(), P, rot, bm, ch)[len(hdr):], k
            n_frames += 1
    assert n_frames > 250 and meta
    loaded = safetensors_io.load_file(znn, device="cuda:0")
    assert "zn_k_decode" in lib.last_kernels()
    for k, v in tensors.items():
        assert loaded[k].is_cuda and loaded[k].dtype == v.dtype and loaded[k].shape == v.shape, k
        assert torch.equal(loaded[k].cpu().contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), k
    del loaded
    import safetensors
    import safetensors.torch
    orig_a, orig_b = safetensors.torch.safe_open, safetensors.safe_open
    try:
        zipnn_safetensors()
        with safetensors.safe_open(znn, framework="pt", device="cuda:0") as f:
            for k, v in tensors.items():
                t = f.get_tensor(k)
                assert t.is_cuda and torch.equal(t.cpu().contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), k
        assert "zn_k_decode" in lib.last_kernels()
    finally:
        safetensors.torch.safe_open, safetensors.safe_open = orig_a, orig_b
        from zipnn_amd import zipnn as _Z
        _Z._patches_applied.pop(_Z._zipnn_safetensors, None)      # (applied once per process: let a later test apply it again)
