"""GPU parity tests (-m gpu): the real libzipnn_hip.so on an MI355X against the CPU oracle,
the golden frames the reference produced, and size-independent properties at full size.
Bit-exact is the bar (integer/byte work): compressed bytes AND decompressed bytes."""
import hashlib

import numpy as np
import pytest
import torch

import golden_util as G
import oracle_lib as O
from test_oracle import gen_bytes

pytestmark = pytest.mark.gpu
HDR = bytes(range(32))
C = 256 * 1024
KB = 1024


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    return L


def _cases():
    cs = []
    for nb in (1, 2, 3, 6, 7, 1001, 1002, C - 2, C - 1, C, C + 1, C + 2, C + 6, 2 * C + 31338, 5 * C):
        cs += [("bf16", nb, 2, 1, 10, C), ("fp16", nb, 2, 0, 10, C), ("rand", nb, 2, 1, 10, C), ("const", nb, 2, 1, 10, C)]
    for nb in (4, 8, 1000, C - 4, C, C + 4, 2 * C + 4096, 1002, 7):
        cs += [("fp32", nb, 4, 1, 220, C), ("rand", nb, 4, 1, 220, C)]
    for nb in (1, 5, 1000, 128 * KB - 1, 128 * KB, 128 * KB + 1, 300001):
        cs += [("fp8", nb, 1, 1, 10, 128 * KB), ("rand", nb, 1, 1, 10, 128 * KB)]
    cs += [("bf16", 5 * 65536 + 10, 2, 1, 10, 65536), ("bf16", 9 * 16384 + 2, 2, 1, 10, 16384), ("bf16", 0, 2, 1, 10, C)]
    # thousands of (plane, chunk) entries: multi-workgroup size scan, plane starts inside scan blocks
    cs += [("bf16", 1024 * 1500 + 10, 2, 1, 10, 1024), ("fp32", 512 * 777 + 4, 4, 1, 220, 512), ("rand", 256 * 2049, 1, 1, 10, 256)]
    return cs


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"{c[0]}-{c[1]}-P{c[2]}-c{c[5]}")
def test_c_abi_bit_exact_vs_oracle(lib, case):
    kind, nb, P, rot, bm, chunk = case
    d = gen_bytes(kind, nb, 5)
    want = O.compress_frame(HDR, d, P, rot, bm, chunk, threads=4)
    got = bytes(lib.compress(HDR, d, P, rot, bm, chunk, 0.95))
    assert got == want
    if nb:
        assert bytes(lib.decompress(want[32:], P, rot, bm, chunk, nb)) == d


EDGE = [("skew", 4 * C, 1, 1, 10, 128 * KB, 8), ("skew", 4 * C, 2, 0, 10, C, 4), ("skew", 4 * C, 4, 1, 220, C, 4), ("skew", 4 * C, 2, 1, 10, C, 4), ("burst", 4 * C, 1, 1, 10, 128 * KB, 8),
        ("burst16", 8 * C, 2, 0, 10, C, 8), ("u11", 8 * C, 2, 1, 10, C, 8), ("burst16", 3 * 65536, 2, 0, 10, 65536, 3)]


@pytest.mark.gpu
def test_tree_descriptions_written_by_the_wave_on_hardware(lib):
    """The encoder's table kernel writes the tree description with the whole wave (v_readlane + scalar ALU chain,
    zn_wave_write_ctable): 236 planes of different statistics — FSE-coded weights, raw 4-bit weights, the secondary
    normalisation, equal weights, descriptions huff0 gives up on — frame identical to the oracle's (the serial
    HUF_writeCTable), and decoded back by the fused kernel, whose parser reads what the wave wrote."""
    from test_kernels_simt import _tree_description_planes
    chunk = 16384
    d = _tree_description_planes(chunk)
    want = O.compress_frame(HDR, d, 1, 0, 10, chunk, threads=4)
    lib.set_encode_onepass(True)
    try:
        got = bytes(lib.compress(HDR, d, 1, 0, 10, chunk, 0.95))          # the table job inside the one-pass encoder (wave 0 of a four-wave workgroup)
        assert got == want
        assert "zn_k_encode_onepass" in lib.last_kernels()
        lib.set_encode_onepass(False)
        got = bytes(lib.compress(HDR, d, 1, 0, 10, chunk, 0.95))          # … and as the table kernel's one-wave workgroup
    finally:
        lib.set_encode_onepass(1)
    assert got == want
    assert "zn_k_encode_tables" in lib.last_kernels()
    assert bytes(lib.decompress(got[32:], 1, 0, 10, chunk, len(d))) == d
    assert "zn_k_decode_fused" in lib.last_kernels()


@pytest.mark.parametrize("case", EDGE, ids=lambda c: f"{c[0]}-{c[1]}-P{c[2]}-c{c[5]}")
def test_fused_kernels_on_hostile_distributions(lib, case):
    """1-bit codes, tiles far denser than the stream average (staging buffer flushed in lane groups), 11-bit
    codes, every plane Huffman-coded (one accumulate pass per further plane): frame identical to the oracle's, decode through the fused kernel gives the input back."""
    from test_kernels_simt import _gen2
    kind, nb, P, rot, bm, chunk, want_fused = case
    d = _gen2(kind, nb, 13)
    want = O.compress_frame(HDR, d, P, rot, bm, chunk, threads=4)
    assert bytes(lib.compress(HDR, d, P, rot, bm, chunk, 0.95)) == want
    assert bytes(lib.decompress(want[32:], P, rot, bm, chunk, nb)) == d
    assert lib.last_fused_chunks() == want_fused


def test_two_streams_share_the_device_workspace_safely(lib):
    """Un-checked (asynchronous) decompress calls on two streams interleave; the library orders their use of
    its per-device workspace with an event, so both results are right."""
    from zipnn_amd import codec
    dev = torch.device("cuda:0")
    da = torch.frombuffer(bytearray(gen_bytes("bf16", 24 * C + 1000, 1)), dtype=torch.uint8).to(dev)
    db = torch.frombuffer(bytearray(gen_bytes("fp32", 16 * C + 4, 2)), dtype=torch.uint8).to(dev)
    ba = codec.compress_device(lib, da, 2, 1, 10, C, 0.95).clone()
    bb = codec.compress_device(lib, db, 4, 1, 220, C, 0.95).clone()
    oa = torch.zeros_like(da); ob = torch.zeros_like(db)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(20):
        with torch.cuda.stream(s1):
            codec.decompress_device(lib, ba, 2, 1, 10, C, da.numel(), out=oa, check=False)
        with torch.cuda.stream(s2):
            codec.decompress_device(lib, bb, 4, 1, 220, C, db.numel(), out=ob, check=False)
    torch.cuda.synchronize()
    assert torch.equal(oa, da) and torch.equal(ob, db)


def test_workspace_order_between_streams_runs_of_calls_and_a_destroyed_stream(lib):
    """As long as a device has seen one stream the workspace records no event (the stream orders the calls); the first call on a second stream synchronises
    the device and switches to an event per call.  Runs of asynchronous calls on three streams, whole-chunk tensors (the small-input kernel) and ragged
    ones; then a raw HIP stream that is used, synchronised and destroyed before the next call comes on another stream — the library never touches a stream
    handle after the call it came with."""
    import ctypes
    from zipnn_amd import codec
    dev = torch.device("cuda:0")
    specs = [("bf16", 32 * C, 2, 1, 10), ("fp32", 16 * C + 4, 4, 1, 220), ("bf16", 3 * C + 1000, 2, 1, 10), ("fp8", 9 * C, 1, 0, 10)]
    data = [torch.frombuffer(bytearray(gen_bytes(k, nb, 7 + i)), dtype=torch.uint8).to(dev) for i, (k, nb, *_r) in enumerate(specs)]
    bodies = [codec.compress_device(lib, d, P, rot, bm, C, 0.95).clone() for d, (_k, _n, P, rot, bm) in zip(data, specs)]
    outs = [torch.zeros_like(d) for d in data]
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    r = np.random.default_rng(5)
    for _ in range(40):
        s = streams[int(r.integers(3))]
        with torch.cuda.stream(s):
            for _k in range(int(r.integers(1, 5))):                  # a run of calls on this stream
                i = int(r.integers(len(specs)))
                _kind, nb, P, rot, bm = specs[i]
                codec.decompress_device(lib, bodies[i], P, rot, bm, C, nb, out=outs[i], check=False)
    torch.cuda.synchronize()
    for o, d in zip(outs, data):
        assert torch.equal(o, d)
    hip = ctypes.CDLL("libamdhip64.so")
    raw = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(raw)) == 0
    outs[0].zero_()
    lib.decompress_dev(bodies[0].data_ptr(), bodies[0].numel(), 2, 1, 10, C, specs[0][1], outs[0].data_ptr(), stream=raw.value, check=False)
    assert hip.hipStreamSynchronize(raw) == 0 and hip.hipStreamDestroy(raw) == 0
    assert torch.equal(outs[0], data[0])
    outs[1].zero_()
    codec.decompress_device(lib, bodies[1], 4, 1, 220, C, specs[1][1], out=outs[1], check=True)      # the previous stream no longer exists
    assert torch.equal(outs[1], data[1])


@pytest.mark.parametrize("group", [1, 2, 3, 4])
def test_fused_decode_chunk_groups(lib, group, decode_group, request):
    """Workgroups decode `group` consecutive chunks; mixed Huffman / raw / RLE / two-Huffman-plane chunks, short last group."""
    from test_kernels_simt import _gen2
    decode_group(lib, group)
    lib.set_decode_wide(0)                 # (a call this small would go to the wide kernel, one chunk per workgroup)
    request.addfinalizer(lambda: lib.set_decode_wide(1))
    ch = 65536
    r = np.random.default_rng(5)
    parts = []
    for k in range(23):
        kind = ["bf16", "rand", "const", "u11", "pair", "bf16", "burst16"][k % 7]
        parts.append(r.choice(np.array([1, 2, 3, 4], dtype=np.uint8), ch, p=[0.7, 0.1, 0.1, 0.1]).tobytes() if kind == "pair" else _gen2(kind, ch, 20 + k))
    d = b"".join(parts) + _gen2("bf16", 1000, 3)
    want = O.compress_frame(HDR, d, 2, 0, 10, ch, threads=4)
    assert bytes(lib.compress(HDR, d, 2, 0, 10, ch, 0.95)) == want
    assert bytes(lib.decompress(want[32:], 2, 0, 10, ch, len(d))) == d
    assert lib.last_fused_chunks() == 23               # incl. the three "pair" chunks (two Huffman planes: two passes)


@pytest.mark.parametrize("kind,P,rot,bm", [("bf16", 2, 1, 10), ("fp32", 4, 1, 220), ("fp16", 2, 0, 10), ("fp8", 1, 0, 10), ("slowsync", 2, 0, 10), ("mixed", 2, 0, 10)])
def test_wide_decoder_for_small_inputs_on_hardware(lib, kind, P, rot, bm, request):
    """zn_k_decode_wide (16 waves per chunk, four per huff0 stream, tile tops guessed and checked across waves): every mode of
    zn_set_decode_wide gives the input back — 1, 7 + tail, 20 + a 1 KB tail, 200 and 257 chunks, repeated (the waves of a workgroup race differently
    every time), with the frame equal to the oracle's.  Automatic mode uses it up to one chunk per CU."""
    from test_kernels_simt import _gen2, _slow_sync_bf16
    request.addfinalizer(lambda: lib.set_decode_wide(1))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for nb in (C, 7 * C + C // 2 + 10, 20 * C + 1000, 200 * C, (cus + 1) * C, (2 * cus + 1) * C):
        if kind == "slowsync":
            d = _slow_sync_bf16(nb, 3)
        elif kind == "mixed":          # chunk by chunk: weights-like, incompressible, constant, two Huffman planes, dense
            d = b"".join(_gen2(["bf16", "rand", "const", "u11", "bf16", "burst16"][k % 6], min(C, nb - k * C), 50 + k) for k in range((nb + C - 1) // C))
        else:
            d = _gen2(kind, nb, 31)
        frame = O.compress_frame(HDR, d, P, rot, bm, C, threads=8)
        assert bytes(lib.compress(HDR, d, P, rot, bm, C, 0.95)) == frame
        K = (nb + C - 1) // C
        for mode in (1, 2, 3, 0):
            lib.set_decode_wide(mode)
            for _ in range(6 if nb <= 8 * C else 2):
                assert bytes(lib.decompress(frame[32:], P, rot, bm, C, nb)) == d, (kind, nb, mode)
            used = lib.last_kernels().split(";")[0]
            full = nb // C
            slots = full + (4 * P + 32 if nb % C else 0)         # (a partial last chunk: four tail workgroups per plane + its merge workgroups)
            want = {0: "zn_k_decode_fused", 2: "zn_k_decode_wide", 3: "zn_k_decode_wide^2",
                    1: "zn_k_decode_fused" if rot != 1 or slots > 2 * cus else "zn_k_decode_wide" if slots <= cus else "zn_k_decode_wide^2"}[mode]
            # (automatic: sign-rotated layouts whose full chunks and — round 6 — tail workgroups find a workgroup slot each: one per CU in the 16-wave form, two in the 8-wave form)
            assert used.split("+")[0].replace("^rest", "") == want, (used, mode, K)       # (a call of whole chunks: the fused kernel's rest instance, no generic launches)
            assert lib.last_fused_chunks() >= (nb // C if kind in ("bf16", "fp32", "fp16", "fp8", "slowsync") else 0)


@pytest.mark.parametrize("name", G.names())
def test_golden_frames_through_zipnn_api(lib, name):
    from zipnn_amd import ZipNN
    meta, blob = G.get(name)
    ctor = dict(meta["ctor"])
    back = ZipNN(**ctor).decompress(blob)
    if meta["kind"] == "torch":
        assert str(back.dtype) == "torch." + meta["dtype"] and list(back.shape) == meta["shape"]
        raw = back.contiguous().view(torch.uint8).numpy().tobytes()
        src = back.clone()
    else:
        raw, src = bytes(back), bytes(back)
    assert G.sha(raw) == meta["in_sha256"]
    assert G.sha(bytes(ZipNN(**ctor).compress(src))) == meta["frame_sha256"]
    if meta["kind"] == "torch":   # device-resident variant: same frame, same tensor
        assert G.sha(bytes(ZipNN(**ctor).compress(back.cuda()))) == meta["frame_sha256"]
        dev = ZipNN(**ctor).decompress(blob, decompress_cpu_gpu="cuda")
        assert dev.is_cuda and dev.cpu().view(torch.uint8).numpy().tobytes() == raw


@pytest.mark.parametrize("name", G.delta_names())
def test_reference_written_delta_frames_through_zipnn_api(lib, name):
    """Frames the REFERENCE wrote in its delta mode (tests/golden/make_golden_delta.py; reference zipnn/zipnn.py:625-640, 983-1004,
    its tests/simple_stress_tests.py:85-150,180-203) decode on the GPU — XOR fused into the decode kernels — to the reference's input,
    and the GPU encoder (XOR fused into stats / emit) writes the reference's frame back, byte for byte."""
    from zipnn_amd import ZipNN
    meta, blob, base = G.delta_get(name)
    ctor = dict(meta["ctor"])
    back = bytes(ZipNN(**ctor).decompress(blob, delta_second_data=base))
    assert len(back) == meta["in_len"] and G.sha(back) == meta["in_sha256"]
    assert G.sha(bytes(ZipNN(**ctor).compress(back, delta_second_data=base))) == meta["frame_sha256"]


def test_reference_stress_sizes_roundtrip(lib):
    """Sizes of the reference's tests/simple_stress_tests.py:19-70 (chunk boundary ±1 KiB)."""
    from zipnn_amd import ZipNN
    sizes = [255 * KB, 256 * KB, 257 * KB, 511 * KB, 512 * KB, 513 * KB, 1024 * KB, int(0.99 * KB * KB), KB * KB,
             int(1.01 * KB * KB), int(1.99 * KB * KB), 2 * KB * KB, int(2.1 * KB * KB)]
    for s in sizes:
        t = (torch.rand(s // 2) * 2 - 1).to(torch.bfloat16)
        z = ZipNN(input_format="torch")
        frame = z.compress(t.clone())
        assert torch.equal(ZipNN(input_format="torch").decompress(frame), t)
        raw = t.view(torch.uint8).numpy().tobytes()
        p = G.parse_frame(bytes(frame))
        assert bytes(frame) == O.compress_frame(p["header"], raw, 2, 1, 10, C, threads=4)
        b = np.random.default_rng(s).integers(0, 256, s, dtype=np.uint8).tobytes()
        assert bytes(ZipNN(bytearray_dtype="bfloat16").decompress(ZipNN(bytearray_dtype="bfloat16").compress(b))) == b


def test_256MiB_bf16_bit_exact_vs_oracle(lib):
    """BASELINE.json configs[0] size on the GPU: frame identical to the oracle's, and round trip."""
    from zipnn_amd import codec
    g = torch.Generator().manual_seed(1234)
    x = (torch.randn(128 * KB * KB, generator=g) * 0.02).to(torch.bfloat16)
    raw = x.view(torch.uint8).numpy()
    want = O.compress_frame(bytes(32), raw, 2, 1, 10, C, threads=8)
    body = codec.compress_device(lib, codec.flat_bytes(x.cuda()), 2, 1, 10, C, 0.95)
    got = body.cpu().numpy().tobytes()
    assert hashlib.sha256(got).hexdigest() == hashlib.sha256(want[32:]).hexdigest()
    out = codec.decompress_device(lib, body, 2, 1, 10, C, raw.size)
    assert torch.equal(out.cpu(), torch.from_numpy(raw))
    assert lib.last_fused_chunks() == raw.size // C      # every chunk through the single-pass kernel
    assert 0.655 < len(want) / raw.size < 0.670          # README: 66.3 % on bf16


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32", "fp8"])
def test_full_size_roundtrip_properties(lib, dtype):
    """1 GiB per dtype (4 GiB bf16 is exercised by bench.py): decode(encode(x)) == x, the body's
    metadata is self-consistent, and the whole body equals the CPU oracle's, byte for byte."""
    from zipnn_amd import codec
    n_bytes = 1 << 30
    torch.manual_seed(7)
    if dtype == "bf16":
        x = (torch.randn(n_bytes // 2, device="cuda") * 0.02).to(torch.bfloat16); P, rot, bm = 2, 1, 10
    elif dtype == "fp16":
        x = (torch.randn(n_bytes // 2, device="cuda") * 0.02).half(); P, rot, bm = 2, 0, 10
    elif dtype == "fp8":
        x = (torch.randn(n_bytes, device="cuda") * 0.02).to(torch.float8_e4m3fn); P, rot, bm = 1, 0, 10
    else:
        x = torch.randn(n_bytes // 4, device="cuda") * 0.02; P, rot, bm = 4, 1, 220
    C = 256 * KB if P > 1 else 128 * KB          # (the reference caps fp8 chunks at 128 KiB, zipnn.py:721)
    flat = codec.flat_bytes(x)
    body = codec.compress_device(lib, flat, P, rot, bm, C, 0.95)
    out = codec.decompress_device(lib, body, P, rot, bm, C, n_bytes)
    assert torch.equal(out, flat)
    K = n_bytes // C
    hb = body[: 9 * P * K].cpu().numpy()
    types = hb[: P * K].reshape(P, K)
    cum = hb[P * K:].view(np.uint64).reshape(P, K)
    assert set(np.unique(types)) <= {0, 1}
    assert (np.diff(cum.astype(np.int64), axis=1) > 0).all()
    assert 9 * P * K + int(cum[:, -1].sum()) == body.numel()
    # the WHOLE 1 GiB body equals the CPU oracle's (16 host threads: a second or so)
    want = O.compress_frame(b"", flat.cpu().numpy(), P, rot, bm, C, threads=16)
    assert body.numel() == len(want) and hashlib.sha256(body.cpu().numpy().tobytes()).hexdigest() == hashlib.sha256(want).hexdigest()


def test_beyond_4GiB_offsets_roundtrip(lib):
    """5 GiB + a ragged tail: every byte offset in the path is 64-bit (input offsets > 2^32, payload offsets
    > 2^32 in the second plane).  Round trip exact; the last full chunk and the tail equal the oracle's bytes."""
    from zipnn_amd import codec
    n_bytes = 5 * (1 << 30) + 3 * C + 1234
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    x = torch.empty(n_bytes // 2, dtype=torch.bfloat16, device="cuda")
    for off in range(0, x.numel(), 1 << 27):
        m = min(1 << 27, x.numel() - off)
        x[off:off + m] = (torch.randn(m, generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    flat = codec.flat_bytes(x)
    body = codec.compress_device(lib, flat, 2, 1, 10, C, 0.95)
    K = (n_bytes + C - 1) // C
    cum = body[2 * K: 2 * K + 16 * K].cpu().numpy().view(np.uint64).reshape(2, K)
    assert int(cum[0, -1]) > (1 << 31) and 18 * K + int(cum[:, -1].sum()) == body.numel()
    out = codec.decompress_device(lib, body, 2, 1, 10, C, n_bytes)
    assert lib.last_fused_chunks() == K - 1
    assert torch.equal(out, flat)
    # the bytes of the last full chunk and of the tail chunk, against the oracle
    for c in (K - 2, K - 1):
        raw = flat[c * C: min((c + 1) * C, n_bytes)].cpu().numpy().tobytes()
        ofr = O.compress_frame(b"", raw, 2, 1, 10, C)
        osz = np.frombuffer(ofr[2:2 + 16], dtype=np.uint64); opay = ofr[18:]
        base = 18 * K; off_o = 0
        for p in range(2):
            lo = int(cum[p, c - 1])
            mine = body[base + lo: base + int(cum[p, c])].cpu().numpy().tobytes()
            assert mine == opay[off_o: off_o + int(osz[p])]
            off_o += int(osz[p]); base += int(cum[p, -1])


def test_batched_decode_many_tensors(lib):
    """zn_decompress_batch_dev on the GPU: every plane count, tails, tiny and empty tensors in one call; the
    results equal the inputs and the per-tensor decode."""
    from zipnn_amd import codec
    dev = torch.device("cuda:0")
    specs = [("bf16", 40 * C + 10, 2, 1, 10, C), ("fp32", 9 * C + 4, 4, 1, 220, C), ("fp8", 5 * 128 * KB + 1, 1, 1, 10, 128 * KB),
             ("bf16", 7, 2, 1, 10, C), ("bf16", 0, 2, 1, 10, C), ("fp16", 33 * C, 2, 0, 10, C), ("rand", 4 * C, 2, 1, 10, C),
             ("const", 2 * C, 2, 1, 10, C), ("fp32", 1000, 4, 1, 220, C)] + [("bf16", 3 * C + 2 * i, 2, 1, 10, C) for i in range(40)]
    datas, items = [], []
    for i, (kind, nb, P, rot, bm, chunk) in enumerate(specs):
        d = gen_bytes(kind, nb, 50 + i)
        frame = O.compress_frame(HDR, d, P, rot, bm, chunk, threads=4)
        body = frame[32:]
        datas.append(d)
        items.append(((torch.frombuffer(bytearray(body), dtype=torch.uint8) if body else torch.empty(0, dtype=torch.uint8)).to(dev), P, rot, bm, chunk, nb))
    outs = codec.decompress_device_batch(lib, items)
    for d, o in zip(datas, outs):
        assert o.cpu().numpy().tobytes() == d
    assert "zn_k_decode_fused" in lib.last_kernels()


def test_mixed_batch_of_two_full_kinds_runs_on_two_streams(lib):
    """A batch whose one-plane tensors and whose multi-plane tensors each fill the chip (>= 512 chunks per kind: what a checkpoint with an fp8 copy of its
    linears looks like) forks the two kinds' launches onto two streams of the library's own and joins them: same bytes as the sources,
    with ragged tensors of both kinds in it, through the unchecked (check = 0 + zn_decode_status) entry as well."""
    from zipnn_amd import codec
    dev = torch.device("cuda:0")
    specs = [("fp8", 330 * 128 * KB + 7001, 1, 0, 10, 128 * KB), ("bf16", 300 * C, 2, 1, 10, C), ("fp8", 200 * 128 * KB, 1, 0, 10, 128 * KB),
             ("fp32", 100 * C + 12, 4, 1, 220, C), ("bf16", 130 * C + 100000, 2, 1, 10, C), ("fp16", 9 * C, 2, 0, 10, C)]
    datas, items = [], []
    for i, (kind, nb, P, rot, bm, chunk) in enumerate(specs):
        d = gen_bytes(kind, nb, 80 + i)
        frame = O.compress_frame(HDR, d, P, rot, bm, chunk, threads=8)
        datas.append(d)
        items.append((torch.frombuffer(bytearray(frame[32:]), dtype=torch.uint8).to(dev), P, rot, bm, chunk, nb))
    for check in (True, False):
        outs = codec.decompress_device_batch(lib, items, check=check)
        if not check:
            lib.decode_status()
        assert "(two streams)" in lib.last_kernels()
        for d, o in zip(datas, outs):
            assert o.cpu().numpy().tobytes() == d


@pytest.mark.parametrize("case", [("bf16", 5 * C + C // 2 + 10, 2, 1, 10, C, 1), ("bf16", C // 2 + 3, 2, 1, 10, C, 1),
                                  ("fp32", 2 * C + C // 2 + 4, 4, 1, 220, C, 1), ("fp8", 128 * KB + 70001, 1, 1, 10, 128 * KB, 1),
                                  ("fp16", 3 * C - 2, 2, 0, 10, C, 1), ("skew", C + 130000, 2, 0, 10, C, 2),
                                  ("burst", 100001, 1, 1, 10, 128 * KB, 1), ("rand", C + 30000, 2, 1, 10, C, 0)],
                         ids=lambda c: f"{c[0]}-{c[1]}-P{c[2]}")
def test_partial_last_chunk_through_the_parallel_tail_kernel(lib, case):
    """Big partial last chunks: Huffman planes by the tail workgroups of zn_k_decode_fused (ragged streams, padded scratch), exact output."""
    from test_kernels_simt import _gen2
    kind, nb, P, rot, bm, chunk, want_tail_planes = case
    d = _gen2(kind, nb, 17)
    want = O.compress_frame(HDR, d, P, rot, bm, chunk, threads=4)
    assert bytes(lib.compress(HDR, d, P, rot, bm, chunk, 0.95)) == want
    assert bytes(lib.decompress(want[32:], P, rot, bm, chunk, nb)) == d
    assert lib.last_tail_planes() == want_tail_planes


def test_large_ragged_tensor_keeps_its_merge_inside_the_launch(lib):
    """More than ZN_REST_MAX_CHUNKS chunks + a partial one (round 6): the launch takes the rest instance — tail workgroups in front, merge workgroups at its end — instead of
    the plain instance + the generic merge kernel behind it; exact bytes, and a small tail (a plane of 1 500 bytes: from 512 bytes up the tail workgroups take it).
    An even tensor of the same size still takes the plain instance and the (idle) generic launches."""
    from zipnn_amd import codec
    dev = torch.device("cuda:0")
    for tail, tail_planes in ((200000, 1), (3000, 1), (600, 0)):
        n = 2100 * C + tail
        g = torch.Generator(device=dev); g.manual_seed(3)
        x = (torch.randn(n // 2, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        flat = codec.flat_bytes(x)
        body = codec.compress_device(lib, flat, 2, 1, 10, C, 0.95).clone()
        out = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
        for _ in range(3):
            codec.decompress_device(lib, body, 2, 1, 10, C, n, out=out)
            assert torch.equal(out, flat)
        assert lib.last_kernels() == "zn_k_decode_fused^rest+tail+merge" and lib.last_tail_planes() == tail_planes
        del x, flat, body, out
    n = 2100 * C
    x = (torch.randn(n // 2, device=dev) * 0.02).to(torch.bfloat16)
    flat = codec.flat_bytes(x)
    body = codec.compress_device(lib, flat, 2, 1, 10, C, 0.95).clone()
    assert torch.equal(codec.decompress_device(lib, body, 2, 1, 10, C, n), flat)
    assert lib.last_kernels() == "zn_k_decode_fused;zn_k_decode_planes;zn_k_merge_planes"


def test_streaming_blob_decodes_in_one_batched_launch(lib):
    """is_streaming BYTE frames (1 MiB each): the decompress side parses every header on the host and decodes all
    frames with one batched launch; bytes equal the input, and a delta (XOR) second buffer composes."""
    from zipnn_amd import ZipNN
    raw = gen_bytes("bf16", 24 * (1 << 20) + 12346, 77)
    z = ZipNN(bytearray_dtype="bfloat16", is_streaming=True, streaming_chunk=1 << 20)
    blob = z.compress(raw)
    assert isinstance(blob, bytearray) and len(blob) < len(raw)
    back = ZipNN(bytearray_dtype="bfloat16", is_streaming=True, streaming_chunk=1 << 20).decompress(blob)
    assert isinstance(back, bytearray) and bytes(back) == raw
    assert "zn_k_decode_fused" in lib.last_kernels()
    other = gen_bytes("bf16", len(raw), 78)
    zd = ZipNN(bytearray_dtype="bfloat16", is_streaming=True, streaming_chunk=1 << 20, delta_compressed_type="byte")
    blob2 = zd.compress(raw, delta_second_data=other)
    back2 = ZipNN(bytearray_dtype="bfloat16", is_streaming=True, streaming_chunk=1 << 20, delta_compressed_type="byte").decompress(blob2, delta_second_data=other)
    assert bytes(back2) == raw


def test_batched_compress_many_tensors(lib):
    """zn_compress_batch_dev on the GPU: every body equals the oracle's, the batch decodes back in one call."""
    from zipnn_amd import codec
    from test_kernels_simt import _gen2
    dev = torch.device("cuda:0")
    specs = [("bf16", 40 * C + 10, 2, 1, 10, C), ("fp32", 9 * C + 4, 4, 1, 220, C), ("fp8", 5 * 128 * KB + 1, 1, 1, 10, 128 * KB),
             ("bf16", 7, 2, 1, 10, C), ("bf16", 0, 2, 1, 10, C), ("fp16", 33 * C, 2, 0, 10, C), ("rand", 4 * C, 2, 1, 10, C),
             ("const", 2 * C, 2, 1, 10, C), ("fp32", 1000, 4, 1, 220, C), ("bf16", 4096 * 5 + 2, 2, 1, 10, 4096),
             ("skew", C + 130000, 2, 0, 10, C)] + [("bf16", 3 * C + 2 * i, 2, 1, 10, C) for i in range(20)]
    datas, items = [], []
    for i, (kind, nb, P, rot, bm, chunk) in enumerate(specs):
        d = _gen2(kind, nb, 80 + i)
        datas.append(d)
        items.append(((torch.frombuffer(bytearray(d), dtype=torch.uint8) if d else torch.empty(0, dtype=torch.uint8)).to(dev), P, rot, bm, chunk, 0.95))
    bodies = codec.compress_device_batch(lib, items)
    for (kind, nb, P, rot, bm, chunk), d, b in zip(specs, datas, bodies):
        assert b.cpu().numpy().tobytes() == O.compress_frame(HDR, d, P, rot, bm, chunk, threads=4)[32:], kind
    outs = codec.decompress_device_batch(lib, [(b, P, rot, bm, chunk, nb) for b, (kind, nb, P, rot, bm, chunk) in zip(bodies, specs)])
    for d, o in zip(datas, outs):
        assert o.cpu().numpy().tobytes() == d


def test_safetensors_file_through_hbm_batched_both_ways(lib, tmp_path):
    """compress_safetensors_file(device="cuda:0") stages the tensors in HBM and compresses the file with one batched
    call; load_file decodes it with one batched call; a CPU-side per-tensor read of the same file agrees."""
    import os
    import safetensors
    from safetensors.torch import save_file
    from zipnn_amd import safetensors_io, zipnn_safetensors
    g = torch.Generator().manual_seed(3)
    tensors = {"w_bf16": (torch.randn(700, 1000, generator=g) * 0.02).to(torch.bfloat16),
               "w_fp16": (torch.randn(300, 1001, generator=g) * 0.02).half(),
               "w_fp32": torch.randn(513, 400, generator=g) * 0.02,
               "ids": torch.arange(1000), "tiny": torch.randn(3, generator=g).to(torch.bfloat16),
               "w_fp8": (torch.randn(200, 3000, generator=g) * 0.02).to(torch.float8_e4m3fn),
               "noise": torch.randint(0, 256, (40000,), generator=g, dtype=torch.uint8).view(torch.float16),     # does not shrink: stored as it is
               "empty": torch.empty(0, 7, dtype=torch.bfloat16)}
    src = os.path.join(tmp_path, "m.safetensors")
    save_file(tensors, src, {"format": "pt"})
    znn = safetensors_io.compress_safetensors_file(src, device="cuda:0")          # one upload, one batched compress, one download (_compress_file_on_device)
    assert os.path.getsize(znn) < os.path.getsize(src)
    per_tensor = safetensors_io.compress_safetensors_file(src, out_path=os.path.join(tmp_path, "p.znn.safetensors"), device="cuda:0", batched=False)
    from test_plugin_simt import _same_safetensors_container
    assert _same_safetensors_container(znn, per_tensor)                            # the same file as tensor by tensor
    assert "zn_k_encode_emit" in lib.last_kernels() or "zn_k_encode_onepass" in lib.last_kernels()
    loaded = safetensors_io.load_file(znn, device="cuda:0")
    for k, v in tensors.items():
        assert loaded[k].dtype == v.dtype and loaded[k].shape == v.shape and loaded[k].is_cuda
        assert torch.equal(loaded[k].cpu().contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), k
    cpu_path = safetensors_io.compress_safetensors_file(src, out_path=os.path.join(tmp_path, "c.znn.safetensors"))
    with safetensors.safe_open(cpu_path, "pt", "cpu") as fa, safetensors.safe_open(znn, "pt", "cpu") as fb:
        for k in fa.keys():
            assert torch.equal(fa.get_tensor(k).view(torch.uint8), fb.get_tensor(k).view(torch.uint8)), k


def _random_cases(n_cases, seed, max_bytes):
    r = np.random.default_rng(seed)
    kinds = ["bf16", "fp16", "fp32", "fp8", "rand", "const", "skew", "burst", "u11"]
    out = []
    for _ in range(n_cases):
        P = int(r.choice([1, 2, 2, 2, 4]))
        kind = str(r.choice(kinds))
        bm = 220 if P == 4 else 10
        rot = int(r.integers(0, 2)) if P > 1 else int(r.integers(0, 2))
        # chunk: any multiple of P — tiny, odd multiples, fused-eligible ones, the default
        chunk = int(r.choice([P * int(r.integers(1, 400)), 4096 * P, 16384, 65536, 3 * 16384, C, 12 * P * 1024 + P]))
        chunk -= chunk % P
        chunk = max(chunk, P)
        nb = int(r.integers(0, max_bytes))
        if r.random() < 0.3:
            nb -= nb % chunk                                  # exact multiples too
        thr = float(r.choice([0.95, 0.95, 0.5, 1.0, 0.99]))
        out.append((kind, nb, P, rot, bm, chunk, thr))
    return out


def test_randomised_geometry_sweep_bit_exact(lib):
    """160 random (distribution, size, planes, rotate, chunk size, threshold) combinations, incl. chunk sizes the fused
    kernels do not take: frame == oracle frame byte for byte, decode == input; then all of them again through the
    batched entry points."""
    from test_kernels_simt import _gen2
    from zipnn_amd import codec
    dev = torch.device("cuda:0")
    cases = _random_cases(160, 2026, 3 * C)
    datas, frames = [], []
    for i, (kind, nb, P, rot, bm, chunk, thr) in enumerate(cases):
        d = _gen2(kind, nb, 1000 + i)
        nb = len(d)                                            # 'u11' rounds down to whole bf16 values
        cases[i] = (kind, nb, P, rot, bm, chunk, thr)
        want = O.compress_frame(HDR, d, P, rot, bm, chunk, thr, threads=4)
        got = bytes(lib.compress(HDR, d, P, rot, bm, chunk, thr))
        assert got == want, (i, cases[i])
        if nb:
            assert bytes(lib.decompress(want[32:], P, rot, bm, chunk, nb)) == d, (i, cases[i])
        datas.append(d); frames.append(want)
    flats = [(torch.frombuffer(bytearray(d), dtype=torch.uint8) if d else torch.empty(0, dtype=torch.uint8)).to(dev) for d in datas]
    bodies = codec.compress_device_batch(lib, [(f, P, rot, bm, chunk, thr) for f, (kind, nb, P, rot, bm, chunk, thr) in zip(flats, cases)])
    for i, (b, fr) in enumerate(zip(bodies, frames)):
        assert b.cpu().numpy().tobytes() == fr[32:], (i, cases[i])
    outs = codec.decompress_device_batch(lib, [(b, P, rot, bm, chunk, nb) for b, (kind, nb, P, rot, bm, chunk, thr) in zip(bodies, cases)])
    for i, (o, d) in enumerate(zip(outs, datas)):
        assert o.cpu().numpy().tobytes() == d, (i, cases[i])


@pytest.mark.parametrize("case", [("bf16", 6 * C + 1234, 2, 1, 10, C), ("fp32", 3 * C + 4 * 77, 4, 1, 220, C), ("fp8", 5 * 65536 + 5, 1, 1, 10, 65536),
                                  ("bf16", 70001, 2, 1, 10, 4442), ("fp16", 4 * C, 2, 0, 10, C)],
                         ids=lambda c: f"{c[0]}-{c[1]}-P{c[2]}-c{c[5]}")
def test_delta_xor_fused_into_the_kernels(lib, case):
    """compress(data, delta=base) == oracle frame of data ^ base; decompress(frame, delta=base) == data: host and
    device entry points, aligned (fused kernels) and unaligned (generic kernels) base."""
    from test_kernels_simt import _delta_pair
    from zipnn_amd import codec
    dev = torch.device("cuda:0")
    kind, nb, P, rot, bm, chunk = case
    a, b = _delta_pair(kind, nb, 31)
    nb = len(a)
    x = (np.frombuffer(a, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes()
    want = O.compress_frame(HDR, x, P, rot, bm, chunk, threads=4)
    assert bytes(lib.compress(HDR, a, P, rot, bm, chunk, 0.95, delta=b)) == want
    assert bytes(lib.decompress(want[32:], P, rot, bm, chunk, nb, delta=b)) == a
    assert "zn_k_decode_fused^delta" in lib.last_kernels()
    ta = torch.frombuffer(bytearray(a), dtype=torch.uint8).to(dev)
    for shift in (0, 1):
        pad = torch.zeros(nb + 16, dtype=torch.uint8, device=dev)
        pad[shift:shift + nb] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
        tb = pad[shift:shift + nb]
        body = codec.compress_device(lib, ta, P, rot, bm, chunk, 0.95, delta=tb)
        assert body.cpu().numpy().tobytes() == want[32:]
        out = codec.decompress_device(lib, body, P, rot, bm, chunk, nb, delta=tb)
        assert out.cpu().numpy().tobytes() == a
        if shift:
            assert lib.last_fused_chunks() == 0
        elif nb >= chunk and chunk % 16384 == 0:
            assert lib.last_fused_chunks() == nb // chunk


def test_delta_device_resident_256MiB_roundtrip_and_ratio(lib):
    """A `fine-tuned` bf16 tensor against its base, both in HBM: the body of x ^ base is what compressing the XOR
    computed by torch gives, decoding with the base returns x; a sparse delta compresses far below the plain ratio."""
    from zipnn_amd import codec
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    base = (torch.randn(128 << 20, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    x = base.clone()
    idx = torch.randint(0, x.numel(), (x.numel() // 50,), device=dev, generator=g)
    x[idx] = (x[idx].float() * 1.01).to(torch.bfloat16)
    fx, fb = codec.flat_bytes(x), codec.flat_bytes(base)
    body = codec.compress_device(lib, fx, 2, 1, 10, C, 0.95, delta=fb)
    ref = codec.compress_device(lib, torch.bitwise_xor(fx, fb), 2, 1, 10, C, 0.95)
    assert torch.equal(body, ref)
    out = codec.decompress_device(lib, body, 2, 1, 10, C, fx.numel(), delta=fb)
    assert torch.equal(out, fx)
    assert lib.last_fused_chunks() == fx.numel() // C
    assert body.numel() < 0.2 * fx.numel()


def test_replicated_decode_single_rank(lib):
    """sharding.decompress_replicated without a process group: rank 0 of 1 decodes everything (the N>1 path is covered
    by the gloo test; 8-GPU boxes are the driver's)."""
    from test_oracle import gen_bytes
    from zipnn_amd import sharding
    nb = 9 * C + 4321
    d = gen_bytes("bf16", nb, 4)
    body = O.compress_frame(b"", d, 2, 1, 10, C, threads=4)
    out = sharding.decompress_replicated(lib, body, 2, 1, 10, C, nb, torch.device("cuda:0"))
    assert out.cpu().numpy().tobytes() == d


@pytest.mark.gpu
def test_replicated_decode_through_rccl_with_a_group_of_one(lib):
    """The exchange step of sharding.decompress_replicated on the device: a one-rank `nccl` (= RCCL) process group, so that
    the decoded shard goes through all_gather_into_tensor on the GPU (the 2-rank case: tests/test_sharding_gloo.py on CPU;
    more GPUs than one are the driver's)."""
    import socket
    import torch.distributed as dist
    from test_oracle import gen_bytes
    from zipnn_amd import sharding
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        nb = 11 * C + 777
        d = gen_bytes("bf16", nb, 6)
        body = O.compress_frame(b"", d, 2, 1, 10, C, threads=4)
        out = sharding.decompress_replicated(lib, body, 2, 1, 10, C, nb, torch.device("cuda:0"))
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == d
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_pinned_host_pipe_copies_and_host_entry_points(lib, monkeypatch):
    """zn_copy_to_device / zn_copy_to_host (the pinned, multi-threaded transfer of zn_host_pipe.hpp) move pageable
    buffers bit-exactly for sizes around its slice and stripe boundaries, with several thread counts; the
    host-buffer entry points built on it return the oracle's frame and the original bytes."""
    from zipnn_amd import codec
    rng = np.random.default_rng(11)
    for n, threads, slice_mb in ((1, "8", None), (3 * 1024 * 1024 + 5, "3", None), (70 * 1024 * 1024 + 123, "8", None),
                                 (33 * 1024 * 1024 + 64, "16", None)):
        monkeypatch.setenv("ZN_HOST_THREADS", threads)
        host = rng.integers(0, 256, n, dtype=np.uint8)
        t = codec.to_device(lib, host, torch.device("cuda:0"))
        assert t.is_cuda and t.numel() == n and np.array_equal(t.cpu().numpy(), host)
        t2 = (t ^ 0x5A).contiguous()
        back = codec.to_host(lib, t2)
        assert isinstance(back, bytearray) and np.array_equal(np.frombuffer(back, dtype=np.uint8), host ^ 0x5A)
    # host-buffer entry points, 40 MiB + a ragged tail (several slices each way)
    n = 40 * 1024 * 1024 + 4098
    x = (torch.randn(n // 2, generator=torch.Generator().manual_seed(3)) * 0.02).to(torch.bfloat16)
    raw = x.view(torch.uint8).numpy().tobytes()
    frame = lib.compress(bytes(32), raw, 2, 1, 10, 256 * 1024, 0.95)
    want = O.compress_frame(bytes(32), raw, 2, 1, 10, 256 * 1024)
    assert bytes(frame[32:]) == want[32:]
    assert bytes(lib.decompress(memoryview(frame)[32:], 2, 1, 10, 256 * 1024, n)) == raw


@pytest.mark.gpu
def test_host_entry_points_from_concurrent_threads(lib):
    """Two Python threads call the host-buffer entry points at once (ctypes releases the GIL): the calls serialise on
    the device's staging buffers and both return the right bytes."""
    import threading
    n = 24 * 1024 * 1024
    raws, frames, errs = [], [None, None], []
    for seed in (1, 2):
        x = (torch.randn(n // 2, generator=torch.Generator().manual_seed(seed)) * 0.02).to(torch.bfloat16)
        raws.append(x.view(torch.uint8).numpy().tobytes())

    def work(i):
        try:
            for _ in range(3):
                f = lib.compress(bytes(32), raws[i], 2, 1, 10, 256 * 1024, 0.95)
                back = lib.decompress(memoryview(f)[32:], 2, 1, 10, 256 * 1024, n)
                assert bytes(back) == raws[i]
            frames[i] = bytes(f)
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]; [t.join() for t in ts]
    assert not errs, errs
    for i in range(2):
        assert frames[i][32:] == O.compress_frame(bytes(32), raws[i], 2, 1, 10, 256 * 1024)[32:]


# ---------------------------------------------------------------------------------------------------------------
# round 2: the plugin surface on a real device, the reference-produced checkpoint, whole-frame pins per dtype
# ---------------------------------------------------------------------------------------------------------------
GOLD_ST = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden", "gpt2_small_ref.znn.safetensors")


def _tensor_sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("device", ["cuda:0", 0, "cuda", "torch.device"], ids=["str-cuda0", "int-0", "str-cuda", "torch-device"])
def test_plugin_safe_open_decodes_in_hbm(lib, tmp_path, device):
    """SURVEY §8 a16 on hardware (reference zipnn.py:1592-1643, util_patch.py:11-47): after zipnn_safetensors(), both
    `safetensors.torch.safe_open` (what the reference patches) and top-level `safetensors.safe_open` (what transformers
    ≥ 5 imports) opened with a device return every compressed tensor decoded ON that device by the HIP kernels, equal
    to the original bit for bit; uncompressed tensors pass through; `device` may be a string, an ordinal or a torch.device."""
    import os
    import safetensors
    import safetensors.torch
    from safetensors.torch import save_file
    from zipnn_amd import safetensors_io, zipnn_safetensors
    dev = torch.device("cuda", 0) if device == "torch.device" else device
    g = torch.Generator().manual_seed(31)
    tensors = {"w_bf16": (torch.randn(1100, 513, generator=g) * 0.02).to(torch.bfloat16),          # 2 full chunks + a tail
               "w_fp16": (torch.randn(700, 300, generator=g) * 0.02).to(torch.float16),
               "w_fp32": torch.randn(513, 257, generator=g) * 0.02,
               "w_fp8": (torch.randn(900, 400, generator=g) * 0.02).to(torch.float8_e4m3fn),
               "ids": torch.arange(5000, dtype=torch.int64), "tiny": torch.randn(3, generator=g).to(torch.bfloat16)}
    src = os.path.join(tmp_path, "m.safetensors")
    save_file(tensors, src, {"format": "pt"})
    znn = safetensors_io.compress_safetensors_file(src)
    orig_a, orig_b = safetensors.torch.safe_open, safetensors.safe_open
    try:
        zipnn_safetensors()
        for opener in (safetensors.torch.safe_open, safetensors.safe_open):
            with opener(znn, framework="pt", device=dev) as f:
                assert set(f.keys()) == set(tensors)
                for k, v in tensors.items():
                    got = f.get_tensor(k)
                    assert got.is_cuda and got.dtype == v.dtype and got.shape == v.shape, k
                    assert _tensor_sha(got) == _tensor_sha(v), k
                    if k.startswith("w_"):
                        assert "zn_k_decode" in lib.last_kernels(), (k, lib.last_kernels())      # decoded by the HIP kernels, in HBM
        f = safetensors.safe_open(znn, framework="pt", device=dev)      # without `with`: still works, and closes its host handle
        assert _tensor_sha(f.get_tensor("w_bf16")) == _tensor_sha(tensors["w_bf16"])
        del f
    finally:
        safetensors.torch.safe_open, safetensors.safe_open = orig_a, orig_b
        from zipnn_amd import zipnn as _Z
        _Z._patches_applied.pop(_Z._zipnn_safetensors, None)      # (the patcher applies a patch once per process, like the reference's: let the next test apply it again)


def test_plugin_get_tensor_is_served_by_one_batched_decode_of_the_file(lib, tmp_path):
    """VERDICT r3 item 4 (reference zipnn.py:1592-1626: one decompress per get_tensor): with a device target the first compressed
    name triggers ONE transfer of the data section and ONE batched decode of every compressed tensor of the file; the other names are
    served from that — the cache shrinks by one per call, no further decode is launched — and everything is bit-exact."""
    import os
    from safetensors.torch import save_file
    from zipnn_amd import safetensors_io
    from zipnn_amd import zipnn as Z
    g = torch.Generator().manual_seed(77)
    tensors = {f"layer{i}.w": (torch.randn(300 + 37 * i, 257, generator=g) * 0.02).to(torch.bfloat16 if i % 2 else torch.float32) for i in range(24)}
    tensors["ids"] = torch.arange(1000, dtype=torch.int64)
    src = os.path.join(tmp_path, "m.safetensors")
    save_file(tensors, src, {"format": "pt"})
    znn = safetensors_io.compress_safetensors_file(src)
    with Z.SafeOpen(znn, framework="pt", device="cuda:0") as f:
        comp = set(f.compressed_tensors_metadata)
        assert len(comp) == 24
        names = sorted(f.keys())
        first = next(n for n in names if n in comp)
        t0 = f.get_tensor(first)
        assert isinstance(f._ahead, dict) and len(f._ahead) == 23            # everything else is already decoded, in HBM
        kernels = lib.last_kernels()
        assert "zn_k_decode" in kernels
        left = 23
        for n in names:
            if n == first:
                continue
            got = f.get_tensor(n)
            assert got.is_cuda and _tensor_sha(got) == _tensor_sha(tensors[n]), n
            if n in comp:
                left -= 1
                assert len(f._ahead) == left
        assert _tensor_sha(t0) == _tensor_sha(tensors[first]) and left == 0
    # switched off by the environment knob: the per-tensor path
    os.environ["ZIPNN_AMD_READAHEAD_BYTES"] = "0"
    try:
        with Z.SafeOpen(znn, framework="pt", device="cuda:0") as f:
            assert _tensor_sha(f.get_tensor(first)) == _tensor_sha(tensors[first]) and f._ahead is False
    finally:
        del os.environ["ZIPNN_AMD_READAHEAD_BYTES"]


def test_reference_produced_checkpoint_loads_through_the_plugin_and_load_file(lib):
    """BASELINE.json configs[3] / SURVEY §8d-4: a GPT-2-shaped checkpoint compressed by the REFERENCE's own
    scripts/zipnn_compress_safetensors.py (tests/golden/make_golden_safetensors.py, over oracle/_ref) is consumed
    here: plugin + safe_open(device="cuda:0"), and safetensors_io.load_file (one batched decode).  Every tensor must
    hash to what the generator recorded."""
    import json
    import safetensors
    import safetensors.torch
    from zipnn_amd import safetensors_io, zipnn_safetensors
    info = json.load(open(GOLD_ST + ".json"))
    assert hashlib.sha256(open(GOLD_ST, "rb").read()).hexdigest() == info["file_sha256"]
    loaded = safetensors_io.load_file(GOLD_ST, device="cuda:0")
    assert set(loaded) == set(info["tensors"])
    for k, meta in info["tensors"].items():
        assert loaded[k].is_cuda and str(loaded[k].dtype) == meta["dtype"] and list(loaded[k].shape) == meta["shape"], k
        assert _tensor_sha(loaded[k]) == meta["sha256"], k
    orig_a, orig_b = safetensors.torch.safe_open, safetensors.safe_open
    try:
        zipnn_safetensors()
        with safetensors.torch.safe_open(GOLD_ST, "pt", device="cuda:0") as f:
            n_compressed = 0
            for k, meta in info["tensors"].items():
                got = f.get_tensor(k)
                assert got.is_cuda and _tensor_sha(got) == meta["sha256"], k
                n_compressed += k in f.compressed_tensors_metadata
            assert n_compressed >= 10                      # the reference really compressed the weight matrices
        with safetensors.safe_open(GOLD_ST, framework="pt", device="cpu") as f:          # and the host route
            for k, meta in info["tensors"].items():
                assert _tensor_sha(f.get_tensor(k)) == meta["sha256"], k
    finally:
        safetensors.torch.safe_open, safetensors.safe_open = orig_a, orig_b
        from zipnn_amd import zipnn as _Z
        _Z._patches_applied.pop(_Z._zipnn_safetensors, None)      # (the patcher applies a patch once per process, like the reference's: let the next test apply it again)


@pytest.mark.parametrize("dtype", ["fp16", "fp32", "fp8"])
def test_256MiB_other_dtypes_whole_frame_vs_oracle(lib, dtype):
    """BASELINE.json configs[2] (+ fp8): the WHOLE frame body of a 256 MiB tensor equals the oracle's (sha256), not a
    sample of its chunks, and decodes back; every chunk through the fused kernels."""
    from zipnn_amd import codec
    g = torch.Generator().manual_seed(77)
    n = 256 * KB * KB
    if dtype == "fp16":
        x = (torch.randn(n // 2, generator=g) * 0.02).half(); P, rot, bm, chunk = 2, 0, 10, C
    elif dtype == "fp32":
        x = torch.randn(n // 4, generator=g) * 0.02; P, rot, bm, chunk = 4, 1, 220, C
    else:
        x = (torch.randn(n, generator=g) * 0.02).to(torch.float8_e4m3fn); P, rot, bm, chunk = 1, 0, 10, 128 * KB
    raw = x.view(torch.uint8).reshape(-1).numpy()
    want = O.compress_frame(bytes(32), raw, P, rot, bm, chunk, threads=8)
    body = codec.compress_device(lib, codec.flat_bytes(x.cuda()), P, rot, bm, chunk, 0.95)
    assert hashlib.sha256(body.cpu().numpy().tobytes()).hexdigest() == hashlib.sha256(want[32:]).hexdigest()
    obody = torch.from_numpy(np.frombuffer(want, dtype=np.uint8)[32:].copy()).cuda()
    out = codec.decompress_device(lib, obody, P, rot, bm, chunk, raw.size)       # the ORACLE's frame, decoded on the GPU
    assert torch.equal(out.cpu(), torch.from_numpy(raw))
    assert lib.last_fused_chunks() == raw.size // chunk


def test_plain_host_entry_points_the_reference_binding_calls(lib):
    """zn_compress / zn_decompress (no delta) are what the reference-side stub binds (INTEGRATION.md §1,
    tests/ref_binding/zipnn_core.py): called directly here, next to their *_delta siblings."""
    import ctypes
    L = lib._L
    d = gen_bytes("bf16", 3 * C + 1000, 4)
    want = O.compress_frame(HDR, d, 2, 1, 10, C)
    cap = L.zn_compress_bound(len(d), 2, C, 32)
    out = np.empty(cap, dtype=np.uint8); n_out = ctypes.c_size_t(0)
    src = np.frombuffer(d, dtype=np.uint8); hdr = np.frombuffer(HDR, dtype=np.uint8)
    assert L.zn_compress(hdr.ctypes.data, 32, src.ctypes.data, len(d), 2, 1, 10, C, 0.95, 0, out.ctypes.data, cap, ctypes.byref(n_out)) == 0
    assert out[:n_out.value].tobytes() == want
    back = np.empty(len(d), dtype=np.uint8)
    assert L.zn_decompress(out[32:].ctypes.data, n_out.value - 32, 2, 1, 10, C, len(d), 0, back.ctypes.data) == 0
    assert back.tobytes() == d
    assert torch.cuda.current_device() == 0                  # the host entry points leave the caller's device as it was


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0, 0]], ids=["two-ranges", "five-ranges"])
def test_multi_device_entry_points_on_the_one_gpu_here(lib, devices):
    """zn_compress_multi / zn_decompress_multi with the only GPU of this box listed several times: one host thread per
    range, all on device 0 (its lock serialises them) — the range split, the per-plane assembly and the re-based
    cumSizes run on real hardware; the frame is the oracle's.  (Distinct devices: tests/test_kernels_simt.py, two
    emulated devices; the 8-GPU run is the driver's.)"""
    d = gen_bytes("bf16", 37 * C + 4321, 8)
    want = O.compress_frame(HDR, d, 2, 1, 10, C)
    got = lib.compress_multi(HDR, d, 2, 1, 10, C, 0.95, devices)
    assert bytes(got) == want
    assert bytes(lib.decompress_multi(want[32:], 2, 1, 10, C, len(d), devices)) == d
    x = (torch.randn(3 * C // 4 + 11, generator=torch.Generator().manual_seed(2)) * 0.02).numpy().tobytes()     # fp32, ragged
    want = O.compress_frame(HDR, x, 4, 1, 220, C)
    assert bytes(lib.compress_multi(HDR, x, 4, 1, 220, C, 0.95, devices)) == want
    assert bytes(lib.decompress_multi(want[32:], 4, 1, 220, C, len(x), devices)) == x
    assert torch.cuda.current_device() == 0


@pytest.mark.parametrize("slices", [1, 2, 5])
def test_host_entry_points_one_shot_and_pipelined_on_hardware(lib, slices):
    """zn_compress / zn_decompress with pageable host buffers, as one shot and through the three-stage pipeline over chunk slices
    (two pinned pipes + a kernel stream of its own, real DMA in both directions at once): the oracle's frame, the input back —
    every dtype, ragged sizes, 40+ MiB so that the pipes cut the transfers into several slices of their own."""
    lib.set_host_slices(slices)
    try:
        for kind, nb, P, rot, bm, chunk, seed in (("bf16", 161 * C + 4098, 2, 1, 10, C, 3), ("fp32", 97 * C + 4 * 33, 4, 1, 220, C, 4),
                                                  ("fp8", 211 * (C // 2) + 7, 1, 1, 10, C // 2, 5), ("fp16", 64 * C, 2, 0, 10, C, 6)):
            d = gen_bytes(kind, nb, seed)
            want = O.compress_frame(HDR, d, P, rot, bm, chunk, threads=8)
            assert bytes(lib.compress(HDR, d, P, rot, bm, chunk, 0.95)) == want, (kind, slices)
            assert bytes(lib.decompress(want[32:], P, rot, bm, chunk, nb)) == d, (kind, slices)
        assert torch.cuda.current_device() == 0
    finally:
        lib.set_host_slices(0)


def _device_lists():
    n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    lists = [[0, 0], [0, 0, 0]]
    if n >= 2:
        lists += [[0, 1], list(range(n)), [1, 0, 1]]
    return lists


@pytest.mark.parametrize("devices", _device_lists(), ids=lambda d: "dev" + "".join(map(str, d)))
def test_multi_device_entries_with_the_tensor_resident_in_hbm(lib, devices):
    """zn_decompress_multi_dev / zn_compress_multi_dev / zn_decompress_range_dev on hardware: every listed device holds its chunk
    range in its own HBM; the body is a host buffer.  On a one-GPU box the device is listed several times; with more GPUs visible
    the same test runs on distinct devices (and on all of them)."""
    nb = 41 * C + 6000
    d = gen_bytes("bf16", nb, 12)
    want = O.compress_frame(HDR, d, 2, 1, 10, C, threads=4)
    G = len(devices)
    rng = [lib.multi_range(nb, C, G, i) for i in range(G)]
    outs = [torch.zeros(max(l, 1), dtype=torch.uint8, device=f"cuda:{dv}") for (_, l), dv in zip(rng, devices)]
    torch.cuda.synchronize()
    lib.decompress_multi_dev(want[32:], 2, 1, 10, C, nb, devices, [o.data_ptr() if l else 0 for o, (_, l) in zip(outs, rng)])
    assert b"".join(o.cpu().numpy().tobytes()[:l] for o, (_, l) in zip(outs, rng)) == d
    got = lib.compress_multi_dev(HDR, [o.data_ptr() if l else 0 for o, (_, l) in zip(outs, rng)], nb, 2, 1, 10, C, 0.95, devices)
    assert bytes(got) == want
    # one rank's view: an arbitrary chunk range of the host body into its own device memory
    lo, hi = 5, 23
    out = torch.zeros((hi - lo) * C, dtype=torch.uint8, device=f"cuda:{devices[-1]}")
    torch.cuda.synchronize()
    lib.decompress_range_dev(want[32:], 2, 1, 10, C, nb, lo, hi, devices[-1], out.data_ptr())
    assert out.cpu().numpy().tobytes() == d[lo * C: hi * C]
    assert torch.cuda.current_device() == 0
    # and the ranks' bodies merge into the single-device body
    from zipnn_amd import sharding
    parts = sharding.split_body(want[32:], 2, C, nb, 3)
    K = (nb + C - 1) // C
    assert sharding.merge_bodies([(sub, b - a) for (sub, _, _), (a, b) in zip(parts, sharding.chunk_ranges(K, 3))], 2, lib=lib) == want[32:]


def _rccl_rank(rank, world, port, nb, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from zipnn_amd import _capi, sharding
    torch.cuda.set_device(rank)
    dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    d = gen_bytes("bf16", nb, 6)
    body = O.compress_frame(b"", d, 2, 1, 10, C, threads=4)
    out = sharding.decompress_replicated(_capi.lib(), body, 2, 1, 10, C, nb, torch.device("cuda", rank))
    torch.cuda.synchronize()
    q.put((rank, out.cpu().numpy().tobytes() == d))
    dist.barrier()
    dist.destroy_process_group()


def test_replicated_decode_over_rccl_between_two_gpus(lib):
    """sharding.decompress_replicated with a real exchange: two ranks, two GPUs, all_gather_into_tensor over RCCL / xGMI.
    Skipped where fewer than two GPUs are visible (the builder's box has one; the gloo twin is tests/test_sharding_gloo.py)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rccl_rank, args=(r, 2, port, 13 * C + 999, q)) for r in range(2)]
    [p.start() for p in procs]
    got = sorted(q.get(timeout=300) for _ in range(2))
    [p.join(timeout=60) for p in procs]
    assert got == [(0, True), (1, True)] and all(p.exitcode == 0 for p in procs)


def test_damaged_bodies_are_rejected_or_decoded_never_fatal(lib):
    """The CPU suite's random-damage test (tests/test_kernels_simt.py) on the device: bytes flipped in the size tables, in
    tree descriptions / jump tables, anywhere; truncated bodies.  Every call either raises one of the documented
    exceptions or returns bytes; the device is left usable — the undamaged body decodes bit-exactly right after each."""
    from zipnn_amd import codec
    r = np.random.default_rng(99)
    cases = [("bf16", 9 * C + 5000, 2, 1, 10, C), ("fp32", 5 * C + 4, 4, 1, 220, C), ("fp8", 4 * C + 20001, 1, 0, 10, C // 2)]
    for kind, nb, P, rot, bm, chunk in cases:
        d = gen_bytes(kind, nb, 23)
        body = bytearray(O.compress_frame(HDR, d, P, rot, bm, chunk)[32:])
        good = torch.frombuffer(bytearray(body), dtype=torch.uint8).cuda()
        want = torch.frombuffer(bytearray(d), dtype=torch.uint8)
        K = (nb + chunk - 1) // chunk
        meta = 9 * P * K
        rejected = 0
        for trial in range(40):
            b = bytearray(body)
            mode = trial % 4
            if mode == 0:
                b[int(r.integers(0, meta))] ^= int(r.integers(1, 256))
            elif mode == 1:
                b[meta + int(r.integers(0, min(200, len(b) - meta)))] ^= int(r.integers(1, 256))
            elif mode == 2:
                for _ in range(8):
                    b[int(r.integers(0, len(b)))] ^= int(r.integers(1, 256))
            else:
                b = b[: int(r.integers(1, len(b)))]
            t = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
            try:
                codec.decompress_device(lib, t, P, rot, bm, chunk, nb)
            except (RuntimeError, MemoryError, ValueError):
                rejected += 1
            out = codec.decompress_device(lib, good, P, rot, bm, chunk, nb)
            assert torch.equal(out.cpu(), want)
        assert rejected >= 10          # truncations and size-table damage at the least


def test_bench_two_ranks_dry_run_sharing_this_gpu(lib):
    """bench.py's N > 1 logic — process group, barriers, max over ranks, per-rank times, the llama8b partition over ranks, rank 0's one line —
    executed with TWO ranks that share this box's GPU over gloo (ZN_BENCH_SHARE_GPU=1: RCCL refuses two ranks on one device).  The numbers of
    such a line mean nothing; that it comes out, exact, with both ranks' times on it, is the point."""
    import json, os, socket, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ZN_BENCH_SHARE_GPU="1", ZN_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    with socket.socket() as sk:                       # a port that is free right now
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--gib", "0.125", "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-other-dtypes", "--no-plugin", "--layers", "1"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 and ("address already in use" in r.stderr.lower() or "eaddrinuse" in r.stderr.lower()):
        pytest.skip("the rendezvous port was taken between the probe and the launch")
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["rccl_ranks"] == 2 and j["dry_run_shared_gpu"] is True and j["bit_exact_roundtrip"] is True
    assert len(j["rank_ms_per_step"]["all"]) == 2 and j["llama8b"]["n_gpus"] == 2 and j["llama8b"]["bit_exact_roundtrip"] is True



def test_bench_plain_run_dumps_the_same_outputs_twice(lib, tmp_path):
    """bench.py without --full: the headline line (no compress leg), exactly --steps timed steps, and --dump-outputs writing what the last
    step decoded — the same files from two runs with the same arguments, and the values of the seeded input tensor."""
    import json, os, subprocess, sys
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = []
    for k in range(2):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--gib", "0.0625", "--steps", "3", "--warmup", "1",
               "--dump-outputs", str(tmp_path / f"run{k}")]
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    for j in lines:
        assert j["steps"] == 3 and j["bit_exact_roundtrip"] is True and j["ms_per_step"] > 0 and j["unit"] == "GB/s" and j["higher_is_better"] is True
        assert "compress_GBps" not in j and "llama8b" not in j and "cpu_baseline" not in j
    names = sorted(os.listdir(tmp_path / "run0"))
    assert names == sorted(os.listdir(tmp_path / "run1")) and "decompressed_bf16_sample.npy" in names
    for f in names:
        a, b = np.load(tmp_path / "run0" / f), np.load(tmp_path / "run1" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    n = int(0.0625 * (1 << 30))
    want = bench.make_tensor(n, torch.device("cuda:0"), 1234)
    head = np.load(tmp_path / "run0" / "decompressed_bf16_head.npy")
    assert np.array_equal(head, want[:head.size].float().cpu().numpy())


# ---- round 5: parity against the reference's own C core, directly ----
def _dtype_case(dtype, n, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == "bf16":
        return (torch.randn(n // 2, generator=g) * 0.02).to(torch.bfloat16), 2, 1, 10, C
    if dtype == "fp16":
        return (torch.randn(n // 2, generator=g) * 0.02).half(), 2, 0, 10, C
    if dtype == "fp32":
        return torch.randn(n // 4, generator=g) * 0.02, 4, 1, 220, C
    return (torch.randn(n, generator=g) * 0.02).to(torch.float8_e4m3fn), 1, 0, 10, 128 * KB


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32", "fp8"])
def test_256MiB_frames_equal_the_reference_core_directly(lib, dtype):
    """The HIP path against oracle/_ref ITSELF — the reference's csrc/ compiled where it lies (oracle/Makefile), no restatement in
    between: the frame zipnn_core.zipnn_core writes for a 256 MiB tensor (reference csrc/zipnn_core.c:401-702, 16 threads) is the
    frame the GPU writes, byte for byte; the reference's frame decodes on the GPU to the input; and the reference's combine_dtype
    (:881-1164) decodes the GPU's frame to the input.  Mirrors the reference's own round-trip test, tests/simple_stress_tests.py:34-70."""
    if O.ref_core() is None:
        pytest.skip("oracle/_ref was not built (no /root/reference at build time)")
    from zipnn_amd import codec
    x, P, rot, bm, chunk = _dtype_case(dtype, 256 * KB * KB, 4242)
    raw = x.view(torch.uint8).reshape(-1).numpy()
    ref_frame = O.ref_compress_frame(bytes(32), raw, P, rot, bm, chunk, threads=16)
    body = codec.compress_device(lib, codec.flat_bytes(x.cuda()), P, rot, bm, chunk, 0.95)
    got = body.cpu().numpy().tobytes()
    assert len(got) == len(ref_frame) - 32 and got == ref_frame[32:]
    rbody = torch.from_numpy(np.frombuffer(ref_frame, dtype=np.uint8)[32:].copy()).cuda()
    out = codec.decompress_device(lib, rbody, P, rot, bm, chunk, raw.size)
    assert torch.equal(out.cpu(), torch.from_numpy(raw))
    assert lib.last_fused_chunks() == raw.size // chunk
    assert O.ref_decompress_body(got, P, rot, bm, chunk, raw.size, threads=16) == raw.tobytes()


def test_4GiB_bf16_headline_config_frame_equals_the_reference_core(lib):
    """BASELINE.json configs[1] — the configuration the headline number is quoted on — pinned by the suite: the whole frame of the
    4 GiB bf16 tensor bench.py times (same generator, same seed) equals the one the reference's C core writes (sha256 over 2.8 GB),
    the reference's frame decodes on the GPU to the tensor, and every one of the 16 384 chunks goes through the fused kernels."""
    if O.ref_core() is None:
        pytest.skip("oracle/_ref was not built (no /root/reference at build time)")
    import bench
    from zipnn_amd import codec
    n = 4 << 30
    x = bench.make_tensor(n, torch.device("cuda:0"), 1234)
    flat = codec.flat_bytes(x)
    body = codec.compress_device(lib, flat, 2, 1, 10, C, 0.95)
    raw = flat.cpu().numpy()
    buf = bytearray(raw.tobytes())                               # (the reference rotates its input in place)
    ref_frame = O.ref_core().zipnn_core(bytearray(bytes(32)), buf, 2, 1, 10, 0, C, 0.95, 10, 16)
    del buf
    ref_body = np.frombuffer(memoryview(ref_frame), dtype=np.uint8)[32:]
    got = body.cpu().numpy()
    assert got.size == ref_body.size
    assert hashlib.sha256(got).hexdigest() == hashlib.sha256(ref_body).hexdigest()
    del got
    out = codec.decompress_device(lib, torch.from_numpy(ref_body.copy()).cuda(), 2, 1, 10, C, n)
    assert torch.equal(out, flat)
    assert lib.last_fused_chunks() == n // C
    assert 0.655 < (ref_body.size + 32) / n < 0.670


def test_get_slice_of_compressed_tensors_decodes_chunk_ranges_in_hbm(lib, tmp_path):
    """`get_slice` on compressed tensors.  (1) The checkpoint the REFERENCE wrote (tests/golden/): row ranges, column
    ranges and int indices equal get_tensor(name)[index] on the device.  (2) A file with tensors of many chunks: a row range decodes only
    the chunks that cover it (zn_decompress_range_dev; the library's fused-chunk counter counts exactly those) and is a view of that range.
    The reference returns NotImplementedError here (zipnn/zipnn.py:1615-1617)."""
    import json
    import os
    from safetensors.torch import save_file
    from zipnn_amd import safetensors_io
    from zipnn_amd import zipnn as Z
    info = json.load(open(GOLD_ST + ".json"))
    with Z.SafeOpen(GOLD_ST, framework="pt", device="cuda:0") as f, Z.SafeOpen(GOLD_ST, framework="pt", device="cuda:0") as f2:
        names = [k for k in info["tensors"] if k in f.compressed_tensors_metadata]
        assert len(names) >= 10
        for k in names:
            whole = f2.get_tensor(k)
            s = f.get_slice(k)
            assert s.get_shape() == list(whole.shape)
            rows = whole.shape[0]
            for idx in [slice(0, rows), slice(rows // 3, rows // 2), slice(rows - 1, rows), 0, slice(None, None, 2)] + ([(slice(None), slice(0, 3)), (slice(1, rows // 2), -1)] if whole.dim() > 1 else []):
                got = s[idx]
                assert got.is_cuda and got.dtype == whole.dtype and torch.equal(got, whole[idx]), (k, idx)
    g = torch.Generator().manual_seed(99)
    tensors = {"w": (torch.randn(4096, 1024, generator=g) * 0.02).to(torch.bfloat16),                       # 8 MiB: 32 chunks
               "e": torch.randn(3000, 700, generator=g) * 0.02,                                               # 8.4 MB fp32, a partial last chunk
               "q": (torch.randn(2048, 1024, generator=g) * 0.02).to(torch.float8_e4m3fn)}                    # 2 MiB fp8: 16 chunks of 128 KiB
    src = os.path.join(tmp_path, "big.safetensors")
    save_file(tensors, src, {"format": "pt"})
    znn = safetensors_io.compress_safetensors_file(src, device="cuda:0")
    with Z.SafeOpen(znn, framework="pt", device="cuda:0") as f:
        s = f.get_slice("w")
        part = s[1024:1536]                                        # rows of 2 KiB: bytes [2 MiB, 3 MiB) = chunks 8 .. 11
        assert s.last_chunk_range == (8, 12) and lib.last_fused_chunks() == 4
        assert part.is_cuda and torch.equal(part.cpu(), tensors["w"][1024:1536]) and part.untyped_storage().nbytes() <= 4 * C
        part = s[100:101, 5:9]
        assert s.last_chunk_range == (0, 1) and torch.equal(part.cpu(), tensors["w"][100:101, 5:9])
        tp = [s[r * 1024:(r + 1) * 1024] for r in range(4)]         # what four tensor-parallel ranks would each take
        assert torch.equal(torch.cat(tp).cpu(), tensors["w"])
        se = f.get_slice("e")
        assert torch.equal(se[2990:].cpu(), tensors["e"][2990:]) and se.last_chunk_range == (31, 33)          # 8 400 000 bytes: 33 chunks, the last one partial
        assert torch.equal(se[:, 10:20].cpu(), tensors["e"][:, 10:20]) and se.last_chunk_range == (0, 33)
        sq = f.get_slice("q")
        assert torch.equal(sq[128:256].view(torch.uint8).cpu(), tensors["q"][128:256].view(torch.uint8)) and sq.last_chunk_range == (1, 2)
    with Z.SafeOpen(znn, framework="pt", device="cpu") as f:       # host target: decoded in HBM, the rows come back
        got = f.get_slice("w")[7:9]
        assert not got.is_cuda and torch.equal(got, tensors["w"][7:9])


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32", "fp8"])
def test_onepass_encoder_on_hardware(lib, dtype):
    """The one-pass encoder (zn_k_encode_onepass: histogram, code table, decoupled look-back and emit of a chunk by one workgroup; the chunk's second
    read aimed at the Infinity Cache) forced on for every dtype: 96 MiB + a partial last chunk — more chunks than workgroups fit the chip at once, so the
    look-back really waits on running predecessors — equals the oracle's body byte for byte, equals the four-kernel encoder's, and decodes back.
    Then a tensor that breaks its layout speculation (every plane compressible): the four-kernel encoder takes over, same bytes."""
    from zipnn_amd import codec
    n = 96 * KB * KB + 250_000
    x, P, rot, bm, chunk = _dtype_case(dtype, n // 4 * 4, 99)
    flat = codec.flat_bytes(x.cuda())
    raw = x.view(torch.uint8).reshape(-1).numpy()
    want = O.compress_frame(bytes(32), raw, P, rot, bm, chunk, threads=8)[32:]
    try:
        lib.set_encode_onepass(2)
        for rep in range(2):                                   # (twice: the look-back words carry a generation tag, nothing is zeroed between calls)
            one = codec.compress_device(lib, flat, P, rot, bm, chunk, 0.95)
            assert "zn_k_encode_onepass" in lib.last_kernels() and "speculation failed" not in lib.last_kernels()
            assert one.cpu().numpy().tobytes() == want
        lib.set_encode_onepass(0)
        four = codec.compress_device(lib, flat, P, rot, bm, chunk, 0.95)
        assert "zn_k_encode_onepass" not in lib.last_kernels() and torch.equal(four, one)
        out = codec.decompress_device(lib, one, P, rot, bm, chunk, raw.size)
        assert torch.equal(out.cpu(), torch.from_numpy(raw))
        if P > 1:
            lib.set_encode_onepass(2)
            g = torch.Generator().manual_seed(5)
            z = torch.zeros(8 * KB * KB, dtype=torch.uint8)
            z[::7] = torch.randint(0, 4, (z[::7].numel(),), generator=g, dtype=torch.uint8)       # sparse: every plane is Huffman-coded
            zb = codec.compress_device(lib, z.cuda(), P, rot, bm, chunk, 0.95)
            assert "speculation failed" in lib.last_kernels()
            assert zb.cpu().numpy().tobytes() == O.compress_frame(bytes(32), z.numpy(), P, rot, bm, chunk, threads=8)[32:]
    finally:
        lib.set_encode_onepass(1)


def _binding_cases():
    """The sixteen cases of tests/run_reference_cases.py (= the reference's tests/simple_stress_tests.py:19-264 with sizes trimmed), as the
    core calls the reference's Python package makes for them: (name, [data pieces], numBuf, bits_mode, bytes_mode, origChunkSize) — a streaming
    case is one core call per streaming chunk (zipnn/zipnn.py:612-635), a delta case codes data ^ base (:625-640)."""
    rng = np.random.default_rng(123)
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()      # noqa: E731
    g = torch.Generator().manual_seed(9)
    tb = lambda t: t.contiguous().view(torch.uint8).reshape(-1).numpy().tobytes()      # noqa: E731
    xor = lambda a, b: bytes(np.frombuffer(a, np.uint8) ^ np.frombuffer(b, np.uint8))    # noqa: E731
    cut = lambda d, sc: [d[o:o + sc] for o in range(0, len(d), sc)]                         # noqa: E731
    cs = []
    for kb in (255, 256, 257):
        cs.append((f"torch_bf16_{kb}k", [tb((torch.rand(kb * KB, generator=g) * 2 - 1).to(torch.bfloat16))], 2, 1, 10, C))
    cs.append(("bytes_255k", [rb(255 * KB)], 2, 1, 10, C))
    cs.append(("torch_bf16_weights", [tb((torch.randn(300 * KB, generator=g) * 0.02).to(torch.bfloat16))], 2, 1, 10, C))
    cs.append(("torch_fp32", [tb(torch.randn(70 * KB, generator=g) * 0.02)], 4, 1, 220, C))
    hc = torch.ones(100, 100); hc[50:] = torch.rand(50, 100, generator=g) * 2 - 1
    cs.append(("torch_fp16_half_const", [tb(hc.to(torch.float16))], 2, 0, 10, C))
    for sc in (2 ** 19, 2 ** 20):
        cs.append((f"streaming_{sc}", cut(rb(10 * KB), sc), 2, 1, 10, C))
    cs.append(("streaming_multi_frame", cut(tb((torch.randn(400 * KB, generator=g) * 0.02).to(torch.bfloat16)), 2 ** 18), 2, 1, 10, C))
    a, b, c = rb(10 * KB), rb(10 * KB), rb(10 * KB)
    cs.append(("delta_byte", [xor(a + b, a + c)], 2, 1, 10, C))
    cs.append(("delta_byte_streaming", cut(xor(a + b, a + c), 2 ** 20), 2, 1, 10, C))
    cs.append(("delta_file", [xor(a + b, a + c)], 2, 1, 10, C))
    fa, fb, fc = (rng.random(8 * KB).astype(np.float32) for _ in range(3))
    cs.append(("bytes_float32", [fa.tobytes()], 4, 1, 220, C))
    cs.append(("bytes_float32_streaming", cut(fa.tobytes(), 2 ** 20), 4, 1, 220, C))
    cs.append(("bytes_float32_streaming_delta", cut(xor(np.concatenate([fa, fb]).tobytes(), np.concatenate([fa, fc]).tobytes()), 2 ** 20), 4, 1, 220, C))
    return cs


@pytest.fixture(scope="module")
def ref_binding():
    """tests/ref_binding/zipnn_core.py — the module INTEGRATION.md §1 tells a zipnn maintainer to drop in for the compiled extension
    (reference csrc/zipnn_core_module.c:9-23) — loaded over the REAL library (no $ZIPNN_HIP_LIB: its default, zipnn_amd/libzipnn_hip.so)."""
    import importlib.util
    import os
    assert not os.environ.get("ZIPNN_HIP_LIB"), "this test is about the in-tree library"
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_binding", "zipnn_core.py")
    spec = importlib.util.spec_from_file_location("zn_ref_binding_on_hardware", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod._L._name.endswith(os.path.join("zipnn_amd", "libzipnn_hip.so"))
    return mod


@pytest.mark.parametrize("case", _binding_cases(), ids=lambda c: c[0])
def test_integration_stub_on_hardware_equals_the_reference_extension(lib, ref_binding, case):
    """The two functions of the reference's extension module — zipnn_core.zipnn_core(...) and zipnn_core.combine_dtype(...)
    (csrc/zipnn_core_module.c:9-23; called at zipnn/zipnn.py:714-725, 1143-1151) — called with the SAME positional arguments on
    oracle/_ref (the reference's C compiled where it lies) and on the INTEGRATION stub over the GPU: same frame bytes, same
    header length field written back into the caller's header, same decoded bytes, each core decoding the other's frame."""
    ref = O.ref_core()
    if ref is None:
        pytest.skip("oracle/_ref was not built (no /root/reference at build time)")
    name, pieces, P, rot, bm, chunk = case
    for piece in pieces:
        h_ref, h_gpu = bytearray(range(32)), bytearray(range(32))
        f_ref = bytes(ref.zipnn_core(h_ref, bytearray(piece), P, rot, bm, 0, chunk, 0.95, 10, 4))       # (a copy: the reference rotates its input in place)
        f_gpu = bytes(ref_binding.zipnn_core(h_gpu, bytearray(piece), P, rot, bm, 0, chunk, 0.95, 10, 4))
        assert f_gpu == f_ref, name
        assert h_gpu == h_ref                                                                               # zipnn_core.c:121
        n = len(piece)
        assert bytes(ref_binding.combine_dtype(f_ref[32:], P, rot, bm, chunk, n, 4)) == piece              # the reference's frame through the stub
        assert bytes(ref.combine_dtype(f_gpu[32:], P, rot, bm, chunk, n, 4)) == piece                       # the stub's frame through the reference


def test_onepass_automatic_mode_backs_off_and_never_takes_delta_calls(lib):
    """the one-pass encoder's layout speculation (every plane but the last raw) fails on sparse / delta tensors, and a failed call runs twice.
    Automatic mode therefore (a) never takes a call with a delta base and (b) sits out the next automatic calls of the device after a misspeculation.
    6 144+ full chunks of 16 KiB (the automatic threshold counts chunks), bodies compared with the oracle's every time."""
    from zipnn_amd import codec
    chunk, K = 16384, 6400
    n = chunk * K
    g = torch.Generator().manual_seed(77)
    sparse = torch.zeros(n, dtype=torch.uint8)
    sparse[::5] = torch.randint(0, 6, (sparse[::5].numel(),), generator=g, dtype=torch.uint8)        # both planes Huffman-coded: the speculation fails
    w = (torch.randn(n // 2, generator=g) * 0.02).to(torch.bfloat16).view(torch.uint8)
    want_sparse = O.compress_frame(bytes(32), sparse.numpy(), 2, 1, 10, chunk, threads=8)[32:]
    want_w = O.compress_frame(bytes(32), w.numpy(), 2, 1, 10, chunk, threads=8)[32:]
    sd, wd = sparse.cuda(), w.cuda()
    lib.release_workspace()                                    # a device without history
    lib.set_encode_onepass(1)
    assert codec.compress_device(lib, wd, 2, 1, 10, chunk, 0.95).cpu().numpy().tobytes() == want_w
    assert "zn_k_encode_onepass" in lib.last_kernels() and "failed" not in lib.last_kernels()            # plain weights: taken, and right
    assert codec.compress_device(lib, sd, 2, 1, 10, chunk, 0.95).cpu().numpy().tobytes() == want_sparse
    assert "speculation failed" in lib.last_kernels()                                                     # the cliff, once
    for _ in range(3):                                                                                    # … then the device sits out (8 calls)
        assert codec.compress_device(lib, sd, 2, 1, 10, chunk, 0.95).cpu().numpy().tobytes() == want_sparse
        assert "zn_k_encode_onepass" not in lib.last_kernels() and "zn_k_encode_emit" in lib.last_kernels()
    lib.release_workspace()                                    # (forgets the back-off)
    base = (w.clone().view(torch.bfloat16).float() * 1.001).to(torch.bfloat16).view(torch.uint8)
    want_delta = O.compress_frame(bytes(32), (w ^ base).numpy(), 2, 1, 10, chunk, threads=8)[32:]
    got = codec.compress_device(lib, wd, 2, 1, 10, chunk, 0.95, delta=base.cuda())
    assert "zn_k_encode_onepass" not in lib.last_kernels()                                                # a delta call: never speculated
    assert got.cpu().numpy().tobytes() == want_delta
    lib.release_workspace()


def test_decode_status_after_the_workspace_is_released(lib):
    """a thread that holds the token of an unverified check = 0 decode must not be told "ok" once the status words are gone."""
    from zipnn_amd import codec
    from zipnn_amd._capi import ZnError
    d = gen_bytes("bf16", 3 * C + 100, 8)
    body = torch.from_numpy(np.frombuffer(O.compress_frame(HDR, d, 2, 1, 10, C)[32:], dtype=np.uint8).copy()).cuda()
    out = codec.decompress_device(lib, body, 2, 1, 10, C, len(d), check=False)
    lib.decode_status()                                        # the verdict of that call: ok
    assert out.cpu().numpy().tobytes() == d
    codec.decompress_device(lib, body, 2, 1, 10, C, len(d), check=False)
    torch.cuda.synchronize()
    lib.release_workspace()
    with pytest.raises(ZnError):
        lib.decode_status()                                    # "cannot vouch for it", not a guess
    lib.decode_status()                                        # (asked and answered: the token is spent)


@pytest.mark.parametrize("mode", [4, 7, 5, 6, 0])
def test_host_entry_points_in_every_transfer_mode(lib, mode):
    """zn_set_host_direct (round 6): the host-buffer entry points — what the INTEGRATION stub binds (reference zipnn/zipnn.py:714-725,
    1143-1151) — with the staged pipe + huge-page hint (4, the default), with the caller's buffers pinned and moved by DMA (7: direct both ways; 5 / 6: one
    direction only) and with neither (0): 320 MiB of bf16 (above the 128 MiB / 192 MiB thresholds of the direct path and of the slice pipeline), a ragged tail,
    fresh AND recycled result buffers, one-shot and pipelined — the same frame as the oracle's every time, the same bytes back."""
    import ctypes
    L = lib._L
    n = 320 * KB * KB + 250_000
    g = torch.Generator().manual_seed(606)
    x = (torch.randn(n // 2, generator=g) * 0.02).to(torch.bfloat16).view(torch.uint8).numpy()
    hdr = np.frombuffer(HDR, dtype=np.uint8)
    want = O.compress_frame(HDR, x, 2, 1, 10, C, threads=8)
    cap = L.zn_compress_bound(n, 2, C, 32)
    sz = ctypes.c_size_t(0)
    warm_frame, warm_back = np.empty(cap, dtype=np.uint8), np.empty(n, dtype=np.uint8)
    try:
        lib.set_host_direct(mode)
        for slices in (0, 1, 5):
            lib.set_host_slices(slices)
            for fresh in (False, True, False):
                fr = np.empty(cap, dtype=np.uint8) if fresh else warm_frame
                assert L.zn_compress(hdr.ctypes.data, 32, x.ctypes.data, n, 2, 1, 10, C, ctypes.c_float(0.95), 0, fr.ctypes.data, cap, ctypes.byref(sz)) == 0
                assert sz.value == len(want) and fr[:sz.value].tobytes() == want, (mode, slices, fresh)
                bk = np.empty(n, dtype=np.uint8) if fresh else warm_back
                bk[:64] = 0
                assert L.zn_decompress(fr.ctypes.data + 32, sz.value - 32, 2, 1, 10, C, n, 0, bk.ctypes.data) == 0
                assert np.array_equal(bk, x), (mode, slices, fresh)
    finally:
        lib.set_host_direct(4); lib.set_host_slices(0)
    assert torch.cuda.current_device() == 0
