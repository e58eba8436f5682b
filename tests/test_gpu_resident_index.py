"""GPU tests (-m gpu): decode hints (include/zipnn_hip.h) on the real libzipnn_hip.so — a ResidentCheckpoint with an index decodes to the
source bytes and to what the same store decodes without it, the device builds the hints the emulated library builds, and hints are advice.  Small calls take
the wide kernel, which reads no hints: the fused form is forced for these tests."""
import numpy as np
import pytest
import torch

import hint_layout as HL
import oracle_lib as O
import test_index_simt as E
from test_gpu_batch_scale import _stage

pytestmark = pytest.mark.gpu
KB = 1024
GUARD = 256
# dtype -> (torch dtype, planes, bits_mode, bytes_mode, chunk)
DTYPES = {"bf16": (torch.bfloat16, 2, 1, 10, 256 * KB), "fp32": (torch.float32, 4, 1, 220, 256 * KB), "fp16": (torch.float16, 2, 0, 10, 256 * KB),
          "fp8": (torch.float8_e4m3fn, 1, 0, 10, 128 * KB)}
SIZES = {"9": 0, "9+1000B": 1000}


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    L.set_decode_wide(0)
    yield L
    L.set_decode_wide(1); L.set_decode_group(0)
    L.release_workspace()


def _stream():
    return torch.cuda.current_stream().cuda_stream


_SRC = {}


def _source(dtype, size, seed=11):
    """N(0, 0.02) in `dtype`, 9 chunks (+ 1000 bytes) long — made once, never modified."""
    key = (dtype, size, seed)
    if key not in _SRC:
        tdt, P, rot, bm, ch = DTYPES[dtype]
        es = torch.empty(0, dtype=tdt).element_size()
        g = torch.Generator().manual_seed(seed)
        _SRC[key] = (torch.randn((9 * ch + SIZES[size]) // es, generator=g) * 0.02).to(tdt)
    return _SRC[key]


def _guarded(nbytes, dev):
    buf = torch.full((nbytes + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xAB).all()) and bool((buf[GUARD + nbytes:] == 0xAB).all())


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_store_with_index_decodes_what_it_decodes_without(lib, dtype, size):
    from zipnn_amd.resident import ResidentCheckpoint
    dev = torch.device("cuda:0")
    tdt, P, rot, bm, ch = DTYPES[dtype]
    w = _source(dtype, size)
    v = _source(dtype, size, seed=12)
    sd = {"w": w, "v": v}
    plain = ResidentCheckpoint.from_state_dict(sd, dev)
    store = ResidentCheckpoint.from_state_dict(sd, dev, index=True)
    assert store.info("w")["compressed"] and store.info("w")["index_bytes"] > 0
    assert store.index_bytes > 0 and store.resident_bytes == plain.resident_bytes + store.index_bytes
    nb = w.numel() * w.element_size()
    want = {k: t.view(torch.uint8).to(dev) for k, t in sd.items()}
    # get_tensor into a guarded destination
    buf, flat = _guarded(nb, dev)
    out = flat.view(tdt)
    store.get_tensor("w", out=out)
    assert "zn_k_decode_hinted" in lib.last_kernels(), lib.last_kernels()
    assert torch.equal(flat, want["w"]) and _guards_intact(buf, nb)
    assert torch.equal(plain.get_tensor("w").view(torch.uint8), flat)
    assert "hinted" not in lib.last_kernels()
    # get_tensors into a guarded buffer
    need = store.scratch_bytes(["w", "v"])
    buf, into = _guarded(need, dev)
    got = store.get_tensors(["w", "v"], into=into)
    assert "zn_k_decode_hinted" in lib.last_kernels()
    ref = plain.get_tensors(["w", "v"])
    for k in ("w", "v"):
        assert torch.equal(got[k].view(torch.uint8), want[k]) and torch.equal(ref[k].view(torch.uint8), want[k]), k
    # (the bytes between and behind the two tensors belong to the buffer, not to a tensor)
    used = torch.zeros(need + 2 * GUARD, dtype=torch.bool, device=dev)
    for k in ("w", "v"):
        o = got[k].data_ptr() - buf.data_ptr()
        used[o:o + nb] = True
    assert bool((buf[~used] == 0xAB).all())
    # the window [2, 7)
    e = store._entries["w"]
    buf, flat = _guarded(5 * ch, dev)
    store._decode([(e, 2, 7, flat.data_ptr())], True)
    assert "zn_k_decode_hinted" in lib.last_kernels()
    assert torch.equal(flat, want["w"][2 * ch: 7 * ch]) and _guards_intact(buf, 5 * ch)
    # a plan, run three times
    buf, into = _guarded(need, dev)
    plan = store.plan(["w", "v"], into=into)
    for _ in range(3):
        for k in ("w", "v"):
            plan.tensors[k].view(torch.uint8).fill_(0)
        views = plan.run()
        plan.status()
        for k in ("w", "v"):
            assert torch.equal(views[k].view(torch.uint8), want[k]), k
    assert "zn_k_decode_hinted" in lib.last_kernels()
    assert bool((buf[:GUARD] == 0xAB).all()) and bool((buf[GUARD + need:] == 0xAB).all())
    plan.close()
    store.drop_index()
    assert torch.equal(store.get_tensor("w").view(torch.uint8), want["w"])


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_device_builds_the_hints_the_emulated_library_builds(lib, simt_lib, dtype):
    """The same body at the same alignment: the index built by the device equals, byte for byte, the one the kernels' sources build on the CPU."""
    dev = torch.device("cuda:0")
    tdt, P, rot, bm, ch = DTYPES[dtype]
    data = _source(dtype, "9+1000B").view(torch.uint8).numpy().tobytes()
    frame = O.compress_frame(b"", data, P, rot, bm, ch, threads=4)
    body = _stage(lib, [frame], dev)[0]
    host = torch.empty(len(frame), dtype=torch.uint8)
    host.copy_(torch.frombuffer(bytearray(frame), dtype=torch.uint8))
    assert body.data_ptr() % 4 == host.data_ptr() % 4

    def item(b):
        return (b.data_ptr(), b.numel(), P, rot, bm, ch, len(data), 0, 10, 0, None)
    n = lib.hint_size_dev(item(body), _stream())
    assert n == simt_lib.hint_size_dev(item(host))
    hd = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
    lib.hint_build_dev(item(body), hd.data_ptr(), n, _stream())
    assert "zn_k_decode_hinted^build" in lib.last_kernels()
    hh = torch.full((n,), 0x5A, dtype=torch.uint8)
    simt_lib.hint_build_dev(item(host), hh.data_ptr(), n)
    assert torch.equal(hd.cpu(), hh)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_wrong_hints_change_nothing_on_the_device(lib, dtype):
    """Random hint bytes, and tensor A's index with tensor B of the same geometry: identical bytes."""
    dev = torch.device("cuda:0")
    tdt, P, rot, bm, ch = DTYPES[dtype]
    srcs = [_source(dtype, "9").view(torch.uint8), _source(dtype, "9", seed=12).view(torch.uint8)]
    nb = srcs[0].numel()
    bodies = _stage(lib, [O.compress_frame(b"", s.numpy().tobytes(), P, rot, bm, ch, threads=4) for s in srcs], dev)

    def item(b, dst=0):
        return (b.data_ptr(), b.numel(), P, rot, bm, ch, nb, 0, 9, dst, None)
    sizes = [lib.hint_size_dev(item(b), _stream()) for b in bodies]
    ha = torch.zeros(max(sizes), dtype=torch.uint8, device=dev)
    lib.hint_build_dev(item(bodies[0]), ha.data_ptr(), ha.numel(), _stream())
    hdr = ((P * 9 + 1) * 4 + 63) // 64 * 64
    rnd = ha.clone()
    g = torch.Generator(device=dev); g.manual_seed(5)
    rnd[hdr:] = torch.randint(0, 256, (rnd.numel() - hdr,), generator=g, device=dev, dtype=torch.uint8)
    for body, src, hints in ((bodies[0], srcs[0], rnd), (bodies[1], srcs[1], ha), (bodies[0], srcs[0], ha)):
        buf, flat = _guarded(nb, dev)
        lib.decompress_hinted_batch_dev([(item(body, flat.data_ptr()), hints.data_ptr(), hints.numel())], _stream(), True)
        assert "zn_k_decode_hinted" in lib.last_kernels()
        assert torch.equal(flat.cpu(), src) and _guards_intact(buf, nb)


def test_hooked_module_with_index_computes_what_plain_parameters_compute(lib):
    from zipnn_amd.resident import ResidentCheckpoint
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(1024, 1536), torch.nn.GELU(), torch.nn.Linear(1536, 1024)).to(torch.bfloat16)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(0.5)
    net = net.to(dev)
    x = torch.randn(4, 1024, device=dev).to(torch.bfloat16)
    with torch.no_grad():
        ref = net(x)
        store = ResidentCheckpoint.from_state_dict(net.state_dict(), dev, index=True)
        assert store.index_bytes > 0
        hook = store.hook(net)
        got = net(x)
        hook.status()
        assert "zn_k_decode_hinted" in lib.last_kernels(), lib.last_kernels()
        assert torch.equal(got, ref)
        hook.remove()
        assert torch.equal(net(x), ref)


# ---- the shapes of tests/test_index_simt.py on hardware: tables past one sizing block, hostile distributions, chunk groups, shifted bodies, batches, two streams ----

_EMU = {}


def _to_dev(t, dev, shift=0):
    """A CPU byte tensor -> device memory, `shift` bytes into a 256-byte aligned allocation."""
    big = torch.zeros(t.numel() + 16, dtype=torch.uint8, device=dev)
    assert big.data_ptr() % 16 == 0
    v = big[shift:shift + t.numel()]
    v.copy_(t)
    return v


def _ditem(b, spec, lo=0, hi=None, dst=0, delta=None):
    P, rot, bm, ch, n = spec
    return (b.data_ptr(), b.numel(), P, rot, bm, ch, n, lo, -(-n // ch) if hi is None else hi, dst, delta)


def _dev_build(lib, body, spec):
    n = lib.hint_size_dev(_ditem(body, spec), _stream())
    assert "zn_k_hint_size" in lib.last_kernels()
    h = torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=body.device)       # (0xFF is no hint: what the build's tiles do not write must have been zeroed)
    lib.hint_build_dev(_ditem(body, spec), h.data_ptr(), n, _stream())
    assert "zn_k_hint_size" in lib.last_kernels() and "zn_k_decode_hinted^build" in lib.last_kernels(), lib.last_kernels()
    assert bool((h[n:] == 0xFF).all()), "the build wrote behind the index"
    return h[:n], n


def _emulated_index(simt_lib, body_cpu, spec, shift=0):
    """The index the kernels' sources build on the CPU for the same body at the same address modulo 4 — built once per (body, shift)."""
    key = (body_cpu.data_ptr(), shift)
    if key not in _EMU:
        host = E._shifted(body_cpu, shift) if shift else body_cpu
        assert host.data_ptr() % 4 == shift
        n = simt_lib.hint_size_dev(E._item(host, spec))
        h = torch.full((n,), 0x5A, dtype=torch.uint8)
        simt_lib.hint_build_dev(E._item(host, spec), h.data_ptr(), n)
        _EMU[key] = h
    return _EMU[key]


def _dev_decode(lib, jobs, check=True):
    """jobs: [(device body, spec, lo, hi, device hints or None, device delta base or None)] -> the decoded windows (device tensors), through one hinted
    batched call; every destination is 16-byte aligned inside one buffer filled with 0xAB, whose other bytes must stay what they were."""
    dev = jobs[0][0].device
    sizes = [E._wsize(s, lo, hi) for (_, s, lo, hi, _, _) in jobs]
    offs, o = [], GUARD
    for sz in sizes:
        offs.append(o)
        o += (sz + 15) // 16 * 16 + GUARD
    buf = torch.full((o,), 0xAB, dtype=torch.uint8, device=dev)
    items = []
    for (b, s, lo, hi, h, dl), off, sz in zip(jobs, offs, sizes):
        win = _ditem(b, s, lo, hi, buf.data_ptr() + off if sz else 0, dl.data_ptr() if dl is not None else None)
        items.append((win, h.data_ptr() if h is not None else None, h.numel() if h is not None else 0))
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=dev)
    for off, sz in zip(offs, sizes):
        mask[off:off + sz] = False
    try:
        lib.decompress_hinted_batch_dev(items, _stream(), check)
    finally:
        torch.cuda.synchronize()
        assert bool((buf[mask] == 0xAB).all()), "bytes outside a destination were written"
    return [buf[off:off + sz] for off, sz in zip(offs, sizes)]


def _src_dev(d, dev):
    return E._u8(d).to(dev)


@pytest.mark.parametrize("case", [E.TABLES[2], E.TABLES[3], E.TABLES[4], E.TABLES[5], E.TABLES[6]], ids=E._table_id)
def test_device_index_table_across_sizing_blocks(lib, simt_lib, case):
    """zn_k_hint_size past its 256-chunk blocks on hardware (the LDS-carried running offset, K no multiple of 256, windows that begin past chunks 256 and
    512): the index equals the emulated one byte for byte and its table the layout rule's; the windows decode from it to the source's slices."""
    dev = torch.device("cuda:0")
    kind, chunk, chunks, extra = case
    d, body_cpu, spec = E._case(kind, chunks, 31, extra, chunk=chunk)
    P, K = spec[0], -(-len(d) // chunk)
    body = _to_dev(body_cpu, dev)
    assert body.data_ptr() % 4 == 0
    h, n = _dev_build(lib, body, spec)
    hc = h.cpu()
    want, hdr = HL.expected_table(body_cpu.numpy().tobytes(), P, chunk, len(d))
    got = hc[:4 * len(want)].numpy().view("<u4")
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"offset table differs from the layout rule first at entry {bad[0]} (chunk {bad[0] // P}): {got[bad[0]]} != {want[bad[0]]}"
    assert n == int(want[-1])
    E._check_index_bytes(hc, n, spec, body_cpu)
    emu = _emulated_index(simt_lib, body_cpu, spec)
    assert emu.numel() == n
    tbl = 4 * len(want)
    assert torch.equal(hc[:tbl], emu[:tbl]) and torch.equal(hc[hdr:], emu[hdr:])
    src = _src_dev(d, dev)
    wins = [(0, K)] + E._table_windows(K)
    outs = []
    for lo, hi in wins:          # (one call per window: each is a launch whose first chunk is c_lo)
        outs.append(_dev_decode(lib, [(body, spec, lo, hi, h, None)])[0])
        if (lo + 1) * chunk <= len(d):
            assert "zn_k_decode_hinted" in lib.last_kernels(), (lo, hi, lib.last_kernels())
    for (lo, hi), out in zip(wins, outs):
        assert torch.equal(out, src[lo * chunk: min(hi * chunk, len(d))]), (lo, hi)


def _edge_case(case):
    """A row of test_gpu_parity.EDGE at no more than 4 chunks -> (source, oracle body as a CPU tensor, spec)."""
    from test_kernels_simt import _gen2
    kind, nb, P, rot, bm, chunk, _ = case
    chunks = min(nb // chunk, 4)
    d = _gen2(kind, chunks * chunk, 13)
    return d, E._u8(O.compress_frame(b"", d, P, rot, bm, chunk, threads=4)), (P, rot, bm, chunk, len(d))


def _edge_cases():
    from test_gpu_parity import EDGE
    return EDGE


@pytest.mark.parametrize("case", _edge_cases(), ids=lambda c: f"{c[0]}-P{c[2]}-r{c[3]}-c{c[5] // KB}k")
def test_hostile_distributions_decode_hinted_on_the_device(lib, case):
    """1-bit codes, tiles written in several lane groups, 11-bit codes, every plane Huffman-coded (the further planes decode unhinted behind a hinted first
    one): the oracle's frame, indexed and decoded from the index, is the source — and what the same body decodes to without an index."""
    dev = torch.device("cuda:0")
    d, body_cpu, spec = _edge_case(case)
    body = _to_dev(body_cpu, dev)
    h, n = _dev_build(lib, body, spec)
    want = E._check_index_bytes(h.cpu(), n, spec, body_cpu)
    assert n > int(want[0])                  # every one of these has a Huffman-coded plane: an index with hint bytes
    K = len(d) // spec[3]
    hinted = _dev_decode(lib, [(body, spec, 0, K, h, None)])[0]
    assert _hinted_launches(lib) == ["zn_k_decode_hinted"], lib.last_kernels()
    plain = _dev_decode(lib, [(body, spec, 0, K, None, None)])[0]
    assert "hinted" not in lib.last_kernels()
    src = _src_dev(d, dev)
    assert torch.equal(hinted, src) and torch.equal(plain, src)


@pytest.mark.parametrize("group", [1, 2, 3, 4])
def test_hinted_chunk_groups_on_the_device(lib, decode_group, group):
    """Groups of 1-4 chunks per workgroup that mix Huffman, raw, RLE and two-Huffman-plane chunks, with a partial tail behind them."""
    dev = torch.device("cuda:0")
    d, body_cpu, spec, kinds = E._mixed_kinds_body()
    body = _to_dev(body_cpu, dev)
    decode_group(lib, 0)
    h, n = _dev_build(lib, body, spec)
    E._mixed_table_check(h.cpu(), n, spec, body_cpu, kinds)
    decode_group(lib, group)
    out = _dev_decode(lib, [(body, spec, 0, 12, h, None)])[0]
    assert _hinted_launches(lib) == ["zn_k_decode_hinted+tail"], lib.last_kernels()
    assert torch.equal(out, _src_dev(d, dev))


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_hints_built_where_the_body_lies_on_the_device(lib, simt_lib, shift):
    """The body 1, 2, 3 bytes into a device buffer (a file's data section puts bodies anywhere), the destination 16-byte aligned: tile boundaries move with the
    address modulo 4, so the index is the emulated one of the same shift — and not the one of shift 0."""
    dev = torch.device("cuda:0")
    d, body_cpu, spec = E._case("bf16", 3, 5, 0, chunk=E.C2)
    body = _to_dev(body_cpu, dev, shift)
    assert body.data_ptr() % 4 == shift
    h, n = _dev_build(lib, body, spec)
    hdr = E._header_bytes(spec)
    hc = h.cpu()
    E._check_index_bytes(hc, n, spec, body_cpu)
    emu, emu0 = _emulated_index(simt_lib, body_cpu, spec, shift), _emulated_index(simt_lib, body_cpu, spec, 0)
    assert emu.numel() == n == emu0.numel()
    assert torch.equal(hc[hdr:], emu[hdr:]) and torch.equal(hc[:4 * (2 * 3 + 1)], emu[:4 * (2 * 3 + 1)])
    assert not torch.equal(hc[hdr:], emu0[hdr:]), "the hints do not depend on where the body lies: this test tests no placement"
    out = _dev_decode(lib, [(body, spec, 0, 3, h, None)])[0]
    assert out.data_ptr() % 16 == 0
    assert "zn_k_decode_hinted" in lib.last_kernels()
    assert torch.equal(out, _src_dev(d, dev))


def _hinted_launches(lib):
    return [k for k in lib.last_kernels().split(";") if k.startswith("zn_k_decode_hinted")]


def test_hinted_batch_at_checkpoint_scale(lib):
    """129 ragged two-plane tensors with their one- and four-plane companions, whole-chunk and empty ones between them, an index per tensor: one call with
    every second index withheld (one launch per plane count, null entries in the parallel table), one plan run three times, and a delta item, which falls back."""
    from test_gpu_batch_scale import _batch
    from test_kernels_simt import _delta_pair
    dev = torch.device("cuda:0")
    specs, datas, frames = _batch(129)
    bodies = _stage(lib, frames, dev)
    sp5 = [(P, rot, bm, ch, nb) for (_k, nb, P, rot, bm, ch) in specs]
    planes = sorted({s[0] for s in sp5 if s[4]})
    assert planes == [1, 2, 4]
    # one arena of indexes, each 16-byte aligned
    sizes = [lib.hint_size_dev(_ditem(b, s), _stream()) if s[4] else 0 for b, s in zip(bodies, sp5)]
    offs, o = [], 0
    for sz in sizes:
        offs.append(o); o += (sz + 15) // 16 * 16
    arena = torch.full((o + 16,), 0xFF, dtype=torch.uint8, device=dev)
    hints = []
    for b, s, sz, off in zip(bodies, sp5, sizes, offs):
        if sz:
            lib.hint_build_dev(_ditem(b, s), arena.data_ptr() + off, sz, _stream())
        hints.append(arena[off:off + sz] if sz else None)
    assert bool((arena[o:] == 0xFF).all())
    assert sum(1 for s, sz in zip(sp5, sizes) if sz > HL.header_bytes(s[0], -(-s[4] // s[3]))) >= 40      # most tensors with a full chunk have hint bytes
    want = torch.cat([_src_dev(d, dev) for d in datas])
    jobs = [(b, s, 0, -(-s[4] // s[3]), h, None) for b, s, h in zip(bodies, sp5, hints)]
    half = [(b, s, lo, hi, h if i % 2 == 0 else None, dl) for i, (b, s, lo, hi, h, dl) in enumerate(jobs)]
    for P in planes:             # each plane count keeps tensors with an index, and has some without
        assert any(j[4] is not None and j[1][0] == P for j in half) and any(j[4] is None and j[1][0] == P and j[1][4] for j in half)
    outs = _dev_decode(lib, half)
    assert len(_hinted_launches(lib)) == len(planes), lib.last_kernels()
    assert torch.equal(torch.cat(outs), want)
    # a plan over all of them, with every index
    nbs = [s[4] for s in sp5]
    doffs, o = [], GUARD
    for nb in nbs:
        doffs.append(o); o += (nb + 15) // 16 * 16 + 16
    buf = torch.full((o + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    plan = lib.plan_create_hinted([(_ditem(b, s, 0, None, buf.data_ptr() + off if s[4] else 0), h.data_ptr() if h is not None else None, h.numel() if h is not None else 0)
                                   for b, s, h, off in zip(bodies, sp5, hints, doffs)])
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=dev)
    for off, nb in zip(doffs, nbs):
        mask[off:off + nb] = False
    try:
        for _ in range(3):
            buf.fill_(0xAB)
            lib.plan_run(plan, _stream(), True)
            assert len(_hinted_launches(lib)) == len(planes), lib.last_kernels()
            assert torch.equal(torch.cat([buf[off:off + nb] for off, nb in zip(doffs, nbs)]), want)
            assert bool((buf[mask] == 0xAB).all())
    finally:
        torch.cuda.synchronize()
        lib.plan_destroy(plan)
    # a tensor with a delta base, in a call of its own: its index is accepted and not read
    data, base = _delta_pair("bf16", 3 * E.C2, 9)
    coded = (np.frombuffer(data, dtype=np.uint8) ^ np.frombuffer(base, dtype=np.uint8)).tobytes()
    sd = (2, 1, 10, E.C2, len(data))
    bd = _to_dev(E._u8(O.compress_frame(b"", coded, 2, 1, 10, E.C2)), dev)
    hd, _ = _dev_build(lib, bd, sd)
    out = _dev_decode(lib, [(bd, sd, 0, 3, hd, _src_dev(base, dev))])[0]
    assert "hinted" not in lib.last_kernels(), lib.last_kernels()
    assert torch.equal(out, _src_dev(data, dev))


_FRAMES = {}


def _weights_body(dtype, size, seed, dev):
    """-> (source bytes on the device, the oracle's body on the device, spec) of _source(dtype, size, seed); the frame is made once."""
    tdt, P, rot, bm, ch = DTYPES[dtype]
    key = (dtype, size, seed)
    src = _source(dtype, size, seed).view(torch.uint8)
    if key not in _FRAMES:
        _FRAMES[key] = E._u8(O.compress_frame(b"", src.numpy().tobytes(), P, rot, bm, ch, threads=4))
    return src.to(dev), _to_dev(_FRAMES[key], dev), (P, rot, bm, ch, src.numel())


def test_index_builds_beside_running_hinted_decodes(lib):
    """hint_size_dev and hint_build_dev take the device workspace (totals, done flags, status words) on the caller's stream while unchecked hinted plan runs
    of other bodies are in flight on another one: both sets decode to their sources, and the indexes built meanwhile are the ones built with the device idle."""
    dev = torch.device("cuda:0")
    set1 = [_weights_body("bf16", "9", 11, dev), _weights_body("bf16", "9", 12, dev), _weights_body("fp8", "9", 11, dev)]
    set2 = [_weights_body("fp16", "9+1000B", 11, dev), _weights_body("bf16", "9+1000B", 12, dev)]
    idle = [_dev_build(lib, b, s)[0].clone() for (_src, b, s) in set2]
    h1 = [_dev_build(lib, b, s)[0] for (_src, b, s) in set1]
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)

    def layout(cases):
        offs, o = [], GUARD
        for (src, _b, _s) in cases:
            offs.append(o); o += (src.numel() + 15) // 16 * 16 + GUARD
        return offs, torch.full((o,), 0xAB, dtype=torch.uint8, device=dev)
    offs1, buf1 = layout(set1)
    offs2, buf2 = layout(set2)
    plan = lib.plan_create_hinted([(_ditem(b, s, 0, None, buf1.data_ptr() + off), h.data_ptr(), h.numel()) for (_src, b, s), h, off in zip(set1, h1, offs1)])
    h2 = [torch.empty(t.numel(), dtype=torch.uint8, device=dev) for t in idle]
    torch.cuda.synchronize()
    try:
        for rnd in range(4):
            with torch.cuda.stream(sa):
                buf1.fill_(0xAB)
                lib.plan_run(plan, sa.cuda_stream, False)
                assert len(_hinted_launches(lib)) == 2, lib.last_kernels()
            with torch.cuda.stream(sb):
                buf2.fill_(0xAB)
                for (_src, b, s), h, want in zip(set2, h2, idle):
                    h.fill_(0xFF)
                    assert lib.hint_size_dev(_ditem(b, s), sb.cuda_stream) == want.numel()
                    lib.hint_build_dev(_ditem(b, s), h.data_ptr(), h.numel(), sb.cuda_stream)
                lib.decompress_hinted_batch_dev([(_ditem(b, s, 0, None, buf2.data_ptr() + off), h.data_ptr(), h.numel()) for (_src, b, s), h, off in zip(set2, h2, offs2)],
                                                sb.cuda_stream, False)
                assert _hinted_launches(lib) == ["zn_k_decode_hinted+tail"], lib.last_kernels()
            lib.decode_status(sa.cuda_stream)
            lib.decode_status(sb.cuda_stream)
            for cases, offs, buf in ((set1, offs1, buf1), (set2, offs2, buf2)):
                mask = torch.ones(buf.numel(), dtype=torch.bool, device=dev)
                for (src, _b, _s), off in zip(cases, offs):
                    assert torch.equal(buf[off:off + src.numel()], src), rnd
                    mask[off:off + src.numel()] = False
                assert bool((buf[mask] == 0xAB).all()), rnd
            for h, want in zip(h2, idle):
                assert torch.equal(h, want), rnd
            if rnd == 1:
                torch.cuda.synchronize()
                lib.release_workspace()
    finally:
        torch.cuda.synchronize()
        lib.plan_destroy(plan)


def test_damaged_body_same_verdict_with_and_without_hints_on_the_device(lib):
    """Exactly the body, positions and flips of test_index_simt.test_damaged_body_same_verdict_with_and_without_hints (which passes on the emulated kernels, under
    guard bytes, in this tree): damaged AFTER the build, the hinted decode raises what the unhinted one raises or returns what it returns, and neither writes
    outside its destination."""
    from zipnn_amd._capi import ZnError
    dev = torch.device("cuda:0")
    P, K = 2, 3
    d, good_cpu, spec = E._case("bf16", 3, 5, 0, chunk=E.C2)
    good = _to_dev(good_cpu, dev)
    body = good.clone()
    assert body.data_ptr() % 4 == 0
    h, _ = _dev_build(lib, body, spec)
    r = np.random.default_rng(23)
    t0, c0, p0 = 0, P * K, 9 * P * K
    spots = [t0 + int(r.integers(0, P * K)), c0 + 8 * int(r.integers(0, P * K)), c0 + 8 * int(r.integers(0, P * K)) + 5, c0 + 8 * (K - 1)]
    spots += [p0 + int(r.integers(0, good.numel() - p0)) for _ in range(6)]
    spots += [good.numel() - 1 - int(r.integers(0, 20000)) for _ in range(4)]
    outcomes = {"ok": 0, "error": 0}

    def verdict(hints):
        try:
            out = _dev_decode(lib, [(body, spec, 0, 3, hints, None)])[0]
            assert ("hinted" in lib.last_kernels()) == (hints is not None)
            return ("ok", out.cpu().numpy().tobytes())
        except (ZnError, MemoryError) as e:
            return (type(e).__name__, str(e))
    for pos in spots:
        for flip in (0xFF, 0x01):
            body.copy_(good); body[pos] ^= flip
            plain, hinted = verdict(None), verdict(h)
            assert plain == hinted, (pos, flip, plain[0], hinted[0])
            outcomes["ok" if plain[0] == "ok" else "error"] += 1
    assert outcomes["ok"] > 0 and outcomes["error"] > 0, outcomes
