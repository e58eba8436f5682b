"""CPU tests (-m "not gpu"): decode hints — the sidecar index of sub-block start positions that a resident store keeps beside a body (include/zipnn_hip.h,
DESIGN §3.6) — on the SIMT-emulated kernels.  Bodies are the oracle's (oracle_lib.compress_frame) or the golden file's; expected outputs are the source bytes,
and, where the point is "hints change nothing", the unhinted decode of the same body."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from test_kernels_simt import _delta_pair, _gen2, _u8

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gpt2_small_ref.znn.safetensors")
GUARD = 64
C2 = 64 * 1024       # chunk of the window / batch tests: a bf16 exponent stream of it is three tiles long (a regular tile, a last tile, more than one carry)
# kind -> (planes, bits_mode, bytes_mode, chunk): the inputs of test_register_resident_form_decodes_weights_like_tensors
WEIGHTS = {"bf16": (2, 1, 10, 256 * 1024), "fp32": (4, 1, 220, 256 * 1024), "fp16": (2, 0, 10, 256 * 1024), "fp8": (1, 0, 10, 128 * 1024)}


def _raw():
    return ctypes.CDLL(os.path.join(HERE, "simt", "libzipnn_simt.so"))


def _tile_counters(reset=True):
    a = (ctypes.c_ulonglong * 8)()
    _raw().zn_debug_tile_counters(a, 1 if reset else 0)
    return list(a)       # [tiles, tiles in the looping form, fix-up iterations, tiles written in several lane groups, ...]


def _hint_counters(reset=True):
    a = (ctypes.c_ulonglong * 4)()
    _raw().zn_debug_hint_counters(a, 1 if reset else 0)
    return list(a)       # [tiles started from hints, those that needed a fix-up, tiles of hinted launches without hints, hint bytes written]


def _weights(kind, chunks=3, seed=11, extra=0):
    P, rot, bm, chunk = WEIGHTS[kind]
    g = torch.Generator().manual_seed(seed)
    n = chunks * chunk + extra
    if kind == "fp8":
        x = (torch.randn(n, generator=g) * 0.02).to(torch.float8_e4m3fn)
    else:
        x = (torch.randn(n // (4 if kind == "fp32" else 2), generator=g) * 0.02).to({"fp32": torch.float32, "fp16": torch.float16}.get(kind, torch.bfloat16))
    return x.view(torch.uint8).numpy().tobytes()


_CACHE = {}


def _case(kind, chunks=3, seed=11, extra=0, chunk=None):
    """-> (source bytes, body tensor, spec) — computed once per module run, never modified (tests that damage a body work on a copy)."""
    key = (kind, chunks, seed, extra, chunk)
    if key not in _CACHE:
        P, rot, bm, ch = WEIGHTS[kind]
        if chunk is not None:
            d = _gen2(kind, (chunks * chunk + extra) // P * P, seed); ch = chunk
        else:
            d = _weights(kind, chunks, seed, extra)
        _CACHE[key] = (d, _u8(O.compress_frame(b"", d, P, rot, bm, ch)), (P, rot, bm, ch, len(d)))
    return _CACHE[key]


def _item(body, spec, lo=0, hi=None, dst=0, delta=None):
    P, rot, bm, ch, n = spec
    K = -(-n // ch)
    return (body.data_ptr(), body.numel(), P, rot, bm, ch, n, lo, K if hi is None else hi, dst, delta)


def _header_bytes(spec):
    P, _, _, ch, n = spec
    return ((P * -(-n // ch) + 1) * 4 + 63) // 64 * 64


def _build(lib, body, spec, cap=None):
    n = lib.hint_size_dev(_item(body, spec))
    assert n >= _header_bytes(spec)
    h = torch.full((max(cap or n, n),), 0x5A, dtype=torch.uint8)
    lib.hint_build_dev(_item(body, spec), h.data_ptr(), h.numel())
    return h, n


def _wsize(spec, lo, hi):
    return len(range(lo * spec[3], min(hi * spec[3], spec[4])))


def _decode(lib, jobs, check=True, plan_runs=0):
    """jobs: [(body, spec, lo, hi, hints or None, delta or None)] -> decoded windows, through one (hinted) batched call — or a hinted plan run
    `plan_runs` times; guard bytes around every destination are checked."""
    sizes = [_wsize(s, lo, hi) for (_, s, lo, hi, _, _) in jobs]
    offs, o = [], GUARD
    for sz in sizes:
        offs.append(o)
        o += (sz + 15) // 16 * 16 + GUARD
    buf = torch.full((o,), 0xAB, dtype=torch.uint8)
    items = []
    for (b, s, lo, hi, h, dl), off in zip(jobs, offs):
        win = _item(b, s, lo, hi, buf.data_ptr() + off, dl.data_ptr() if dl is not None else None)
        items.append((win, h.data_ptr() if h is not None else None, h.numel() if h is not None else 0))
    if plan_runs:
        plan = lib.plan_create_hinted(items)
        try:
            for _ in range(plan_runs):
                for off, sz in zip(offs, sizes):
                    buf[off:off + sz] = 0xAB
                lib.plan_run(plan, 0, check)
        finally:
            lib.plan_destroy(plan)
    else:
        lib.decompress_hinted_batch_dev(items, 0, check)
    mask = torch.ones(buf.numel(), dtype=torch.bool)
    for off, sz in zip(offs, sizes):
        mask[off:off + sz] = False
    assert bool((buf[mask] == 0xAB).all()), "bytes outside a destination were written"
    return [buf[off:off + sz].numpy().tobytes() for off, sz in zip(offs, sizes)]


@pytest.fixture()
def fused(simt_lib, decode_group):
    """The fused form for every call of the test (small calls would take the wide kernel, which reads no hints); counters zeroed."""
    simt_lib.set_decode_wide(0)
    _tile_counters(); _hint_counters()
    yield simt_lib
    simt_lib.set_decode_wide(1)


@pytest.mark.parametrize("kind", list(WEIGHTS))
def test_hinted_decode_needs_no_fixups(fused, kind):
    """Build, then decode from the hints: the source bytes, every full-chunk Huffman tile started from its hints, and not one fix-up iteration — where the
    unhinted decode of fp16 / fp8 needs them all the time (test_register_resident_form_decodes_weights_like_tensors asserts fixups > 0)."""
    lib = fused
    d, body, spec = _case(kind)
    h, n = _build(lib, body, spec)
    built = _hint_counters()
    assert built[3] > 0 and built[3] <= n - _header_bytes(spec)
    _tile_counters()
    assert _decode(lib, [(body, spec, 0, 3, h, None)])[0] == d
    assert "zn_k_decode_hinted" in lib.last_kernels()
    tiles = _tile_counters()
    hc = _hint_counters()
    print(f"{kind}: tiles {tiles[0]}, looping {tiles[1]}, fix-up iterations {tiles[2]}, hinted {hc[0]}, hinted with fix-up {hc[1]}, index {n} B = {100.0 * n / len(d):.2f} % of the tensor")
    assert tiles[0] > 20
    assert hc[0] == tiles[0]
    assert hc[1] == 0
    assert tiles[2] == 0
    assert hc[2] == 0


@pytest.mark.parametrize("kind", ["dense3", "sparse"])
def test_hinted_looping_form(fused, kind):
    """The run-time-D looping form (distributions of test_looping_form_still_decodes_what_the_fast_form_leaves) starts its count pass from the hints."""
    lib = fused
    chunk = 256 * 1024
    r = np.random.default_rng(3)
    if kind == "dense3":
        probs = np.array([0.14] + [0.86 / 60] * 60); probs /= probs.sum()
        d = r.choice(np.arange(61, dtype=np.uint8), 2 * chunk, p=probs).tobytes(); P, rot = 1, 0; chunk = 128 * 1024
    else:
        b = np.zeros(2 * chunk, dtype=np.uint8); m = r.random(2 * chunk) < 0.08; b[m] = r.integers(0, 255, int(m.sum())); d = b.tobytes(); P, rot = 2, 1
    spec = (P, rot, 10, chunk, len(d))
    body = _u8(O.compress_frame(b"", d, P, rot, 10, chunk))
    h, _ = _build(lib, body, spec)
    _tile_counters(); _hint_counters()
    assert _decode(lib, [(body, spec, 0, -(-len(d) // chunk), h, None)])[0] == d
    tiles, hc = _tile_counters(), _hint_counters()
    assert tiles[1] > 0                       # the looping form ran …
    assert hc[0] > 0 and hc[1] == 0           # … from hints, and closed its chain at once


def test_hinted_windows_and_partial_last_chunk(fused):
    """One index serves every window of its body (the table is indexed by the body's chunk numbers); a partial last chunk decodes unhinted."""
    lib = fused
    for extra in (0, 1000):
        d, body, spec = _case("bf16", 3, 5, extra, chunk=C2)
        h, _ = _build(lib, body, spec)
        K = -(-len(d) // C2)
        for lo, hi in ((1, 3), (2, 3), (0, K), (K - 1, K)):
            _hint_counters()
            got = _decode(lib, [(body, spec, lo, hi, h, None)])[0]
            assert got == d[lo * C2: min(hi * C2, len(d))], (extra, lo, hi, lib.last_kernels())
            hc = _hint_counters()
            assert hc[1] == 0, (extra, lo, hi, hc)
            if lo < 3:
                assert hc[0] > 0


@pytest.mark.parametrize("group", [1, 2, 3, 4])
def test_hinted_decode_in_every_group_size(fused, decode_group, group):
    lib = fused
    d, body, spec = _case("bf16", 9, 6, 0, chunk=C2)
    decode_group(lib, 0)
    h, _ = _build(lib, body, spec)
    decode_group(lib, group)
    _hint_counters()
    assert _decode(lib, [(body, spec, 0, 9, h, None)])[0] == d
    hc = _hint_counters()
    assert hc[0] > 0 and hc[1] == 0 and hc[2] == 0


def test_hinted_plans_batches_and_mixed_calls(fused):
    lib = fused
    da, ba, sa = _case("bf16", 3, 5, 0, chunk=C2)
    db, bb, sb = _case("fp8", 3, 7, 1000, chunk=C2)
    dc, bc, sc = _case("fp16", 3, 8, 0, chunk=C2)
    ha, _ = _build(lib, ba, sa)
    hb, _ = _build(lib, bb, sb)
    hc_, _ = _build(lib, bc, sc)
    Kb = -(-len(db) // C2)
    # a hinted plan, run twice
    _hint_counters()
    got = _decode(lib, [(ba, sa, 0, 3, ha, None), (bc, sc, 1, 3, hc_, None)], plan_runs=2)
    assert got == [da, dc[C2:]]
    c = _hint_counters()
    assert c[0] > 0 and c[1] == 0
    # tensors of different dtypes (and plane counts) in one call
    got = _decode(lib, [(ba, sa, 0, 3, ha, None), (bb, sb, 0, Kb, hb, None), (bc, sc, 0, 3, hc_, None)])
    assert got == [da, db, dc]
    assert _hint_counters()[1] == 0
    # one hinted item beside one unhinted item of the same plane count: one launch, the unhinted tensor's tiles take the run-in
    got = _decode(lib, [(ba, sa, 0, 3, ha, None), (bc, sc, 0, 3, None, None)])
    assert got == [da, dc]
    c = _hint_counters()
    assert c[0] > 0 and c[2] > 0 and c[1] == 0
    # a hinted item with a delta base decodes unhinted (the delta instances read no hints)
    data, base = _delta_pair("bf16", 3 * C2, 9)
    coded = (np.frombuffer(data, dtype=np.uint8) ^ np.frombuffer(base, dtype=np.uint8)).tobytes()
    bd = _u8(O.compress_frame(b"", coded, 2, 1, 10, C2)); sd = (2, 1, 10, C2, len(data))
    hd, _ = _build(lib, bd, sd)
    _hint_counters()
    got = _decode(lib, [(bd, sd, 0, 3, hd, _u8(base))])
    assert got == [data]
    assert _hint_counters()[0] == 0 and "hinted" not in lib.last_kernels()


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_hints_are_advice(fused, kind):
    """Random, all-zero, all-0xFF hints, a scrambled offset table and another tensor's hints: the same bytes as the unhinted decode, and the call returns."""
    lib = fused
    d, body, spec = _case(kind, 3, 5, 0, chunk=C2)
    d2, body2, spec2 = _case(kind, 3, 6, 0, chunk=C2)
    n2 = lib.hint_size_dev(_item(body2, spec2))
    h, n = _build(lib, body, spec, cap=max(n2, 0))
    hdr = _header_bytes(spec)
    r = torch.Generator().manual_seed(99)
    rnd = h.clone(); rnd[hdr:] = torch.randint(0, 256, (rnd.numel() - hdr,), generator=r, dtype=torch.uint8)
    _hint_counters()
    assert _decode(lib, [(body, spec, 0, 3, rnd, None)])[0] == d
    c = _hint_counters()
    assert c[0] > 0 and c[1] > 0              # hints were used, and were wrong
    for fill in (0x00, 0xFF):
        bad = h.clone(); bad[hdr:] = fill
        assert _decode(lib, [(body, spec, 0, 3, bad, None)])[0] == d
    scr = torch.randint(0, 256, (h.numel(),), generator=r, dtype=torch.uint8)       # the offset table too
    assert _decode(lib, [(body, spec, 0, 3, scr, None)])[0] == d
    ff = torch.full((h.numel(),), 0xFF, dtype=torch.uint8)
    assert _decode(lib, [(body, spec, 0, 3, ff, None)])[0] == d
    # tensor A's hints with tensor B of the same geometry
    assert h.numel() >= n2
    assert _decode(lib, [(body2, spec2, 0, 3, h, None)])[0] == d2


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_hints_hold_for_the_address_they_were_built_at(fused, shift):
    """Tile boundaries depend on the body's address modulo 4: built where the body lies — 1, 2, 3 bytes into a buffer — the hints need no fix-up."""
    lib = fused
    d, body0, spec = _case("bf16", 3, 5, 0, chunk=C2)
    big = torch.zeros(body0.numel() + 8, dtype=torch.uint8)
    assert big.data_ptr() % 4 == 0
    big[shift:shift + body0.numel()] = body0
    body = big[shift:shift + body0.numel()]
    h, _ = _build(lib, body, spec)
    _hint_counters()
    assert _decode(lib, [(body, spec, 0, 3, h, None)])[0] == d
    c = _hint_counters()
    assert c[0] > 0 and c[1] == 0


def test_damaged_body_same_verdict_with_and_without_hints(fused):
    """The body is damaged AFTER the build (patterns of test_damaged_bodies_through_the_window_call): the hinted decode raises what the unhinted one
    raises or returns what it returns, and writes nothing outside its destination (guard bytes, checked by _decode)."""
    from zipnn_amd._capi import ZnError
    lib = fused
    P, K = 2, 3
    d, good, spec = _case("bf16", 3, 5, 0, chunk=C2)
    body = good.clone()
    h, _ = _build(lib, body, spec)
    r = np.random.default_rng(23)
    t0, c0, p0 = 0, P * K, 9 * P * K
    spots = [t0 + int(r.integers(0, P * K)), c0 + 8 * int(r.integers(0, P * K)), c0 + 8 * int(r.integers(0, P * K)) + 5, c0 + 8 * (K - 1)]
    spots += [p0 + int(r.integers(0, good.numel() - p0)) for _ in range(6)]
    spots += [good.numel() - 1 - int(r.integers(0, 20000)) for _ in range(4)]          # the exponent plane's streams (the last plane of the body)
    outcomes = {"ok": 0, "error": 0}

    def verdict(hints):
        try:
            return ("ok", _decode(lib, [(body, spec, 0, 3, hints, None)])[0])
        except (ZnError, MemoryError) as e:
            return (type(e).__name__, str(e))
    for pos in spots:
        for flip in (0xFF, 0x01):
            body.copy_(good); body[pos] ^= flip
            plain, hinted = verdict(None), verdict(h)
            assert plain == hinted, (pos, flip, plain[0], hinted[0])
            outcomes["ok" if plain[0] == "ok" else "error"] += 1
    assert outcomes["ok"] > 0 and outcomes["error"] > 0, outcomes


def test_hint_arguments(fused):
    lib = fused
    d, body, spec = _case("bf16", 3, 5, 0, chunk=C2)
    h, n = _build(lib, body, spec)
    out = torch.empty(len(d), dtype=torch.uint8)
    win = _item(body, spec, 0, 3, out.data_ptr())
    for hp, hl in ((h.data_ptr(), n - 1), (h.data_ptr(), 16), (None, n), (h.data_ptr(), 0), (h.data_ptr() + 4, n)):
        with pytest.raises(ValueError):
            lib.decompress_hinted_batch_dev([(win, hp, hl)])
        with pytest.raises(ValueError):
            lib.plan_create_hinted([(win, hp, hl)])
    with pytest.raises(ValueError):
        lib.hint_build_dev(_item(body, spec), h.data_ptr(), n - 1)       # capacity below the size
    with pytest.raises(ValueError):
        lib.hint_build_dev(_item(body, spec), None, n)
    with pytest.raises(ValueError):
        lib.hint_size_dev((body.data_ptr(), body.numel(), 3, 1, 10, C2, len(d), 0, 3, 0, None))      # three planes
    lib.decompress_hinted_batch_dev([])
    lib.decompress_hinted_batch_dev([(win, h.data_ptr(), n)])
    assert out.numpy().tobytes() == d
    lib.decompress_hinted_batch_dev([(win, None, 0)])                      # NULL, 0: no hints
    assert out.numpy().tobytes() == d


# ---- store level ------------------------------------------------------------------------------------------------------------------------------

def test_store_with_index_equals_load_file(use_simt):
    from zipnn_amd import safetensors_io
    from zipnn_amd.resident import ResidentCheckpoint
    lib = use_simt
    lib.set_decode_wide(0)
    try:
        want = safetensors_io.load_file(GOLDEN, device="cpu")
        plain = ResidentCheckpoint.from_file(GOLDEN, "cpu")
        store = ResidentCheckpoint.from_file(GOLDEN, "cpu", index=True)
        assert store.index_bytes > 0
        assert store.resident_bytes == plain.resident_bytes + store.index_bytes
        assert sum(store.info(k)["index_bytes"] for k in store.keys()) <= store.index_bytes
        for k in store.keys():                 # (the golden model's tensors are shorter than a chunk: the hinted calls' argument path, tails and all)
            assert torch.equal(store.get_tensor(k).view(torch.uint8), want[k].view(torch.uint8)), k
        got = store.get_tensors(store.keys())
        for k in store.keys():
            assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), k
        big = max((k for k in store.keys() if len(want[k].shape) == 2), key=lambda k: want[k].numel())
        rows = want[big].shape[0]
        sl = store.get_slice(big)
        for a, b in ((0, 3), (rows // 2, rows // 2 + 40), (rows - 5, rows)):
            assert torch.equal(sl[a:b].view(torch.uint8), want[big][a:b].view(torch.uint8)), (big, a, b)

        class Net(torch.nn.Module):
            def __init__(self, w, b):
                super().__init__()
                self.fc = torch.nn.Linear(w.shape[1], w.shape[0]).to(w.dtype)
                self.fc.weight.data, self.fc.bias.data = w.clone(), b.clone()

            def forward(self, x):
                return self.fc(x)
        g = torch.Generator().manual_seed(1)
        w = (torch.randn(96, 512, generator=g) * 0.02).to(torch.float32)
        b_ = (torch.randn(96, generator=g) * 0.02).to(torch.float32)
        net = Net(w, b_)
        x = torch.randn(2, 512, generator=g)
        ref = net(x)
        st2 = ResidentCheckpoint.from_state_dict(net.state_dict(), "cpu", index=True)
        hk = st2.hook(net)
        assert torch.equal(net(x), ref)
        hk.remove()
        store.drop_index()
        assert store.index_bytes == 0 and store.resident_bytes == plain.resident_bytes
        for k in store.keys()[:6]:
            assert torch.equal(store.get_tensor(k).view(torch.uint8), want[k].view(torch.uint8)), k
    finally:
        lib.set_decode_wide(1)


def test_index_of_bf16_weights_is_a_percent_of_the_tensor(use_simt):
    """bf16 N(0, 0.02): the exponent plane compresses to about a third of its 128 KiB per 256 KiB chunk, a 1 KiB tile of it takes 64 hint bytes — about
    3 KiB per chunk, 1.2 % of the tensor; the cap is 2 %."""
    from zipnn_amd.resident import ResidentCheckpoint
    g = torch.Generator().manual_seed(4)
    sd = {"w": (torch.randn(4 * 128 * 1024, generator=g) * 0.02).to(torch.bfloat16)}
    store = ResidentCheckpoint.from_state_dict(sd, "cpu", index=True)
    share = store.index_bytes / store.nbytes
    print(f"bf16 N(0, 0.02): index_bytes / nbytes = {share:.4f}")
    assert store.info("w")["compressed"] and store.index_bytes > 0
    assert store.index_bytes <= 0.02 * store.nbytes
    use_simt.set_decode_wide(0)
    try:
        _hint_counters()
        assert torch.equal(store.get_tensor("w"), sd["w"])
        plan = store.plan(["w"])
        assert torch.equal(plan.run()["w"], sd["w"])
        plan.close()
        c = _hint_counters()
        assert c[0] > 0 and c[1] == 0         # the store's own calls decode from the index
    finally:
        use_simt.set_decode_wide(1)


def test_two_tensor_store_decodes_hinted_on_a_fresh_workspace(use_simt):
    """The pinned staging buffer is shared by compress and decode calls: a two-tensor compress sizes it, and the hinted decode of the same two tensors, whose
    staged table is longer (the segments' indexes ride behind them), must find room — on a workspace that has seen nothing larger before."""
    from zipnn_amd.resident import ResidentCheckpoint
    use_simt.release_workspace()
    g = torch.Generator().manual_seed(6)
    sd = {k: (torch.randn(2 * 128 * 1024, generator=g) * 0.02).to(torch.bfloat16) for k in ("w", "v")}
    store = ResidentCheckpoint.from_state_dict(sd, "cpu", index=True)
    use_simt.set_decode_wide(0)
    try:
        _hint_counters()
        got = store.get_tensors(["w", "v"])
        assert torch.equal(got["w"], sd["w"]) and torch.equal(got["v"], sd["v"])
        c = _hint_counters()
        assert c[0] > 0 and c[1] == 0
    finally:
        use_simt.set_decode_wide(1)


# ---- index tables past one sizing block, hostile distributions, mixed chunk groups (tests/test_gpu_resident_index.py runs the same shapes on hardware) ----

# (kind, chunk, chunks, extra bytes): zn_k_hint_size sizes 256 chunks per iteration and carries the running offset to the next — below, at, one past 256, a
# partial last chunk behind 300, past 512; four planes and one plane past 256
TABLES = [("bf16", 4096, 255, 0), ("bf16", 4096, 256, 0), ("bf16", 4096, 257, 0), ("bf16", 4096, 300, 100), ("bf16", 4096, 520, 0),
          ("fp32", 8192, 260, 0), ("fp8", 4096, 258, 0)]
TABLE_WINDOWS = [(250, 290), (255, 258), (511, 514)]


def _table_id(c):
    return f"{c[0]}-{c[2]}x{c[1]}" + (f"+{c[3]}B" if c[3] else "")


def _table_windows(K):
    """The windows of the table tests that lie inside K chunks (clipped at K), and the last chunk alone."""
    return [(lo, min(hi, K)) for lo, hi in TABLE_WINDOWS if lo < K] + [(K - 1, K)]


def _shifted(body0, shift):
    """A copy of the body `shift` bytes into a 4-byte aligned buffer."""
    big = torch.zeros(body0.numel() + 8, dtype=torch.uint8)
    assert big.data_ptr() % 4 == 0
    big[shift:shift + body0.numel()] = body0
    return big[shift:shift + body0.numel()]


def _check_index_bytes(h, n, spec, body):
    """What holds for every index the build writes: the table is the layout rule's and non-decreasing; a hint is at most 10, lane 0's is 0."""
    import hint_layout as HL
    P, _, _, ch, nb = spec
    want, hdr = HL.expected_table(body.numpy().tobytes(), P, ch, nb)
    assert hdr == _header_bytes(spec) and int(want[-1]) == n
    got = h[:4 * len(want)].numpy().view("<u4")
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"offset table differs from the layout rule first at entry {bad[0]} (chunk {bad[0] // P}): {got[bad[0]]} != {want[bad[0]]}"
    assert bool((np.diff(got.astype(np.int64)) >= 0).all())
    hints = h[hdr:n].numpy()
    assert hints.size % 64 == 0
    assert int(hints.max(initial=0)) <= 10
    assert bool((hints[0::64] == 0).all())
    return want


@pytest.mark.parametrize("case", TABLES, ids=_table_id)
def test_index_table_equals_the_layout_rule_across_sizing_blocks(fused, case):
    """Hundreds of chunks: the sizing kernel's running offset crosses its 256-chunk blocks (K below, at, past a multiple of 256; windows whose first chunk
    lies past chunk 256 and 512).  The table equals tests/hint_layout.py's — the layout of DESIGN §3.6 restated without the kernels — and the decodes it
    serves start every tile from a hint and need no fix-up."""
    lib = fused
    kind, chunk, chunks, extra = case
    d, body, spec = _case(kind, chunks, 31, extra, chunk=chunk)
    K = -(-len(d) // chunk)
    n = lib.hint_size_dev(_item(body, spec))
    h = torch.full((n + 256,), 0xFF, dtype=torch.uint8)      # (0xFF is no hint: what the build's tiles do not write must have been zeroed)
    _hint_counters()
    lib.hint_build_dev(_item(body, spec), h.data_ptr(), h.numel())
    assert "zn_k_hint_size" in lib.last_kernels() and "zn_k_decode_hinted^build" in lib.last_kernels()
    written = _hint_counters()[3]
    assert 0 < written <= n - _header_bytes(spec)
    _check_index_bytes(h, n, spec, body)
    assert bool((h[n:] == 0xFF).all()), "the build wrote behind the index"
    h = h[:n]
    _hint_counters(); _tile_counters()
    assert _decode(lib, [(body, spec, 0, K, h, None)])[0] == d
    assert "zn_k_decode_hinted" in lib.last_kernels()
    hc = _hint_counters()
    assert hc[0] > 0 and hc[1] == 0 and hc[2] == 0, hc
    for lo, hi in _table_windows(K):
        _hint_counters()
        got = _decode(lib, [(body, spec, lo, hi, h, None)])[0]
        assert got == d[lo * chunk: min(hi * chunk, len(d))], (lo, hi)
        hc = _hint_counters()
        assert hc[1] == 0 and hc[2] == 0, (lo, hi, hc)
        if (lo + 1) * chunk <= len(d):
            assert hc[0] > 0, (lo, hi, hc)


def test_index_of_a_body_three_bytes_into_its_buffer_serves_a_window_past_chunk_512(fused):
    """Tile boundaries move with the body's address modulo 4, and the hints with them: the table is the same, the bytes are not, and a window whose first
    chunk lies in the sizing kernel's third block decodes from them without a fix-up."""
    lib = fused
    kind, chunk, chunks, extra = TABLES[4]
    assert chunks == 520
    d, body, spec = _case(kind, chunks, 31, extra, chunk=chunk)
    sb = _shifted(body, 3)
    hs, ns = _build(lib, sb, spec)
    want = _check_index_bytes(hs, ns, spec, sb)
    P = spec[0]
    for lo, hi, bd in ((511, 514, sb), (511, 514, body)):
        _hint_counters()
        assert _decode(lib, [(bd, spec, lo, hi, hs, None)])[0] == d[lo * chunk: hi * chunk]
        hc = _hint_counters()
        assert hc[0] > 0 and hc[2] == 0, hc
        assert (hc[1] == 0) == (bd is sb), hc      # (at another address the same hints are bad guesses: fix-ups, the same bytes)
    assert int(want[514 * P]) > int(want[511 * P])


# (kind, planes, bits_mode, bytes_mode, chunk, chunks, every plane Huffman-coded): other instances of zn_fused_wave than weights take — 1-bit codes (the smallest
# sub-blocks, where zn_hint_stream_bytes is tightest), tiles written in several lane groups, 11-bit codes (g up to 10), further planes decoded unhinted behind a
# hinted first one; rand and const have no Huffman plane: their index is the header alone
HOSTILE = [("skew", 1, 1, 10, 128 * 1024, 2, False), ("skew", 2, 0, 10, C2, 2, True), ("skew", 4, 1, 220, C2, 2, True), ("burst", 1, 1, 10, 128 * 1024, 2, False),
           ("burst16", 2, 0, 10, 256 * 1024, 2, False), ("burst16", 2, 0, 10, C2, 3, False), ("u11", 2, 1, 10, C2, 4, False),
           ("rand", 2, 1, 10, C2, 2, False), ("const", 2, 1, 10, C2, 2, False)]


def _hostile(case, seed=13):
    kind, P, rot, bm, chunk, chunks, _ = case
    key = ("hostile", kind, P, rot, chunk, chunks, seed)
    if key not in _CACHE:
        d = _gen2(kind, chunks * chunk, seed)
        _CACHE[key] = (d, _u8(O.compress_frame(b"", d, P, rot, bm, chunk)), (P, rot, bm, chunk, len(d)))
    return _CACHE[key]


@pytest.mark.parametrize("case", HOSTILE, ids=lambda c: f"{c[0]}-P{c[1]}-r{c[2]}-c{c[4] // 1024}k")
def test_hinted_decode_of_hostile_distributions(fused, case):
    lib = fused
    kind, P, rot, bm, chunk, chunks, all_huf = case
    d, body, spec = _hostile(case)
    h, n = _build(lib, body, spec)
    _check_index_bytes(h, n, spec, body)
    _hint_counters(); _tile_counters()
    assert _decode(lib, [(body, spec, 0, chunks, h, None)])[0] == d
    tiles, hc = _tile_counters(), _hint_counters()
    print(f"{kind} P{P}: tiles {tiles[0]}, looping {tiles[1]}, in lane groups {tiles[3]}, hinted {hc[0]}, with fix-up {hc[1]}, unhinted {hc[2]}, index {n} B")
    assert hc[1] == 0, hc
    if kind in ("rand", "const"):
        assert n == _header_bytes(spec) == 64 and hc[0] == 0
    else:
        assert "zn_k_decode_hinted" in lib.last_kernels()
        assert hc[0] > 0
        if all_huf:
            assert hc[0] < tiles[0], (hc, tiles)      # the further planes' tiles take the run-in
        else:
            assert hc[0] == tiles[0], (hc, tiles)
    assert _decode(lib, [(body, spec, 0, chunks, None, None)])[0] == d      # … and without the index (a store after drop_index)
    assert "hinted" not in lib.last_kernels()


def _mixed_kinds_body():
    """The 11-chunk body of test_kernels_simt.test_fused_decode_chunk_groups (bf16, raw, RLE, 11-bit codes, two Huffman planes per chunk, at 16 KiB chunks)
    and its 1000-byte partial tail -> (source, body tensor, spec, kinds per chunk)."""
    if "mixed" not in _CACHE:
        ch = 16384
        r = np.random.default_rng(5)
        parts, kinds = [], []
        for k in range(11):
            kind = ["bf16", "rand", "const", "u11", "skewpair", "bf16"][k % 6]
            kinds.append(kind)
            if kind == "skewpair":
                parts.append(r.choice(np.array([1, 2, 3, 4], dtype=np.uint8), ch, p=[0.7, 0.1, 0.1, 0.1]).tobytes())
            else:
                parts.append(_gen2(kind, ch, 20 + k))
        d = b"".join(parts) + _gen2("bf16", 1000, 3)
        _CACHE["mixed"] = (d, _u8(O.compress_frame(b"", d, 2, 0, 10, ch)), (2, 0, 10, ch, len(d)), kinds)
    return _CACHE["mixed"]


def _mixed_table_check(h, n, spec, body, kinds):
    """The table is the layout rule's; raw and RLE chunks and the partial tail have no region, every other chunk has one."""
    want = _check_index_bytes(h, n, spec, body)
    P = spec[0]
    for c, kind in enumerate(kinds + ["tail"]):
        size = int(want[(c + 1) * P]) - int(want[c * P])
        assert (size == 0) == (kind in ("rand", "const", "tail")), (c, kind, size)


@pytest.mark.parametrize("group", [1, 2, 3, 4])
def test_hinted_chunk_groups_of_mixed_kinds(fused, decode_group, group):
    """A workgroup's group of chunks mixes Huffman, raw, RLE and two-Huffman-plane chunks, and the call has a partial tail: built at the automatic
    grouping, decoded at every group size."""
    lib = fused
    d, body, spec, kinds = _mixed_kinds_body()
    decode_group(lib, 0)
    h, n = _build(lib, body, spec)
    _mixed_table_check(h, n, spec, body, kinds)
    decode_group(lib, group)
    _hint_counters()
    assert _decode(lib, [(body, spec, 0, 12, h, None)])[0] == d
    assert "zn_k_decode_hinted+tail" in lib.last_kernels(), lib.last_kernels()
    hc = _hint_counters()
    assert hc[0] > 0 and hc[1] == 0, hc
