"""CPU tests (-m "not gpu"): chunk windows of device-resident bodies (zn_decompress_window_batch_dev) and prepared decodes (zn_plan_*) on
the SIMT-emulated kernels.  Every body fed to the new calls is the ORACLE's (oracle_lib.compress_frame, and the reference build's where
oracle/_ref exists) or a golden frame; every expected output is the source bytes."""
import numpy as np
import pytest
import torch

import golden_util as G
import oracle_lib as O
from test_kernels_simt import _delta_pair, _gen2, _oracle_bodies, _ragged_batch, _u8

C = 8192            # every decode form takes chunks of this size (whole rows per stream for 1, 2 and 4 planes)
GUARD = 64
DTYPES = {"bf16": ("bf16", 2, 1, 10), "fp16": ("fp16", 2, 0, 10), "fp32": ("fp32", 4, 1, 220), "fp8": ("fp8", 1, 1, 10)}
SIZES = {"whole": 5 * C, "partial": 5 * C + 2 * 1237 * 2, "small": 3000}
# (zn_set_decode_wide, zn_set_decode_group): the fused kernel with 1..4 chunks per workgroup, the 16- and the 8-wave small-input kernel
FORMS = {"fused-g1": (0, 1), "fused-g2": (0, 2), "fused-g3": (0, 3), "fused-g4": (0, 4), "wide16": (2, 0), "wide8": (3, 0)}


def _windows(K):
    """[0, K), [0, 1), [K-1, K), an interior range, lo == hi"""
    w = [(0, K), (0, 1), (K - 1, K), (min(1, K - 1), max(K - 1, 1)), (K // 2, K // 2)]
    return [(lo, hi) for lo, hi in w if 0 <= lo <= hi <= K]


def _want(data, chunk, lo, hi):
    return data[lo * chunk: min(hi * chunk, len(data))]


def _guarded(sizes):
    """One buffer of 0xAB with a guard in front of, between and behind the destinations -> (buffer, offsets)."""
    offs, o = [], GUARD
    for sz in sizes:
        offs.append(o)
        o += (sz + 15) // 16 * 16 + GUARD
    return torch.full((o,), 0xAB, dtype=torch.uint8), offs


def _assert_guards(buf, offs, sizes):
    mask = torch.ones(buf.numel(), dtype=torch.bool)
    for off, sz in zip(offs, sizes):
        mask[off:off + sz] = False
    assert bool((buf[mask] == 0xAB).all()), "bytes outside a destination were written"


def _items(bodies, specs, wins, buf, offs, deltas=None):
    """(body tensor, spec, window) -> item tuples of ZnLib.decompress_window_batch_dev"""
    out = []
    for i, (b, (_k, nb, P, rot, bm, ch), (lo, hi), off) in enumerate(zip(bodies, specs, wins, offs)):
        sz = len(range(lo * ch, min(hi * ch, nb)))
        d = deltas[i].data_ptr() if deltas is not None and deltas[i] is not None else None
        out.append((b.data_ptr(), b.numel(), P, rot, bm, ch, nb, lo, hi, buf.data_ptr() + off if sz else 0, d))
    return out


def _win_size(spec, win):
    return len(range(win[0] * spec[5], min(win[1] * spec[5], spec[1])))


def _decode_windows(lib, bodies, specs, wins, deltas=None, check=True):
    sizes = [_win_size(s, w) for s, w in zip(specs, wins)]
    buf, offs = _guarded(sizes)
    lib.decompress_window_batch_dev(_items(bodies, specs, wins, buf, offs, deltas), 0, check)
    _assert_guards(buf, offs, sizes)
    return [buf[off:off + sz].numpy().tobytes() for off, sz in zip(offs, sizes)]


@pytest.fixture()
def form(simt_lib, decode_group):
    def set_(name):
        wide, group = FORMS[name]
        simt_lib.set_decode_wide(wide)
        decode_group(simt_lib, group)
    yield set_
    simt_lib.set_decode_wide(1)


@pytest.mark.parametrize("delta", [False, True], ids=["plain", "delta"])
@pytest.mark.parametrize("form_name", list(FORMS))
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_window_equals_slice(simt_lib, form, dtype, size, form_name, delta):
    """Chunks [lo, hi) of the oracle's body, decoded where the body lies == source[lo·chunk : min(hi·chunk, n)], in every decode form, with and
    without a delta base (the oracle's frame of tensor ^ base; the library offsets the base to the window)."""
    kind, P, rot, bm = DTYPES[dtype]
    nb = SIZES[size] // P * P
    if delta:
        data, base = _delta_pair(kind, nb, 7)
        coded = (np.frombuffer(data, dtype=np.uint8) ^ np.frombuffer(base, dtype=np.uint8)).tobytes()
    else:
        data, base, coded = _gen2(kind, nb, 7), None, None
    body = _u8(O.compress_frame(b"", coded if delta else data, P, rot, bm, C))
    bt = _u8(base) if delta else None
    K = -(-nb // C)
    form(form_name)
    spec = (kind, nb, P, rot, bm, C)
    for lo, hi in _windows(K):
        got = _decode_windows(simt_lib, [body], [spec], [(lo, hi)], deltas=[bt] if delta else None)[0]
        assert got == _want(data, C, lo, hi), (lo, hi, simt_lib.last_kernels())
    ks = simt_lib.last_kernels()
    if form_name.startswith("wide") and not delta and K > 1:
        assert "zn_k_decode_wide" in ks                     # (forced: every call without a delta base)


def test_window_of_reference_built_frame(simt_lib):
    """The same through a frame the reference's own build wrote (oracle/_ref)."""
    if O.ref_core() is None:
        pytest.skip("oracle/_ref not built (no reference checkout on this host)")
    data = _gen2("bf16", 6 * C + 700, 3)
    body = _u8(O.ref_compress_frame(b"", data, 2, 1, 10, C))
    spec = ("bf16", len(data), 2, 1, 10, C)
    for win in _windows(7):
        assert _decode_windows(simt_lib, [body], [spec], [win])[0] == _want(data, C, *win)


def test_windows_of_golden_frames(simt_lib):
    """Windows of the committed golden frames (written by the reference): consecutive windows put together are the frame's input (its recorded sha256)."""
    n = 0
    for meta, blob in G.load():
        if len(G.split_frames(blob)) != 1:
            continue
        f = G.parse_frame(blob)
        nb, chunk = f["orig_len"], f["chunk"]
        K = -(-nb // chunk) if chunk else 0
        if nb != meta["in_len"] or not 2 <= K <= 6:
            continue
        body = _u8(bytes(f["body"]))
        spec = (meta["name"], nb, f["num_buf"], f["bits_mode"], f["bytes_mode"], chunk)
        cuts = [(0, 1), (1, K - 1), (K - 1, K)]
        parts = [_decode_windows(simt_lib, [body], [spec], [w])[0] for w in cuts]
        assert G.sha(b"".join(parts)) == meta["in_sha256"], meta["name"]
        n += 1
    assert n >= 1


@pytest.mark.parametrize("form_name", ["fused-g1", "fused-g3", "wide16"])
def test_batch_mixes_windows_and_whole_tensors_of_every_plane_count(simt_lib, form, form_name):
    """One call: windows of several tensors of 1, 2 and 4 planes (ragged and whole) beside whole tensors and empty windows — one launch per plane
    count, every segment with its own window of its own body."""
    specs, datas = _ragged_batch(9, 31, chunk=C, n1=5, n4=5, full_max=5, whole_every=4)
    bodies = [_u8(b) for b in _oracle_bodies(specs, datas)]
    r = np.random.default_rng(5)
    wins = []
    for i, (_k, nb, _P, _r, _b, ch) in enumerate(specs):
        K = -(-nb // ch)
        if i % 3 == 0 or K == 0:
            wins.append((0, K))                             # a whole tensor
        else:
            lo = int(r.integers(0, K + 1)); hi = int(r.integers(lo, K + 1))
            wins.append((lo, hi))
    assert any(lo == hi for lo, hi in wins) and any(hi - lo > 1 for lo, hi in wins) and len({s[2] for s in specs}) == 3
    form(form_name)
    got = _decode_windows(simt_lib, bodies, specs, wins)
    for g, d, s, w in zip(got, datas, specs, wins):
        assert g == _want(bytes(d), s[5], *w), (s, w)
    assert simt_lib.last_kernels().count("zn_k_decode_fused") == 3


def test_same_windows_through_the_host_body_path(simt_lib):
    """zn_decompress_range_dev — the host-resident body, re-based size tables — and the window call give the same bytes."""
    for kind, P, rot, bm in DTYPES.values():
        data = _gen2(kind, (4 * C + 1500) // P * P, 11)
        frame = O.compress_frame(b"", data, P, rot, bm, C)
        body = _u8(frame)
        spec = (kind, len(data), P, rot, bm, C)
        for lo, hi in _windows(5):
            sz = _win_size(spec, (lo, hi))
            out = torch.zeros(max(sz, 1), dtype=torch.uint8)
            simt_lib.decompress_range_dev(frame, P, rot, bm, C, len(data), lo, hi, 0, out.data_ptr() if sz else 0)
            assert out[:sz].numpy().tobytes() == _decode_windows(simt_lib, [body], [spec], [(lo, hi)])[0] == _want(data, C, lo, hi)


@pytest.mark.parametrize("nb", [5 * C, 5 * C + 3000, 3000])
def test_whole_window_is_the_batch_call(simt_lib, nb):
    """[0, K) through the new call == zn_decompress_batch_dev: same bytes, same kernels, same zn_last_fused_chunks / zn_last_tail_planes."""
    specs = [("bf16", nb, 2, 1, 10, C), ("fp32", nb // 4 * 4, 4, 1, 220, C), ("fp8", nb, 1, 1, 10, C)]
    datas = [_gen2(k, n, 13 + i) for i, (k, n, *_r) in enumerate(specs)]
    bodies = [_u8(b) for b in _oracle_bodies(specs, datas)]
    outs = [torch.zeros(n, dtype=torch.uint8) for (_k, n, *_r) in specs]
    simt_lib.decompress_batch_dev([(b.data_ptr(), b.numel(), P, rot, bm, ch, n, o.data_ptr(), None) for b, o, (_k, n, P, rot, bm, ch) in zip(bodies, outs, specs)])
    old = (simt_lib.last_kernels(), simt_lib.last_fused_chunks(), simt_lib.last_tail_planes())
    assert [o.numpy().tobytes() for o in outs] == [bytes(d) for d in datas]
    got = _decode_windows(simt_lib, bodies, specs, [(0, -(-n // ch)) for (_k, n, _P, _r, _b, ch) in specs])
    assert (simt_lib.last_kernels(), simt_lib.last_fused_chunks(), simt_lib.last_tail_planes()) == old
    assert got == [bytes(d) for d in datas]


def test_window_arguments(simt_lib):
    """chunk_lo > chunk_hi and chunk_hi past the last chunk: ZN_E_ARG (ValueError); lo == hi: an empty item that needs neither body bytes beyond the
    tables nor a destination; a body too short for its tables: corrupt, whatever the window."""
    data = _gen2("bf16", 3 * C + 100, 2)
    body = _u8(O.compress_frame(b"", data, 2, 1, 10, C))
    out = torch.zeros(len(data), dtype=torch.uint8)

    def call(lo, hi, b=body, dst=out.data_ptr(), chunk=C, P=2, bm=10):
        simt_lib.decompress_window_batch_dev([(b.data_ptr(), b.numel(), P, 1, bm, chunk, len(data), lo, hi, dst)])
    for lo, hi in ((2, 1), (0, 5), (5, 5), (4, 9), (1 << 40, 1 << 41), (3, 2 ** 64 - 1)):
        with pytest.raises(ValueError):
            call(lo, hi)
    for lo in (0, 2, 4):
        call(lo, lo, dst=0)                                  # empty windows
    with pytest.raises(ValueError):
        call(0, 1, dst=0)                                    # a non-empty one needs a destination
    with pytest.raises(ValueError):
        call(0, 1, chunk=0)
    with pytest.raises(ValueError):
        call(0, 1, P=3)
    from zipnn_amd._capi import ZnError
    with pytest.raises(ZnError):
        call(1, 2, b=body[:40])                              # 2 planes x 4 chunks of tables do not fit 40 bytes
    simt_lib.decompress_window_batch_dev([])                 # an empty batch
    call(0, 4)
    assert out.numpy().tobytes() == data


def _tables(body, P, K):
    """offsets inside a body: (types, cumSizes, payload)"""
    return 0, P * K, 9 * P * K


@pytest.mark.parametrize("kind,P,rot,bm", list(DTYPES.values()), ids=list(DTYPES))
def test_damaged_bodies_through_the_window_call(simt_lib, kind, P, rot, bm):
    """Bytes of the types, of cumSizes (rows inside and outside the window, and the plane totals at kb - 1) and of the payload are flipped: every
    call reports corrupt data / a bad type or decodes — it never writes outside its destination (guard bytes) and never faults.  (scripts/simt_sanitize.sh
    runs this file under ASan + UBSan: reads outside the body would show there.)"""
    from zipnn_amd._capi import ZnError
    nb = (6 * C + 2500) // P * P
    K = 7
    data = _gen2(kind, nb, 17)
    good = bytearray(O.compress_frame(b"", data, P, rot, bm, C))
    t0, c0, p0 = _tables(good, P, K)
    spec = (kind, nb, P, rot, bm, C)
    r = np.random.default_rng(23)
    wins = [(2, 4), (0, K), (K - 1, K), (0, 1)]
    spots = [("types", t0 + int(r.integers(0, P * K))) for _ in range(3)]
    spots += [("cum-low", c0 + 8 * int(r.integers(0, P * K))) for _ in range(3)]            # low byte of an entry: sizes shift by < 256
    spots += [("cum-high", c0 + 8 * int(r.integers(0, P * K)) + int(r.integers(3, 8))) for _ in range(3)]      # high bytes: huge sizes, sums that would wrap
    spots += [("cum-total", c0 + 8 * (q * K + K - 1) + j) for q in range(P) for j in (0, 7)]                  # the plane totals
    spots += [("payload", p0 + int(r.integers(0, len(good) - p0))) for _ in range(3)]
    outcomes = {"ok": 0, "error": 0}
    for what, pos in spots:
        for flip in (0xFF, 0x01):
            bad = bytearray(good); bad[pos] ^= flip
            body = _u8(bytes(bad))
            for win in wins:
                try:
                    got = _decode_windows(simt_lib, [body], [spec], [win])[0]        # (asserts the guard bytes)
                    outcomes["ok"] += 1
                    if what == "types" and not (win[0] <= (pos - t0) % K < win[1]):
                        assert got == _want(data, C, *win)      # a type byte of a chunk outside the window is never looked at
                except (ZnError, MemoryError):
                    outcomes["error"] += 1
    assert outcomes["ok"] > 0 and outcomes["error"] > 0, outcomes
    # a wrong orig_size (so a wrong kb) against the same body.  Where the tables of the claimed geometry cannot fit the body the call must say corrupt (the
    # host's check; the kernels repeat it on kb); where they fit, the parse reads entries of a table that is not there — bytes of the same body —: any
    # outcome but a write outside the destination (guard bytes) or a read outside the body (the sanitizer runs)
    body = _u8(bytes(good))
    fits = 0
    for claim in (nb + 40 * C, nb + 4000 * C, nb + 40000 * C):
        kb = -(-claim // C)
        if len(good) < 9 * P * kb:
            with pytest.raises(ZnError):
                _decode_windows(simt_lib, [body], [(kind, claim, P, rot, bm, C)], [(kb - 2, kb - 1)])
        else:
            fits += 1
            for win in ((kb - 2, kb - 1), (0, 2), (kb // 2, kb // 2 + 1)):
                try:
                    _decode_windows(simt_lib, [body], [(kind, claim, P, rot, bm, C)], [win])
                except (ZnError, MemoryError):
                    pass
    assert 1 <= fits <= 2


# ---- plans --------------------------------------------------------------------------------------------------------------------
def _plan_case(seed, n2=6):
    specs, datas = _ragged_batch(n2, seed, chunk=C, n1=3, n4=3, full_max=4, whole_every=5)
    bodies = [_u8(b) for b in _oracle_bodies(specs, datas)]
    r = np.random.default_rng(seed)
    wins = []
    for i, (_k, nb, _P, _r, _b, ch) in enumerate(specs):
        K = -(-nb // ch)
        lo = int(r.integers(0, K + 1)) if i % 2 else 0
        wins.append((lo, K if i % 2 == 0 else int(r.integers(lo, K + 1))))
    sizes = [_win_size(s, w) for s, w in zip(specs, wins)]
    buf, offs = _guarded(sizes)
    want = [_want(bytes(d), s[5], *w) for d, s, w in zip(datas, specs, wins)]
    return specs, bodies, wins, sizes, buf, offs, want


def _check_plan_output(case):
    specs, bodies, wins, sizes, buf, offs, want = case
    _assert_guards(buf, offs, sizes)
    assert [buf[o:o + s].numpy().tobytes() for o, s in zip(offs, sizes)] == want


def test_plan_runs_repeatedly(simt_lib):
    """A plan run three times (the destination wiped in between) gives the same bytes; it survives zn_release_workspace (it owns its table)."""
    case = _plan_case(41)
    specs, bodies, wins, sizes, buf, offs, want = case
    plan = simt_lib.plan_create(_items(bodies, specs, wins, buf, offs))
    try:
        for i in range(3):
            buf.fill_(0xAB)
            simt_lib.plan_run(plan, 0, True)
            _check_plan_output(case)
        ks = simt_lib.last_kernels()
        simt_lib.release_workspace()
        buf.fill_(0xAB)
        simt_lib.plan_run(plan, 0, True)
        _check_plan_output(case)
        assert simt_lib.last_kernels() == ks
    finally:
        simt_lib.plan_destroy(plan)


def test_two_plans_interleaved_with_ordinary_calls(simt_lib):
    a, b = _plan_case(43), _plan_case(47, n2=4)
    pa = simt_lib.plan_create(_items(a[1], a[0], a[2], a[4], a[5]))
    pb = simt_lib.plan_create(_items(b[1], b[0], b[2], b[4], b[5]))
    data = _gen2("bf16", 3 * C + 10, 1)
    frame = O.compress_frame(b"", data, 2, 1, 10, C)
    try:
        for _ in range(2):
            simt_lib.plan_run(pa, 0, True)
            assert bytes(simt_lib.decompress(frame, 2, 1, 10, C, len(data))) == data       # a host-buffer call in between
            simt_lib.plan_run(pb, 0, True)
            got = _decode_windows(simt_lib, [a[1][0]], [a[0][0]], [a[2][0]])                # … and a one-shot window call
            assert got[0] == a[6][0]
            _check_plan_output(a)
            _check_plan_output(b)
            a[4].fill_(0xAB); b[4].fill_(0xAB)
            simt_lib.plan_run(pb, 0, True); simt_lib.plan_run(pa, 0, True)
            _check_plan_output(a)
            _check_plan_output(b)
    finally:
        simt_lib.plan_destroy(pa)
        simt_lib.plan_destroy(pb)


def test_plan_status_after_unchecked_runs(simt_lib):
    """check = 0 + zn_decode_status: ok for a good plan; a plan over a damaged body reports it there, not at the run."""
    from zipnn_amd._capi import ZnError
    case = _plan_case(53)
    specs, bodies, wins, sizes, buf, offs, want = case
    plan = simt_lib.plan_create(_items(bodies, specs, wins, buf, offs))
    try:
        simt_lib.plan_run(plan, 0, False)
        simt_lib.decode_status()
        _check_plan_output(case)
    finally:
        simt_lib.plan_destroy(plan)
    data = _gen2("bf16", 4 * C, 3)
    bad = bytearray(O.compress_frame(b"", data, 2, 1, 10, C)); bad[2 * 4 + 8 * 5 + 7] ^= 0x40      # a cumSizes entry of plane 1: a size beyond the body
    body = _u8(bytes(bad))
    out, o = _guarded([4 * C])
    plan = simt_lib.plan_create(_items([body], [("bf16", 4 * C, 2, 1, 10, C)], [(0, 4)], out, o))
    try:
        simt_lib.plan_run(plan, 0, False)                    # launches; says nothing
        with pytest.raises((ZnError, MemoryError)):
            simt_lib.decode_status()
        with pytest.raises((ZnError, MemoryError)):
            simt_lib.plan_run(plan, 0, True)
        _assert_guards(out, o, [4 * C])
    finally:
        simt_lib.plan_destroy(plan)


def test_plan_arguments_and_lifetime(simt_lib):
    """zn_plan_create checks what the one-shot call checks; an empty plan runs; create / destroy in a loop does not grow the process."""
    import resource
    data = _gen2("bf16", 3 * C, 2)
    body = _u8(O.compress_frame(b"", data, 2, 1, 10, C))
    out = torch.zeros(len(data), dtype=torch.uint8)
    with pytest.raises(ValueError):
        simt_lib.plan_create([(body.data_ptr(), body.numel(), 2, 1, 10, C, len(data), 2, 1, out.data_ptr())])
    with pytest.raises(ValueError):
        simt_lib.plan_create([(body.data_ptr(), body.numel(), 2, 1, 10, C, len(data), 0, 4, out.data_ptr())])
    empty = simt_lib.plan_create([])
    simt_lib.plan_run(empty, 0, True)
    simt_lib.plan_destroy(empty)
    case = _plan_case(59)
    items = _items(case[1], case[0], case[2], case[4], case[5])

    for _ in range(5):
        p = simt_lib.plan_create(items)
        simt_lib.plan_run(p, 0, False)
        simt_lib.plan_destroy(p)
    _check_plan_output(case)

    def cycle(n):
        for _ in range(n):
            simt_lib.plan_destroy(simt_lib.plan_create(items))
    cycle(2000)                                              # (allocator warm-up)
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    cycle(30000)
    grown = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before
    assert grown < 8192, f"30 000 create / destroy cycles grew the process by {grown} KiB"      # (a leaked table alone would be 30 000 x 12 segments x 96 bytes = 35 MB)
