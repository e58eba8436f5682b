"""Shared by tests/test_encode_decisions_simt.py (emulated kernels) and tests/test_gpu_encode_decisions.py (hardware): the encoder's keep-or-store rules, each
on both sides of its edge, at every place zipnn_amd/csrc/zn_encode_fused.hip restates them — the full-chunk stats kernel, the one-pass encoder, the table job
(behind the stats kernel, inside the one-pass encoder, for ragged planes), their P = 1 / 2 / 4 and XOR instances.

    R1  mx == n                      RLE, kept iff 1.0 < n * thr
    R2  mx <= (n >> 7) + 4           raw, no table is tried
    R3  h + 12 >= n, or n < 12       raw            (h: length of the tree description)
    R4  a stream fails BIT_closeCStream's capacity test against cap = the chunk size      raw
    R5  pos >= n - 1                 raw            (pos: tree description + jump table + the four streams)
    R6  cs < (double)n * (double)(float)thr         kept, else raw

Planes are constructed (pure numpy, seeded) so that a rule's two outcomes lie one count, one byte or one float32 step apart.  Every check asserts (a) the
library's frame equals the oracle's, (b) the frame's type bytes and stored sizes equal decide() — the rule chain restated here over the plane's histogram and
what oracle_lib.huf_compress returns —, (c) both outcomes of the edge under test occur: every check_* function asserts the rule names decide() gave its
planes, and a scan that misses a side is a failure, never a skip; and decodes the frame back with the library.  huf_trace() says which of R3 / R4 / R5 ended a
plane that HUF_compress gave up on, from the oracle's own stage functions."""
import functools
import hashlib

import numpy as np

import hint_layout as HL
import oracle_lib as O

HDR = bytes(range(32))
HUF_MAX = 128 * 1024                   # huff0's largest block
PLANE = 16384                          # the plane of the smallest fused geometry: chunk = PLANE * P
BM = {1: 10, 2: 10, 4: 220}            # planes -> bytes_mode
R2_LENGTHS = (16384, 10001, 4097, 1000, 300, 200, 129, 127, 64, 20)
TAILS = (10001, 4097, 129, 127, 20)    # ragged plane lengths behind one full chunk
ONLY = (1000, 300, 200, 64)            # … and as a tensor's only chunk
R3_LENGTHS = tuple(range(9, 24))
R5_SCAN = range(120, 300)              # k of r5_plane: the scans below find both sides of R5 in here, with the oracle alone
R4_SCAN = range(230, 280)              # … and of R4 at n == cap == 16384


# ---- constructions ----
def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def r2_limit(n):
    return (n >> 7) + 4


def r2_plane(n, mx, seed=1):
    """n // mx symbols that occur exactly mx times, the remainder in one more symbol, shuffled: the largest count is mx."""
    full, rem = divmod(n, mx)
    assert 2 <= full and full + (rem > 0) <= 256
    a = np.concatenate([np.repeat(np.arange(full, dtype=np.uint8), mx), np.full(rem, full, dtype=np.uint8)])
    np.random.default_rng(seed).shuffle(a)
    assert int(np.bincount(a).max()) == mx
    return a


def const_plane(n, v=0x5A):
    return np.full(n, v, dtype=np.uint8)


def near_const_plane(n, v=0x5A):
    """A constant plane with one byte changed: two symbols, counts n - 1 and 1."""
    a = const_plane(n, v)
    a[n // 3] = v ^ 0xFF
    return a


def r3_plane(n):
    a = np.zeros(n, dtype=np.uint8)
    a[::3] = 1
    return a


@functools.lru_cache(maxsize=8)
def _r5_base(n):
    r = np.random.default_rng(0)
    return r.integers(1, 256, n, dtype=np.uint8), r.permutation(n)


def r5_plane(n, k):
    """Bytes 1 .. 255 with k positions zeroed: huff0's output shrinks byte by byte as k grows, through n - 1 (not smaller: raw) and n - 2 (kept)."""
    a, perm = _r5_base(n)
    a = a.copy()
    a[perm[:k]] = 0
    return a


def interleave(planes):
    """Equal-length planes -> the bytes of a chunk (plane p is bytes p, p + P, …)."""
    return np.stack(planes, axis=1).reshape(-1)


def chunk_with(plane, P, pos, seed):
    """A chunk of P planes: `plane` at position pos (negative: from the end), noise elsewhere."""
    planes = [noise(plane.size, 1000 * seed + p) for p in range(P)]
    planes[pos % P] = plane
    return interleave(planes)


def rotate_fwd(buf, P):
    """numpy restatement of the oracle's zo_rotate_fwd (whole 32-bit words; a rest is left alone)."""
    out = np.array(buf, dtype=np.uint8)
    u = out[:out.size // 4 * 4].view("<u4")
    if P == 2:
        u[:] = ((u << 1) & 0xFF00FF00) | ((u >> 8) & 0x00800080) | (u & 0x007F007F)
    else:
        u[:] = ((u << 1) & 0xFF000000) | ((u >> 8) & 0x00800000) | (u & 0x007FFFFF)
    return out


def rotate_inv(buf, P):
    """numpy restatement of zo_rotate_inv: the source whose sign-rotated planes are `buf`'s."""
    out = np.array(buf, dtype=np.uint8)
    u = out[:out.size // 4 * 4].view("<u4")
    if P == 2:
        u[:] = ((u << 8) & 0x80008000) | ((u >> 1) & 0x7F807F80) | (u & 0x007F007F)
    else:
        u[:] = ((u << 8) & 0x80000000) | ((u >> 1) & 0x7F800000) | (u & 0x007FFFFF)
    return out


# ---- the rule chain, restated ----
def decide(hist, n, cap, thr, ret):
    """One plane: histogram, length, HUF_compress's dstCapacity (unused by the rules restated here: it acts through `ret`), threshold, and what
    oracle_lib.huf_compress(plane, cap) returned (0, 1, a size, or an error value) -> (type byte, stored size, rule that decided)."""
    thr = float(np.float32(thr))                 # the threshold travels as a float, the compare is done in double
    mx = int(np.max(hist)) if n else 0
    if n == 0:
        return 0, 0, "empty"
    if n <= HUF_MAX and mx == n:
        assert ret == 1
        return (1, 1, "R1+") if 1.0 < float(n) * thr else (0, n, "R1-")
    if n <= HUF_MAX and mx <= (n >> 7) + 4:
        assert ret == 0
        return 0, n, "R2"
    cs = ret & 0xFFFFFFFF                        # the call site keeps 32 bits: an error value becomes a huge size and fails R6
    if cs == 0:
        return 0, n, "R345"                      # which of R3 / R4 / R5: huf_trace()
    return (1, cs, "R6+") if float(cs) < float(n) * thr else (0, n, "R6-")


def float_rule(n, cs, thr):
    """R6 as a float multiply would decide it (the mistake the double compare avoids)."""
    return bool(np.float32(cs) < np.float32(n) * np.float32(thr))


def double_rule(n, cs, thr):
    return float(cs) < float(n) * float(np.float32(thr))


def thresholds_around(cs, n):
    """Four consecutive float32 values from one step below float32(cs / n) to two steps above it."""
    t = [np.nextafter(np.float32(cs / n), np.float32(0))]
    for _ in range(3):
        t.append(np.nextafter(t[-1], np.float32(np.inf)))
    return [float(x) for x in t]


def _ptr(a):
    return O._ptr(a)


def huf_trace(plane, cap):
    """HUF_compress's path through the oracle's own stage functions (table log, code lengths, tree description) and the stream sizes from the per-quarter
    histograms -> (rule that ends it: "R1" / "R2" / "R3" / "R4" / "R5" / "size" / "error", pos — the size before R5, where it gets that far).  Agrees with
    oracle_lib.huf_compress by assertion."""
    L = O.lib()
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    n = plane.size
    ret = O.huf_compress(plane, cap)[0]
    cnt = np.bincount(plane, minlength=256).astype(np.uint32)
    mx = int(cnt.max())
    if mx == n:
        assert ret == 1
        return "R1", 1
    if mx <= (n >> 7) + 4:
        assert ret == 0
        return "R2", 0
    max_sv = int(np.flatnonzero(cnt)[-1])
    nb, val = np.zeros(256, dtype=np.uint8), np.zeros(256, dtype=np.uint16)
    log = L.zo_huf_build_ctable(_ptr(cnt), max_sv, L.zo_optimal_table_log(11, n, max_sv, 1), _ptr(nb), _ptr(val))
    buf = np.zeros(max(cap, 1), dtype=np.uint8)
    h = L.zo_huf_write_ctable(_ptr(buf), cap, _ptr(nb), max_sv, log) if not L.zo_huf_is_error(log) else log
    if L.zo_huf_is_error(h):
        assert ret == h
        return "error", 0
    if h + 12 >= n or n < 12:
        assert ret == 0
        return "R3", 0
    if cap - h < 17:
        assert ret == 0
        return "R4", 0
    pos, seg = h + 6, (n + 3) // 4
    for q in range(4):
        bits = int(nb[plane[q * seg:min((q + 1) * seg, n)]].astype(np.int64).sum()) + 1
        rem = cap - pos
        if rem <= 8 or (bits >> 3) >= rem - 8:
            assert ret == 0
            return "R4", 0
        pos += (bits + 7) >> 3
    if pos >= n - 1:
        assert ret == 0
        return "R5", pos
    assert ret == pos, (ret, pos)
    return "size", pos


@functools.lru_cache(maxsize=None)
def r5_sides(n, cap):
    """-> (k_raw, k_kept): r5_plane(n, k_raw) has pos == n - 1 (R5 stores it raw; `>= n` would keep it) and r5_plane(n, k_kept) has pos == n - 2 (kept with
    thr = 1.0; `>= n - 2` would not).  cap > n.  A scan that misses either is a failure."""
    assert cap > n
    hit = {}
    for k in R5_SCAN:
        rule, pos = huf_trace(r5_plane(n, k), cap)
        assert rule in ("R2", "R5", "size"), (n, cap, k, rule)       # (R2: at n = 16384 the zeros are not yet the 133 that make a table worth trying)
        hit.setdefault((rule, pos), k)
    assert ("R5", n - 1) in hit and ("size", n - 2) in hit, ("R5 scan missed", n, cap, sorted(hit))
    return hit[("R5", n - 1)], hit[("size", n - 2)]


@functools.lru_cache(maxsize=None)
def r4_sides(n=PLANE):
    """-> (k_raw, k_kept) at n == cap: r5_plane(n, k_raw) fails the capacity test of a stream although its size, with room to spare, is below n - 1 (R5 alone
    would keep it); r5_plane(n, k_kept) is the largest block that passes, n - 8 bytes."""
    raw = kept = None
    for k in R4_SCAN:
        p = r5_plane(n, k)
        rule, pos = huf_trace(p, n)
        if rule == "R4":
            roomy = huf_trace(p, 4 * n)
            if roomy[0] == "size":               # R4, and only R4, stores this one raw
                raw = k
        elif rule == "size" and kept is None:
            kept = k
    assert raw is not None and kept is not None, ("R4 scan missed", n, raw, kept)
    assert huf_trace(r5_plane(n, kept), n)[1] == n - 8
    return raw, kept


# ---- frames ----
def planes_of(coded, P, chunk):
    """-> [[plane of chunk c, p]]: the split rule of the frame (the first len % P planes of a chunk get one byte more)."""
    coded = np.asarray(coded, dtype=np.uint8)
    return [[np.ascontiguousarray(coded[c0:c0 + chunk][p::P]) for p in range(P)] for c0 in range(0, coded.size, chunk)]


def expected_tables(coded, P, chunk, thr):
    """decide() for every plane -> (types [P][K], sizes [P][K], rules [P][K])."""
    pl = planes_of(coded, P, chunk)
    K = len(pl)
    types, sizes = np.zeros((P, K), dtype=np.uint8), np.zeros((P, K), dtype=np.int64)
    rules = [[None] * K for _ in range(P)]
    for c in range(K):
        for p in range(P):
            a = pl[c][p]
            ret = O.huf_compress(a, chunk)[0] if a.size else 0
            types[p, c], sizes[p, c], rules[p][c] = decide(np.bincount(a, minlength=256), a.size, chunk, thr, ret)
    return types, sizes, rules


_FRAMES = {}


def oracle_frame(coded, P, rot, chunk, thr):
    """The oracle's frame (cached: the encoder modes share it) — compared once with the reference core's where oracle/_ref is built."""
    coded = np.ascontiguousarray(coded, dtype=np.uint8)
    key = (hashlib.sha1(coded.tobytes()).digest(), P, rot, chunk, float(np.float32(thr)))
    if key not in _FRAMES:
        fr = O.compress_frame(HDR, coded, P, rot, BM[P], chunk, threshold=thr, threads=2)
        if O.ref_core() is not None:
            assert O.ref_compress_frame(HDR, coded, P, rot, BM[P], chunk, threshold=thr) == fr, ("oracle and reference core differ", P, rot, chunk, thr)
        _FRAMES[key] = fr
    return _FRAMES[key]


def _diff(got, want):
    if len(got) != len(want):
        return ("length", len(got), len(want))
    x = np.flatnonzero(np.frombuffer(got, dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8))
    return ("bytes differ", int(x.size), "first at", int(x[0]) if x.size else None)


def fused(P, chunk):
    """zn_encode_fused_ok's geometry rule (16-byte aligned buffers assumed): full chunks of such a tensor go through the stats kernel / the one-pass encoder."""
    return chunk % 16384 == 0 and chunk % (8192 * P) == 0 and chunk // P <= HUF_MAX


def check_frame(lib, src, P, chunk, thr, mode=None, rot=0, base=None):
    """One compress call (zn_compress / zn_compress_delta) under zn_set_encode_onepass(mode) (None: as it is), and the decode of its frame.
    src: the bytes handed to the library; base: the delta base; the planes the rules see are those of src ^ base, sign-rotated where rot.
    -> (rules [P][K] of decide(), sizes [P][K])."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    x = src if base is None else src ^ np.ascontiguousarray(base, dtype=np.uint8)
    n = x.size
    K = -(-n // chunk)
    want = oracle_frame(x, P, rot, chunk, thr)
    seen = rotate_fwd(x, P) if rot and P > 1 else x
    if rot and P > 1:
        assert n % chunk == 0 and chunk % 4 == 0
    types, sizes, rules = expected_tables(seen, P, chunk, thr)
    wt, ws, _ = HL.body_tables(want[32:], P, K)
    assert np.array_equal(wt, types) and np.array_equal(ws, sizes), ("the oracle's tables and the restated decision differ", P, chunk, thr, wt.tolist(), types.tolist())
    delta = None if base is None else np.ascontiguousarray(base, dtype=np.uint8).tobytes()
    if mode is not None:
        lib.set_encode_onepass(mode)
    try:
        got = bytes(lib.compress(HDR, src.tobytes(), P, rot, BM[P], chunk, thr, delta=delta))
        ks = lib.last_kernels()
    finally:
        if mode is not None:
            lib.set_encode_onepass(1)
    gt, gs, _ = HL.body_tables(got[32:], P, K) if len(got) >= 32 + 9 * P * K else (None, None, None)
    assert gt is not None and np.array_equal(gt, types), ("type bytes", P, chunk, thr, mode, ks, None if gt is None else gt.tolist(), types.tolist())
    assert np.array_equal(gs, sizes), ("stored sizes", P, chunk, thr, mode, ks, gs.tolist(), sizes.tolist())
    assert got == want, ("frame", P, chunk, thr, mode, ks) + _diff(got, want)
    nfull = n // chunk if fused(P, chunk) else 0
    if mode is not None and nfull:
        if mode == 2:
            assert "zn_k_encode_onepass" in ks, ks
            misspec = bool(types[:P - 1].any())          # a plane in front of the last one is kept, in a full chunk or in the tail: the layout speculation fails
            assert ("speculation failed" in ks) == misspec, (ks, types.tolist())
        else:
            assert "zn_k_encode_stats" in ks and "zn_k_encode_onepass" not in ks, ks
    back = bytes(lib.decompress(got[32:], P, rot, BM[P], chunk, n, delta=delta))
    assert back == src.tobytes(), ("decode", P, chunk, thr, mode) + _diff(back, src.tobytes())
    return rules, sizes


# ---- the tensors ----
def edge_planes(n, cap):
    """-> [(name, plane)]: both sides of R1, R2 and — R5 where cap > n, R4 where cap == n — of the table job, at thr = 1.0 and length n."""
    L = r2_limit(n)
    out = [("R2 raw", r2_plane(n, L)), ("R2 kept", r2_plane(n, L + 1)), ("R1 rle", const_plane(n)), ("R1 off by one byte", near_const_plane(n))]
    if cap > n:
        k_raw, k_kept = r5_sides(n, cap)
        out += [("R5 raw", r5_plane(n, k_raw)), ("R5 kept", r5_plane(n, k_kept))]
    else:
        k_raw, k_kept = r4_sides(n)
        out += [("R4 raw", r5_plane(n, k_raw)), ("R4 kept", r5_plane(n, k_kept))]
    return out


def edge_tensor(P, pos, n=PLANE, cap=None):
    """One chunk per edge side: the constructed plane at position pos of its chunk, noise in the other planes."""
    cap = cap or n * P
    return np.concatenate([chunk_with(pl, P, pos, 7 + i) for i, (_, pl) in enumerate(edge_planes(n, cap))])


def check_edges(lib, P, pos, mode, n=PLANE, base_seed=None):
    """Full chunks (chunk = n * P) at thr = 1.0: R1, R2 and R4 / R5 on both sides in one call; then R1's threshold edge (1 / n raw, 1.5 / n kept) and R6's
    four thresholds around cs / n of the R2-kept plane.  base_seed: through a delta base of noise (src = planes ^ base)."""
    chunk = n * P
    t = edge_tensor(P, pos, n)
    base = None if base_seed is None else noise(t.size, base_seed)
    def go(coded, thr):
        b = None if base is None else base[:coded.size]
        return check_frame(lib, coded if b is None else coded ^ b, P, chunk, thr, mode, base=b)
    rules, sizes = go(t, 1.0)
    p = pos % P
    col = [rules[p][c] for c in range(6)]
    assert col[:4] == ["R2", "R6+", "R1+", "R6+"], col
    assert col[4:] == ["R345", "R6+"], col
    assert int(sizes[p, 5]) == (n - 2 if P > 1 else n - 8), sizes[p].tolist()
    # R1: the threshold edge on an RLE plane (n is a power of two: 1 / n is exact, 1.0 < 1.0 is false)
    one = chunk_with(const_plane(n), P, pos, 3)
    r_raw, _ = go(one, 1.0 / n)
    r_kept, _ = go(one, 1.5 / n)
    assert (r_raw[p][0], r_kept[p][0]) == ("R1-", "R1+")
    # R6: around cs / n of the R2-kept plane
    cs = int(sizes[p, 1])
    one = chunk_with(r2_plane(n, r2_limit(n) + 1), P, pos, 8)
    got = [go(one, thr)[0][p][0] for thr in thresholds_around(cs, n)]
    assert "R6-" in got and "R6+" in got and got == sorted(got, key=lambda r: r == "R6+"), got
    return got


# ---- ragged planes ----
# a layout places one constructed plane in a tensor: -> (bytes, P, chunk, (plane, chunk) where it lies)
def tail1(plane):
    """P = 1, chunk 16384: the tail behind one full chunk of noise."""
    return np.concatenate([noise(PLANE, 77), plane]), 1, PLANE, (0, 1)


def only1(plane):
    """P = 1, chunk 16384: the tensor's only chunk."""
    return plane, 1, PLANE, (0, 0)


def tail2(pos):
    """P = 2, chunk 32768 (fused full chunks): the tail behind one full chunk, the plane at position pos, noise beside it."""
    return lambda plane: (np.concatenate([noise(2 * PLANE, 78), chunk_with(plane, 2, pos, 21)]), 2, 2 * PLANE, (pos % 2, 1))


def refused2(pos):
    """P = 2, chunk 20002: a geometry the fused kernels refuse — full chunks of two 10001-byte planes go through the ragged workgroups."""
    def f(plane):
        assert plane.size == 10001
        return np.concatenate([noise(20002, 79), chunk_with(plane, 2, pos, 22), noise(2 * 333, 80)]), 2, 20002, (pos % 2, 1)
    return f


def refused4(pos):
    """P = 4, chunk 16384 (not a multiple of 8192 * 4): planes of 4096 through the ragged workgroups."""
    def f(plane):
        assert plane.size == 4096
        return np.concatenate([chunk_with(plane, 4, pos, 23), noise(PLANE, 81)]), 4, PLANE, (pos % 4, 0)
    return f


def check_ragged(lib, layout, n, r5=False, base_seed=None, mode=None):
    """A ragged plane of n bytes on both sides of R1 (count and threshold), R2, R6 and — r5 — R5.  -> [(n, cs, thr)] of the R6 cases in which a float
    multiply would have decided differently."""
    def run(plane, thr):
        src, P, chunk, (p, c) = layout(plane)
        assert not (fused(P, chunk) and (c + 1) * chunk <= src.size), "not a ragged plane"
        base = None if base_seed is None else noise(src.size, base_seed)
        rules, sizes = check_frame(lib, src if base is None else src ^ base, P, chunk, thr, mode, base=base)
        return rules[p][c], int(sizes[p, c]), chunk
    L = r2_limit(n)
    assert run(r2_plane(n, L), 1.0)[0] == "R2"
    rule, cs, cap = run(r2_plane(n, L + 1), 1.0)
    assert rule == "R6+" and huf_trace(r2_plane(n, L + 1), cap) == ("size", cs)
    assert run(const_plane(n), 1.0)[:2] == ("R1+", 1)
    assert run(near_const_plane(n), 1.0)[0] == "R6+"
    assert run(const_plane(n), 0.5 / n)[0] == "R1-" and run(const_plane(n), 1.5 / n)[0] == "R1+"
    if n & (n - 1) == 0:
        assert run(const_plane(n), 1.0 / n)[0] == "R1-"          # 1.0 < 1.0 is false
    if r5:
        k_raw, k_kept = r5_sides(n, cap)
        assert run(r5_plane(n, k_raw), 1.0)[0] == "R345"
        assert run(r5_plane(n, k_kept), 1.0)[:2] == ("R6+", n - 2)
    got, odd = [], []
    for thr in thresholds_around(cs, n):
        got.append(run(r2_plane(n, L + 1), thr)[0])
        assert (got[-1] == "R6+") == double_rule(n, cs, thr)
        if float_rule(n, cs, thr) != double_rule(n, cs, thr):
            odd.append((n, cs, thr))
    assert "R6-" in got and "R6+" in got, got
    return odd


def check_r3(lib):
    """a[::3] = 1, else 0, as the only chunk: 9 .. 14 bytes raw (fewer than 12 bytes, or a tree description of one byte + 12 >= n), 15 .. 23 kept in 12 bytes."""
    for n in R3_LENGTHS:
        rules, sizes = check_frame(lib, r3_plane(n), 1, PLANE, 1.0)
        if n < 15:
            assert rules[0][0] == "R345" and huf_trace(r3_plane(n), PLANE)[0] == "R3", n
        else:
            assert rules[0][0] == "R6+" and int(sizes[0, 0]) == 12, n


def float_double_triples(count=3):
    """-> [(n, cs, thr, plane)]: the first `count` R6 cases of a fixed scan — R2-kept planes of 10001 and 4097 bytes, the four thresholds around cs / n —
    in which float32(cs) < float32(n) * thr and the double compare disagree."""
    out = []
    for n in (10001, 4097):
        for seed in (1, 2, 3):
            pl = r2_plane(n, r2_limit(n) + 1, seed)
            rule, cs = huf_trace(pl, PLANE)
            assert rule == "size"
            for thr in thresholds_around(cs, n):
                if float_rule(n, cs, thr) != double_rule(n, cs, thr) and len(out) < count:
                    out.append((n, cs, thr, pl))
    assert len(out) >= 2, "the scan found fewer than two float / double disagreements"
    return out


def check_float_double(lib):
    """The disagreeing triples through the ragged table job (a tail) — and, as the only plane sizes at which a float product is inexact are not powers of two,
    nowhere else: the library decides as the double compare does."""
    for n, cs, thr, pl in float_double_triples():
        assert float_rule(n, cs, thr) != double_rule(n, cs, thr)
        src, P, chunk, (p, c) = tail1(pl)
        rules, sizes = check_frame(lib, src, P, chunk, thr)
        assert rules[p][c] == ("R6+" if double_rule(n, cs, thr) else "R6-"), (n, cs, thr)


# ---- the largest fused plane ----
def check_largest_plane(lib, mode):
    """P = 1, chunk 131072: RLE, RLE with one byte changed (counts 131071 and 1: the per-quarter counts are 16-bit values, the sort key is count << 8), and R2's
    two sides at L = 1028."""
    n = HUF_MAX
    L = r2_limit(n)
    assert L == 1028
    t = np.concatenate([const_plane(n), near_const_plane(n), r2_plane(n, L), r2_plane(n, L + 1)])
    rules, sizes = check_frame(lib, t, 1, n, 1.0, mode)
    assert rules[0] == ["R1+", "R6+", "R2", "R6+"], rules


# ---- sign rotate ----
def check_rotated(lib, P, mode):
    """bits_mode 1: the source is the inverse rotate of the wanted planes, so the planes the rules see are the constructed ones."""
    wanted = edge_tensor(P, -1)
    src = rotate_inv(wanted, P)
    assert np.array_equal(rotate_fwd(src, P), wanted) and not np.array_equal(src, wanted)
    rules, sizes = check_frame(lib, src, P, PLANE * P, 1.0, mode, rot=1)
    assert rules[P - 1] == ["R2", "R6+", "R1+", "R6+", "R345", "R6+"], rules


# ---- per-item thresholds ----
def check_batch_thresholds(lib, dev):
    """One zn_compress_batch_dev call: a two-plane tensor (a full chunk and a ragged tail, a kept plane in each) eight times — the four thresholds around cs / n
    of either plane — and an RLE tensor at 1 / n and 1.5 / n.  Every body is the oracle's for its own threshold."""
    import torch
    from zipnn_amd import codec
    full, tail = r2_plane(PLANE, r2_limit(PLANE) + 1), r2_plane(10001, r2_limit(10001) + 1)
    t = np.concatenate([chunk_with(full, 2, -1, 8), chunk_with(tail, 2, -1, 21)])
    rle = const_plane(PLANE)
    specs = []
    for pl, cap in ((full, 2 * PLANE), (tail, 2 * PLANE)):
        cs = huf_trace(pl, cap)[1]
        specs += [(t, 2, 2 * PLANE, thr) for thr in thresholds_around(cs, pl.size)]
    specs += [(rle, 1, PLANE, 1.0 / PLANE), (rle, 1, PLANE, 1.5 / PLANE)]
    flats = [torch.frombuffer(bytearray(d.tobytes()), dtype=torch.uint8).to(dev) for d, _, _, _ in specs]
    bodies = codec.compress_device_batch(lib, [(f, P, 0, BM[P], chunk, thr) for f, (d, P, chunk, thr) in zip(flats, specs)])
    seen = []
    for b, (d, P, chunk, thr) in zip(bodies, specs):
        want = oracle_frame(d, P, 0, chunk, thr)[32:]
        got = b.cpu().numpy().tobytes()
        K = -(-d.size // chunk)
        types, sizes, rules = expected_tables(d, P, chunk, thr)
        gt, gs, _ = HL.body_tables(got, P, K)
        assert np.array_equal(gt, types) and np.array_equal(gs, sizes), (P, chunk, thr, gt.tolist(), types.tolist())
        assert got == want, (P, chunk, thr) + _diff(got, want)
        assert bytes(lib.decompress(got, P, 0, BM[P], chunk, d.size)) == d.tobytes()
        seen.append([rules[P - 1][c] for c in range(K)])
    assert [s[0] for s in seen[:4]].count("R6-") in (1, 2, 3) and all(s[1] == "R6+" for s in seen[:4]), seen[:4]
    assert [s[1] for s in seen[4:8]].count("R6-") in (1, 2, 3), seen[4:8]
    assert seen[8:] == [["R1-"], ["R1+"]], seen[8:]
