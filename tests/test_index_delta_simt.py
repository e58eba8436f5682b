"""CPU tests (-m "not gpu"): sync indexes of kind ZN_HINT_DELTA (include/zipnn_hip.h) — decode hints for bodies that hold tensor ^ base, built
and read by the delta instances of the hinted kernels — on the SIMT-emulated kernels.  Bodies are the oracle's frames of tensor ^ base; expected outputs are
the tensor's bytes and, where the point is "hints change nothing", the unhinted decode of the same body.  tests/test_gpu_resident_index_delta.py runs the same
shapes on hardware (tests/index_delta_util.py holds what the two share)."""
import numpy as np
import pytest
import torch

import hint_layout as HL
import hint_layout_delta as HLD
import index_delta_util as D
import oracle_lib as O
from test_index_simt import _hint_counters, _tile_counters, _u8

CPU = torch.device("cpu")
C2 = D.C2


@pytest.fixture()
def fused(simt_lib, decode_group):
    """The fused form for every call of the test (small calls would take the wide kernel, which reads no hints); counters zeroed."""
    simt_lib.set_decode_wide(0)
    _tile_counters(); _hint_counters()
    yield simt_lib
    simt_lib.set_decode_wide(1)


def _on_cpu(case):
    a, b, body, spec = case
    return a, b, D.to_dev(body, CPU), D.to_dev(b, CPU), spec


def _regions(body, spec):
    """-> per chunk, the hint bytes of each plane under the DELTA layout rule."""
    P, _, _, ch, n = spec
    bb = D.got(body)
    return [HLD.plane_regions(bb, P, ch, n, c) for c in range(-(-n // ch))]


# ---- dtypes and plane patterns ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp32", "fp8"])
def test_delta_index_decodes_every_pass_from_hints_without_a_fixup(fused, kind):
    """A fine-tune over its base (3 % of the bytes differ: every plane of tensor ^ base is Huffman-coded, the planes behind the first go through
    zn_fused_more_passes): built as DELTA, decoded with the base to the fine-tune's bytes; EVERY tile of every pass starts from its hint and not one needs
    a fix-up — the build and the decode chose the same sub-block sizes."""
    lib = fused
    a, b, body, base, spec = _on_cpu(D.pair_case(kind))
    regions = _regions(body, spec)
    assert all(all(r > 0 for r in rs) for rs in regions), regions          # every plane of every chunk is Huffman-coded and has a region
    h, n = D.build(lib, body, spec)
    built = _hint_counters()
    assert 0 < built[3] <= n - D.header_bytes(spec)
    _tile_counters()
    assert D.decode(lib, body, spec, base, h) == a
    assert D.hinted_launches(lib) == ["zn_k_decode_hinted^delta"], lib.last_kernels()
    tiles, hc = _tile_counters(), _hint_counters()
    print(f"{kind} delta: tiles {tiles[0]}, looping {tiles[1]}, hinted {hc[0]}, hinted with fix-up {hc[1]}, unhinted {hc[2]}, index {n} B = {100.0 * n / len(a):.2f} % of the tensor, {100.0 * n / body.numel():.1f} % of the body")
    assert hc[0] == tiles[0] > 20
    assert hc[1] == 0
    assert hc[2] == 0
    # … and the PLAIN index of the same body has a region for the first plane alone: it is smaller unless there is one plane
    assert (lib.hint_size_dev(D.item(body, spec), 0, D.PLAIN) < n) == (spec[0] > 1)


@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp8"])
def test_delta_index_of_a_dense_body_serves_the_register_resident_form(fused, kind):
    """tensor ^ base as dense as plain weights: the delta instances take 4-dword sub-blocks (their register-resident form; a dense code is capped there or
    keeps its long sub-blocks in the looping form — never the plain instance's dense-code form) — sizes the PLAIN build of the same body does not choose for
    fp16 and fp8, which is why a DELTA index is built by the delta instance."""
    lib = fused
    a, b, body, base, spec = _on_cpu(D.dense_case(kind))
    h, n = D.build(lib, body, spec)
    _hint_counters(); _tile_counters()
    assert D.decode(lib, body, spec, base, h) == a
    tiles, hc = _tile_counters(), _hint_counters()
    assert hc[0] == tiles[0] > 20 and hc[1] == 0 and hc[2] == 0, (tiles, hc)
    if kind == "bf16":
        assert tiles[1] == 0, tiles                   # (the exponent plane: the compile-time 4-dword instance took every tile)
    assert D.decode(lib, body, spec, base, h, inplace=True) == a
    assert _hint_counters()[1] == 0


@pytest.mark.parametrize("group", [1, 2, 3, 4])
def test_delta_index_of_mixed_chunk_kinds_in_every_group_size(fused, decode_group, group):
    """One workgroup's group of chunks mixes: every plane Huffman-coded; the first plane raw and only the later one Huffman-coded; raw; RLE; the first
    Huffman-coded and the later raw — with a partial last chunk behind them, whose tail workgroups read no hints.  Built at the automatic grouping, decoded
    at every group size, to a separate destination and in place."""
    lib = fused
    a, b, body, base, spec = _on_cpu(D.kinds_case(D.CHUNK_KINDS, extra=1000))
    regions = _regions(body, spec)
    for kind, rs in zip(D.CHUNK_KINDS + ("tail",), regions):
        want = {"all_huf": (True, True), "raw_huf": (False, True), "huf_raw": (True, False)}.get(kind, (False, False))
        assert tuple(r > 0 for r in rs) == want, (kind, rs)
    decode_group(lib, 0)
    h, n = D.build(lib, body, spec)
    decode_group(lib, group)
    for inplace in (False, True):
        _hint_counters(); _tile_counters()
        assert D.decode(lib, body, spec, base, h, inplace=inplace) == a
        assert D.hinted_launches(lib) == ["zn_k_decode_hinted^delta^inplace+tail" if inplace else "zn_k_decode_hinted^delta+tail"], lib.last_kernels()
        hc = _hint_counters()
        assert hc[0] > 0 and hc[1] == 0 and hc[2] == 0, hc       # (the tail's tiles belong to no hinted stream decoder: they count nowhere)


def test_first_plane_raw_later_plane_huffman(fused):
    """Chunks whose FIRST plane is stored raw: the one Huffman-coded plane is plane 1, decoded by the first pass from the region of entry c P + 1."""
    lib = fused
    a, b, body, base, spec = _on_cpu(D.kinds_case(("raw_huf",) * 3))
    h, n = D.build(lib, body, spec)
    offs = h[:4 * 7].numpy().view("<u4")
    assert all(offs[2 * c] == offs[2 * c + 1] < offs[2 * c + 2] for c in range(3)), offs       # plane 0: an empty region; plane 1: the chunk's hints
    _hint_counters(); _tile_counters()
    assert D.decode(lib, body, spec, base, h) == a
    tiles, hc = _tile_counters(), _hint_counters()
    assert hc[0] == tiles[0] > 0 and hc[1] == 0 and hc[2] == 0, (tiles, hc)


# ---- every decode path ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["bf16", "fp32", "fp8"])
def test_windows_partial_last_chunk_and_in_place(fused, kind):
    """One index serves every window of its body, to a separate destination and in place over the window's own rows of the base; the tail of a partial last
    chunk stays unhinted and its bytes are right."""
    lib = fused
    for extra in (0, 1000):
        a, b, body, base, spec = _on_cpu(D.pair_case(kind, 4, extra))
        K = -(-len(a) // C2)
        h, _ = D.build(lib, body, spec)
        for lo, hi in ((1, 3), (0, K), (K - 1, K)):
            for inplace in (False, True):
                _hint_counters()
                got = D.decode(lib, body, spec, base, h, lo=lo, hi=hi, inplace=inplace)
                assert got == D.want_window(a, b, spec, lo, hi, inplace), (extra, lo, hi, inplace, lib.last_kernels())
                hc = _hint_counters()
                assert hc[1] == 0 and hc[2] == 0, (extra, lo, hi, inplace, hc)
                if (lo + 1) * C2 <= len(a):
                    assert hc[0] > 0 and "zn_k_decode_hinted^delta" in lib.last_kernels(), (extra, lo, hi, inplace, hc, lib.last_kernels())


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_delta_index_built_where_the_body_lies(fused, shift):
    """Tile boundaries depend on the body's address modulo 4: built 1, 2, 3 bytes into a buffer, the hints need no fix-up there — and do at another address."""
    lib = fused
    a, b, body0, base, spec = _on_cpu(D.pair_case("bf16"))
    body = D.to_dev(body0, CPU, shift)
    assert body.data_ptr() % 4 == shift and body0.data_ptr() % 4 == 0
    h, _ = D.build(lib, body, spec)
    for bd in (body, body0):
        _hint_counters()
        assert D.decode(lib, bd, spec, base, h) == a
        c = _hint_counters()
        assert c[0] > 0 and c[2] == 0 and (c[1] == 0) == (bd is body), (shift, c)


@pytest.mark.parametrize("group", [1, 2, 3, 4])
def test_delta_index_in_every_group_size(fused, decode_group, group):
    lib = fused
    a, b, body, base, spec = _on_cpu(D.pair_case("bf16", 4, 0, seed=6))
    decode_group(lib, 0)
    h, _ = D.build(lib, body, spec)
    decode_group(lib, group)
    _hint_counters()
    assert D.decode(lib, body, spec, base, h, inplace=True) == a
    hc = _hint_counters()
    assert hc[0] > 0 and hc[1] == 0 and hc[2] == 0, hc


def test_hinted_plan_run_twice_in_place_gives_the_base_back(fused):
    lib = fused
    for kind in ("bf16", "fp8"):
        a, b, body, base, spec = _on_cpu(D.pair_case(kind))
        h, _ = D.build(lib, body, spec)
        _hint_counters()
        assert D.decode(lib, body, spec, base, h, inplace=True, plan_runs=1) == a
        assert "zn_k_decode_hinted^delta" in lib.last_kernels()
        assert D.decode(lib, body, spec, base, h, inplace=True, plan_runs=2) == b
        assert D.decode(lib, body, spec, base, h, inplace=True, plan_runs=3) == a
        c = _hint_counters()
        assert c[0] > 0 and c[1] == 0 and c[2] == 0, c


def test_batch_of_delta_and_plain_items_reads_each_kind_where_it_belongs(fused):
    """One call: two delta items with DELTA indexes (one in place), a delta item without an index, an item without a base that brings a PLAIN index.  The
    two-plane launch has delta bases: it runs the delta instance, reads the DELTA indexes and ignores the PLAIN one; the one-plane launch has none and reads
    its PLAIN index as ever."""
    lib = fused
    a1, b1, body1, base1, s1 = _on_cpu(D.pair_case("bf16"))
    a2, b2, body2, base2, s2 = _on_cpu(D.pair_case("fp16", seed=10))
    a3, b3, body3, base3, s3 = _on_cpu(D.pair_case("bf16", seed=12))
    d4 = D._gen2("bf16", 3 * C2, 5); body4 = _u8(O.compress_frame(b"", d4, 2, 1, 10, C2)); s4 = (2, 1, 10, C2, len(d4))
    d5 = D._gen2("fp8", 3 * C2, 5); body5 = _u8(O.compress_frame(b"", d5, 1, 0, 10, C2)); s5 = (1, 0, 10, C2, len(d5))
    h1, _ = D.build(lib, body1, s1)
    h2, _ = D.build(lib, body2, s2)
    h4, _ = D.build(lib, body4, s4, D.PLAIN)
    h5, _ = D.build(lib, body5, s5, D.PLAIN)
    out = torch.full((5, 3 * C2), 0xAB, dtype=torch.uint8)
    out[1].copy_(base2)                      # item 2 runs in place
    hp = lambda h: (h.data_ptr(), h.numel())
    items = [(D.item(body1, s1, 0, 3, out[0].data_ptr(), base1.data_ptr()),) + hp(h1) + (D.DELTA,),
             (D.item(body2, s2, 0, 3, out[1].data_ptr(), out[1].data_ptr()),) + hp(h2) + (D.DELTA,),
             (D.item(body3, s3, 0, 3, out[2].data_ptr(), base3.data_ptr()), None, 0, D.DELTA),
             (D.item(body4, s4, 0, 3, out[3].data_ptr(), None),) + hp(h4) + (D.PLAIN,),
             (D.item(body5, s5, 0, 3, out[4].data_ptr(), None),) + hp(h5) + (D.PLAIN,)]
    _hint_counters(); _tile_counters()
    lib.decompress_hinted_batch_dev(items)
    assert [D.got(out[i]) for i in range(5)] == [a1, a2, a3, d4, d5]
    assert sorted(D.hinted_launches(lib)) == ["zn_k_decode_hinted", "zn_k_decode_hinted^delta^inplace"], lib.last_kernels()
    hc = _hint_counters()
    assert hc[0] > 0 and hc[1] == 0 and hc[2] > 0, hc        # items 3 and 4 ran their tiles from the run-in
    # the same through a plan
    plan = lib.plan_create_hinted(items)
    try:
        out.fill_(0xAB); out[1].copy_(base2)
        lib.plan_run(plan, 0, True)
    finally:
        lib.plan_destroy(plan)
    assert [D.got(out[i]) for i in range(5)] == [a1, a2, a3, d4, d5]
    assert _hint_counters()[1] == 0


# ---- the in-place undo ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [2, 4])
def test_in_place_undo_runs_with_the_same_hints_again(fused, P):
    """tests/delta_inplace_util.tl12_case: chunk 0's LAST plane has a tableLog-12 code — the fused kernel has XORed the planes before it into the base when
    it finds out, runs the same passes once more (from the same hints) to hand the base back, and leaves the chunk to the generic path; chunk 1's first plane
    has one, the fused kernel takes nothing.  The same bytes with and without the index."""
    from delta_inplace_util import tl12_case
    lib = fused
    case, a, b, body_bytes = tl12_case(P)
    spec = (case[2], case[3], case[4], case[5], case[1])
    body, base = D.to_dev(body_bytes, CPU), D.to_dev(b, CPU)
    h, n = D.build(lib, body, spec)
    assert n > D.header_bytes(spec)
    _hint_counters()
    hinted = D.decode(lib, body, spec, base, h, inplace=True)
    assert D.hinted_launches(lib) == ["zn_k_decode_hinted^delta^inplace"], lib.last_kernels()
    hc = _hint_counters()
    assert hc[0] > 0 and hc[1] == 0, hc
    plain = D.decode(lib, body, spec, base, None, inplace=True)
    assert "hinted" not in lib.last_kernels()
    assert hinted == plain == a
    assert D.decode(lib, body, spec, base, h) == a          # (a separate destination: no undo, the generic path redoes the chunk)


# ---- advice -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_delta_hints_are_advice(fused, kind):
    """Zero, 0xFF and random hint bytes, a scrambled table, another body's index, a PLAIN index handed over as DELTA and a DELTA index handed over as PLAIN to
    an item without a base: bytes and verdict are the unhinted call's."""
    lib = fused
    a, b, body, base, spec = _on_cpu(D.pair_case(kind))
    a2, b2, body2, base2, spec2 = _on_cpu(D.pair_case(kind, seed=10))
    h, n = D.build(lib, body, spec)
    hdr = D.header_bytes(spec)
    r = torch.Generator().manual_seed(99)
    for inplace in (False, True):
        assert D.decode(lib, body, spec, base, None, inplace=inplace) == a
        rnd = h.clone(); rnd[hdr:] = torch.randint(0, 256, (rnd.numel() - hdr,), generator=r, dtype=torch.uint8)
        _hint_counters()
        assert D.decode(lib, body, spec, base, rnd, inplace=inplace) == a
        c = _hint_counters()
        assert c[0] > 0 and c[1] > 0, c           # hints were used, and were wrong
        for fill in (0x00, 0xFF):
            bad = h.clone(); bad[hdr:] = fill
            assert D.decode(lib, body, spec, base, bad, inplace=inplace) == a
        scr = torch.randint(0, 256, (h.numel(),), generator=r, dtype=torch.uint8)       # the offset table too
        assert D.decode(lib, body, spec, base, scr, inplace=inplace) == a
        assert D.decode(lib, body, spec, base, torch.full((h.numel(),), 0xFF, dtype=torch.uint8), inplace=inplace) == a
    # body 2's index with body 1 (a buffer long enough for either)
    n2 = lib.hint_size_dev(D.item(body2, spec2), 0, D.DELTA)
    other = torch.zeros(max(n, n2), dtype=torch.uint8)
    lib.hint_build_dev(D.item(body2, spec2), other.data_ptr(), other.numel(), 0, D.DELTA)
    assert D.decode(lib, body, spec, base, other) == a
    # a PLAIN index of this body, passed as DELTA (padded to the DELTA length: the argument check is against the kind named)
    npl = lib.hint_size_dev(D.item(body, spec), 0, D.PLAIN)
    pl = torch.zeros(max(n, npl), dtype=torch.uint8)
    lib.hint_build_dev(D.item(body, spec), pl.data_ptr(), pl.numel(), 0, D.PLAIN)
    _hint_counters()
    assert D.decode(lib, body, spec, base, pl) == a
    assert "zn_k_decode_hinted^delta" in lib.last_kernels()
    # a DELTA index passed as PLAIN to an item without a base: it decodes tensor ^ base, as the unhinted call does
    coded = D.xor(a, b)
    assert D.decode(lib, body, spec, None, None, kind=D.PLAIN) == coded
    assert D.decode(lib, body, spec, None, h, kind=D.PLAIN) == coded
    assert D.hinted_launches(lib) == ["zn_k_decode_hinted"], lib.last_kernels()
    # … and the pairings that read nothing: DELTA beside no base, PLAIN beside a base
    assert D.decode(lib, body, spec, None, h, kind=D.DELTA) == coded
    assert "hinted" not in lib.last_kernels()
    assert D.decode(lib, body, spec, base, pl, kind=D.PLAIN) == a
    assert "hinted" not in lib.last_kernels()


def test_damaged_delta_body_same_verdict_with_and_without_hints(fused):
    """The body is damaged AFTER the build: the hinted decode raises what the unhinted one raises or returns what it returns, to a separate destination and
    in place, and writes nothing outside its destination (guard bytes, checked by decode)."""
    from zipnn_amd._capi import ZnError
    lib = fused
    P, K = 2, 3
    a, b, good, base, spec = _on_cpu(D.kinds_case(("all_huf", "raw_huf", "huf_raw")))      # (raw planes: damage there changes bytes, not the verdict)
    body = good.clone()
    h, _ = D.build(lib, body, spec)
    r = np.random.default_rng(23)
    t0, c0, p0 = 0, P * K, 9 * P * K
    spots = [t0 + int(r.integers(0, P * K)), c0 + 8 * int(r.integers(0, P * K)), c0 + 8 * int(r.integers(0, P * K)) + 5, c0 + 8 * (K - 1)]
    spots += [p0 + int(r.integers(0, good.numel() - p0)) for _ in range(6)]
    spots += [good.numel() - 1 - int(r.integers(0, 3000)) for _ in range(3)]
    outcomes = {"ok": 0, "error": 0}

    def verdict(hints, inplace):
        try:
            return ("ok", D.decode(lib, body, spec, base, hints, inplace=inplace))
        except (ZnError, MemoryError) as e:
            return (type(e).__name__, str(e))
    for i, pos in enumerate(spots):
        flip = (0xFF, 0x01)[i % 2]
        inplace = i % 3 == 0
        body.copy_(good); body[pos] ^= flip
        plain, hinted = verdict(None, inplace), verdict(h, inplace)
        assert plain == hinted, (pos, flip, inplace, plain[0], hinted[0])
        outcomes["ok" if plain[0] == "ok" else "error"] += 1
    assert outcomes["ok"] > 0 and outcomes["error"] > 0, outcomes


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------------

def test_delta_hint_arguments(fused):
    lib = fused
    a, b, body, base, spec = _on_cpu(D.pair_case("bf16"))
    h, n = D.build(lib, body, spec)
    npl = lib.hint_size_dev(D.item(body, spec), 0, D.PLAIN)
    assert npl < n and npl == lib.hint_size_dev(D.item(body, spec))
    out = torch.empty(len(a), dtype=torch.uint8)
    win = D.item(body, spec, 0, 3, out.data_ptr(), base.data_ptr())
    bad = [(h.data_ptr(), n, 2), (h.data_ptr(), n, -1), (None, 0, 7),                      # an unknown kind, with and without an index
           (h.data_ptr(), n - 1, D.DELTA), (h.data_ptr(), npl, D.DELTA), (h.data_ptr(), 16, D.DELTA),      # short (the PLAIN length is short for DELTA: the size is remembered per kind)
           (None, n, D.DELTA), (h.data_ptr(), 0, D.DELTA), (h.data_ptr() + 4, n, D.DELTA)]       # pointer <=> length, alignment
    for hp, hl, kind in bad:
        with pytest.raises(ValueError):
            lib.decompress_hinted_batch_dev([(win, hp, hl, kind)])
        with pytest.raises(ValueError):
            lib.plan_create_hinted([(win, hp, hl, kind)])
    for kind in (2, -1):
        with pytest.raises(ValueError):
            lib.hint_size_dev(D.item(body, spec), 0, kind)
        with pytest.raises(ValueError):
            lib.hint_build_dev(D.item(body, spec), h.data_ptr(), n, 0, kind)
    with pytest.raises(ValueError):
        lib.hint_build_dev(D.item(body, spec), h.data_ptr(), n - 1, 0, D.DELTA)       # capacity below the size
    with pytest.raises(ValueError):
        lib.hint_build_dev(D.item(body, spec), None, n, 0, D.DELTA)
    lib.decompress_hinted_batch_dev([(win, h.data_ptr(), npl, D.PLAIN)])              # long enough for the kind named (and not read: the item has a base)
    assert out.numpy().tobytes() == a and "hinted" not in lib.last_kernels()
    lib.decompress_hinted_batch_dev([(win, None, 0, D.DELTA)])                        # NULL, 0: no hints
    assert out.numpy().tobytes() == a and "hinted" not in lib.last_kernels()
    # the entry points without a kind are kind PLAIN: a delta item decodes unhinted, whatever the index was built as
    _hint_counters()
    for run in (lambda it: lib.decompress_hinted_batch_dev([it]), lambda it: _run_plan(lib, it)):
        out.fill_(0)
        run((win, h.data_ptr(), n))
        assert out.numpy().tobytes() == a
        assert "zn_k_decode_fused^delta" in lib.last_kernels() and "hinted" not in lib.last_kernels(), lib.last_kernels()
    assert _hint_counters()[0] == 0


def _run_plan(lib, it):
    plan = lib.plan_create_hinted([it])
    try:
        lib.plan_run(plan, 0, True)
    finally:
        lib.plan_destroy(plan)


# ---- layout ---------------------------------------------------------------------------------------------------------------------------------------------

# (kind, chunk, chunks, extra bytes): zn_k_hint_size sizes 256 chunks per iteration and carries the running offset to the next
TABLES = [("bf16", 4096, 257, 100), ("fp32", 8192, 258, 0)]


@pytest.mark.parametrize("case", TABLES, ids=lambda c: f"{c[0]}-{c[2]}x{c[1]}" + (f"+{c[3]}B" if c[3] else ""))
def test_delta_index_table_equals_the_layout_rule_across_sizing_blocks(fused, case):
    """Bodies past 256 chunks (K no multiple of 256, a partial last chunk): the DELTA table equals tests/hint_layout_delta.py's — every Huffman-coded plane has
    a region —, the PLAIN size is the old entry point's, and a window that begins before chunk 256 and ends past it decodes from the DELTA index without a
    fix-up."""
    lib = fused
    kind, chunk, chunks, extra = case
    a, b, body, base, spec = _on_cpu(D.pair_case(kind, chunks, extra, seed=31, chunk=chunk))
    P, K = spec[0], -(-len(a) // chunk)
    bb = D.got(body)
    h, n = D.build(lib, body, spec)
    want, hdr = HLD.expected_table(bb, P, chunk, len(a))
    assert hdr == D.header_bytes(spec) and int(want[-1]) == n
    got = h[:4 * len(want)].numpy().view("<u4")
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"offset table differs from the layout rule first at entry {bad[0]} (chunk {bad[0] // P}, plane {bad[0] % P}): {got[bad[0]]} != {want[bad[0]]}"
    assert bool((np.diff(got.astype(np.int64)) >= 0).all())
    hints = h[hdr:n].numpy()
    assert hints.size % 64 == 0 and int(hints.max(initial=0)) <= 10 and bool((hints[0::64] == 0).all())
    if P > 1:
        assert int(np.count_nonzero(np.diff(got.astype(np.int64)))) > K          # more regions than chunks: the further planes have theirs
    assert lib.hint_size_dev(D.item(body, spec), 0, D.PLAIN) == lib.hint_size_dev(D.item(body, spec)) == int(HL.expected_table(bb, P, chunk, len(a))[0][-1])
    for lo, hi in ((254, min(258, K)), (K - 1, K)):
        _hint_counters()
        assert D.decode(lib, body, spec, base, h, lo=lo, hi=hi) == a[lo * chunk: min(hi * chunk, len(a))], (lo, hi)
        hc = _hint_counters()
        assert hc[1] == 0 and hc[2] == 0, (lo, hi, hc)
        if (lo + 1) * chunk <= len(a):
            assert hc[0] > 0, (lo, hi, hc)


@pytest.mark.parametrize("case", ["bf16", "fp32", "fp8", "kinds"])
def test_plain_index_through_the_functions_that_take_a_kind_is_the_old_one(fused, case):
    """ZN_HINT_PLAIN through zn_hint_size_dev2 / zn_hint_build_dev2: the size and every byte of the index the functions without a kind give, whose table is the
    layout rule's of tests/hint_layout.py; read through zn_decompress_hinted_batch_dev2 by an item without a base, it serves every tile."""
    lib = fused
    a, b, body, base, spec = _on_cpu(D.kinds_case(D.CHUNK_KINDS, extra=1000) if case == "kinds" else D.pair_case(case))
    h_old = torch.full((lib.hint_size_dev(D.item(body, spec)),), 0xFF, dtype=torch.uint8)
    lib.hint_build_dev(D.item(body, spec), h_old.data_ptr(), h_old.numel())
    h_new, n_new = D.build(lib, body, spec, D.PLAIN)
    assert n_new == h_old.numel() and torch.equal(h_new, h_old)
    want, _ = HL.expected_table(D.got(body), spec[0], spec[3], spec[4])
    assert bool((h_new[:4 * len(want)].numpy().view("<u4") == want).all())
    _hint_counters()
    assert D.decode(lib, body, spec, None, h_new, kind=D.PLAIN) == D.xor(a, b)
    hc = _hint_counters()
    assert hc[0] > 0 and hc[1] == 0, hc


# ---- the store ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("base_kind", ["dict", "store+index"])
def test_variant_store_with_delta_index(use_simt, base_kind, tmp_path):
    """A variant over plain tensors and one over an indexed resident base, build_index(deltas=True): every entry point gives the fine-tune's tensors (what the
    un-indexed variant gives, tests/resident_delta_util.py), the store's own calls decode from the index without a fix-up, save_file writes what it wrote
    before, and drop_index frees everything."""
    import resident_delta_util as U
    from zipnn_amd.resident import ResidentCheckpoint
    lib = use_simt
    base, ft, base_sd, ft_sd = D.variant_store(base_kind, CPU)
    from delta_file_util import same_file
    before = ft.save_file(str(tmp_path / "before.znn.safetensors"))
    _hint_counters()
    D.check_store_with_delta_index(base_kind, base, ft, base_sd, ft_sd, CPU, lib)
    c = _hint_counters()
    assert c[0] > 0 and c[1] == 0, c
    after = ft.save_file(str(tmp_path / "after.znn.safetensors"))
    assert same_file(after, before)             # the index is not saved (same_file: everything but the order of the metadata keys, which safetensors does not fix)
    held = ft.resident_bytes - ft.index_bytes
    ft.drop_index()
    assert ft.index_bytes == 0 and ft.resident_bytes == held and all(ft.info(n)["index_bytes"] == 0 for n in ft.keys())
    assert U._bytes_equal(ft.get_tensor("w.bf16"), ft_sd["w.bf16"])
    if base_kind == "dict":
        return
    # index="deltas" at construction is index=True plus build_index(deltas=True) (index=True alone: tests/resident_delta_util.py pins that delta entries get none)
    ft4 = ResidentCheckpoint.from_file(str(tmp_path / "after.znn.safetensors"), CPU, base=base, index="deltas")
    assert ft4.info("w.bf16")["index_bytes"] > 0 and ft4.info("absent")["index_bytes"] > 0
    lib.set_decode_wide(0)
    try:
        assert U._bytes_equal(ft4.get_tensor("w.bf16"), ft_sd["w.bf16"])
        assert "zn_k_decode_hinted^delta" in lib.last_kernels()
    finally:
        lib.set_decode_wide(1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32", "fp8"])
def test_delta_index_size_of_a_fine_tune(use_simt, dtype):
    """N(0, 0.02) weights and a fine-tune of them (the weights plus N(0, 0.0005)): the DELTA index as a share of the tensor and of the delta body — a
    measurement of the emulated build, printed; asserted: it is smaller than the body it serves."""
    from zipnn_amd.resident import ResidentCheckpoint
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "fp8": torch.float8_e4m3fn}[dtype]
    g = torch.Generator().manual_seed(4)
    n = 4 * 256 * 1024 // torch.empty(0, dtype=tdt).element_size()
    w = torch.randn(n, generator=g) * (0.02 if dtype != "fp8" else 0.5)
    ft = w + torch.randn(n, generator=g) * (0.0005 if dtype != "fp8" else 0.0125)
    base_sd, ft_sd = {"w": w.to(tdt)}, {"w": ft.to(tdt)}
    base = {"w": base_sd["w"].clone()}
    store = ResidentCheckpoint.from_state_dict(ft_sd, CPU, base=base)
    assert store.info("w")["delta"] is True
    assert store.build_index() == 0 and store.build_index(deltas=True) > 0
    i = store.info("w")
    print(f"{dtype} N(0, 0.02) fine-tune pair: DELTA index {i['index_bytes']} B = {100.0 * i['index_bytes'] / i['nbytes']:.2f} % of the tensor, "
          f"{100.0 * i['index_bytes'] / i['resident_bytes']:.1f} % of the delta body ({i['resident_bytes']} B)")
    assert 0 < i["index_bytes"] < i["resident_bytes"]
    use_simt.set_decode_wide(0)
    try:
        _hint_counters()
        assert torch.equal(store.get_tensor("w").view(torch.uint8), ft_sd["w"].view(torch.uint8))
        c = _hint_counters()
        assert c[0] > 0 and c[1] == 0 and c[2] == 0, c
    finally:
        use_simt.set_decode_wide(1)
