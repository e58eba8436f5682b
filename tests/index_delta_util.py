"""Shared by tests/test_index_delta_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_resident_index_delta.py (hardware): sync indexes
of kind ZN_HINT_DELTA (include/zipnn_hip.h) — bodies of tensor ^ base decoded from an index by the delta instances.  Bodies are the CPU oracle's
frames (oracle_lib.compress_frame) of tensor ^ base; expected outputs are the tensor's bytes, and, where the point is "hints change nothing", what the same call
gives without an index.  Everything is small: 64 KiB chunks (a stream of them is a few tiles long), three or four chunks per tensor."""
import functools

import numpy as np
import torch

import oracle_lib as O
from test_kernels_simt import _delta_pair, _gen2

PLAIN, DELTA = 0, 1
C2 = 64 * 1024
GUARD = 64
# kind -> (planes, bits_mode, bytes_mode): the frame parameters of the dtypes
LAYOUT = {"bf16": (2, 1, 10), "fp16": (2, 0, 10), "fp32": (4, 1, 220), "fp8": (1, 0, 10)}


def xor(a, b):
    return (np.frombuffer(a, dtype=np.uint8) ^ np.frombuffer(b, dtype=np.uint8)).tobytes()


@functools.lru_cache(maxsize=None)
def pair_case(kind, chunks=3, extra=0, seed=9, chunk=C2):
    """-> (tensor bytes, base bytes, body of tensor ^ base, spec): test_kernels_simt._delta_pair's recipe — the base with 3 % of its bytes perturbed, so that
    every plane of the body is Huffman-coded."""
    P, rot, bm = LAYOUT[kind]
    a, b = _delta_pair(kind, (chunks * chunk + extra) // P * P, seed)
    return a, b, O.compress_frame(b"", xor(a, b), P, rot, bm, chunk), (P, rot, bm, chunk, len(a))


@functools.lru_cache(maxsize=None)
def dense_case(kind, chunks=3, seed=9):
    """-> (tensor, base, body, spec) where tensor ^ base is itself weights-like (test_kernels_simt._gen2 of `kind`): the Huffman plane is as dense as a plain
    body's, so the delta instances choose the sub-block sizes of their register-resident form (4 dwords) or cap a longer one — where a sparse delta takes
    short sub-blocks and the looping form."""
    P, rot, bm = LAYOUT[kind]
    coded = _gen2(kind, chunks * C2, seed)
    b = _gen2("rand", len(coded), seed + 1)
    return xor(coded, b), b, O.compress_frame(b"", coded, P, rot, bm, C2), (P, rot, bm, C2, len(coded))


def _sparse(n, seed, frac=0.03):
    r = np.random.default_rng(seed)
    x = np.zeros(n, dtype=np.uint8)
    hit = r.random(n) < frac
    x[hit] = r.integers(1, 256, int(hit.sum()), dtype=np.uint8)
    return x


# what tensor ^ base looks like in one chunk of a two-plane body without the sign rotate (plane p = the bytes at offsets p mod 2)
CHUNK_KINDS = ("all_huf", "raw_huf", "raw_raw", "rle_rle", "huf_raw", "all_huf")


def _coded_chunk(kind, seed, chunk=C2):
    r = np.random.default_rng(seed)
    rnd = lambda: r.integers(0, 256, chunk // 2, dtype=np.uint8)
    p0, p1 = {"all_huf": lambda: (_sparse(chunk // 2, seed), _sparse(chunk // 2, seed + 1)), "raw_huf": lambda: (rnd(), _sparse(chunk // 2, seed)),
              "raw_raw": lambda: (rnd(), rnd()), "rle_rle": lambda: (np.full(chunk // 2, 7, dtype=np.uint8), np.zeros(chunk // 2, dtype=np.uint8)),
              "huf_raw": lambda: (_sparse(chunk // 2, seed), rnd())}[kind]()
    return np.stack([p0, p1], axis=1).reshape(-1).tobytes()


@functools.lru_cache(maxsize=None)
def kinds_case(kinds, extra=0, seed=40):
    """kinds: a tuple of CHUNK_KINDS names, one per chunk -> (tensor, base, body, spec) of a two-plane body (fp16's layout) whose chunks are of those kinds;
    extra: bytes of a partial last chunk (sparse)."""
    coded = b"".join(_coded_chunk(k, seed + 3 * i) for i, k in enumerate(kinds)) + _sparse(extra, seed + 99).tobytes()
    b = _gen2("fp16", len(coded), seed)
    return xor(coded, b), b, O.compress_frame(b"", coded, 2, 0, 10, C2), (2, 0, 10, C2, len(coded))


def to_dev(data, dev, shift=0):
    """bytes or a CPU byte tensor -> device memory, `shift` bytes into a 16-byte aligned allocation."""
    t = data if isinstance(data, torch.Tensor) else (torch.frombuffer(bytearray(data), dtype=torch.uint8) if len(data) else torch.empty(0, dtype=torch.uint8))
    big = torch.zeros(t.numel() + 32, dtype=torch.uint8, device=dev)
    s = (-big.data_ptr()) % 16 + shift
    v = big[s:s + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == shift
    return v


def got(v):
    return v.cpu().numpy().tobytes()


def stream_of(dev):
    return torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == "cuda" else 0


def item(body, spec, lo=0, hi=None, dst=0, delta=None):
    P, rot, bm, ch, n = spec
    return (body.data_ptr(), body.numel(), P, rot, bm, ch, n, lo, -(-n // ch) if hi is None else hi, dst, delta)


def header_bytes(spec):
    P, _, _, ch, n = spec
    return ((P * -(-n // ch) + 1) * 4 + 63) // 64 * 64


def build(lib, body, spec, kind=DELTA):
    """-> (the index of `body` where it lies, its length): sized and built through the entry points that take a kind; nothing is written behind it."""
    st = stream_of(body.device)
    n = lib.hint_size_dev(item(body, spec), st, kind)
    assert n >= header_bytes(spec)
    h = torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=body.device)      # (0xFF is no hint: what the build's tiles do not write must have been zeroed)
    assert h.data_ptr() % 16 == 0
    lib.hint_build_dev(item(body, spec), h.data_ptr(), n, st, kind)
    ks = lib.last_kernels()
    assert "zn_k_hint_size" in ks and ("zn_k_decode_hinted^delta^build" if kind == DELTA else "zn_k_decode_hinted^build") in ks, ks
    assert bool((h[n:] == 0xFF).all()), "the build wrote behind the index"
    return h[:n], n


def _guarded(nbytes, dev, fill=None):
    buf = torch.full((nbytes + 2 * GUARD + 16,), 0xAB, dtype=torch.uint8, device=dev)
    s = GUARD + (-(buf.data_ptr() + GUARD)) % 16
    v = buf[s:s + nbytes]
    if fill is not None:
        v.copy_(fill)
    return buf, v


def _guards_ok(buf, v):
    s = v.data_ptr() - buf.data_ptr()
    return bool((buf[:s] == 0xAB).all()) and bool((buf[s + v.numel():] == 0xAB).all())


def decode(lib, body, spec, base, hints, kind=DELTA, lo=0, hi=None, inplace=False, plan_runs=0, check=True):
    """One hinted call (or a hinted plan run `plan_runs` times) over the window [lo, hi) of `body`, a body of tensor ^ base; base: the whole tensor's base on
    the device, or None for a body decoded without one.  hints None: no index.
    Separate destination -> the window's bytes.  inplace: the destination is a copy of the WHOLE base and the window runs over its own rows of it
    (d_dst == d_delta + lo * chunk) -> the whole buffer's bytes.  Guard bytes around the destination are checked."""
    P, _, _, ch, n = spec
    K = -(-n // ch)
    hi = K if hi is None else hi
    dev = body.device
    st = stream_of(dev)
    wn = len(range(lo * ch, min(hi * ch, n)))
    if inplace:
        buf, dst = _guarded(n, dev, base)
        win = item(body, spec, lo, hi, dst.data_ptr() + lo * ch, dst.data_ptr())
    else:
        buf, dst = _guarded(wn, dev)
        win = item(body, spec, lo, hi, dst.data_ptr(), base.data_ptr() if base is not None else None)
    it = (win, hints.data_ptr() if hints is not None else None, hints.numel() if hints is not None else 0, kind)
    try:
        if plan_runs:
            plan = lib.plan_create_hinted([it])
            try:
                for _ in range(plan_runs):
                    lib.plan_run(plan, st, check)
            finally:
                if dev.type == "cuda":
                    torch.cuda.synchronize()
                lib.plan_destroy(plan)
        else:
            lib.decompress_hinted_batch_dev([it], st, check)
    finally:
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert _guards_ok(buf, dst), "bytes outside the destination were written"
    return got(dst)


def want_window(a, b, spec, lo, hi, inplace):
    ch, n = spec[3], spec[4]
    end = min(hi * ch, n)
    return b[:lo * ch] + a[lo * ch:end] + b[end:] if inplace else a[lo * ch:end]


def hinted_launches(lib):
    return [k for k in lib.last_kernels().split(";") if k.startswith("zn_k_decode_hinted")]


# ---- the store ----
def variant_store(kind, dev):
    """-> (base, variant store over it, base_sd, ft_sd): tests/resident_delta_util.py's state dicts over a base of `kind` (resident_delta_util.BASES); the
    variant records digests of the fine-tune's tensors (digests=True), so that verify() has something to hold its decodes against."""
    import resident_delta_util as U
    from zipnn_amd import ResidentCheckpoint
    base_sd, ft_sd = U.state_dicts()
    base = U.make_base(kind, base_sd, dev)
    return base, ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base, digests=True), base_sd, ft_sd


class launches_of:
    """with launches_of(lib) as seen: …  — the zn_last_kernels() behind every hinted batched call the block makes (a later call of another kind, a digest
    launch for instance, replaces what zn_last_kernels says)."""

    def __init__(self, lib):
        self.lib, self.seen = lib, []

    def __enter__(self):
        inner = self.lib.decompress_hinted_batch_dev

        def spy(*a, **k):
            r = inner(*a, **k)
            self.seen.append(self.lib.last_kernels())
            return r
        self.lib.decompress_hinted_batch_dev = spy
        return self.seen

    def __exit__(self, *exc):
        del self.lib.decompress_hinted_batch_dev          # (the instance attribute: the class's method shows again)


def check_store_with_delta_index(kind, base, ft, base_sd, ft_sd, dev, lib, wide_after=1):
    """build_index(deltas=True) on the variant store `ft`: the delta entries — and, beyond the plain ones build_index() indexes, only they — hold an index,
    and every entry point — get_tensor(s), get_slice, plan (run twice), hook, verify, apply_ / revert_ — gives what the un-indexed variant gives: the
    fine-tune's tensors, bit for bit.  The fused form is forced meanwhile (zn_set_decode_wide(0)); wide_after: the mode left behind."""
    import resident_delta_util as U
    names = list(ft_sd.keys())
    deltas = [n for n in names if ft.info(n)["delta"] is True]
    assert set(deltas) >= {"w.bf16", "w.fp32", "w.fp8", "0.weight", "1.weight"}
    held = ft.resident_bytes
    assert ft.build_index() > 0                                  # the default: plain entries only
    assert all(ft.info(n)["index_bytes"] == 0 for n in names if ft.info(n)["delta"] is not False)
    assert ft.info("absent")["index_bytes"] > 0
    plain_index = ft.index_bytes
    added = ft.build_index(deltas=True)
    assert added > 0 and ft.index_bytes == plain_index + added and ft.resident_bytes == held + ft.index_bytes
    for n in names:
        assert (ft.info(n)["index_bytes"] > 0) == (ft.info(n)["delta"] is True or (ft.info(n)["delta"] is False and ft.info(n)["compressed"])), n
    assert ft.build_index(deltas=True) == 0                      # (tensors already indexed keep their index)
    lib.set_decode_wide(0)
    try:
        res = ft.get_tensors(names)
        assert any(k.startswith("zn_k_decode_hinted^delta") for k in hinted_launches(lib)), lib.last_kernels()
        for n in names:
            assert U._bytes_equal(res[n], ft_sd[n]), n
        # verify(): every tensor decoded through the store's normal path into a scratch buffer and digested — the delta windows from the DELTA index
        with launches_of(lib) as seen:
            ok = ft.verify()
        assert sorted(ok) == sorted(names) and all(ok.values()), ok
        assert any("zn_k_decode_hinted^delta" in k for k in seen), seen
        # apply_ / revert_ (in place over live base weights) read the index as well
        U.check_apply_revert(kind, base_sd, ft_sd, dev, base=base, ft=ft)
        for n in ("w.fp32", "identical", "0.weight"):
            assert U._bytes_equal(ft.get_tensor(n), ft_sd[n]), n
        assert "zn_k_decode_hinted^delta" in lib.last_kernels(), lib.last_kernels()
        for n, idx in (("w.bf16", slice(250, 261)), ("w.fp32", slice(120, 129)), ("w.fp8", slice(0, 2))):
            assert U._bytes_equal(ft.get_slice(n)[idx], ft_sd[n][idx]), (n, idx)
        ft.status()
        plan = ft.plan(names)
        for _ in range(2):
            views = plan.run()
            plan.status()
            for n in names:
                assert U._bytes_equal(views[n], ft_sd[n]), n
        plan.close()
        x = (torch.randn(4, 512, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(dev)
        want = U.model_of(ft_sd, dev)(x)
        m = U.model_of(base_sd, dev)
        h = ft.hook(m)
        out = m(x)
        h.status()
        assert U._bytes_equal(out, want)
        h.remove()
    finally:
        lib.set_decode_wide(wide_after)
