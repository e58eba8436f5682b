"""GPU tests (-m gpu): chunk windows of device-resident bodies, prepared decodes (zn_plan_*) and zipnn_amd.ResidentCheckpoint on the real
libzipnn_hip.so.  Bodies are the CPU oracle's or the golden file's; expected outputs are the source bytes.  No damaged bodies here: those stay
on the emulator (tests/test_window_simt.py)."""
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from test_gpu_batch_scale import _assert_same, _stage
from test_kernels_simt import _delta_pair, _gen2, _oracle_bodies, _ragged_batch

pytestmark = pytest.mark.gpu
KB = 1024
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpt2_small_ref.znn.safetensors")
DTYPES = {"bf16": ("bf16", 2, 1, 10, 256 * KB), "fp16": ("fp16", 2, 0, 10, 256 * KB), "fp32": ("fp32", 4, 1, 220, 256 * KB), "fp8": ("fp8", 1, 1, 10, 128 * KB)}
FORMS = {"auto": (1, 0), "fused-g1": (0, 1), "fused-g2": (0, 2), "fused-g3": (0, 3), "fused-g4": (0, 4), "wide16": (2, 0), "wide8": (3, 0)}
GUARD = 256


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    yield L
    L.set_decode_wide(1); L.set_decode_group(0)
    L.release_workspace()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _win_size(nb, ch, lo, hi):
    return max(min(hi * ch, nb) - lo * ch, 0)


def _decode(lib, bodies, specs, wins, deltas=None, check=True):
    """-> decoded windows (views of one guarded buffer); asserts that nothing outside them was written."""
    dev = bodies[0].device
    sizes = [_win_size(s[1], s[5], *w) for s, w in zip(specs, wins)]
    offs, o = [], GUARD
    for sz in sizes:
        offs.append(o); o += (sz + 255) // 256 * 256 + GUARD
    buf = torch.full((o,), 0xAB, dtype=torch.uint8, device=dev)
    lib.decompress_window_batch_dev([(b.data_ptr(), b.numel(), P, rot, bm, ch, nb, lo, hi, buf.data_ptr() + off if sz else 0,
                                      (deltas[i].data_ptr() if deltas is not None and deltas[i] is not None else None))
                                     for i, (b, (_k, nb, P, rot, bm, ch), (lo, hi), off, sz) in enumerate(zip(bodies, specs, wins, offs, sizes))], _stream(), check)
    mask = torch.ones(o, dtype=torch.bool, device=dev)
    for off, sz in zip(offs, sizes):
        mask[off:off + sz] = False
    assert bool((buf[mask] == 0xAB).all()), "bytes outside a destination were written"
    return [buf[off:off + sz] for off, sz in zip(offs, sizes)]


def _windows(K):
    w = [(0, K), (0, 1), (K - 1, K), (min(1, K - 1), max(K - 1, 1)), (K // 2, K // 2)]
    return [(lo, hi) for lo, hi in w if 0 <= lo <= hi <= K]


@pytest.mark.parametrize("delta", [False, True], ids=["plain", "delta"])
@pytest.mark.parametrize("size", ["whole", "partial", "small"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_window_equals_slice_at_real_chunk_sizes(lib, decode_group, dtype, size, delta):
    """256 KiB chunks (128 KiB for fp8), every decode form, with and without a delta base: chunks [lo, hi) == source[lo·chunk : min(hi·chunk, n)]."""
    dev = torch.device("cuda:0")
    kind, P, rot, bm, ch = DTYPES[dtype]
    nb = {"whole": 6 * ch, "partial": 6 * ch + 100 * KB + 4 * 37, "small": 70 * KB}[size] // P * P
    if delta:
        data, base = _delta_pair(kind, nb, 5)
        coded = (np.frombuffer(data, dtype=np.uint8) ^ np.frombuffer(base, dtype=np.uint8)).tobytes()
    else:
        data, base, coded = _gen2(kind, nb, 5), None, None
    body, src = _stage(lib, [O.compress_frame(b"", coded if delta else data, P, rot, bm, ch, threads=4), data], dev)
    bt = _stage(lib, [base], dev)[0] if delta else None
    K = -(-nb // ch)
    spec = (kind, nb, P, rot, bm, ch)
    try:
        for name, (wide, group) in FORMS.items():
            lib.set_decode_wide(wide); decode_group(lib, group)
            for lo, hi in _windows(K):
                got = _decode(lib, [body], [spec], [(lo, hi)], deltas=[bt] if delta else None)[0]
                assert torch.equal(got, src[lo * ch: min(hi * ch, nb)]), (name, lo, hi, lib.last_kernels())
    finally:
        lib.set_decode_wide(1)


def test_one_gib_tensor_in_windows(lib):
    """A 1 GiB + 100 KB bf16 tensor (4 097 chunks): windows of 1, 3, 1 024 and 4 095 chunks, the one that ends in the partial chunk included."""
    dev = torch.device("cuda:0")
    ch = 256 * KB
    g = torch.Generator(device=dev); g.manual_seed(3)
    src = (torch.randn((1 << 29) + 50 * KB, generator=g, device=dev) * 0.02).to(torch.bfloat16).view(torch.uint8)
    nb = src.numel()
    K = -(-nb // ch)
    assert K == 4097 and nb % ch
    body = _stage(lib, [O.compress_frame(b"", src.cpu().numpy(), 2, 1, 10, ch, threads=16)], dev)[0]
    spec = ("bf16", nb, 2, 1, 10, ch)
    for lo, hi in ((0, 1), (2048, 2049), (K - 1, K), (7, 10), (K - 3, K), (0, 1024), (3000, 4024), (K - 1024, K), (0, 4095), (2, K), (0, K)):
        got = _decode(lib, [body], [spec], [(lo, hi)])[0]
        assert torch.equal(got, src[lo * ch: min(hi * ch, nb)]), (lo, hi, lib.last_kernels())
        del got


def test_ragged_batch_half_windows_half_whole(lib):
    """300 ragged two-plane tensors (and one- / four-plane ones) in one call: every other item a window, the rest whole."""
    dev = torch.device("cuda:0")
    specs, datas = _ragged_batch(300, 71, chunk=8192, n1=60, n4=40, full_max=6)
    bodies = _stage(lib, _oracle_bodies(specs, datas), dev)
    srcs = _stage(lib, datas, dev)
    r = np.random.default_rng(3)
    wins = []
    for i, (_k, nb, _P, _r, _b, ch) in enumerate(specs):
        K = -(-nb // ch)
        lo = int(r.integers(0, K + 1)) if i % 2 else 0
        wins.append((lo, int(r.integers(lo, K + 1)) if i % 2 else K))
    for check in (True, False):
        outs = _decode(lib, bodies, specs, wins, check=check)
        if not check:
            lib.decode_status(_stream())
        _assert_same(outs, [s[lo * sp[5]: min(hi * sp[5], sp[1])] for s, sp, (lo, hi) in zip(srcs, specs, wins)], specs)
    assert lib.last_kernels().count("zn_k_decode_fused") == 3


def test_plans_on_two_streams(lib):
    """Two plans, each on a stream of its own, run alternately and against one-shot calls on the default stream; a plan survives zn_release_workspace."""
    dev = torch.device("cuda:0")
    cases = []
    for seed in (5, 6):
        specs, datas = _ragged_batch(40, seed, chunk=64 * KB, n1=10, n4=10, full_max=8)
        bodies = _stage(lib, _oracle_bodies(specs, datas, threads=8), dev)
        srcs = _stage(lib, datas, dev)
        wins = [(0, -(-nb // ch)) if i % 3 else (min(1, -(-nb // ch)), -(-nb // ch)) for i, (_k, nb, _P, _r, _b, ch) in enumerate(specs)]
        sizes = [_win_size(s[1], s[5], *w) for s, w in zip(specs, wins)]
        offs, o = [], 0
        for sz in sizes:
            offs.append(o); o += (sz + 255) // 256 * 256
        buf = torch.zeros(max(o, 1), dtype=torch.uint8, device=dev)
        plan = lib.plan_create([(b.data_ptr(), b.numel(), P, rot, bm, ch, nb, lo, hi, buf.data_ptr() + off if sz else 0)
                                for b, (_k, nb, P, rot, bm, ch), (lo, hi), off, sz in zip(bodies, specs, wins, offs, sizes)])
        want = [s[lo * sp[5]: min(hi * sp[5], sp[1])] for s, sp, (lo, hi) in zip(srcs, specs, wins)]
        cases.append((plan, buf, offs, sizes, want, specs, torch.cuda.Stream(dev), bodies, srcs))
    torch.cuda.synchronize()
    try:
        for rnd in range(4):
            for (plan, buf, offs, sizes, want, specs, st, bodies, srcs) in cases:
                with torch.cuda.stream(st):
                    buf.zero_()
                    lib.plan_run(plan, st.cuda_stream, False)
            one = _decode(lib, [cases[0][7][0]], [cases[0][5][0]], [(0, -(-cases[0][5][0][1] // cases[0][5][0][5]))])[0]      # a one-shot call between them
            assert torch.equal(one, cases[0][8][0])
            for (plan, buf, offs, sizes, want, specs, st, bodies, srcs) in cases:
                lib.decode_status(st.cuda_stream)
                _assert_same([buf[o:o + s] for o, s in zip(offs, sizes)], want, specs)
            if rnd == 1:
                torch.cuda.synchronize()
                lib.release_workspace()
    finally:
        torch.cuda.synchronize()
        for c in cases:
            lib.plan_destroy(c[0])


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8).cpu(), b.contiguous().reshape(-1).view(torch.uint8).cpu())


def test_store_on_the_reference_written_checkpoint(lib):
    from safetensors import safe_open
    from zipnn_amd import ResidentCheckpoint, decompress_safetensors_tensor, safetensors_io
    store = ResidentCheckpoint.from_file(GOLDEN, "cuda:0")
    want = safetensors_io.load_file(GOLDEN, device="cuda:0")
    assert sorted(store.keys()) == sorted(want.keys())
    assert store.resident_bytes < store.nbytes
    got = store.get_tensors(store.keys())
    assert "zn_k_decode" in lib.last_kernels()
    for k, v in want.items():
        assert got[k].is_cuda and _bytes_equal(got[k], v), k
        assert _bytes_equal(store.get_tensor(k), v), k
    names = [k for k in store.keys() if store.info(k)["compressed"]]
    plan = store.plan(names)
    side = torch.cuda.Stream()
    for st in (None, side):
        for t in plan.tensors.values():
            t.zero_()
        torch.cuda.synchronize()
        plan.run(stream=st)
        plan.status()
        for k in names:
            assert _bytes_equal(plan.tensors[k], want[k]), k
    plan.close()
    for k in names:
        i = store.info(k)
        if len(i["shape"]) == 2 and i["shape"][0] >= 64:
            s = store.get_slice(k)
            for idx in (0, -1, slice(3, 40), slice(5, 60, 7), (slice(10, 20), slice(1, 5))):
                assert _bytes_equal(s[idx], want[k][idx]), (k, idx)
    store.status()
    with safe_open(GOLDEN, "pt", "cpu") as f:                 # … and against the per-tensor path on the host frames
        k = names[0]
        assert _bytes_equal(decompress_safetensors_tensor(f.get_tensor(k)), want[k])


def test_slices_of_a_large_matrix_from_an_oracle_body(lib):
    from zipnn_amd.resident import ResidentCheckpoint, _Entry
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    full = (torch.randn(4099, 1031, generator=g) * 0.02).to(torch.bfloat16)
    data = full.view(torch.uint8).numpy().tobytes()
    body = _stage(lib, [O.compress_frame(b"", data, 2, 1, 10, 256 * KB, threads=8)], dev)[0]
    store = ResidentCheckpoint(dev, [_Entry("w", torch.bfloat16, full.shape, len(data), body=body, params=(2, 1, 10, 256 * KB))], body.numel())
    s = store.get_slice("w")
    K = -(-len(data) // (256 * KB))
    for idx in (0, 4098, slice(1000, 1300), slice(4000, None), slice(7, 4000, 129), (slice(2000, 2100), slice(3, 9)), Ellipsis):
        assert _bytes_equal(s[idx], full[idx]), idx
        assert 0 <= s.last_chunk_range[0] <= s.last_chunk_range[1] <= K
    assert _bytes_equal(s[1000:1300], full[1000:1300]) and s.last_chunk_range == (1000 * 2062 // (256 * KB), -(-1300 * 2062 // (256 * KB)))
    store.status()


class _MLP(torch.nn.Module):
    def __init__(self, d, h, layers):
        super().__init__()
        self.blocks = torch.nn.ModuleList(torch.nn.Sequential(torch.nn.Linear(d, h + 64 * i), torch.nn.GELU(), torch.nn.Linear(h + 64 * i, d)) for i in range(layers))
        self.norm = torch.nn.LayerNorm(d)

    def forward(self, x):
        for b in self.blocks:
            x = x + b(x)
        return self.norm(x)


def test_hook_on_a_bf16_mlp_stack(lib):
    from zipnn_amd import ResidentCheckpoint
    torch.manual_seed(4)
    model = _MLP(1024, 2048, 4).to(torch.bfloat16).to("cuda:0").eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(16, 1024, device="cuda:0", dtype=torch.bfloat16)
    with torch.no_grad():
        ref = model(x)
    store = ResidentCheckpoint.from_state_dict(sd, "cuda:0")
    assert store.info("blocks.0.0.weight")["compressed"] and store.resident_bytes < 0.8 * store.nbytes
    for k, v in sd.items():
        assert _bytes_equal(store.get_tensor(k), v), k
    handle = store.hook(model)
    params = [p for _, p in model.named_parameters()]
    assert all(p.numel() == 0 for p in params)
    with torch.no_grad():
        for _ in range(3):
            assert torch.equal(model(x), ref)
            assert all(p.numel() == 0 for p in params)
    handle.status()
    handle.remove()
    for n, p in model.named_parameters():
        assert _bytes_equal(p.data, sd[n]), n
    with torch.no_grad():
        assert torch.equal(model(x), ref)
