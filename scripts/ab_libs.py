#!/usr/bin/env python
"""Developer tool (GPU box): time the decode of prebuilt library variants against each other, interleaved
(A B A B ...) so that clock drift hits both.  Usage: python scripts/ab_libs.py [--small] [--rounds N] libA.so libB.so ...
(--small: the 64 MiB and the ragged 100 MiB + 250 000 B bf16 tensors of bench.py's size sweep instead of the large cases; --rounds: interleaved rounds, best of all)
--delta: the 1 GiB bf16 delta decode of DESIGN §3.4 instead (a base that differs from the tensor in 2 % of the elements; zn_decompress_delta_dev into a separate destination).
(the variants are built here, in the container, e.g. from `git archive <commit> zipnn_amd/csrc`)."""
import ctypes, os, sys, time
import torch


def load(path):
    L = ctypes.CDLL(path)
    sz, vp, ci = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    L.zn_compress_bound.restype = sz; L.zn_compress_bound.argtypes = [sz, ci, sz, sz]
    L.zn_compress_dev.argtypes = [vp, sz, ci, ci, ci, sz, ctypes.c_float, vp, sz, ctypes.POINTER(sz), vp]
    L.zn_decompress_dev.argtypes = [vp, sz, ci, ci, ci, sz, sz, vp, vp, ci]
    L.zn_compress_delta_dev.argtypes = [vp, vp, sz, ci, ci, ci, sz, ctypes.c_float, vp, sz, ctypes.POINTER(sz), vp]
    L.zn_decompress_delta_dev.argtypes = [vp, sz, vp, ci, ci, ci, sz, sz, vp, vp, ci]
    return L


def main_delta(libs, rounds):
    n, C, P, rot, bm = 1 << 30, 262144, 2, 1, 10
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    x = (torch.randn(n // 2, generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    base = x.clone()
    hit = torch.rand(n // 2, generator=g, device="cuda") < 0.02
    base[hit] = (torch.randn(int(hit.sum()), generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    flat, bflat = x.view(torch.uint8).reshape(-1), base.view(torch.uint8).reshape(-1)
    st = torch.cuda.current_stream().cuda_stream
    L0 = libs[0][1]
    cap = L0.zn_compress_bound(n, P, C, 0)
    body = torch.empty(cap, dtype=torch.uint8, device="cuda"); ln = ctypes.c_size_t(0)
    assert L0.zn_compress_delta_dev(flat.data_ptr(), bflat.data_ptr(), n, P, rot, bm, C, 0.95, body.data_ptr(), cap, ctypes.byref(ln), None) == 0
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    best = {k: 1e9 for k, _ in libs}
    for k, L in libs:
        assert L.zn_decompress_delta_dev(body.data_ptr(), ln.value, bflat.data_ptr(), P, rot, bm, C, n, out.data_ptr(), st, 1) == 0
        print("   roundtrip", k, torch.equal(out, flat))
    for rnd in range(rounds):
        for k, L in libs:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(10):
                L.zn_decompress_delta_dev(body.data_ptr(), ln.value, bflat.data_ptr(), P, rot, bm, C, n, out.data_ptr(), st, 0)
            torch.cuda.synchronize(); best[k] = min(best[k], (time.perf_counter() - t0) / 10)
    for k, _ in libs:
        print(f"bf16 1GiB delta (ratio {ln.value / n:.3f}) {k:34s} decode {best[k] * 1e3:.4f} ms {n / best[k] / 1e9:6.0f} GB/s", flush=True)


def main():
    argv = sys.argv[1:]
    small = "--small" in argv
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 4
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--rounds")]
    libs = [(os.path.basename(p), load(p)) for p in paths]
    if "--delta" in argv:
        return main_delta(libs, rounds)
    C0 = 262144
    cases = [("bf16 4GiB", 4 << 30, 2, 1, 10, torch.bfloat16), ("fp32 1GiB", 1 << 30, 4, 1, 220, torch.float32), ("fp16 1GiB", 1 << 30, 2, 0, 10, torch.float16), ("fp8 1GiB", 1 << 30, 1, 0, 10, torch.float8_e4m3fn)]
    if small:
        cases = [("bf16 64MiB", 64 << 20, 2, 1, 10, torch.bfloat16), ("bf16 100MiB+250000", (100 << 20) + 250000, 2, 1, 10, torch.bfloat16)]
    st = torch.cuda.current_stream().cuda_stream
    for name, n, P, rot, bm, dt in cases:
        C = C0 if P > 1 else 131072
        es = torch.empty(0, dtype=dt).element_size()
        x = torch.empty(n // es, dtype=dt, device="cuda")
        g = torch.Generator(device="cuda"); g.manual_seed(5)
        step = 1 << 27
        for off in range(0, x.numel(), step):
            x[off:off + step] = (torch.randn(min(step, x.numel() - off), generator=g, device="cuda") * 0.02).to(dt)
        flat = x.view(torch.uint8).reshape(-1)
        L0 = libs[0][1]
        cap = L0.zn_compress_bound(n, P, C, 0)
        body = torch.empty(cap, dtype=torch.uint8, device="cuda"); ln = ctypes.c_size_t(0)
        assert L0.zn_compress_dev(flat.data_ptr(), n, P, rot, bm, C, 0.95, body.data_ptr(), cap, ctypes.byref(ln), None) == 0
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        best = {k: 1e9 for k, _ in libs}; bestc = {k: 1e9 for k, _ in libs}
        for k, L in libs:
            assert L.zn_decompress_dev(body.data_ptr(), ln.value, P, rot, bm, C, n, out.data_ptr(), st, 1) == 0
            ok_ = torch.equal(out, flat); print("   roundtrip", k, ok_)
        body2 = torch.empty(cap, dtype=torch.uint8, device="cuda"); ln2 = ctypes.c_size_t(0)
        reps = 10 if n >= (1 << 30) else 200
        for rnd in range(rounds):
            for k, L in libs:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(reps):
                    L.zn_decompress_dev(body.data_ptr(), ln.value, P, rot, bm, C, n, out.data_ptr(), st, 0)
                torch.cuda.synchronize(); best[k] = min(best[k], (time.perf_counter() - t0) / reps)
                t0 = time.perf_counter()
                for _ in range(4):
                    L.zn_compress_dev(flat.data_ptr(), n, P, rot, bm, C, 0.95, body2.data_ptr(), cap, ctypes.byref(ln2), st)
                torch.cuda.synchronize(); bestc[k] = min(bestc[k], (time.perf_counter() - t0) / 4)
        for k, _ in libs:
            print(f"{name:10s} {k:34s} decode {best[k] * 1e3:.4f} ms {n / best[k] / 1e9:6.0f} GB/s   compress {bestc[k] * 1e3:.3f} ms {n / bestc[k] / 1e9:6.0f} GB/s", flush=True)
        del x, flat, body, out, body2


if __name__ == "__main__":
    main()
