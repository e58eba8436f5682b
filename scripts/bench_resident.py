#!/usr/bin/env python
"""Probe (GPU box): what a checkpoint that stays compressed in HBM costs and saves (zipnn_amd.ResidentCheckpoint).

Llama-3-8B block shapes (bench.llama8b_shapes, as bench.py's `llama8b` workload), seeded N(0, 0.02) bf16 tensors, compressed by this library.
Everything timed is checked against the source bytes.  Legs:
  a  resident bytes against original bytes
  b  per-block plan.run time, by device events
  c  a window of k chunks of a large tensor against a whole tensor of k chunks, k = 64, 1 024, 4 096
  d  host time to ENQUEUE a block while an earlier decode is still running: plan.run against zn_decompress_batch_dev
  e  a full forward of a stack of torch.nn.Linear blocks with hook(), against the same stack with plain parameters
Each leg runs in a child process under a time limit of its own; a leg that fails or runs out of time ends the probe.
    python scripts/bench_resident.py [--layers 4] [--out profiles/resident_decode]
--index: the sync index instead (ResidentCheckpoint.build_index), into profiles/resident_index.{json,txt}:
  i  per dtype (bf16, fp32, fp16, fp8 e4m3; about 1 GiB each, N(0, 0.02)): plan.run unhinted / hinted / unhinted / hinted on the same store, the build time
     per GiB and index_bytes / nbytes
  j  the four Llama-3-8B blocks of leg b, per block unhinted / hinted / unhinted / hinted, and leg e's hooked forward with and without the index
--delta: variant stores instead (ResidentCheckpoint.from_state_dict(..., base=...)), into profiles/resident_delta.{json,txt}: the blocks of leg b as
the base and two fine-tunes of them — (a) the base with 2 % of the elements replaced (the input of DESIGN §3.4), (b) every element moved by a small relative
step, so that low mantissa bits change everywhere:
  k  per fine-tune: variant resident bytes against a plain store of the same tensors; plan.run of one block from the plain store, from a variant over plain
     base tensors and from a variant over a resident base, interleaved (A B C A B C: the plain store's two runs are the A/A spread); apply_ + revert_ of
     one block; store build times
--digest: content digests instead ("zn64-1"), into profiles/resident_digest.{json,txt}:
  m  one 1 GiB device tensor digested where it lies, 16-byte aligned and at a +1 byte offset, interleaved with plan.run decoding a 1 GiB bf16 N(0, 0.02)
     tensor in the same process (decode digest decode digest: the decode's two runs are the A/A spread, and the decode is the yardstick — a verify that costs
     more than the decode it follows is not worth having); a ragged batch of 291 tensors (the Llama-3-8B tensor list at a quarter of its widths, packed back
     to back at whatever byte address they fall on) in one launch; store.verify() on the four-block store of leg b
--delta-file: delta checkpoint files instead (ResidentCheckpoint.save_file / from_file(base=)), into profiles/resident_delta_file.{json,txt}: the
blocks of leg b as the base, the two fine-tunes of --delta:
  n  per fine-tune: bytes of the delta file against the plain `.znn.safetensors` of the same tensors and the raw tensors; wall time of from_file(delta,
     base=store) against from_state_dict(ft_sd, base=store) with ft_sd already on the device; from_file with verify_base over a base store with recorded
     digests, over one without, and with verify_base=False; plan.run of one block from the built variant and from the loaded one, interleaved (A B A B: the
     built variant's two runs are the A/A spread — the two run the same kernels on byte-equal bodies)
--delta-index: the sync index of variant stores instead (build_index(deltas=True), DESIGN §3.6 "Two kinds"), into profiles/resident_delta_index.{json,txt}:
  p  per fine-tune of --delta: plan.run of one block from a variant over a resident indexed base, without and with the variant's DELTA index, interleaved in
     both orders (A B A B B A B A: the four runs without are the A/A spread), the build time of the DELTA index and its size
--sparse-file: sparse variants written down and read back (save_file(sparse=True), from_file(check_patches=)), into profiles/resident_sparse_file.{json,txt}:
  f  file bytes against the delta and the plain file; from_file with and without the patch check; the check call against a device copy; plan.run loaded against built
--sparse: sparse variant stores instead (from_state_dict(..., base=..., sparse=True)), into profiles/resident_sparse.{json,txt}:
  s  per fine-tune of --delta, over a resident indexed base: resident bytes and build time without and with sparse=True; plan.run of one block from either
     store, interleaved in both orders (A B A B B A B A: the four runs of the delta store are the A/A spread); apply_ + revert_ of one block from either
--rebase: patch merges and ResidentCheckpoint.rebased instead, into profiles/resident_rebase.{json,txt}:
  r  a chain of four 2 % steps and two sibling fine-tunes over a resident indexed base, every comparison interleaved in both orders (A B A B B A B A: the four A
     runs are the A/A spread): rebased against get_tensors + from_state_dict; the merge call against the build call on the same pairs; plan.run of one block
     from the chain against the flattened store; sw.apply_ against a.revert_ + b.apply_; resident bytes of b over the base against b over a
--shard: patch selects and ResidentCheckpoint.sharded instead, into profiles/resident_shard.{json,txt}:
  h  one rank of a split of 8 of a 2 % fine-tune over a resident indexed base (q/k/v/gate/up along dim 0, o/down along dim 1), every comparison interleaved in
     both orders (A B A B B A B A: the four A runs are the A/A spread): sharded against get_tensors + narrow + from_state_dict; the select call against the build
     call on the same shard pairs, dim 0 and dim 1 apart; plan.run of one block from the sharded store against a store built from the shard tensors
--strided: apply_ / revert_ on non-contiguous live tensors instead (zn_patch_apply_strided_batch_dev), into profiles/resident_strided.{json,txt}:
  t  apply_ + revert_ of one block of a 2 % fine-tune kept sparse over a resident indexed base, on contiguous targets, transposed storage, dim-1 narrows of a
     twice-as-wide buffer and a 16-row tile shuffle; each strided layout against contiguous() + the contiguous apply + copy_ back, interleaved with the
     contiguous run in both orders (C S W C S W W S C W S C: the contiguous runs are the A/A spread)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_SECONDS = {"a": 240, "b": 240, "c": 300, "d": 240, "e": 300}
INDEX_LEG_SECONDS = {"i": 420, "j": 300}
DELTA_LEG_SECONDS = {"k": 420}
DIGEST_LEG_SECONDS = {"m": 420}
DELTA_FILE_LEG_SECONDS = {"n": 420}
CH = 256 * 1024


def _blocks(layers, seed=7):
    """-> (state dict of `layers` Llama-3-8B blocks on the device, [names of block i])"""
    import torch
    import bench
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    sd, per = {}, [[] for _ in range(layers)]
    for name, shape, _linear in bench.llama8b_shapes(layers=layers):
        if not name.startswith("model.layers."):
            continue
        sd[name] = (torch.randn(shape, generator=g, device="cuda") * 0.02).to(torch.bfloat16)
        per[int(name.split(".")[2])].append(name)
    return sd, per


def _same(a, b):
    import torch
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _events_ms(fn, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "reps": reps}


def leg_a(args):
    from zipnn_amd import ResidentCheckpoint
    sd, per = _blocks(args.layers)
    store = ResidentCheckpoint.from_state_dict(sd, "cuda:0")
    for k, v in sd.items():
        assert _same(store.get_tensor(k), v), k
    return {"layers": args.layers, "tensors": len(sd), "original_bytes": store.nbytes, "resident_bytes": store.resident_bytes,
            "ratio": store.resident_bytes / store.nbytes}


def leg_b(args):
    import torch
    from zipnn_amd import ResidentCheckpoint
    sd, per = _blocks(args.layers)
    store = ResidentCheckpoint.from_state_dict(sd, "cuda:0")
    scratch = torch.empty(max(store.scratch_bytes(n) for n in per), dtype=torch.uint8, device="cuda")
    res = []
    for i, names in enumerate(per):
        plan = store.plan(names, into=scratch)
        t = _events_ms(plan.run, args.reps)
        plan.status()
        for k in names:
            assert _same(plan.tensors[k], sd[k]), k
        nbytes = sum(store.info(k)["nbytes"] for k in names)
        t.update(block=i, bytes=nbytes, gb_per_s=nbytes / t["median_ms"] / 1e6)
        res.append(t)
        plan.close()
    return {"blocks": res}


def leg_c(args):
    import torch
    from zipnn_amd import _capi, codec
    lib = _capi.lib()
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    K_BIG = 8192
    big = (torch.randn(K_BIG * CH // 2, generator=g, device="cuda") * 0.02).to(torch.bfloat16).view(torch.uint8)
    body_big = codec.compress_device(lib, big, 2, 1, 10, CH, 0.95).clone()
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for k in (64, 1024, 4096):
        lo = (K_BIG - k) // 2
        whole_src = big[lo * CH:(lo + k) * CH]
        body_k = codec.compress_device(lib, whole_src, 2, 1, 10, CH, 0.95).clone()
        out = torch.empty(k * CH, dtype=torch.uint8, device="cuda")
        win = [(body_big.data_ptr(), body_big.numel(), 2, 1, 10, CH, big.numel(), lo, lo + k, out.data_ptr())]
        whole = [(body_k.data_ptr(), body_k.numel(), 2, 1, 10, CH, k * CH, 0, k, out.data_ptr())]
        r = {"chunks": k}
        for name, items in (("window", win), ("whole", whole), ("window_again", win), ("whole_again", whole)):      # interleaved: A B A B
            out.zero_()
            t = _events_ms(lambda: lib.decompress_window_batch_dev(items, st, False), args.reps)
            lib.decode_status(st)
            assert torch.equal(out, whole_src), (k, name)
            r[name] = t
            r[name + "_kernels"] = lib.last_kernels()
        res.append(r)
    return {"windows": res}


def leg_d(args):
    import torch
    from zipnn_amd import ResidentCheckpoint, _capi
    lib = _capi.lib()
    sd, per = _blocks(max(args.layers, 2))
    store = ResidentCheckpoint.from_state_dict(sd, "cuda:0")
    scratch = [torch.empty(max(store.scratch_bytes(n) for n in per), dtype=torch.uint8, device="cuda") for _ in range(2)]
    plans = [store.plan(per[i], into=scratch[i]) for i in range(2)]
    items = [[store._entries[k].window(0, store._entries[k].chunks, plans[i].tensors[k].data_ptr()) for k in per[i]] for i in range(2)]
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, first, second in (("plan_run", lambda: plans[0].run(), lambda: plans[1].run()),
                                ("batch_call", lambda: lib.decompress_window_batch_dev(items[0], st, False), lambda: lib.decompress_window_batch_dev(items[1], st, False))):
        ts = []
        for _ in range(args.reps + 3):
            torch.cuda.synchronize()
            for _ in range(4):
                first()                                   # earlier decodes, still running when the next one is enqueued
            t0 = time.perf_counter(); second(); t1 = time.perf_counter()
            ts.append((t1 - t0) * 1e6)
        torch.cuda.synchronize()
        lib.decode_status(st)
        for i in range(2):
            for k in per[i]:
                assert _same(plans[i].tensors[k], sd[k]), k
        out[name] = {"median_us": statistics.median(ts[3:]), "min_us": min(ts[3:]), "reps": args.reps}
    for p in plans:
        p.close()
    return {"enqueue_while_busy": out, "tensors_per_block": len(per[0])}


def leg_e(args):
    import torch
    from zipnn_amd import ResidentCheckpoint
    torch.manual_seed(5)
    hidden, inter = 4096, 14336

    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.up, self.down = torch.nn.Linear(hidden, inter, bias=False), torch.nn.Linear(inter, hidden, bias=False)

        def forward(self, x):
            return x + self.down(torch.nn.functional.silu(self.up(x)))
    model = torch.nn.Sequential(*[Block() for _ in range(args.layers)]).to(torch.bfloat16).to("cuda").eval()
    for p in model.parameters():
        p.data.mul_(0.3)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    res = {"layers": args.layers, "batches": []}
    store = ResidentCheckpoint.from_state_dict(sd, "cuda:0")
    res["original_bytes"], res["resident_bytes"] = store.nbytes, store.resident_bytes
    for batch in (1, 16, 256):
        x = torch.randn(batch, hidden, device="cuda", dtype=torch.bfloat16)
        with torch.no_grad():
            ref = model(x)
            plain = _events_ms(lambda: model(x), args.reps)
            handle = store.hook(model)
            assert torch.equal(model(x), ref)
            hooked = _events_ms(lambda: model(x), args.reps)
            handle.status()
            handle.remove()
            assert torch.equal(model(x), ref)
        res["batches"].append({"batch": batch, "plain": plain, "hooked": hooked, "scratch_bytes": int(handle.scratch.numel())})
    return res


def _abab(store, names, scratch, reps, sd=None):
    """plan.run of `names`: unhinted, hinted, unhinted, hinted on the SAME store (the index is built once and taken away / given back) ->
    {"plain": [ms, ms], "hinted": [ms, ms], "kernels": …}; the A/A spread is the two plain runs'."""
    hints = {k: store._entries[k].hints for k in names}
    out = {"plain": [], "hinted": [], "kernels": {}}
    for leg in ("plain", "hinted", "plain", "hinted"):
        for k in names:
            store._entries[k].hints = hints[k] if leg == "hinted" else None
        plan = store.plan(names, into=scratch)
        t = _events_ms(plan.run, reps)
        plan.status()
        out[leg].append(t["median_ms"])
        out["kernels"][leg] = _capi_kernels()
        if sd is not None:
            for k in names:
                assert _same(plan.tensors[k], sd[k]), (leg, k)
        plan.close()
    for k in names:
        store._entries[k].hints = hints[k]
    a, h = out["plain"], out["hinted"]
    out["aa_spread"] = abs(a[0] - a[1]) / min(a)
    out["gain"] = 1.0 - (sum(h) / 2) / (sum(a) / 2)
    return out


def _capi_kernels():
    from zipnn_amd import _capi
    return _capi.lib().last_kernels()


def leg_i(args):
    import torch
    from zipnn_amd import ResidentCheckpoint
    res = []
    for name in ("bfloat16", "float32", "float16", "float8_e4m3fn"):
        tdt = getattr(torch, name)
        es = torch.empty(0, dtype=tdt).element_size()
        g = torch.Generator(device="cuda"); g.manual_seed(13)
        sd = {f"t{i}": (torch.randn((128 << 20) // es, generator=g, device="cuda") * 0.02).to(tdt) for i in range(8)}      # 8 x 128 MiB
        store = ResidentCheckpoint.from_state_dict(sd, "cuda:0")
        names = [k for k in sd if store.info(k)["compressed"]]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store.build_index(all_dtypes=True)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        nbytes = sum(store.info(k)["nbytes"] for k in names)
        scratch = torch.empty(store.scratch_bytes(names), dtype=torch.uint8, device="cuda")
        r = _abab(store, names, scratch, args.reps, sd)
        r.update(dtype=name, tensors=len(names), nbytes=nbytes, resident_bytes=store.resident_bytes, index_bytes=store.index_bytes,
                 index_share=store.index_bytes / nbytes, build_s_per_gib=build_s / (nbytes / 2 ** 30))
        res.append(r)
        del store, sd, scratch
        torch.cuda.empty_cache()
    return {"dtypes": res}


def leg_j(args):
    import torch
    from zipnn_amd import ResidentCheckpoint
    sd, per = _blocks(args.layers)
    store = ResidentCheckpoint.from_state_dict(sd, "cuda:0", index=True)
    scratch = torch.empty(max(store.scratch_bytes(n) for n in per), dtype=torch.uint8, device="cuda")
    blocks = []
    for i, names in enumerate(per):
        r = _abab(store, names, scratch, args.reps, sd)
        r.update(block=i, bytes=sum(store.info(k)["nbytes"] for k in names))
        blocks.append(r)
    out = {"blocks": blocks, "index_bytes": store.index_bytes, "nbytes": store.nbytes}
    del store, sd, scratch
    # leg e's forward, hooked without and with the index
    torch.manual_seed(5)
    hidden, inter = 4096, 14336

    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.up, self.down = torch.nn.Linear(hidden, inter, bias=False), torch.nn.Linear(inter, hidden, bias=False)

        def forward(self, x):
            return x + self.down(torch.nn.functional.silu(self.up(x)))
    model = torch.nn.Sequential(*[Block() for _ in range(args.layers)]).to(torch.bfloat16).to("cuda").eval()
    for p in model.parameters():
        p.data.mul_(0.3)
    msd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(1, hidden, device="cuda", dtype=torch.bfloat16)
    fw = {}
    with torch.no_grad():
        ref = model(x)
        fw["plain_ms"] = _events_ms(lambda: model(x), args.reps)["median_ms"]
        for leg in ("hooked", "hooked_index", "hooked_again", "hooked_index_again"):
            st = ResidentCheckpoint.from_state_dict(msd, "cuda:0", index=leg.startswith("hooked_index"))
            handle = st.hook(model)
            assert torch.equal(model(x), ref)
            fw[leg + "_ms"] = _events_ms(lambda: model(x), args.reps)["median_ms"]
            fw[leg + "_kernels"] = _capi_kernels()
            handle.status()
            handle.remove()
    out["forward_batch1"] = fw
    return out


def _fine_tune(sd, kind, seed):
    """(a) "sparse": 2 % of the elements replaced by fresh N(0, 0.02) values; (b) "drift": every element times 1 + 2^-7 N(0, 1), rounded back to bf16."""
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if kind == "sparse":
            t = v.clone()
            hit = torch.rand(v.shape, generator=g, device="cuda") < 0.02
            t[hit] = (torch.randn(int(hit.sum()), generator=g, device="cuda") * 0.02).to(v.dtype)
        else:
            t = (v.float() * (1.0 + torch.randn(v.shape, generator=g, device="cuda") / 128.0)).to(v.dtype)
        out[k] = t
    return out


def leg_k(args):
    import torch
    from zipnn_amd import ResidentCheckpoint
    sd, per = _blocks(args.layers)
    names = per[0]
    res = {"layers": args.layers, "block_bytes": sum(sd[k].numel() * 2 for k in names), "fine_tunes": []}

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    base_store, t_base = timed(lambda: ResidentCheckpoint.from_state_dict(sd, "cuda:0", index=True))
    res["base"] = {"nbytes": base_store.nbytes, "resident_bytes": base_store.resident_bytes, "index_bytes": base_store.index_bytes, "build_s": t_base}
    for kind in ("sparse", "drift"):
        ft = _fine_tune(sd, kind, 21)
        plain, t_plain = timed(lambda: ResidentCheckpoint.from_state_dict(ft, "cuda:0"))
        over_dict, t_dict = timed(lambda: ResidentCheckpoint.from_state_dict(ft, "cuda:0", base=sd))
        over_store, t_store = timed(lambda: ResidentCheckpoint.from_state_dict(ft, "cuda:0", base=base_store))
        r = {"kind": kind, "nbytes": plain.nbytes, "plain_resident_bytes": plain.resident_bytes, "variant_resident_bytes": over_dict.resident_bytes,
             "variant_over_store_resident_bytes": over_store.resident_bytes, "delta_entries": sum(1 for k in ft if over_dict.info(k)["delta"] is True),
             "tensors": len(ft), "build_s": {"plain": t_plain, "over_tensors": t_dict, "over_store": t_store}}
        scratch = torch.empty(plain.scratch_bytes(names), dtype=torch.uint8, device="cuda")
        runs = {"plain": [], "over_tensors": [], "over_store": []}
        kernels = {}
        for _ in range(2):                                    # A B C A B C
            for leg, st in (("plain", plain), ("over_tensors", over_dict), ("over_store", over_store)):
                plan = st.plan(names, into=scratch)
                t = _events_ms(plan.run, args.reps)
                plan.status()
                for k in names:
                    assert _same(plan.tensors[k], ft[k]), (kind, leg, k)
                runs[leg].append(t["median_ms"])
                kernels[leg] = _capi_kernels()
                plan.close()
        r["plan_run_ms"] = runs
        r["kernels"] = kernels
        r["aa_spread"] = abs(runs["plain"][0] - runs["plain"][1]) / min(runs["plain"])
        # apply_ + revert_ of one block on tensors that hold the base (each leaves the tensors as it found them after the pair)
        live = {k: sd[k].clone() for k in names}
        t_ar = _events_ms(lambda: (over_store.apply_(live, check=False), over_store.revert_(live, check=False)), args.reps)
        over_store.status()
        for k in names:
            assert _same(live[k], sd[k]), (kind, "revert", k)
        over_store.apply_(live)
        for k in names:
            assert _same(live[k], ft[k]), (kind, "apply", k)
        r["apply_revert_ms"] = t_ar["median_ms"]
        r["apply_kernels"] = _capi_kernels()
        res["fine_tunes"].append(r)
        del plain, over_dict, over_store, ft, live, scratch
        torch.cuda.empty_cache()
    return res


def leg_n(args):
    import tempfile
    import torch
    from zipnn_amd import ResidentCheckpoint
    sd, per = _blocks(args.layers)
    names = per[0]
    res = {"layers": args.layers, "block_bytes": sum(sd[k].numel() * 2 for k in names), "fine_tunes": []}

    def timed(fn, reps=1):
        ts, r = [], None
        for _ in range(reps):
            r = None
            torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return r, statistics.median(ts)
    base = ResidentCheckpoint.from_state_dict(sd, "cuda:0", index=True, digests=True)
    bare = ResidentCheckpoint.from_state_dict(sd, "cuda:0", index=True)              # the same base without recorded digests
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ("sparse", "drift"):
            ft = _fine_tune(sd, kind, 21)
            built, t_build = timed(lambda: ResidentCheckpoint.from_state_dict(ft, "cuda:0", base=base), 3)
            d_path, t_save = timed(lambda: built.save_file(os.path.join(tmp, kind + ".delta.znn.safetensors")))
            p_path = ResidentCheckpoint.from_state_dict(ft, "cuda:0").save_file(os.path.join(tmp, kind + ".plain.znn.safetensors"))
            loaded, t_load = timed(lambda: ResidentCheckpoint.from_file(d_path, "cuda:0", base=base), 5)
            _, t_load_bare = timed(lambda: ResidentCheckpoint.from_file(d_path, "cuda:0", base=bare), 5)
            _, t_load_nocheck = timed(lambda: ResidentCheckpoint.from_file(d_path, "cuda:0", base=base, verify_base=False), 5)
            for k in ft:
                assert built.info(k)["delta"] == loaded.info(k)["delta"], (kind, k)
                if built.info(k)["compressed"]:
                    assert torch.equal(built._entries[k].body, loaded._entries[k].body), (kind, k)
            r = {"kind": kind, "raw_bytes": built.nbytes, "delta_file_bytes": os.path.getsize(d_path), "plain_file_bytes": os.path.getsize(p_path),
                 "delta_entries": sum(1 for k in ft if built.info(k)["delta"] is True), "tensors": len(ft),
                 "built_resident_bytes": built.resident_bytes, "loaded_resident_bytes": loaded.resident_bytes,
                 "wall_s": {"from_state_dict": t_build, "save_file": t_save, "from_file": t_load, "from_file_base_without_digests": t_load_bare,
                            "from_file_verify_base_off": t_load_nocheck}}
            scratch = torch.empty(built.scratch_bytes(names), dtype=torch.uint8, device="cuda")
            runs, kernels = {"built": [], "loaded": []}, {}
            for _ in range(2):                                    # A B A B
                for leg, st in (("built", built), ("loaded", loaded)):
                    plan = st.plan(names, into=scratch)
                    t = _events_ms(plan.run, args.reps)
                    plan.status()
                    for k in names:
                        assert _same(plan.tensors[k], ft[k]), (kind, leg, k)
                    runs[leg].append(t["median_ms"])
                    kernels[leg] = _capi_kernels()
                    plan.close()
            r["plan_run_ms"], r["kernels"] = runs, kernels
            r["aa_spread"] = abs(runs["built"][0] - runs["built"][1]) / min(runs["built"])
            r["loaded_vs_built"] = (sum(runs["loaded"]) / 2) / (sum(runs["built"]) / 2) - 1.0
            res["fine_tunes"].append(r)
            del built, loaded, ft, scratch
            torch.cuda.empty_cache()
    return res


def leg_m(args):
    import torch
    import bench
    from zipnn_amd import ResidentCheckpoint, _capi, codec
    lib = _capi.lib()
    st = torch.cuda.current_stream().cuda_stream
    n = 1 << 30
    g = torch.Generator(device="cuda"); g.manual_seed(17)
    x = (torch.randn(n // 2, generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    store = ResidentCheckpoint.from_state_dict({"x": x}, "cuda:0", digests=True)
    plan = store.plan(["x"])
    buf = torch.empty(n + 256, dtype=torch.uint8, device="cuda")
    a = (-buf.data_ptr()) % 256
    aligned, shifted = buf[a:a + n], buf[a + 1:a + 1 + n]
    aligned.copy_(x.view(torch.uint8))
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    want = store.digests()["x"]
    res = {"bytes": n, "decode_ms": [], "digest_aligned_ms": []}
    for _ in range(2):                                    # A B A B
        res["decode_ms"].append(_events_ms(plan.run, args.reps)["median_ms"])
        plan.status()
        assert _same(plan.tensors["x"], x)
        res["decode_kernels"] = _capi_kernels()
        res["digest_aligned_ms"].append(_events_ms(lambda: codec.digest_device_batch(lib, [aligned], st, out=out), args.reps)["median_ms"])
        assert codec.digests_to_ints(out) == [want]
    shifted.copy_(x.view(torch.uint8))
    assert shifted.data_ptr() % 16 == 1
    res["digest_plus1_ms"] = _events_ms(lambda: codec.digest_device_batch(lib, [shifted], st, out=out), args.reps)["median_ms"]
    assert codec.digests_to_ints(out) == [want]
    res["digest_kernels"] = _capi_kernels()
    torch.cuda.synchronize(); t0 = time.perf_counter(); host = lib.digest_host(x[:1 << 26].view(torch.uint8).cpu().numpy()); res["host_ms_per_128MiB"] = (time.perf_counter() - t0) * 1e3
    assert host == codec.digests_to_ints(codec.digest_device_batch(lib, [shifted[:1 << 27]]))[0]      # (the buffer now holds the tensor from +1 on)
    d, h = res["decode_ms"], res["digest_aligned_ms"]
    res["aa_spread"] = abs(d[0] - d[1]) / min(d)
    res["verdict_ok"] = (sum(h) / 2) <= (sum(d) / 2) * (1.0 + res["aa_spread"])
    plan.close()
    del store, plan, x, buf, aligned, shifted
    torch.cuda.empty_cache()
    # a ragged batch: the 291 tensors of the Llama-3-8B list at a quarter of its widths, bf16, back to back from byte 3 of one buffer
    sizes = []
    for _, shape, _l in bench.llama8b_shapes(hidden=1024, inter=3584, vocab=32064):
        k = 2
        for dd in shape:
            k *= dd
        sizes.append(k + (len(sizes) % 3))                # (… and not all of them even)
    total = sum(sizes) + 64
    rag = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda", generator=g)
    flats, o = [], 3
    for k in sizes:
        flats.append(rag[o:o + k]); o += k
    outs = torch.zeros(len(flats), dtype=torch.int64, device="cuda")
    tb = _events_ms(lambda: codec.digest_device_batch(lib, flats, st, out=outs), args.reps)
    got = codec.digests_to_ints(outs)
    for i in (0, 1, 5, 8, 290):
        assert got[i] == lib.digest_host(flats[i].cpu().numpy()), i
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); codec.digest_device_batch(lib, flats, st, out=outs); ts.append((time.perf_counter() - t0) * 1e6)
    res["ragged"] = {"tensors": len(flats), "bytes": sum(sizes), "median_ms": tb["median_ms"], "gb_per_s": sum(sizes) / tb["median_ms"] / 1e6, "enqueue_us": statistics.median(ts)}
    del rag, flats
    torch.cuda.empty_cache()
    # store.verify() on the four-block store: against the plan.run of its blocks
    sd, per = _blocks(args.layers)
    bstore = ResidentCheckpoint.from_state_dict(sd, "cuda:0", digests=True)
    assert all(bstore.verify().values())
    ts = []
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter(); bstore.verify(); ts.append((time.perf_counter() - t0) * 1e3)
    scratch = torch.empty(max(bstore.scratch_bytes(nm) for nm in per), dtype=torch.uint8, device="cuda")
    dec = 0.0
    for names in per:
        p = bstore.plan(names, into=scratch)
        dec += _events_ms(p.run, args.reps)["median_ms"]
        p.close()
    res["verify"] = {"layers": args.layers, "tensors": len(sd), "bytes": bstore.nbytes, "verify_wall_ms": statistics.median(ts), "plan_run_all_blocks_ms": dec}
    return res


def main_digest(args):
    results = {}
    for leg, limit in DIGEST_LEG_SECONDS.items():
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--layers", str(args.layers), "--reps", str(args.reps)],
                           capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"leg {leg} failed (exit {p.returncode}); nothing further is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            return 1
        results[leg] = json.loads(line[0][7:])
        print(f"leg {leg}: ok", flush=True)
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "resident_digest")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(results, open(out + ".json", "w"), indent=1)
    m = results["m"]
    d, h = m["decode_ms"], m["digest_aligned_ms"]
    gbs = lambda ms: m["bytes"] / ms / 1e6      # noqa: E731
    lines = ["content digest probe (zn64-1, zn_k_digest): device events, median ms; every digest checked against the store's / the host function's",
             f"1 GiB bf16 N(0, 0.02), interleaved: plan.run decode {d[0]:.4f} / {d[1]:.4f} ms (A/A spread {100 * m['aa_spread']:.1f} %)   [{m['decode_kernels']}]",
             f"    digest, 16-byte aligned {h[0]:.4f} / {h[1]:.4f} ms ({gbs(sum(h) / 2):.0f} GB/s); at +1 byte {m['digest_plus1_ms']:.4f} ms ({gbs(m['digest_plus1_ms']):.0f} GB/s)   [{m['digest_kernels']}]",
             f"    verdict (aligned digest no slower than the decode, within the decode's A/A spread): {'MET' if m['verdict_ok'] else 'MISSED'}",
             f"    zn_digest_host, 128 MiB: {m['host_ms_per_128MiB']:.1f} ms",
             f"ragged batch, {m['ragged']['tensors']} tensors, {m['ragged']['bytes']} B, one launch: {m['ragged']['median_ms']:.4f} ms ({m['ragged']['gb_per_s']:.0f} GB/s), host time to enqueue {m['ragged']['enqueue_us']:.0f} us",
             f"store.verify() of {m['verify']['layers']} Llama-3-8B blocks ({m['verify']['tensors']} tensors, {m['verify']['bytes']} B): {m['verify']['verify_wall_ms']:.3f} ms wall, read-back included; "
             f"plan.run of the same blocks: {m['verify']['plan_run_all_blocks_ms']:.3f} ms of device time"]
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


def main_delta(args):
    results = {}
    for leg, limit in DELTA_LEG_SECONDS.items():
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--layers", str(args.layers), "--reps", str(args.reps)],
                           capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"leg {leg} failed (exit {p.returncode}); nothing further is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            return 1
        results[leg] = json.loads(line[0][7:])
        print(f"leg {leg}: ok", flush=True)
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "resident_delta")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(results, open(out + ".json", "w"), indent=1)
    k = results["k"]
    lines = [f"variant store probe (ResidentCheckpoint.from_state_dict(..., base=...)): {k['layers']} Llama-3-8B blocks, bf16; device events, median ms; every result checked against its source",
             f"base store: {k['base']['resident_bytes']} of {k['base']['nbytes']} bytes resident (index {k['base']['index_bytes']} B), built in {k['base']['build_s']:.2f} s"]
    for r in k["fine_tunes"]:
        lines.append(f"({r['kind']}) resident: variant {r['variant_resident_bytes']} B = {r['variant_resident_bytes'] / r['nbytes']:.4f} of the tensors, plain store {r['plain_resident_bytes']} B = "
                     f"{r['plain_resident_bytes'] / r['nbytes']:.4f}; {r['delta_entries']} of {r['tensors']} tensors delta-coded")
        q = r["plan_run_ms"]
        lines.append(f"    plan.run of one block ({k['block_bytes']} B): plain store {q['plain'][0]:.4f} / {q['plain'][1]:.4f} (A/A spread {100 * r['aa_spread']:.1f} %), variant over plain tensors "
                     f"{q['over_tensors'][0]:.4f} / {q['over_tensors'][1]:.4f}, variant over a resident base {q['over_store'][0]:.4f} / {q['over_store'][1]:.4f}")
        lines.append(f"    apply_ + revert_ of one block: {r['apply_revert_ms']:.4f} ms   [{r['apply_kernels']}]")
        b = r["build_s"]
        lines.append(f"    store build: plain {b['plain']:.2f} s, variant over plain tensors {b['over_tensors']:.2f} s, over a resident base {b['over_store']:.2f} s")
        lines.append(f"    kernels: over tensors [{r['kernels']['over_tensors']}]  over store [{r['kernels']['over_store']}]")
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


def main_delta_file(args):
    results = {}
    for leg, limit in DELTA_FILE_LEG_SECONDS.items():
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--layers", str(args.layers), "--reps", str(args.reps)],
                           capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"leg {leg} failed (exit {p.returncode}); nothing further is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            return 1
        results[leg] = json.loads(line[0][7:])
        print(f"leg {leg}: ok", flush=True)
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "resident_delta_file")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(results, open(out + ".json", "w"), indent=1)
    n = results["n"]
    lines = [f"delta file probe (ResidentCheckpoint.save_file / from_file(base=)): {n['layers']} Llama-3-8B blocks, bf16, over a resident base with an index; wall times are medians, "
             "ended by a device sync; plan.run by device events, median ms; loaded bodies checked byte-equal to the built ones, every decode against its source"]
    for r in n["fine_tunes"]:
        w, q = r["wall_s"], r["plan_run_ms"]
        lines.append(f"({r['kind']}) file bytes: delta {r['delta_file_bytes']} = {r['delta_file_bytes'] / r['raw_bytes']:.4f} of the raw tensors ({r['raw_bytes']} B), plain .znn.safetensors "
                     f"{r['plain_file_bytes']} = {r['plain_file_bytes'] / r['raw_bytes']:.4f}; {r['delta_entries']} of {r['tensors']} tensors delta-coded; resident: built {r['built_resident_bytes']} B, loaded {r['loaded_resident_bytes']} B")
        lines.append(f"    wall: from_file(delta, base=store) {w['from_file'] * 1e3:.1f} ms against from_state_dict(ft_sd, base=store) {w['from_state_dict'] * 1e3:.1f} ms (ft_sd on the device); save_file {w['save_file'] * 1e3:.1f} ms")
        lines.append(f"    verify_base: base with recorded digests {w['from_file'] * 1e3:.1f} ms, base without (digested at load) {w['from_file_base_without_digests'] * 1e3:.1f} ms, verify_base=False {w['from_file_verify_base_off'] * 1e3:.1f} ms")
        lines.append(f"    plan.run of one block ({n['block_bytes']} B): built variant {q['built'][0]:.4f} / {q['built'][1]:.4f} (A/A spread {100 * r['aa_spread']:.1f} %), loaded variant "
                     f"{q['loaded'][0]:.4f} / {q['loaded'][1]:.4f} ({100 * r['loaded_vs_built']:+.1f} % against built)")
        lines.append(f"    kernels: built [{r['kernels']['built']}]  loaded [{r['kernels']['loaded']}]")
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


def leg_p(args):
    """--delta-index: plan.run of one Llama-3-8B-shaped block from a variant over a resident INDEXED base, without and with the variant's DELTA index
    — interleaved, both orders (A B A B, then B A B A) —, the build time of that index and its size."""
    import torch
    from zipnn_amd import ResidentCheckpoint
    sd, per = _blocks(args.layers)
    names = per[0]
    res = {"layers": args.layers, "block_bytes": sum(sd[k].numel() * 2 for k in names), "fine_tunes": []}
    base = ResidentCheckpoint.from_state_dict(sd, "cuda:0", index=True)
    for kind in ("sparse", "drift"):
        ft = _fine_tune(sd, kind, 21)
        store = ResidentCheckpoint.from_state_dict(ft, "cuda:0", base=base, index=True)
        dn = [k for k in names if store.info(k)["delta"] is True]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        added = store.build_index(deltas=True)
        torch.cuda.synchronize(); build_s = time.perf_counter() - t0
        hints = {k: store._entries[k].hints for k in dn}
        scratch = torch.empty(store.scratch_bytes(names), dtype=torch.uint8, device="cuda")
        runs, kernels = {"plain": [], "hinted": []}, {}
        for leg in ("plain", "hinted", "plain", "hinted", "hinted", "plain", "hinted", "plain"):
            for k in dn:
                store._entries[k].hints = hints[k] if leg == "hinted" else None
            plan = store.plan(names, into=scratch)
            t = _events_ms(plan.run, args.reps)
            plan.status()
            for k in names:
                assert _same(plan.tensors[k], ft[k]), (kind, leg, k)
            runs[leg].append(t["median_ms"])
            kernels[leg] = _capi_kernels()
            plan.close()
        for k in dn:
            store._entries[k].hints = hints[k]
        a, h = runs["plain"], runs["hinted"]
        dbytes = sum(store.info(k)["nbytes"] for k in dn)
        res["fine_tunes"].append({"kind": kind, "delta_entries": len(dn), "tensors": len(names), "plan_run_ms": runs, "kernels": kernels,
                                  "aa_spread": (max(a) - min(a)) / min(a), "gain": 1.0 - (sum(h) / len(h)) / (sum(a) / len(a)),
                                  "delta_index_bytes": added, "delta_index_share": added / max(sum(store.info(k)["nbytes"] for k in store.keys() if store.info(k)["delta"] is True), 1),
                                  "build_s": build_s, "block_delta_bytes": dbytes})
        del store, ft, scratch
        torch.cuda.empty_cache()
    return res


def main_delta_index(args):
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--leg", "p", "--layers", str(args.layers), "--reps", str(args.reps)],
                       capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(f"leg p failed (exit {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        return 1
    res = json.loads(line[0][7:])
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "resident_delta_index")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lines = [f"command: python scripts/bench_resident.py --delta-index --layers {args.layers} --reps {args.reps}",
             "DELTA sync index probe (ResidentCheckpoint.build_index(deltas=True)): plan.run of one Llama-3-8B block (bf16) from a variant over a resident indexed base,",
             "without / with the variant's DELTA index, interleaved in both orders (A B A B B A B A), device events, median ms; every result checked against the fine-tune"]
    for r in res["fine_tunes"]:
        q = r["plan_run_ms"]
        lines.append(f"  {r['kind']:<7} ({r['delta_entries']} of {r['tensors']} tensors of the block are delta entries): without " + " / ".join(f"{x:.4f}" for x in q["plain"]) +
                     "   with " + " / ".join(f"{x:.4f}" for x in q["hinted"]) + f"   gain {100 * r['gain']:+.1f} %  (A/A spread of the runs without: {100 * r['aa_spread']:.1f} %)")
        lines.append(f"          DELTA index of the store {r['delta_index_bytes']} B = {100 * r['delta_index_share']:.2f} % of the delta-coded tensors, built in {r['build_s']:.3f} s")
        lines.append(f"          kernels without [{r['kernels']['plain']}]  with [{r['kernels']['hinted']}]")
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    json.dump(res, open(out + ".json", "w"), indent=1)
    print("\n".join(lines))
    return 0


def leg_s(args):
    """--sparse: the two fine-tunes of --delta as variant stores over a resident indexed base, built without and with sparse=True: resident bytes,
    build time, plan.run of one block from either store — interleaved, both orders (A B A B, then B A B A) —, apply_ + revert_ on live tensors from either."""
    import torch
    from zipnn_amd import ResidentCheckpoint
    sd, per = _blocks(args.layers)
    names = per[0]
    res = {"layers": args.layers, "block_bytes": sum(sd[k].numel() * 2 for k in names), "fine_tunes": []}
    base = ResidentCheckpoint.from_state_dict(sd, "cuda:0", index=True)

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    for kind in ("sparse", "drift"):
        ft = _fine_tune(sd, kind, 21)
        stores, build_s = {}, {}
        stores["delta"], build_s["delta"] = timed(lambda: ResidentCheckpoint.from_state_dict(ft, "cuda:0", base=base))
        stores["sparse"], build_s["sparse"] = timed(lambda: ResidentCheckpoint.from_state_dict(ft, "cuda:0", base=base, sparse=True))
        sp = stores["sparse"]
        scratch = torch.empty(sp.scratch_bytes(names), dtype=torch.uint8, device="cuda")
        runs, kernels = {"delta": [], "sparse": []}, {}
        for leg in ("delta", "sparse", "delta", "sparse", "sparse", "delta", "sparse", "delta"):
            plan = stores[leg].plan(names, into=scratch)
            t = _events_ms(plan.run, args.reps)
            plan.status()
            for k in names:
                assert _same(plan.tensors[k], ft[k]), (kind, leg, k)
            runs[leg].append(t["median_ms"])
            kernels[leg] = _capi_kernels()
            plan.close()
        ar, ar_kernels = {}, {}
        for leg in ("delta", "sparse"):
            live = {k: sd[k].clone() for k in names}
            st = stores[leg]
            ar[leg] = _events_ms(lambda: (st.apply_(live, check=False), st.revert_(live, check=False)), args.reps)["median_ms"]
            st.status()
            for k in names:
                assert _same(live[k], sd[k]), (kind, leg, "revert", k)
            st.apply_(live)
            ar_kernels[leg] = _capi_kernels()
            for k in names:
                assert _same(live[k], ft[k]), (kind, leg, "apply", k)
            del live
        a, s = runs["delta"], runs["sparse"]
        res["fine_tunes"].append({"kind": kind, "tensors": len(ft), "nbytes": sp.nbytes, "sparse_entries": sum(1 for k in ft if sp.info(k)["delta"] == "sparse"),
                                  "patch_entries": sum(sp.info(k)["patch_entries"] or 0 for k in ft),
                                  "resident_bytes": {leg: stores[leg].resident_bytes for leg in stores}, "build_s": build_s, "plan_run_ms": runs, "kernels": kernels,
                                  "aa_spread": (max(a) - min(a)) / min(a), "gain": 1.0 - (sum(s) / len(s)) / (sum(a) / len(a)),
                                  "apply_revert_ms": ar, "apply_kernels": ar_kernels})
        del stores, sp, ft, scratch
        torch.cuda.empty_cache()
    return res


def leg_r(args):
    """--rebase: see the module docstring."""
    import torch
    from zipnn_amd import ResidentCheckpoint, _capi, codec
    lib = _capi.lib()
    sd, per = _blocks(args.layers)
    names = per[0]
    base = ResidentCheckpoint.from_state_dict(sd, "cuda:0", index=True)
    sds, chain = [sd], [base]
    for k in range(4):
        sds.append(_fine_tune(sds[-1], "sparse", 41 + k))
        chain.append(ResidentCheckpoint.from_state_dict(sds[-1], "cuda:0", base=chain[-1], sparse=True))
    s4, ft4 = chain[-1], sds[-1]
    order = ("A", "B", "A", "B", "B", "A", "B", "A")

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def abab(fa, fb, timer):
        runs = {"A": [], "B": []}
        for leg in order:
            runs[leg].append(timer(fa if leg == "A" else fb))
        a, b = runs["A"], runs["B"]
        return {"A_ms": a, "B_ms": b, "aa_spread": (max(a) - min(a)) / min(a), "B_over_A": (sum(b) / len(b)) / (sum(a) / len(a))}
    res = {"layers": args.layers, "tensors": len(sd), "nbytes": base.nbytes,
           "sparse_entries_s4": sum(1 for k in ft4 if s4.info(k)["delta"] == "sparse"), "patch_entries_s4": sum(s4.info(k)["patch_entries"] or 0 for k in ft4)}
    # 1. the chain flattened: rebased (B) against the route it replaces (A)
    flat = s4.rebased(base)
    for k in ft4:
        assert flat.info(k)["delta"] == s4.info(k)["delta"] or flat.info(k)["delta"] == "sparse", k
    got = flat.get_tensors(list(ft4))
    for k in ft4:
        assert _same(got[k], ft4[k]), ("flat", k)
    del got
    res["flat_sparse_entries"] = sum(1 for k in ft4 if flat.info(k)["delta"] == "sparse")
    res["flat_patch_entries"] = sum(flat.info(k)["patch_entries"] or 0 for k in ft4)
    res["flat_resident_bytes"], res["s4_resident_bytes"] = flat.resident_bytes, s4.resident_bytes
    res["rebase_wall"] = abab(lambda: ResidentCheckpoint.from_state_dict(s4.get_tensors(list(ft4)), "cuda:0", base=base, sparse=True), lambda: s4.rebased(base),
                              lambda fn: wall(fn)[1])
    s4.rebased(base)
    res["rebase_kernels"] = _capi_kernels()
    # 2. the merge call alone (B) against the build call on the same pairs from materialised tensors (A): patch(s1 over base) (+) patch(s2 over s1) = patch(s2 over base)
    sp = [k for k in sd if chain[1].info(k)["delta"] == "sparse" and chain[2].info(k)["delta"] == "sparse"]
    pa, pb = [chain[1]._entries[k].patch for k in sp], [chain[2]._entries[k].patch for k in sp]
    tri = [(a, b, sd[k].numel() * 2, 2) for a, b, k in zip(pa, pb, sp)]
    sizes = codec.patch_merge_sizes_device_batch(lib, tri)
    pairs = [(codec.flat_bytes(sds[2][k]), codec.flat_bytes(sd[k]), 2) for k in sp]
    assert codec.patch_sizes_device_batch(lib, pairs) == sizes
    offs, o = [], 0
    for n in sizes:
        offs.append(o); o += (n + 255) // 256 * 256
    out_m, out_b = (torch.empty(max(o, 16), dtype=torch.uint8, device="cuda") for _ in range(2))
    mi = [(a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), n, el, out_m.data_ptr() + off, cap) for (a, b, n, el), off, cap in zip(tri, offs, sizes)]
    bi = [(s.data_ptr(), b.data_ptr(), s.numel(), el, out_b.data_ptr() + off, cap) for (s, b, el), off, cap in zip(pairs, offs, sizes)]
    st = torch.cuda.current_stream().cuda_stream
    assert lib.patch_merge_batch_dev(mi, st) == sizes and lib.patch_build_batch_dev(bi, st) == sizes
    for off, n in zip(offs, sizes):
        assert torch.equal(out_m[off:off + n], out_b[off:off + n]), "the merge is not the build"
    res["merge_call"] = abab(lambda: lib.patch_build_batch_dev(bi, st), lambda: lib.patch_merge_batch_dev(mi, st), lambda fn: _events_ms(fn, args.reps)["median_ms"])
    res["merge_call"].update({"items": len(sp), "input_bytes": sum(a.numel() + b.numel() for a, b in zip(pa, pb)), "output_bytes": sum(sizes),
                              "tensor_bytes": sum(sd[k].numel() * 2 for k in sp)})
    del out_m, out_b
    # 3. plan.run of one block: the depth-4 chain (A) against the flattened store (B)
    scratch = torch.empty(flat.scratch_bytes(names), dtype=torch.uint8, device="cuda")

    def plan_ms(store):
        plan = store.plan(names, into=scratch)
        t = _events_ms(plan.run, args.reps)["median_ms"]
        plan.status()
        for k in names:
            assert _same(plan.tensors[k], ft4[k]), k
        plan.close()
        return t
    res["plan_run"] = abab(lambda: s4, lambda: flat, lambda pick: plan_ms(pick()))
    # 4. live weights from sibling a to sibling b and back: a.revert_ + b.apply_ + b.revert_ + a.apply_ (A) against sw.apply_ + sw.revert_ (B); 5. resident bytes
    a, fa = chain[1], sds[1]
    fb = _fine_tune(sd, "sparse", 77)
    b = ResidentCheckpoint.from_state_dict(fb, "cuda:0", base=base, sparse=True)
    sw = b.rebased(a)
    live = {k: fa[k].clone() for k in names}
    sw.apply_(live)
    for k in names:
        assert _same(live[k], fb[k]), ("sw.apply_", k)
    sw.revert_(live)
    for k in names:
        assert _same(live[k], fa[k]), ("sw.revert_", k)
    res["switch"] = abab(lambda: (a.revert_(live, check=False), b.apply_(live, check=False), b.revert_(live, check=False), a.apply_(live, check=False)),
                         lambda: (sw.apply_(live, check=False), sw.revert_(live, check=False)), lambda fn: _events_ms(fn, args.reps)["median_ms"])
    a.status()
    for k in names:
        assert _same(live[k], fa[k]), ("switch", k)
    res["sibling_bytes"] = {"b_over_base": b.resident_bytes, "b_over_a": sw.resident_bytes, "a_over_base": a.resident_bytes, "nbytes": b.nbytes,
                            "entries_b_over_base": sum(b.info(k)["patch_entries"] or 0 for k in fb), "entries_b_over_a": sum(sw.info(k)["patch_entries"] or 0 for k in fb)}
    return res


def main_rebase(args):
    p = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--leg", "r", "--layers", str(args.layers), "--reps", str(args.reps)],
                       capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(f"leg r failed (exit {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        return p.returncode or 1
    res = json.loads(line[0][7:])
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "resident_rebase")
    os.makedirs(os.path.dirname(out), exist_ok=True)

    def row(title, r, a, b):
        return [f"  {title}", f"          {a} " + " / ".join(f"{x:.4f}" for x in r["A_ms"]) + f"   {b} " + " / ".join(f"{x:.4f}" for x in r["B_ms"]) +
                f"   ms; {b} = {r['B_over_A']:.3f} of {a}  (A/A spread of the {a} runs: {100 * r['aa_spread']:.1f} %)"]
    m, sb = res["merge_call"], res["sibling_bytes"]
    lines = [f"command: python scripts/bench_resident.py --rebase --layers {args.layers} --reps {args.reps}",
             "patch merge probe (zn_patch_merge_batch_dev, ResidentCheckpoint.rebased, DESIGN §3.12): a chain of four steps, each 2 % of the elements replaced, and two sibling",
             f"fine-tunes over a resident indexed base of {res['layers']} Llama-3-8B blocks (bf16, {res['tensors']} tensors, {res['nbytes']} B); every comparison interleaved in both orders",
             "(A B A B B A B A), every result checked against the tensors",
             f"  s4 over s3: {res['sparse_entries_s4']} sparse tensors, {res['patch_entries_s4']} entries, the chain's last store holds {res['s4_resident_bytes']} B;"
             f" flattened over the base: {res['flat_sparse_entries']} sparse tensors, {res['flat_patch_entries']} entries, {res['flat_resident_bytes']} B"]
    lines += row("1. the chain flattened, wall ms: get_tensors(s4) + from_state_dict(base=base, sparse=True) against s4.rebased(base)", res["rebase_wall"], "build", "rebased")
    lines.append(f"          kernels of rebased's last call [{res['rebase_kernels']}]")
    lines += row(f"2. the call alone, device events, median ms: zn_patch_build_batch_dev from the tensors ({m['tensor_bytes']} B twice) against zn_patch_merge_batch_dev on the two patches"
                 f" of the same {m['items']} pairs ({m['input_bytes']} B in, {m['output_bytes']} B out)", m, "build", "merge")
    lines += row("3. plan.run of one block, device events, median ms: from the depth-4 chain against the flattened store", res["plan_run"], "chain", "flat")
    lines += row("4. live weights of one block from a to b and back, device events, median ms: a.revert_ + b.apply_ + b.revert_ + a.apply_ against sw.apply_ + sw.revert_ (sw = b.rebased(a))",
                 res["switch"], "two-stores", "sw")
    lines.append(f"  5. resident bytes: b over the base {sb['b_over_base']} B ({sb['entries_b_over_base']} entries), b over a {sb['b_over_a']} B ({sb['entries_b_over_a']} entries),"
                 f" a over the base {sb['a_over_base']} B; the tensors {sb['nbytes']} B")
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    json.dump(res, open(out + ".json", "w"), indent=1)
    print("\n".join(lines))
    return 0


def leg_h(args):
    """--shard: see the module docstring."""
    import torch
    from zipnn_amd import ResidentCheckpoint, _capi, codec
    lib = _capi.lib()
    sd, per = _blocks(args.layers)
    names = per[0]
    base = ResidentCheckpoint.from_state_dict(sd, "cuda:0", index=True)
    ft_sd = _fine_tune(sd, "sparse", 41)
    ft = ResidentCheckpoint.from_state_dict(ft_sd, "cuda:0", base=base, sparse=True)
    ways, rank = 8, 1
    spec = {}
    for k, v in sd.items():
        dim = 0 if any(p in k for p in ("q_proj", "k_proj", "v_proj", "gate_proj", "up_proj")) else 1 if any(p in k for p in ("o_proj", "down_proj")) else None
        if dim is not None:
            spec[k] = (dim, rank * v.shape[dim] // ways, (rank + 1) * v.shape[dim] // ways)

    def cut(d):
        return {k: (v.narrow(spec[k][0], spec[k][1], spec[k][2] - spec[k][1]).contiguous() if k in spec else v) for k, v in d.items()}
    onto, want = cut(sd), cut(ft_sd)
    order = ("A", "B", "A", "B", "B", "A", "B", "A")

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def abab(fa, fb, timer):
        runs = {"A": [], "B": []}
        for leg in order:
            runs[leg].append(timer(fa if leg == "A" else fb))
        a, b = runs["A"], runs["B"]
        return {"A_ms": a, "B_ms": b, "aa_spread": (max(a) - min(a)) / min(a), "B_over_A": (sum(b) / len(b)) / (sum(a) / len(a))}

    def route():                                   # what sharded replaces
        got = ft.get_tensors(list(ft_sd))
        return ResidentCheckpoint.from_state_dict({k: (got[k].narrow(spec[k][0], spec[k][1], spec[k][2] - spec[k][1]).contiguous() if k in spec else got[k]) for k in ft_sd},
                                                  "cuda:0", base=onto, sparse=True)
    mine, direct = ft.sharded(onto, spec), route()
    for s, tag in ((mine, "sharded"), (direct, "route")):
        got = s.get_tensors(list(ft_sd))
        for k in ft_sd:
            assert _same(got[k], want[k]), (tag, k)
        del got
    for k in ft_sd:
        assert mine.info(k)["delta"] == direct.info(k)["delta"] and mine.info(k)["patch_entries"] == direct.info(k)["patch_entries"], k
        if mine.info(k)["delta"] == "sparse":
            assert torch.equal(mine._entries[k].patch, direct._entries[k].patch), k
    res = {"layers": args.layers, "tensors": len(sd), "nbytes": base.nbytes, "ways": ways, "rank": rank, "shard_nbytes": mine.nbytes,
           "ft_resident_bytes": ft.resident_bytes, "shard_resident_bytes": mine.resident_bytes,
           "sparse_entries": sum(1 for k in ft_sd if mine.info(k)["delta"] == "sparse"), "patch_entries": sum(mine.info(k)["patch_entries"] or 0 for k in ft_sd)}
    # 1. sharded (B) against the route it replaces (A), wall
    res["shard_wall"] = abab(route, lambda: ft.sharded(onto, spec), lambda fn: wall(fn)[1])
    ft.sharded(onto, spec)
    res["shard_kernels"] = _capi_kernels()
    # 2. the select call alone (B) against the build call on the same materialised shard pairs (A), dim 0 and dim 1 apart
    st = torch.cuda.current_stream().cuda_stream
    res["select_call"] = {}
    for dim in (0, 1):
        ks = [k for k in spec if spec[k][0] == dim and ft.info(k)["delta"] == "sparse"]
        items = [(ft._entries[k].patch, 2) + codec.narrow_rect(sd[k].shape, *spec[k]) for k in ks]
        args_ = [(it[0].data_ptr(), it[0].numel()) + tuple(it[1:]) for it in items]
        sizes = lib.patch_select_size_batch_dev(args_, st)
        pairs = [(codec.flat_bytes(want[k]), codec.flat_bytes(onto[k]), 2) for k in ks]
        assert codec.patch_sizes_device_batch(lib, pairs) == sizes
        offs, o = [], 0
        for n in sizes:
            offs.append(o); o += (n + 255) // 256 * 256
        out_s, out_b = (torch.empty(max(o, 16), dtype=torch.uint8, device="cuda") for _ in range(2))
        si = [a + (out_s.data_ptr() + off, cap) for a, off, cap in zip(args_, offs, sizes)]
        bi = [(s.data_ptr(), b.data_ptr(), s.numel(), el, out_b.data_ptr() + off, cap) for (s, b, el), off, cap in zip(pairs, offs, sizes)]
        assert lib.patch_select_batch_dev(si, st) == sizes and lib.patch_build_batch_dev(bi, st) == sizes
        for off, n in zip(offs, sizes):
            assert torch.equal(out_s[off:off + n], out_b[off:off + n]), "the select is not the build"
        r = abab(lambda: lib.patch_build_batch_dev(bi, st), lambda: lib.patch_select_batch_dev(si, st), lambda fn: _events_ms(fn, args.reps)["median_ms"])
        r.update({"items": len(ks), "input_bytes": sum(it[0].numel() for it in items), "output_bytes": sum(sizes), "shard_bytes": sum(want[k].numel() * 2 for k in ks)})
        r["select_gb_per_s"] = (r["input_bytes"] + r["output_bytes"]) / (statistics.median(r["B_ms"]) * 1e-3) / 1e9
        res["select_call"][str(dim)] = r
        del out_s, out_b
    # 3. plan.run of one block: a store built directly from the shard tensors (A) against the sharded store (B)
    scratch = torch.empty(mine.scratch_bytes(names), dtype=torch.uint8, device="cuda")

    def plan_ms(store):
        plan = store.plan(names, into=scratch)
        t = _events_ms(plan.run, args.reps)["median_ms"]
        plan.status()
        for k in names:
            assert _same(plan.tensors[k], want[k]), k
        plan.close()
        return t
    res["plan_run"] = abab(lambda: direct, lambda: mine, lambda pick: plan_ms(pick()))
    return res


def main_shard(args):
    p = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--leg", "h", "--layers", str(args.layers), "--reps", str(args.reps)],
                       capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(f"leg h failed (exit {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        return p.returncode or 1
    res = json.loads(line[0][7:])
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "resident_shard")
    os.makedirs(os.path.dirname(out), exist_ok=True)

    def row(title, r, a, b):
        return [f"  {title}", f"          {a} " + " / ".join(f"{x:.4f}" for x in r["A_ms"]) + f"   {b} " + " / ".join(f"{x:.4f}" for x in r["B_ms"]) +
                f"   ms; {b} = {r['B_over_A']:.3f} of {a}  (A/A spread of the {a} runs: {100 * r['aa_spread']:.1f} %)"]
    lines = [f"command: python scripts/bench_resident.py --shard --layers {args.layers} --reps {args.reps}",
             "patch select probe (zn_patch_select_batch_dev, ResidentCheckpoint.sharded, DESIGN §3.13): a 2 % fine-tune, sparse, over a resident indexed base of",
             f"{res['layers']} Llama-3-8B blocks (bf16, {res['tensors']} tensors, {res['nbytes']} B); rank {res['rank']} of a split of {res['ways']}: q/k/v/gate/up along dim 0, o/down along dim 1,",
             "over the rank's shards of the base as plain tensors; every comparison interleaved in both orders (A B A B B A B A), every result checked against the narrowed tensors",
             f"  the shard store: {res['shard_nbytes']} B of tensors, {res['sparse_entries']} sparse tensors, {res['patch_entries']} entries, {res['shard_resident_bytes']} B resident"
             f" (the whole fine-tune: {res['ft_resident_bytes']} B)"]
    lines += row("1. one rank's store, wall ms: get_tensors + narrow().contiguous() + from_state_dict(base=onto, sparse=True) against ft.sharded(onto, spec)", res["shard_wall"], "route", "sharded")
    lines.append(f"          kernels of sharded's last call [{res['shard_kernels']}]")
    for dim in ("0", "1"):
        m = res["select_call"][dim]
        lines += row(f"2. dim {dim}, the call alone, device events, median ms: zn_patch_build_batch_dev from the shard tensors ({m['shard_bytes']} B twice) against zn_patch_select_batch_dev on the"
                     f" whole patches of the same {m['items']} tensors ({m['input_bytes']} B in, {m['output_bytes']} B out: {m['select_gb_per_s']:.1f} GB/s over both)", m, "build", "select")
    lines += row("3. plan.run of one block, device events, median ms: a store built from the shard tensors against the sharded store (identical patches)", res["plan_run"], "built", "sharded")
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    json.dump(res, open(out + ".json", "w"), indent=1)
    print("\n".join(lines))
    return 0


def main_sparse(args):
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--leg", "s", "--layers", str(args.layers), "--reps", str(args.reps)],
                       capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(f"leg s failed (exit {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        return 1
    res = json.loads(line[0][7:])
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "resident_sparse")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lines = [f"command: python scripts/bench_resident.py --sparse --layers {args.layers} --reps {args.reps}",
             "sparse variant probe (ResidentCheckpoint.from_state_dict(..., base=..., sparse=True)): the fine-tunes of --delta over a resident indexed base, built without (delta)",
             "and with sparse=True; plan.run of one Llama-3-8B block (bf16), interleaved in both orders (A B A B B A B A), device events, median ms; every result checked"]
    for r in res["fine_tunes"]:
        q, b = r["plan_run_ms"], r["resident_bytes"]
        lines.append(f"  {r['kind']:<7} {r['sparse_entries']} of {r['tensors']} tensors sparse ({r['patch_entries']} entries): resident {b['sparse']} B against {b['delta']} B"
                     f" = {b['sparse'] / b['delta']:.3f} of the delta store, {b['sparse'] / r['nbytes']:.4f} of the raw bytes; built in {r['build_s']['sparse']:.3f} s against {r['build_s']['delta']:.3f} s")
        lines.append("          plan.run delta " + " / ".join(f"{x:.4f}" for x in q["delta"]) + "   sparse " + " / ".join(f"{x:.4f}" for x in q["sparse"]) +
                     f"   gain {100 * r['gain']:+.1f} %  (A/A spread of the delta runs: {100 * r['aa_spread']:.1f} %)")
        lines.append(f"          apply_ + revert_ of the block on live tensors: delta {r['apply_revert_ms']['delta']:.4f} ms, sparse {r['apply_revert_ms']['sparse']:.4f} ms")
        lines.append(f"          kernels delta [{r['kernels']['delta']}]  sparse [{r['kernels']['sparse']}]  apply_ sparse [{r['apply_kernels']['sparse']}]")
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    json.dump(res, open(out + ".json", "w"), indent=1)
    print("\n".join(lines))
    return 0


def leg_f(args):
    """--sparse-file: the sparse variants of --sparse written by save_file(sparse=True) and read back: file bytes against the delta file and the
    plain file and against Σ (L + 15); from_file with check_patches True against False, interleaved; the check call alone against a device copy of the same
    bytes; plan.run of one block from the loaded store against the built one, interleaved in both orders."""
    import tempfile
    import torch
    from zipnn_amd import ResidentCheckpoint, _capi, codec
    sd, per = _blocks(args.layers)
    names = per[0]
    res = {"layers": args.layers, "fine_tunes": []}
    base = ResidentCheckpoint.from_state_dict(sd, "cuda:0", index=True)

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3
    with tempfile.TemporaryDirectory() as td:
        for kind in ("sparse", "drift"):
            ft = _fine_tune(sd, kind, 21)
            sp = ResidentCheckpoint.from_state_dict(ft, "cuda:0", base=base, sparse=True)
            files = {"sparse": sp.save_file(os.path.join(td, f"{kind}.sparse.znn.safetensors"), sparse=True),
                     "delta": ResidentCheckpoint.from_state_dict(ft, "cuda:0", base=base).save_file(os.path.join(td, f"{kind}.delta.znn.safetensors")),
                     "plain": ResidentCheckpoint.from_state_dict(ft, "cuda:0").save_file(os.path.join(td, f"{kind}.plain.znn.safetensors"))}
            patches = [k for k in ft if sp.info(k)["delta"] == "sparse"]
            r = {"kind": kind, "tensors": len(ft), "nbytes": sp.nbytes, "sparse_entries": len(patches), "file_bytes": {k: os.path.getsize(v) for k, v in files.items()},
                 "entries_sum": sum(sp.info(k)["resident_bytes"] + 15 for k in patches), "patch_bytes": sum(sp.info(k)["resident_bytes"] for k in patches)}
            load = {True: [], False: []}
            for flag in (True, False, True, False, False, True, False, True, True, False):
                st, ms = wall(lambda: ResidentCheckpoint.from_file(files["sparse"], "cuda:0", base=base, check_patches=flag))
                load[flag].append(ms)
                del st
            r["from_file_ms"] = {"checked": sorted(load[True])[len(load[True]) // 2], "unchecked": sorted(load[False])[len(load[False]) // 2], "all": {str(k): v for k, v in load.items()}}
            loaded = ResidentCheckpoint.from_file(files["sparse"], "cuda:0", base=base)
            for k in ft:
                assert sp.info(k)["delta"] == loaded.info(k)["delta"] and sp.info(k)["resident_bytes"] == loaded.info(k)["resident_bytes"], k
            if patches:
                lib = _capi.lib()
                items = [(loaded._entries[k].patch, loaded._entries[k].nbytes, loaded._entries[k].P) for k in patches]
                calls = sorted(wall(lambda: codec.patch_check_device_batch(lib, items))[1] for _ in range(args.reps))
                r["check_call_ms"] = calls[len(calls) // 2]
                # (the call is synchronous: the events below enclose its launch, read-back and sync as well as the kernel)
                src = torch.empty(r["patch_bytes"], dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
                r["copy_same_bytes_ms"] = _events_ms(lambda: dst.copy_(src), args.reps)["median_ms"]
                r["check_events_ms"] = _events_ms(lambda: codec.patch_check_device_batch(lib, items), args.reps)["median_ms"]
                r["addresses_mod_256"] = sorted({loaded._entries[k].patch.data_ptr() % 256 for k in patches})
                scratch = torch.empty(sp.scratch_bytes(names), dtype=torch.uint8, device="cuda")
                runs = {"built": [], "loaded": []}
                stores = {"built": sp, "loaded": loaded}
                for leg in ("built", "loaded", "built", "loaded", "loaded", "built", "loaded", "built"):
                    plan = stores[leg].plan(names, into=scratch)
                    t = _events_ms(plan.run, args.reps)
                    plan.status()
                    for k in names:
                        assert _same(plan.tensors[k], ft[k]), (kind, leg, k)
                    runs[leg].append(t["median_ms"])
                    plan.close()
                r["plan_run_ms"] = runs
                a = runs["built"]
                r["aa_spread"] = (max(a) - min(a)) / min(a)
            res["fine_tunes"].append(r)
            del sp, loaded, ft
            torch.cuda.empty_cache()
    return res


def main_sparse_file(args):
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--leg", "f", "--layers", str(args.layers), "--reps", str(args.reps)],
                       capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(f"leg f failed (exit {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        return 1
    res = json.loads(line[0][7:])
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "resident_sparse_file")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lines = [f"command: python scripts/bench_resident.py --sparse-file --layers {args.layers} --reps {args.reps}",
             "sparse file probe (save_file(sparse=True) / from_file(base=, check_patches=), DESIGN §3.11): the fine-tunes of --sparse over a resident indexed base; walls are",
             "host perf_counter between device syncs (median of 5 per setting, interleaved), plan.run and the copy are device events (median ms); every result checked"]
    for r in res["fine_tunes"]:
        f = r["file_bytes"]
        lines.append(f"  {r['kind']:<7} {r['sparse_entries']} of {r['tensors']} tensors sparse: file {f['sparse']} B against the delta file {f['delta']} B = {f['sparse'] / f['delta']:.3f}, the plain file {f['plain']} B"
                     f" = {f['sparse'] / f['plain']:.3f}, {f['sparse'] / r['nbytes']:.4f} of the raw bytes; sparse entries {r['entries_sum']} B = Σ (L + 15)")
        q = r["from_file_ms"]
        lines.append(f"          from_file wall: check_patches=True {q['checked']:.3f} ms, False {q['unchecked']:.3f} ms" + (f"; the check call alone {r['check_call_ms']:.4f} ms wall"
                     f" = {100 * r['check_call_ms'] / q['checked']:.1f} % of the checked load" if "check_call_ms" in r else ""))
        if "plan_run_ms" in r:
            lines.append(f"          check call between device events {r['check_events_ms']:.4f} ms (launch, read-back and sync included) against a device copy of the same {r['patch_bytes']} B: {r['copy_same_bytes_ms']:.4f} ms"
                         f" = {r['check_events_ms'] / r['copy_same_bytes_ms']:.2f} x")
            p_ = r["plan_run_ms"]
            lines.append("          plan.run built " + " / ".join(f"{x:.4f}" for x in p_["built"]) + "   loaded " + " / ".join(f"{x:.4f}" for x in p_["loaded"]) +
                         f"   (A/A spread of the built runs: {100 * r['aa_spread']:.1f} %; loaded patches at addresses mod 256: {r['addresses_mod_256']})")
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    json.dump(res, open(out + ".json", "w"), indent=1)
    print("\n".join(lines))
    return 0


def leg_t(args):
    """--strided: apply_ + revert_ of one Llama-3-8B block from a sparse variant over a resident indexed base, on live tensors in four layouts:
    contiguous; transposed storage; dim-1 narrows of a twice-as-wide buffer; a 16-row tile shuffle (view(R/16, 16, C/32, 32).permute(0, 2, 1, 3).contiguous(), patched
    through the inverse 4-D view by one zn_patch_apply_strided_batch_dev call per direction, since the view has another shape than the entry).  Each strided layout
    against the workaround that exists without the strided call — contiguous() + the contiguous apply + copy_ back —, interleaved with the contiguous run in both orders."""
    import torch
    from zipnn_amd import ResidentCheckpoint, _capi, codec
    lib = _capi.lib()
    sd, per = _blocks(args.layers)
    names = per[0]
    base = ResidentCheckpoint.from_state_dict(sd, "cuda:0", index=True)
    ft = _fine_tune(sd, "sparse", 21)
    store = ResidentCheckpoint.from_state_dict(ft, "cuda:0", base=base, sparse=True)
    st = torch.cuda.current_stream().cuda_stream
    two_d = [k for k in names if sd[k].dim() == 2]
    assert all(store.info(k)["delta"] == "sparse" for k in two_d)

    def live_of(layout):
        """-> {name: live view holding the base's values} (1-D tensors stay contiguous)"""
        out = {}
        for k in names:
            w = sd[k]
            if layout == "contiguous" or w.dim() != 2:
                out[k] = w.clone()
            elif layout == "transposed":
                out[k] = w.t().contiguous().t()
            elif layout == "narrow":
                fused = torch.zeros(w.shape[0], 2 * w.shape[1], dtype=w.dtype, device=w.device)
                out[k] = fused[:, w.shape[1] // 2: w.shape[1] // 2 + w.shape[1]]
                out[k].copy_(w)
            else:                                             # "tile": the 4-D view whose row-major order is the tensor's, over tile-shuffled storage
                R, C = w.shape
                out[k] = w.view(R // 16, 16, C // 32, 32).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        return out

    def runner(layout, live):
        if layout != "tile":
            return lambda: (store.apply_(live, check=False), store.revert_(live, check=False))
        items = [codec.patch_strided_item(live[k], store.patch(k)) for k in two_d]
        rest = {k: live[k] for k in names if k not in two_d}
        return lambda: (store.apply_(rest, check=False), lib.patch_apply_strided_batch_dev(items, st, False), store.revert_(rest, check=False), lib.patch_apply_strided_batch_dev(items, st, False))

    def workaround(live):
        def once(call):
            tmp = {k: live[k].contiguous().view(sd[k].shape) for k in names}
            call(tmp, check=False)
            for k in two_d:
                live[k].copy_(tmp[k].view(live[k].shape))
        return lambda: (once(store.apply_), once(store.revert_))

    def holds(live, want):
        return all(_same(live[k].contiguous(), want[k]) for k in names)

    res = {"layers": args.layers, "block_bytes": sum(sd[k].numel() * 2 for k in names), "patch_bytes": sum(store.patch(k).numel() for k in two_d), "tensors": len(names), "layouts": []}
    contig = live_of("contiguous")
    run_c = runner("contiguous", contig)
    for layout in ("transposed", "narrow", "tile"):
        live_s, live_w = live_of(layout), live_of(layout)
        fns = {"contiguous": run_c, "strided": runner(layout, live_s), "workaround": workaround(live_w)}
        runs, kernels = {k: [] for k in fns}, {}
        for leg in ("contiguous", "strided", "workaround", "contiguous", "strided", "workaround", "workaround", "strided", "contiguous", "workaround", "strided", "contiguous"):
            runs[leg].append(_events_ms(fns[leg], args.reps)["median_ms"])
            store.status()
            kernels[leg] = _capi_kernels()
        assert holds(contig, sd) and holds(live_s, sd) and holds(live_w, sd), layout          # every pair left the tensors as it found them
        if layout == "tile":
            lib.patch_apply_strided_batch_dev([codec.patch_strided_item(live_s[k], store.patch(k)) for k in two_d], st, True)
            store.apply_({k: live_s[k] for k in names if k not in two_d})
        else:
            store.apply_(live_s)
        assert holds(live_s, ft), layout
        res["layouts"].append({"layout": layout, "runs_ms": runs, "kernels": kernels, "median_ms": {k: statistics.median(v) for k, v in runs.items()}})
        del live_s, live_w, fns
        torch.cuda.empty_cache()
    allc = [x for r in res["layouts"] for x in r["runs_ms"]["contiguous"]]
    res["aa_spread"] = (max(allc) - min(allc)) / min(allc)
    return res


def main_strided(args):
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--leg", "t", "--layers", str(args.layers), "--reps", str(args.reps)],
                       capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(f"leg t failed (exit {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        return 1
    res = json.loads(line[0][7:])
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "resident_strided")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lines = [f"command: python scripts/bench_resident.py --strided --layers {args.layers} --reps {args.reps}",
             f"strided apply probe (ResidentCheckpoint.apply_ / revert_ on non-contiguous live tensors, DESIGN §3.15): one Llama-3-8B block ({res['tensors']} tensors, {res['block_bytes']} B, bf16),",
             f"a 2 % fine-tune kept sparse ({res['patch_bytes']} B of patches) over a resident indexed base; apply_ + revert_ between device events, median ms of {args.reps} pairs per run;",
             "per layout the runs are interleaved in both orders (C S W C S W W S C W S C: contiguous targets, the strided call, the workaround contiguous() + contiguous apply + copy_ back);",
             "after the runs every tensor holds the base's bytes, and the fine-tune's after one more apply",
             f"A/A spread of the {sum(len(r['runs_ms']['contiguous']) for r in res['layouts'])} contiguous runs: {100 * res['aa_spread']:.1f} %"]
    for r in res["layouts"]:
        q, m = r["runs_ms"], r["median_ms"]
        gain = 1.0 - m["strided"] / m["workaround"]
        verdict = "beats the workaround by more than the spread" if gain > res["aa_spread"] else "LOSES to the workaround" if gain < -res["aa_spread"] else "inside the spread of the workaround"
        lines.append(f"  {r['layout']:<11} contiguous " + " / ".join(f"{x:.4f}" for x in q["contiguous"]) + "   strided " + " / ".join(f"{x:.4f}" for x in q["strided"]) +
                     "   workaround " + " / ".join(f"{x:.4f}" for x in q["workaround"]))
        lines.append(f"              medians: contiguous {m['contiguous']:.4f}, strided {m['strided']:.4f}, workaround {m['workaround']:.4f}: the strided call takes {m['strided'] / m['workaround']:.2f} of the workaround's time"
                     f" and {m['strided'] / m['contiguous']:.2f} of the contiguous targets' — {verdict}")
        lines.append(f"              last call's kernels: strided [{r['kernels']['strided']}]  workaround [{r['kernels']['workaround']}]")
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    json.dump(res, open(out + ".json", "w"), indent=1)
    print("\n".join(lines))
    return 0


LOGICAL_LIB = os.path.join(ROOT, "zipnn_amd", "libzipnn_hip_ab_logical.so")      # build_extension(defines=("ZN_PATCH_BUILD_LOGICAL_ORDER",), out=LOGICAL_LIB)


def leg_c(args):
    """--capture: patches of one Llama-3-8B block of a 2 % fine-tune BUILT from live tensors in four layouts against a plain-tensor base:
    the strided build call against contiguous() on every view + the contiguous build call; the same call through the library built with
    -DZN_PATCH_BUILD_LOGICAL_ORDER (load order (i), the baseline) where that library exists; from_live against from_state_dict on contiguous copies, with both builds' peak
    allocated memory above the resting level."""
    import torch
    from zipnn_amd import ResidentCheckpoint, _capi, codec
    lib = _capi.lib()
    logical = _capi.ZnLib(LOGICAL_LIB) if os.path.exists(LOGICAL_LIB) else None
    sd, per = _blocks(1)
    names = per[0]
    ft = _fine_tune(sd, "sparse", 21)

    def live_of(layout):
        out = {}
        for k in names:
            w = ft[k]
            if layout == "contiguous" or w.dim() != 2:
                out[k] = w.clone()
            elif layout == "transposed":
                out[k] = w.t().contiguous().t()
            elif layout == "narrow":
                fused = torch.zeros(w.shape[0], 2 * w.shape[1], dtype=w.dtype, device=w.device)
                out[k] = fused[:, w.shape[1] // 2: w.shape[1] // 2 + w.shape[1]]
                out[k].copy_(w)
            else:                                             # "tile": tile-shuffled storage seen through the view whose row-major order is the tensor's, reshaped back to 2-D where torch can
                R, C = w.shape
                out[k] = w.view(R // 16, 16, C // 32, 32).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        return out

    def base_of(live, k):
        return sd[k].view(live[k].shape)

    def peak(fn):
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        rest = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - rest, out

    res = {"block_bytes": sum(sd[k].numel() * 2 for k in names), "tensors": len(names), "logical": logical is not None, "layouts": []}
    want = None
    for layout in ("contiguous", "transposed", "narrow", "tile"):
        live = live_of(layout)
        pairs = [(live[k], base_of(live, k)) for k in names]
        fns = {"strided": lambda: codec.patch_build_strided_device_batch(lib, pairs),
               "workaround": lambda: codec.patch_build_device_batch(lib, [(codec.flat_bytes(s.contiguous()), codec.flat_bytes(b), 2) for s, b in pairs])}
        if logical is not None:
            fns["logical"] = lambda: codec.patch_build_strided_device_batch(logical, pairs)
        got, kernels = {}, {}
        for leg, fn in fns.items():                           # each leg's kernels, read directly behind its call
            got[leg] = [None if p is None else p.clone() for p in fn()]
            kernels[leg] = (logical if leg == "logical" else lib).last_kernels()
        want = want or got["workaround"]
        for leg, ps in got.items():                           # every leg, every layout: the same patches, byte for byte
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(ps, want)), (layout, leg)
        del got
        order = list(fns) + list(fns) + list(reversed(fns)) + list(reversed(fns))
        runs = {leg: [] for leg in fns}
        for leg in order:
            runs[leg].append(_events_ms(fns[leg], args.reps)["median_ms"])
        targets = {k: live[k] for k in names}
        base = {k: base_of(live, k) for k in names}
        builds = {"from_live": lambda: ResidentCheckpoint.from_live(targets, base),
                  "from_state_dict": lambda: ResidentCheckpoint.from_state_dict({n: v.contiguous() for n, v in targets.items()}, "cuda:0", base=base, sparse=True)}
        bruns, peaks = {leg: [] for leg in builds}, {}
        for leg in ("from_live", "from_state_dict", "from_state_dict", "from_live"):
            bruns[leg].append(_events_ms(builds[leg], 2, warm=1)["median_ms"])
        for leg, fn in builds.items():
            peaks[leg], store = peak(fn)
            kernels[leg] = _capi_kernels()                    # (the last patch call of the build)
            assert all(_same(store.get_tensor(k), ft[k]) for k in names[:3]), (layout, leg)
            kinds = sorted({str(store.info(k)["delta"]) for k in names})
            del store
        res["layouts"].append({"layout": layout, "runs_ms": runs, "median_ms": {k: statistics.median(v) for k, v in runs.items()}, "kernels": kernels,
                               "build_runs_ms": bruns, "build_median_ms": {k: statistics.median(v) for k, v in bruns.items()}, "peak_bytes": peaks, "kinds": kinds})
        del live, pairs, fns, targets, base, builds
        torch.cuda.empty_cache()
    res["aa_spread"] = max((max(v) - min(v)) / min(v) for r in res["layouts"] for v in r["runs_ms"].values())
    res["aa_spread_builds"] = max((max(v) - min(v)) / min(v) for r in res["layouts"] for v in r["build_runs_ms"].values())
    return res


def main_capture(args):
    p = subprocess.run(["timeout", "-k", "10", "840", sys.executable, os.path.abspath(__file__), "--leg", "c", "--reps", str(args.reps)], capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        print(f"leg c failed (exit {p.returncode})\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        return 1
    res = json.loads(line[0][7:])
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "patch_build_strided")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    sp, spb = res["aa_spread"], res["aa_spread_builds"]
    lines = [f"command: python scripts/bench_resident.py --capture --reps {args.reps}",
             f"strided build probe (zn_patch_build_strided_batch_dev and ResidentCheckpoint.from_live, DESIGN §3.16): one Llama-3-8B block ({res['tensors']} tensors, {res['block_bytes']} B, bf16) of a 2 % fine-tune,",
             f"live in four layouts, against plain base tensors; device events, median ms of {args.reps} calls per run; the runs of a layout interleaved in both orders; every leg's patches are byte-equal.",
             "strided: one zn_patch_build_strided_batch_dev call, load order (ii) (along memory: the library's default).  workaround: contiguous() on every view + one zn_patch_build_batch_dev call.",
             "logical: the strided call of the library built with -DZN_PATCH_BUILD_LOGICAL_ORDER, load order (i)." if res["logical"] else "logical: NOT MEASURED (no library built with -DZN_PATCH_BUILD_LOGICAL_ORDER beside this one)",
             f"A/A spread (the largest (max - min) / min among the repeated runs of one leg on one layout): build calls {100 * sp:.1f} %, store builds {100 * spb:.1f} %"]
    for r in res["layouts"]:
        q, m = r["runs_ms"], r["median_ms"]
        lines.append(f"  {r['layout']:<11} " + "   ".join(f"{leg} " + " / ".join(f"{x:.3f}" for x in q[leg]) for leg in q))
        gain = 1.0 - m["strided"] / m["workaround"]
        verdict = "beats the workaround by more than the spread" if gain > sp else "LOSES to the workaround" if gain < -sp else "inside the spread of the workaround"
        lines.append(f"              medians: strided {m['strided']:.3f}, workaround {m['workaround']:.3f}: the strided call takes {m['strided'] / m['workaround']:.2f} of the workaround's time — {verdict}")
        if "logical" in m:
            g2 = 1.0 - m["strided"] / m["logical"]
            lines.append(f"              load order (ii) {m['strided']:.3f} against (i) {m['logical']:.3f}: {'(ii) wins by more than the spread' if g2 > sp else '(ii) LOSES by more than the spread' if g2 < -sp else 'inside the spread'}"
                         f"   [(i): {r['kernels']['logical']}]")
        b, pk = r["build_median_ms"], r["peak_bytes"]
        g3 = 1.0 - b["from_live"] / b["from_state_dict"]
        lines.append(f"              from_live " + " / ".join(f"{x:.1f}" for x in r["build_runs_ms"]["from_live"]) + "   from_state_dict on contiguous copies " + " / ".join(f"{x:.1f}" for x in r["build_runs_ms"]["from_state_dict"]) +
                     f" ms: {b['from_live'] / b['from_state_dict']:.3f} of its time — {'beats it by more than the spread' if g3 > spb else 'LOSES to it' if g3 < -spb else 'inside the spread'}; entries {r['kinds']}")
        lines.append(f"              peak allocated above the resting level: from_live {pk['from_live']} B, from_state_dict {pk['from_state_dict']} B")
        lines.append(f"              kernels: strided call [{r['kernels']['strided']}]  workaround [{r['kernels']['workaround']}]  from_live's last patch call [{r['kernels']['from_live']}]")
    lines += _load_order_decision(res)
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    json.dump(res, open(out + ".json", "w"), indent=1)
    print("\n".join(lines))
    return 0


def _load_order_decision(res):
    """The load-order decision of DESIGN §3.16 from this run's own numbers.  Rule: (ii), the block walked along memory, is the default only if it beats (i), the
    logical order, on the transposed layout by more than the run's A/A spread and loses on no other layout by more than that spread."""
    if not res["logical"]:
        return ["", "load-order decision: NOT MEASURED in this run (no logical-order library)"]
    sp = res["aa_spread"]
    gains = {r["layout"]: 1.0 - r["median_ms"]["strided"] / r["median_ms"]["logical"] for r in res["layouts"]}
    wins = gains["transposed"] > sp
    loses = [k for k, g in gains.items() if k != "transposed" and g < -sp]
    t = next(r for r in res["layouts"] if r["layout"] == "transposed")["median_ms"]
    out = ["", f"load-order decision (DESIGN §3.16), from this run; A/A spread of the build calls {100 * sp:.1f} %:",
           f"  transposed: (ii) {t['strided']:.3f} ms against (i) {t['logical']:.3f} ms ({t['logical'] / t['strided']:.1f} x): " + ("beyond the spread" if wins else "NOT beyond the spread"),
           "  the other layouts, (ii) against (i): " + ", ".join(f"{k} {100 * -g:+.1f} %" for k, g in gains.items() if k != "transposed") +
           (": none loses by more than the spread" if not loses else f": LOSES on {', '.join(loses)}"),
           "  -> " + ("(ii) is the default; (i) stays behind -DZN_PATCH_BUILD_LOGICAL_ORDER as the baseline" if wins and not loses else "the rule asks for (i)")]
    against = {r["layout"]: 1.0 - r["median_ms"]["strided"] / r["median_ms"]["workaround"] for r in res["layouts"]}
    out.append("  against the workaround (a gain or loss counts only beyond the spread): " +
               ", ".join(f"{k} {'gains' if g > sp else 'LOSES' if g < -sp else 'inside the spread'} ({100 * -g:+.1f} %)" for k, g in against.items()))
    return out


def main_index(args):
    results = {}
    for leg, limit in INDEX_LEG_SECONDS.items():
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--layers", str(args.layers), "--reps", str(args.reps)],
                           capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"leg {leg} failed (exit {p.returncode}); nothing further is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            return 1
        results[leg] = json.loads(line[0][7:])
        print(f"leg {leg}: ok", flush=True)
    out = args.out if args.out != os.path.join(ROOT, "profiles", "resident_decode") else os.path.join(ROOT, "profiles", "resident_index")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(results, open(out + ".json", "w"), indent=1)
    lines = ["sync index probe (ResidentCheckpoint.build_index): plan.run unhinted / hinted / unhinted / hinted on one store, device events, median ms; every result checked against its source",
             "(i) per dtype, 8 tensors of 128 MiB, N(0, 0.02):"]
    for r in results["i"]["dtypes"]:
        lines.append(f"    {r['dtype']:<14} unhinted {r['plain'][0]:.4f} / {r['plain'][1]:.4f}  hinted {r['hinted'][0]:.4f} / {r['hinted'][1]:.4f}  gain {100 * r['gain']:+.1f} %  (A/A spread {100 * r['aa_spread']:.1f} %)"
                     f"  index {r['index_bytes']} B = {100 * r['index_share']:.2f} % of the tensors, built in {r['build_s_per_gib']:.3f} s/GiB   [{r['kernels']['hinted']}]")
    j = results["j"]
    lines.append(f"(j) Llama-3-8B blocks (bf16), index {j['index_bytes']} B = {100 * j['index_bytes'] / j['nbytes']:.2f} %:")
    for r in j["blocks"]:
        lines.append(f"    block {r['block']}: unhinted {r['plain'][0]:.4f} / {r['plain'][1]:.4f}  hinted {r['hinted'][0]:.4f} / {r['hinted'][1]:.4f}  gain {100 * r['gain']:+.1f} %  (A/A spread {100 * r['aa_spread']:.1f} %)")
    f = j["forward_batch1"]
    lines.append(f"    forward of {args.layers} MLP blocks, batch 1: plain {f['plain_ms']:.3f} ms, hooked {f['hooked_ms']:.3f} / {f['hooked_again_ms']:.3f} ms, hooked with index {f['hooked_index_ms']:.3f} / {f['hooked_index_again_ms']:.3f} ms"
                 f"   [{f['hooked_index_kernels']}]")
    open(out + ".txt", "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--index", action="store_true", help="the sync index legs (i, j) instead of a-e")
    ap.add_argument("--delta", action="store_true", help="the variant store leg (k) instead of a-e")
    ap.add_argument("--digest", action="store_true", help="the content digest leg (m) instead of a-e")
    ap.add_argument("--delta-file", action="store_true", help="the delta file leg (n) instead of a-e")
    ap.add_argument("--delta-index", action="store_true", help="the DELTA sync index leg (p) instead of a-e")
    ap.add_argument("--sparse", action="store_true", help="the sparse variant leg (s) instead of a-e")
    ap.add_argument("--sparse-file", action="store_true", help="the sparse file leg (f) instead of a-e")
    ap.add_argument("--rebase", action="store_true", help="the patch merge / rebased leg (r) instead of a-e")
    ap.add_argument("--shard", action="store_true", help="the patch select / sharded leg (h) instead of a-e")
    ap.add_argument("--strided", action="store_true", help="the strided apply leg (t) instead of a-e")
    ap.add_argument("--capture", action="store_true", help="the strided build / from_live leg (c) instead of a-e")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_decode"))
    args = ap.parse_args()
    if args.leg:                                          # a child: one leg, its result as one JSON line
        print("RESULT " + json.dumps(globals()["leg_" + args.leg](args)))
        return 0
    if args.index:
        return main_index(args)
    if args.delta:
        return main_delta(args)
    if args.digest:
        return main_digest(args)
    if args.delta_file:
        return main_delta_file(args)
    if args.delta_index:
        return main_delta_index(args)
    if args.sparse:
        return main_sparse(args)
    if args.sparse_file:
        return main_sparse_file(args)
    if args.rebase:
        return main_rebase(args)
    if args.shard:
        return main_shard(args)
    if args.strided:
        return main_strided(args)
    if args.capture:
        return main_capture(args)
    results = {}
    for leg, limit in LEG_SECONDS.items():
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--layers", str(args.layers), "--reps", str(args.reps)],
                           capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"leg {leg} failed (exit {p.returncode}); nothing further is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            return 1
        results[leg] = json.loads(line[0][7:])
        print(f"leg {leg}: ok", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(results, open(args.out + ".json", "w"), indent=1)
    a, b, c, d, e = (results[k] for k in "abcde")
    lines = [f"resident checkpoint probe: {a['layers']} Llama-3-8B blocks, bf16 N(0, 0.02), every timed result checked against its source",
             f"(a) resident {a['resident_bytes']} of {a['original_bytes']} bytes: {a['ratio']:.4f}",
             "(b) plan.run per block (device events, median): " + ", ".join(f"{x['median_ms']:.3f} ms ({x['gb_per_s']:.0f} GB/s)" for x in b["blocks"])]
    for w in c["windows"]:
        lines.append(f"(c) {w['chunks']} chunks: window {w['window']['median_ms']:.4f} / {w['window_again']['median_ms']:.4f} ms, whole tensor {w['whole']['median_ms']:.4f} / {w['whole_again']['median_ms']:.4f} ms"
                     f"   [{w['window_kernels']} | {w['whole_kernels']}]")
    q = d["enqueue_while_busy"]
    lines.append(f"(d) host time to enqueue a block of {d['tensors_per_block']} tensors behind running decodes: plan.run {q['plan_run']['median_us']:.1f} us, batched call {q['batch_call']['median_us']:.1f} us (median)")
    for x in e["batches"]:
        lines.append(f"(e) forward of {e['layers']} MLP blocks, batch {x['batch']}: plain {x['plain']['median_ms']:.3f} ms, hooked {x['hooked']['median_ms']:.3f} ms")
    open(args.out + ".txt", "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
