"""CPU tests (-m "not gpu"): zipnn_amd.ResidentCheckpoint — a checkpoint kept compressed in "device" memory (CPU tensors, emulated kernels) — on a
file the REFERENCE wrote (tests/golden/gpt2_small_ref.znn.safetensors) and on state dicts; expected tensors are the sources."""
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpt2_small_ref.znn.safetensors")


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


@pytest.fixture()
def store(use_simt):
    from zipnn_amd import ResidentCheckpoint
    return ResidentCheckpoint.from_file(GOLDEN, "cpu")


def test_from_file_on_a_reference_written_checkpoint(use_simt, store):
    """Every tensor == what load_file returns (and what the plain safetensors reader + the per-tensor decoder give); get_tensors in one batched call,
    each decoded tensor at a multiple of 256 bytes of one buffer."""
    from zipnn_amd import safetensors_io
    want = safetensors_io.load_file(GOLDEN, device="cpu")
    assert sorted(store.keys()) == sorted(want.keys()) and len(store) == len(want)
    compressed = [k for k in store.keys() if store.info(k)["compressed"]]
    assert compressed and len(compressed) < len(want)                      # the file holds both kinds
    for k, v in want.items():
        i = store.info(k)
        assert i["shape"] == list(v.shape) and i["dtype"] == v.dtype and i["nbytes"] == v.numel() * v.element_size()
        assert _bytes_equal(store.get_tensor(k), v), k
    assert store.nbytes == sum(v.numel() * v.element_size() for v in want.values())
    assert store.resident_bytes == os.path.getsize(GOLDEN) - safetensors_io._read_layout(GOLDEN)[2] < store.nbytes
    into = torch.full((store.scratch_bytes(want.keys()) + 64,), 0x5A, dtype=torch.uint8)
    got = store.get_tensors(list(want.keys()), into=into[:-64])
    assert use_simt.last_kernels().count("zn_k_decode") >= 1
    for k, v in want.items():
        assert _bytes_equal(got[k], v), k
        if store.info(k)["compressed"]:
            assert (got[k].data_ptr() - into.data_ptr()) % 256 == 0
    assert bool((into[-64:] == 0x5A).all())
    out = torch.empty_like(want[compressed[0]])
    assert store.get_tensor(compressed[0], out=out) is out and _bytes_equal(out, want[compressed[0]])
    with pytest.raises(ValueError):
        store.get_tensor(compressed[0], out=torch.empty(3))
    with pytest.raises(KeyError):
        store.get_tensor("no.such.tensor")


def _check_slices(s, full, nbytes, chunk):
    rows, cols = full.shape
    K = -(-nbytes // chunk)
    assert s.get_shape() == [rows, cols] and s.get_dtype() in ("F32", "F16", "BF16")
    row_bytes = nbytes // rows
    for idx in (0, rows - 1, -2, slice(3, 11), slice(rows // 2, rows // 2 + 40), slice(5, rows - 3, 7), (slice(10, 20), slice(1, 5)), (rows // 3, 2),
                (slice(None), 3), slice(0, 0), Ellipsis, (slice(2, 30, 3), slice(None, None, 2))):
        assert _bytes_equal(s[idx], full[idx]), idx
        lo, hi = s.last_chunk_range
        first = idx[0] if isinstance(idx, tuple) else idx
        if isinstance(first, int):
            r = first % rows
            assert (lo, hi) == (r * row_bytes // chunk, -(-(r + 1) * row_bytes // chunk))
        elif isinstance(first, slice) and first != slice(None) and first.indices(rows)[1] > first.indices(rows)[0]:
            a, b, _ = first.indices(rows)
            assert (lo, hi) == (a * row_bytes // chunk, -(-b * row_bytes // chunk)) and hi - lo <= K
        elif first is Ellipsis or first == slice(None):
            assert (lo, hi) == (0, K)
        else:
            assert (lo, hi) == (0, 0)
    with pytest.raises(IndexError):
        s[rows]
    return K


def test_get_slice_on_the_reference_written_checkpoint(use_simt, store):
    """Ints, step-1 and step-k slices, trailing indices == the same index on the full tensor; last_chunk_range covers only the needed chunks."""
    from zipnn_amd import safetensors_io
    want = safetensors_io.load_file(GOLDEN, device="cpu")
    n = 0
    for name in store.keys():
        i = store.info(name)
        if i["compressed"] and len(i["shape"]) == 2 and i["shape"][0] >= 64:
            e = store._entries[name]
            _check_slices(store.get_slice(name), want[name], e.nbytes, e.chunk)
            n += 1
    assert n >= 1
    store.status()
    raw = next(k for k in store.keys() if not store.info(k)["compressed"])
    assert _bytes_equal(store.get_slice(raw)[...], want[raw])


def test_get_slice_decodes_only_the_chunks_it_needs(use_simt):
    """A matrix of many chunks (the ORACLE's body, 8 KiB chunks, a partial last one): a few rows decode a few chunks."""
    import oracle_lib as O
    from zipnn_amd.resident import ResidentCheckpoint, _Entry
    g = torch.Generator().manual_seed(11)
    full = (torch.randn(301, 173, generator=g) * 0.02).to(torch.bfloat16)
    data = full.view(torch.uint8).numpy().tobytes()
    body = torch.frombuffer(bytearray(O.compress_frame(b"", data, 2, 1, 10, 8192)), dtype=torch.uint8)
    store = ResidentCheckpoint("cpu", [_Entry("w", torch.bfloat16, full.shape, len(data), body=body, params=(2, 1, 10, 8192))], body.numel())
    s = store.get_slice("w")
    K = _check_slices(s, full, len(data), 8192)
    assert K == 13
    assert s[5:9].shape == (4, 173) and s.last_chunk_range == (0, 1)
    assert _bytes_equal(s[290:], full[290:]) and s.last_chunk_range == (12, 13)                   # ends in the partial last chunk
    assert _bytes_equal(s[100:160], full[100:160]) and s.last_chunk_range == (4, 7)
    store.status()
    assert _bytes_equal(store.get_tensor("w"), full)


def test_from_state_dict_round_trip_keeps_incompressible_tensors_raw(use_simt):
    from zipnn_amd import ResidentCheckpoint
    g = torch.Generator().manual_seed(5)
    sd = {"a.weight": (torch.randn(300, 257, generator=g) * 0.02).to(torch.bfloat16), "a.bias": (torch.randn(257, generator=g) * 0.02).to(torch.bfloat16),
          "b.weight": torch.randn(64, 100, generator=g) * 0.02, "c.half": (torch.randn(5000, generator=g) * 0.02).half(),
          "noise": torch.randint(0, 256, (40000,), generator=g, dtype=torch.uint8).view(torch.bfloat16),       # incompressible
          "ids": torch.arange(100), "empty": torch.empty(0, dtype=torch.bfloat16), "f8": (torch.randn(9000, generator=g) * 0.5).to(torch.float8_e4m3fn)}
    store = ResidentCheckpoint.from_state_dict(sd, "cpu")
    assert store.keys() == list(sd.keys())
    for k, v in sd.items():
        assert _bytes_equal(store.get_tensor(k), v), k
    assert not store.info("noise")["compressed"] and not store.info("ids")["compressed"] and not store.info("empty")["compressed"]
    assert store.info("a.weight")["compressed"] and store.info("b.weight")["compressed"] and store.info("f8")["compressed"]
    bound = sum((store.info(k)["resident_bytes"] + 255) // 256 * 256 if store.info(k)["compressed"] else store.info(k)["nbytes"] for k in sd)
    assert store.resident_bytes <= bound < store.nbytes
    got = store.get_tensors(list(sd.keys()))
    for k, v in sd.items():
        assert _bytes_equal(got[k], v), k


def test_plan_of_a_store(use_simt, store):
    from zipnn_amd import safetensors_io
    want = safetensors_io.load_file(GOLDEN, device="cpu")
    names = [k for k in store.keys() if store.info(k)["compressed"]][:6] + [k for k in store.keys() if not store.info(k)["compressed"]][:1]
    plan = store.plan(names)
    for _ in range(2):
        for t in plan.tensors.values():
            if t.is_floating_point() and t.numel():
                t.zero_()
        out = plan.run()
        plan.status()
        assert out is plan.tensors and list(out.keys()) == names
        for k in names:
            assert _bytes_equal(out[k], want[k]), k
    plan.close()
    with pytest.raises(RuntimeError):
        plan.run()


class _MLP(torch.nn.Module):
    def __init__(self, d, h, layers, dtype):
        super().__init__()
        self.blocks = torch.nn.ModuleList(torch.nn.Sequential(torch.nn.Linear(d, h + 8 * i), torch.nn.GELU(), torch.nn.Linear(h + 8 * i, d)) for i in range(layers))
        self.norm = torch.nn.LayerNorm(d)
        self.to(dtype)

    def forward(self, x):
        for b in self.blocks:
            x = x + b(x)
        return self.norm(x)


def test_hook_runs_a_model_from_the_store(use_simt):
    """hook(): outputs torch.equal to the plain model's; parameters hold no storage between forwards; one scratch buffer sized for the largest module;
    remove() restores ordinary parameters."""
    from zipnn_amd import ResidentCheckpoint
    torch.manual_seed(3)
    model = _MLP(96, 160, 3, torch.float32).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(4, 96)
    with torch.no_grad():
        ref = model(x)
    store = ResidentCheckpoint.from_state_dict(sd, "cpu")
    handle = store.hook(model)
    hooked = [p for n, p in model.named_parameters()]
    assert all(p.numel() == 0 for p in hooked)
    largest = max(store.scratch_bytes([f"blocks.{i}.{j}.weight", f"blocks.{i}.{j}.bias"]) for i in range(3) for j in (0, 2))
    assert handle.scratch.numel() == largest
    with torch.no_grad():
        for _ in range(2):
            assert torch.equal(model(x), ref)
            assert all(p.numel() == 0 for p in hooked)
    handle.status()
    handle.remove()
    for n, p in model.named_parameters():
        assert _bytes_equal(p.data, sd[n]), n
    with torch.no_grad():
        assert torch.equal(model(x), ref)
    # a subset of the modules
    handle = store.hook(model, modules=[model.blocks[1][0]])
    assert model.blocks[1][0].weight.numel() == 0 and model.blocks[0][0].weight.numel() > 0
    with torch.no_grad():
        assert torch.equal(model(x), ref)
    handle.remove()
    assert _bytes_equal(model.blocks[1][0].weight.data, sd["blocks.1.0.weight"])


class _Scaled(torch.nn.Module):
    """A module that owns a parameter AND calls a child that owns parameters, then uses its own."""

    def __init__(self, d):
        super().__init__()
        self.proj = torch.nn.Linear(d, d)
        self.scale = torch.nn.Parameter(torch.randn(d, d) * 0.1)
        self.inner = torch.nn.Sequential(torch.nn.Linear(d, d), torch.nn.Tanh())
        self.bias = torch.nn.Parameter(torch.randn(d) * 0.1)

    def forward(self, x):
        return self.inner(self.proj(x) @ self.scale) + self.bias


def test_hook_with_a_hooked_module_inside_a_hooked_module(use_simt):
    """A hooked module's own parameters stay valid while a hooked child (and grandchild) decodes: nested modules get disjoint regions of the scratch
    buffer, sized for the largest sum along a chain; modules that are not nested share it."""
    from zipnn_amd import ResidentCheckpoint
    torch.manual_seed(9)
    model = torch.nn.Sequential(_Scaled(64), _Scaled(64), torch.nn.Linear(64, 8)).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(5, 64)
    with torch.no_grad():
        ref = model(x)
    store = ResidentCheckpoint.from_state_dict(sd, "cpu")
    assert store.info("0.scale")["compressed"] and store.info("0.proj.weight")["compressed"]
    handle = store.hook(model)
    assert all(p.numel() == 0 for p in model.parameters())
    own = store.scratch_bytes(["0.scale", "0.bias"])
    deepest = max(store.scratch_bytes(["0.proj.weight", "0.proj.bias"]), store.scratch_bytes(["0.inner.0.weight", "0.inner.0.bias"]))
    assert handle.scratch.numel() == own + deepest            # parent + its largest hooked child; the second block and the head reuse the same bytes
    with torch.no_grad():
        for _ in range(2):
            assert torch.equal(model(x), ref)
            assert all(p.numel() == 0 for p in model.parameters())
    handle.remove()
    for n, p in model.named_parameters():
        assert _bytes_equal(p.data, sd[n]), n
