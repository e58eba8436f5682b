"""GPU tests (-m gpu): decode hints (include/zipnn_hip.h) on the real libzipnn_hip.so — a ResidentCheckpoint with an index decodes to the
source bytes and to what the same store decodes without it, the device builds the hints the emulated library builds, and hints are advice.  Small calls take
the wide kernel, which reads no hints: the fused form is forced for these tests."""
import numpy as np
import pytest
import torch

import oracle_lib as O
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
