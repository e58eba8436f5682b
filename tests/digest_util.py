"""Shared by tests/test_digest_simt.py (emulated kernels, CPU tensors as device memory) and tests/test_gpu_digest.py (hardware): the cases of the content
digest ("zn64-1", include/zipnn_hip.h) and its checks against tests/digest_ref.py, an independent numpy restatement of the definition."""
import json
import os

import numpy as np
import torch

from digest_ref import digest_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpt2_small_ref.znn.safetensors")
K = 256 * 1024
SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 33, 1023, 1025, K - 4, K - 1, K, K + 1, K + 4, 2 * K + 3, 3 * K + 5)
OFFSETS = (0, 1, 2, 3, 5, 8, 13, 15)
CONTENTS = ("random", "zeros", "ones")

_MATRIX = {}


def matrix():
    """-> (host uint8 array, [(start, n)], [reference digest]): every size x byte offset x content as an item of ONE shared allocation whose other bytes are
    random — an item starts `offset` bytes behind a multiple of 256 and has random bytes right in front of it and right behind it, so that a kernel that
    reads past an item's ends gets the wrong answer.  Built (and its reference digests computed) once."""
    if not _MATRIX:
        rng = np.random.default_rng(20240607)
        spans, o = [], 256
        for content in CONTENTS:
            for off in OFFSETS:
                for n in SIZES:
                    spans.append((o + off, n, content))
                    o += (off + n + 255) // 256 * 256 + 256
        host = rng.integers(0, 256, o, dtype=np.uint8)
        host[host == 0] = 1                       # (no zero bytes around the items: a read past an all-zero item's end must not go unnoticed)
        for start, n, content in spans:
            if content != "random":
                host[start:start + n] = 0 if content == "zeros" else 0xFF
        _MATRIX["m"] = (host, [(s, n) for s, n, _ in spans], [digest_ref(host[s:s + n]) for s, n, _ in spans])
    return _MATRIX["m"]


def aligned_device_copy(host, dev):
    """host bytes -> a uint8 tensor on `dev` whose first byte lies at a multiple of 256."""
    raw = torch.empty(host.size + 512, dtype=torch.uint8, device=dev)
    a = (-raw.data_ptr()) % 256
    t = raw[a:a + host.size]
    t.copy_(torch.from_numpy(host))
    assert t.data_ptr() % 256 == 0
    return t


def device_digests(lib, flats, stream=None):
    from zipnn_amd import codec
    return codec.digests_to_ints(codec.digest_device_batch(lib, flats, stream))


def check_matrix(lib, dev):
    host, spans, want = matrix()
    buf = aligned_device_copy(host, dev)
    got = device_digests(lib, [buf[s:s + n] for s, n in spans])
    bad = [(s % 256, n, hex(g), hex(w)) for (s, n), g, w in zip(spans, got, want) if g != w]
    assert not bad, bad[:8]
    assert "zn_k_digest" in lib.last_kernels()
    return buf, spans, want


_RAGGED = {}


def ragged(count=300, top=600000):
    """-> (host array, [(start, n)], [reference digest]): `count` items of 1..top bytes, packed back to back (every byte alignment occurs)."""
    if not _RAGGED:
        rng = np.random.default_rng(5)
        sizes = rng.integers(1, top + 1, count)
        sizes[:4] = (1, top, K, K + 1)
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]) + 3
        host = rng.integers(0, 256, int(starts[-1] + sizes[-1]) + 64, dtype=np.uint8)
        spans = [(int(s), int(n)) for s, n in zip(starts, sizes)]
        _RAGGED["r"] = (host, spans, [digest_ref(host[s:s + n]) for s, n in spans])
    return _RAGGED["r"]


def check_ragged(lib, dev):
    """One launch for the whole batch == every item alone == the batch in reversed order == the reference."""
    host, spans, want = ragged()
    buf = aligned_device_copy(host, dev)
    flats = [buf[s:s + n] for s, n in spans]
    got = device_digests(lib, flats)
    assert got == want
    assert device_digests(lib, flats[::-1]) == want[::-1]
    for i in range(len(flats)):                     # (a single item is another host path: it travels as a kernel argument, with no table and no workspace)
        assert device_digests(lib, [flats[i]]) == [want[i]], i


def sensitivity_cases():
    """{case: bytes}: one base buffer of two blocks and a bit, and the small damages a content digest has to tell apart."""
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, 2 * K + 4096, dtype=np.uint8)
    out = {"base": base}

    def flipped(i, bit=0):
        b = base.copy()
        b[i] ^= 1 << bit
        return b
    out["flip first byte"] = flipped(0)
    out["flip last byte"] = flipped(base.size - 1, 7)
    out["flip last byte of block 0"] = flipped(K - 1)
    out["flip first byte of block 1"] = flipped(K)
    w = base.copy().view("<u4")
    assert w[10] != w[5000]
    w[[10, 5000]] = w[[5000, 10]]
    out["swap two words"] = w.view(np.uint8)
    b = base.copy()
    b[:K], b[K:2 * K] = base[K:2 * K], base[:K]
    out["swap two blocks"] = b
    out["zero byte appended"] = np.concatenate([base, np.zeros(1, dtype=np.uint8)])
    out["byte dropped"] = base[:-1].copy()
    return out


def check_sensitivity(lib, dev):
    cases = sensitivity_cases()
    names = list(cases)
    got = device_digests(lib, [aligned_device_copy(cases[n], dev) for n in names])
    assert got == [digest_ref(cases[n]) for n in names]
    assert len(set(got)) == len(names), dict(zip(names, map(hex, got)))
    # all-zero inputs of different lengths differ too (the length and the block count enter the digest)
    z = aligned_device_copy(np.zeros(2 * K, dtype=np.uint8), dev)
    zs = device_digests(lib, [z[:K - 4], z[:K], z[:2 * K]])
    assert len(set(zs)) == 3 and zs == [digest_ref(np.zeros(n, dtype=np.uint8)) for n in (K - 4, K, 2 * K)]


def _cpu_bytes(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8) if t.element_size() > 1 else t.detach().cpu().contiguous().view(torch.uint8).reshape(-1)


def check_golden_store(dev, want_tensors):
    """from_file(digests=True) on the reference-written checkpoint (it carries no digests: they are recorded from one decode): verify() passes with and
    without the sync index, digests() == the reference digest of every tensor."""
    from zipnn_amd import ResidentCheckpoint
    store = ResidentCheckpoint.from_file(GOLDEN, dev, digests=True)
    assert store.has_digests and sorted(store.digests()) == sorted(want_tensors)
    want = {k: digest_ref(_cpu_bytes(v).numpy()) for k, v in want_tensors.items()}
    assert store.digests() == want
    assert all(store.info(k)["digest"] == want[k] for k in want)
    res = store.verify()
    assert sorted(res) == sorted(want) and all(res.values())
    assert store.build_index() > 0
    assert all(store.verify().values())
    some = list(want)[:3]
    assert store.verify(some) == {k: True for k in some}
    plain = ResidentCheckpoint.from_file(GOLDEN, dev)
    assert not plain.has_digests and plain.info(some[0])["digest"] is None
    for call in (plain.digests, plain.verify, lambda: plain.holds({})):
        try:
            call()
        except ValueError as e:
            assert "digests" in str(e)
        else:
            raise AssertionError("a store without digests answered")
    return store


def check_clean_corruption(dev):
    """A flipped bit in a RAW plane decodes cleanly — no verdict of the decoder can see it — and only the digest tells."""
    from zipnn_amd import ResidentCheckpoint, DigestMismatch
    g = torch.Generator().manual_seed(3)
    sd = {"w": (torch.randn((3 * K + 10) // 2, generator=g) * 0.02).to(torch.bfloat16), "other": (torch.randn(70000, generator=g) * 0.02).to(torch.bfloat16),
          "ints": torch.arange(50, dtype=torch.int32)}
    store = ResidentCheckpoint.from_state_dict(sd, dev, digests=True)
    assert store.digests() == {k: digest_ref(_cpu_bytes(v).numpy()) for k, v in sd.items()}
    assert all(store.verify().values())
    e = store._entries["w"]
    assert e.compressed and e.chunks == 4 and e.P == 2
    assert int(e.body[0]) == 0                              # plane 0 of chunk 0 is stored raw (type 0): its payload is the tensor's own low bytes
    at = e.P * e.chunks * 9                                  # types (1 byte) and cumSizes (8 bytes) per (plane, chunk); then plane 0's payload
    good = int(e.body[at])
    e.body[at] = good ^ 0x10
    got = store.get_tensor("w", check=True)                  # decodes cleanly …
    assert not torch.equal(_cpu_bytes(got), _cpu_bytes(sd["w"]))      # … to wrong weights
    assert store.verify(raise_=False) == {"w": False, "other": True, "ints": True}
    try:
        store.verify()
    except DigestMismatch as ex:
        assert isinstance(ex, ValueError) and ex.names == ["w"] and "'w'" in str(ex)
    else:
        raise AssertionError("verify() passed a damaged store")
    e.body[at] = good
    assert all(store.verify().values())


def variant_state_dicts():
    """-> (base_sd, ft_sd) on the CPU, small enough for the emulator: the two tensors of a Linear(128, 96), an fp32 tensor, one
    the fine-tune leaves as it is ("same"), one whose values have nothing to do with the base's (a plain body), an int64 tensor, one the base lacks."""
    from resident_delta_util import _perturb
    g = torch.Generator().manual_seed(78)
    rn = lambda *s: torch.randn(*s, generator=g) * 0.02
    base = {"weight": rn(96, 128).to(torch.bfloat16), "bias": rn(96).to(torch.bfloat16), "w.fp32": rn(33, 508),
            "identical": rn(64, 128).to(torch.bfloat16), "unrelated": rn(128, 256).to(torch.bfloat16), "steps": torch.arange(40, dtype=torch.int64)}
    ft = {k: _perturb(v, 0.03, 200 + i) for i, (k, v) in enumerate(base.items()) if k not in ("identical", "unrelated", "steps")}
    ft["identical"] = base["identical"].clone()
    ft["unrelated"] = torch.rand(128, 256, generator=g).to(torch.bfloat16)
    ft["steps"] = base["steps"] + 5
    ft["absent"] = rn(40, 128).to(torch.bfloat16)
    return base, ft


def variant_model(sd, dev):
    m = torch.nn.Linear(128, 96).to(torch.bfloat16)
    m.load_state_dict({k: sd[k] for k in ("weight", "bias")})
    return m.to(dev)


def check_variant(dev):
    """A variant store with digests over a resident base with digests: verify, holds, guarded apply_ / revert_."""
    from zipnn_amd import ResidentCheckpoint, DigestMismatch
    base_sd, ft_sd = variant_state_dicts()
    model_of = variant_model
    base = ResidentCheckpoint.from_state_dict(base_sd, dev, digests=True)
    ft = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base, digests=True)
    assert ft.info("identical")["delta"] == "same" and ft.info("identical")["digest"] == base.info("identical")["digest"]
    assert ft.info("unrelated")["delta"] is False and ft.info("unrelated")["compressed"] and ft.info("w.fp32")["delta"] is True and ft.info("weight")["delta"] is True
    assert ft.digests() == {k: digest_ref(_cpu_bytes(v).numpy()) for k, v in ft_sd.items()}
    assert all(ft.verify().values()) and all(base.verify().values())
    model = model_of(base_sd, dev)
    names = sorted(n for n, _ in model.named_parameters())
    assert sorted(ft.holds(model)) == names and not any(ft.holds(model).values())
    assert all(base.holds(model).values())
    ft.apply_(model, guard=True)
    assert all(ft.holds(model).values()) and not any(base.holds(model).values())
    before = {n: _cpu_bytes(p).clone() for n, p in model.named_parameters()}
    try:
        ft.apply_(model, guard=True)
    except DigestMismatch as ex:
        assert sorted(ex.names) == names
    else:
        raise AssertionError("a second guarded apply_ went through")
    assert all(torch.equal(before[n], _cpu_bytes(p)) for n, p in model.named_parameters())      # untouched
    ft.revert_(model, guard=True)
    assert all(torch.equal(_cpu_bytes(p), _cpu_bytes(base_sd[n])) for n, p in model.named_parameters())
    try:
        ft.revert_(model, guard=True)
    except DigestMismatch:
        pass
    else:
        raise AssertionError("a guarded revert_ of base values went through")
    assert all(base.holds(model).values())
    # a base given as plain tensors has no recorded digests: the guard digests what it holds now
    small = ("weight", "bias", "identical", "steps")
    plain_base = {k: base_sd[k].to(dev).clone() for k in small}
    ft2 = ResidentCheckpoint.from_state_dict({k: ft_sd[k] for k in small}, dev, base=plain_base, digests=True)
    live = {n: base_sd[n].to(dev).clone() for n in small}
    ft2.apply_(live, guard=True)
    assert ft2.holds(live) == {n: True for n in live}
    try:
        ft2.apply_(live, guard=True)
    except DigestMismatch as ex:
        assert sorted(ex.names) == ["bias", "steps", "weight"]        # ("identical" holds the base's bytes either way)
    else:
        raise AssertionError("a second guarded apply_ went through")
    ft2.revert_(live, guard=True)
    assert all(torch.equal(_cpu_bytes(live[n]), _cpu_bytes(base_sd[n])) for n in live)
    no_digests = ResidentCheckpoint.from_state_dict({"steps": ft_sd["steps"]}, dev, base=plain_base)
    try:
        no_digests.apply_(live, guard=True)
    except ValueError as ex:
        assert "digests" in str(ex)
    else:
        raise AssertionError("a guard without digests went through")


def small_state_dict():
    g = torch.Generator().manual_seed(21)
    return {"a.weight": (torch.randn(300, 512, generator=g) * 0.02).to(torch.bfloat16), "a.bias": (torch.randn(511, generator=g) * 0.02).to(torch.bfloat16),
            "b.weight": torch.randn(129, 508, generator=g) * 0.02, "noise": torch.randint(0, 256, (70001,), generator=g, dtype=torch.uint8).view(torch.int8),
            "steps": torch.arange(33, dtype=torch.int64), "empty": torch.zeros(0, dtype=torch.float32)}


def read_container(path):
    """-> (header dict, data section bytes) of a safetensors file."""
    with open(path, "rb") as f:
        n = int.from_bytes(f.read(8), "little")
        hdr = json.loads(f.read(n))
        return hdr, f.read()


def check_files(tmp_path, device):
    """compress_safetensors_file(digests=True) -> load_file(verify=True); one flipped data byte of a stored-raw tensor raises, naming it; the default file has
    no digests and is otherwise the same file; verify=True without digests is an error."""
    from safetensors.torch import save_file
    from zipnn_amd import safetensors_io, DigestMismatch
    sd = small_state_dict()
    src = str(tmp_path / "m.safetensors")
    save_file(sd, src, {"format": "pt", "note": "digest test"})
    with_d = safetensors_io.compress_safetensors_file(src, str(tmp_path / "with.znn.safetensors"), device=device, digests=True)
    without = safetensors_io.compress_safetensors_file(src, str(tmp_path / "without.znn.safetensors"), device=device)
    h1, d1 = read_container(with_d)
    h0, d0 = read_container(without)
    assert safetensors_io.DIGESTS_KEY not in h0["__metadata__"]
    rec = json.loads(h1["__metadata__"].pop(safetensors_io.DIGESTS_KEY))
    assert h1 == h0 and list(h1) == list(h0) and d1 == d0
    assert rec["algo"] == "zn64-1" and rec["tensors"] == {k: f"{digest_ref(_cpu_bytes(v).numpy()):016x}" for k, v in sd.items()}
    assert "znn_compressed_vectors" in h0["__metadata__"] or any(e["dtype"] == "U8" for k, e in h0.items() if k != "__metadata__")
    got = safetensors_io.load_file(with_d, device=device, verify=True)
    assert all(torch.equal(_cpu_bytes(got[k]), _cpu_bytes(v)) for k, v in sd.items())
    try:
        safetensors_io.load_file(without, device=device, verify=True)
    except ValueError as ex:
        assert "no digests" in str(ex) and not isinstance(ex, DigestMismatch)
    else:
        raise AssertionError("verify=True passed a file without digests")
    # one data byte of a tensor that is stored as it is ("noise": int8, never compressed)
    lo = h1["noise"]["data_offsets"][0]
    assert h1["noise"]["dtype"] == "I8"
    raw = bytearray(open(with_d, "rb").read())
    raw[len(raw) - len(d1) + lo + 17] ^= 0x04
    damaged = str(tmp_path / "damaged.znn.safetensors")
    open(damaged, "wb").write(raw)
    safetensors_io.load_file(damaged, device=device)                 # loads without complaint …
    try:
        safetensors_io.load_file(damaged, device=device, verify=True)
    except DigestMismatch as ex:
        assert ex.names == ["noise"] and "noise" in str(ex)
    else:
        raise AssertionError("verify=True passed a damaged file")
    # an algorithm this library does not know
    hdr, data = read_container(with_d)
    hdr["__metadata__"][safetensors_io.DIGESTS_KEY] = json.dumps({"algo": "zn64-9", "tensors": rec["tensors"]})
    js = json.dumps(hdr, separators=(",", ":")).encode()
    js += b" " * (-len(js) % 8)
    unknown = str(tmp_path / "unknown.znn.safetensors")
    open(unknown, "wb").write(len(js).to_bytes(8, "little") + js + data)
    try:
        safetensors_io.load_file(unknown, device=device, verify=True)
    except ValueError as ex:
        assert "zn64-9" in str(ex)
    else:
        raise AssertionError("an unknown digest algorithm passed")
    return with_d, without, sd
