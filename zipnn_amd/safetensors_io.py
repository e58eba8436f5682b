"""Tensor-by-tensor safetensors compression (the file producer/consumer either side of the hot path;
SURVEY.md §8f-1).  Same file layout as the reference's scripts/zipnn_compress_safetensors.py:37-148 and
scripts/zipnn_decompress_safetensors.py:34-136: every floating-point tensor that shrinks is stored as a
1-D uint8 tensor holding one TORCH-format ZN frame, and listed (dtype, shape) in the file metadata under
`znn_compressed_vectors`; everything else is stored untouched.  Suffix: `.znn.safetensors`.
"""
import os
import struct

import torch

from .zipnn import (COMPRESSED_DTYPE, COMPRESSION_METHOD, METADATA_KEY, ZipNN, build_compressed_tensor_info,
                    get_compressed_tensors_metadata, set_compressed_tensors_metadata)

SUFFIX = ".znn.safetensors"
_DIGEST_GROUP_BYTES = 256 << 20      # compress_safetensors_file(digests=True), per-tensor path: tensors are digested as they are read, in groups of at most this many bytes
DIGESTS_KEY = "znn_digests"          # file metadata: a JSON string {"algo": "zn64-1", "tensors": {name: 16 hex digits}} — digests of the DECODED bytes of every tensor
DELTA_KEY = "znn_delta"              # file metadata of a DELTA file: a JSON string {"version": 1 | 2, "algo": "zn64-1",
                                     # "tensors": {name: "delta" | "same" | "sparse"}, "base_digests": {name: 16 hex digits}} — which tensors are coded over a base and
                                     # how, and the digests of that base's tensors.  Version 2 is written exactly when a tensor is "sparse" (a "znp1" patch in an entry
                                     # of L + 15 bytes, SPARSE_SLACK); a file without one is version 1, byte for byte what it was before there were patches in files.
DELTA_VERSION = 1
DELTA_VERSION_SPARSE = 2
SPARSE_SLACK = 15                    # a "sparse" entry is the patch plus this many zero bytes: the patch starts at the entry's first 16-byte boundary of the data section


def read_metadata(filename):
    """The `__metadata__` dict of a safetensors container ({} when it has none)."""
    import json
    with open(filename, "rb") as f:
        n = int.from_bytes(f.read(8), "little")
        return dict(json.loads(f.read(n)).get("__metadata__") or {})


def file_digests(metadata):
    """-> {name: digest} from a file's metadata, or None when it carries none.  An algorithm this library does not know is an error."""
    import json
    from . import codec
    raw = metadata.get(DIGESTS_KEY)
    if raw is None:
        return None
    d = json.loads(raw)
    if d.get("algo") != codec.DIGEST_ALGO:
        raise ValueError(f"{DIGESTS_KEY}: unknown digest algorithm {d.get('algo')!r} (this library knows {codec.DIGEST_ALGO!r})")
    return {name: int(h, 16) for name, h in d["tensors"].items()}


def file_delta(metadata):
    """-> ({name: "delta" | "same" | "sparse"}, {name: digest of the BASE tensor's bytes}) from a delta file's metadata, or None for a file that is no delta file.
    A version or a digest algorithm this library does not know, a "sparse" entry in a version 1 file, or an entry without its base digest, is an error."""
    import json
    from . import codec
    raw = metadata.get(DELTA_KEY)
    if raw is None:
        return None
    d = json.loads(raw)
    if d.get("version") not in (DELTA_VERSION, DELTA_VERSION_SPARSE):
        raise ValueError(f"{DELTA_KEY}: unknown version {d.get('version')!r} (this library knows {DELTA_VERSION} and {DELTA_VERSION_SPARSE})")
    if d.get("algo") != codec.DIGEST_ALGO:
        raise ValueError(f"{DELTA_KEY}: unknown digest algorithm {d.get('algo')!r} (this library knows {codec.DIGEST_ALGO!r})")
    kinds = dict(d.get("tensors") or {})
    known = ("delta", "same") if d.get("version") == DELTA_VERSION else ("delta", "same", "sparse")
    odd = [n for n, k in kinds.items() if k not in known]
    if odd:
        raise ValueError(f"{DELTA_KEY}: {odd[0]!r} is {kinds[odd[0]]!r}: a version {d.get('version')} file knows " + ", ".join(f'"{k}"' for k in known))
    base = {name: int(h, 16) for name, h in (d.get("base_digests") or {}).items()}
    missing = [n for n in kinds if n not in base]
    if missing:
        raise ValueError(f"{DELTA_KEY}: base_digests lacks {missing[:3]}{' …' if len(missing) > 3 else ''}")
    return kinds, base


def _delta_over_base(filename, metadata, kinds, based):
    """The tensors a delta file codes over its base, checked against that base before anything is uploaded.  kinds: file_delta's; based: {name: what the base
    holds under that name, with .dtype, .shape and .fits(dtype, shape)} -> {name: (dtype, shape, based[name])}, the dtype and shape as `znn_compressed_vectors`
    gives them.  A ValueError names the tensor that is listed but not compressed, has an unknown dtype, or that the base lacks or holds with another dtype or shape."""
    import json
    infos, over = get_compressed_tensors_metadata(metadata), {}
    for name in kinds:
        if name not in infos:
            raise ValueError(f"{filename}: {name!r} is listed under znn_delta but not under znn_compressed_vectors")
        dt, shape = getattr(torch, str(infos[name].get("dtype")), None), tuple(int(d) for d in json.loads(infos[name].get("shape", "[]")))
        if not isinstance(dt, torch.dtype):
            raise ValueError(f"{filename}: {name!r}: unknown dtype {infos[name].get('dtype')!r}")
        ref = based.get(name)
        if ref is None:
            raise ValueError(f"{filename}: the base has no tensor {name!r}, which the file codes over it")
        if not ref.fits(dt, shape):
            raise ValueError(f"{filename}: {name!r} is {dt} {list(shape)} over a base tensor of the same dtype and shape; the base holds {ref.dtype} {list(ref.shape)}")
        over[name] = (dt, shape, ref)
    return over


def _set_delta_metadata(metadata, kinds, base_digests):
    import json
    from . import codec
    version = DELTA_VERSION_SPARSE if "sparse" in kinds.values() else DELTA_VERSION
    metadata[DELTA_KEY] = json.dumps({"version": version, "algo": codec.DIGEST_ALGO, "tensors": dict(kinds),
                                      "base_digests": {n: f"{base_digests[n]:016x}" for n in kinds}})


def _needs_base(filename):
    return ValueError(f"{filename}: a delta file ({DELTA_KEY}): its tensors are coded over a base — load it with load_file(base=) / ResidentCheckpoint.from_file(base=)")


def _sparse_patch_at(lo):
    """-> where the patch of a "sparse" entry that starts at `lo` lies: the entry's first multiple of 16 — offsets of the DATA SECTION, which a reader uploads
    to an aligned allocation — with zero bytes around it, SPARSE_SLACK in all."""
    return (lo + 15) // 16 * 16


def _save_with_sparse_entries(tensors, path, metadata, patches):
    """safetensors' save_file, then the "sparse" entries filled in -> path.  patches: {name: the patch's bytes}; tensors[name] is that entry zero-filled
    (len(patch) + SPARSE_SLACK bytes).  safetensors decides where an entry lies: the file is written under a temporary name, the patches are put at their places
    (_sparse_patch_at), and the file is renamed to `path`."""
    from safetensors.torch import save_file as st_save_file
    if not patches:
        st_save_file(tensors, path, metadata)
        return path
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        st_save_file(tensors, tmp, metadata)
        _, layout, data_start = _read_layout(tmp)
        with open(tmp, "r+b") as f:
            for name, mv in patches.items():
                lo, hi = layout[name][2], layout[name][3]
                at = _sparse_patch_at(lo)
                assert hi - lo == len(mv) + SPARSE_SLACK and at + len(mv) <= hi
                f.seek(data_start + at)
                f.write(mv)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def _read_sparse_entries(filename, lay, over, check_slack):
    """The "sparse" entries of a delta file, from the file alone, before anything is uploaded.  lay: _read_layout(filename); over: {name: (dtype, shape)} ->
    {name: (offset of the patch in the data section, L, elem)}.  The patch starts at _sparse_patch_at of its entry; its header must describe the tensor and give
    the entry's length; check_slack: the up to 15 bytes of the entry around the patch must be zero.  A ValueError names the tensor."""
    if not over:
        return {}
    import math
    from . import _capi
    _, layout, data_start = lay
    lib, out = _capi.lib(), {}
    with open(filename, "rb") as f:
        for name, (dt, shape) in over.items():
            fdt, _, lo, hi = layout[name]
            elem = torch.empty(0, dtype=dt).element_size()
            n = elem * math.prod(int(d) for d in shape)
            at = _sparse_patch_at(lo)
            if fdt != torch.uint8 or hi - lo < 32 + SPARSE_SLACK:
                raise ValueError(f"{filename}: {name!r} is listed as \"sparse\" but its entry of {hi - lo} bytes cannot hold a patch")
            f.seek(data_start + lo)
            slack = f.read(at - lo)
            head = f.read(32)
            T, L = int.from_bytes(head[16:24], "little"), int.from_bytes(head[24:32], "little")
            if head[:4] != b"ZNP1" or head[4] != elem or int.from_bytes(head[8:16], "little") != n:
                raise ValueError(f"{filename}: {name!r}: the patch's header does not describe a {dt} tensor of {n} bytes")
            if hi - lo != L + SPARSE_SLACK:
                raise ValueError(f"{filename}: {name!r}: an entry of {hi - lo} bytes for a patch of {L} (the entry is the patch and {SPARSE_SLACK} bytes)")
            if T > n // elem or lib.patch_len(n, elem, T) != L:
                raise ValueError(f"{filename}: {name!r}: {L} bytes is not the length of a patch of {T} elements")
            if check_slack:
                f.seek(data_start + at + L)
                if any(slack) or any(f.read(hi - at - L)):
                    raise ValueError(f"{filename}: {name!r}: the bytes around the patch are not zero")
            out[name] = (at, L, elem)
    return out


def _set_digests_metadata(metadata, names, values):
    import json
    from . import codec
    metadata[DIGESTS_KEY] = json.dumps({"algo": codec.DIGEST_ALGO, "tensors": {n: f"{v:016x}" for n, v in zip(names, values)}})


def check_digests(tensors, want, what):
    """tensors: {name: tensor} as decoded; want: {name: digest}.  Device tensors: one batched launch; CPU tensors: the host function.  Raises DigestMismatch."""
    from . import codec
    names = list(tensors.keys())
    missing = [n for n in names if n not in want]
    if missing:
        raise ValueError(f"{what}: {DIGESTS_KEY} lacks {missing[:3]}{' …' if len(missing) > 3 else ''}")
    got = codec.digest_many([tensors[n] for n in names])
    bad = [n for n, g in zip(names, got) if g != want[n]]
    if bad:
        raise codec.DigestMismatch(bad, f"{what}: decoded bytes differ from the file's digests")


def compress_safetensors_file(filename, out_path=None, device="cpu", method=None, batched=None, digests=False, base=None, sparse=False):
    """-> path of the compressed file.  `device` = where tensors are staged for compression
    ("cuda:N" compresses in HBM; the compressed frames come back to the host for writing).  Tensors staged in HBM
    are compressed by ONE batched call for the whole file (`batched=None`: automatic; True forces it).
    digests=True: the metadata also gets `znn_digests`, the content digest ("zn64-1") of every tensor's bytes, compressed or not, taken from the SOURCE
    tensors (on the device path in one launch over the uploaded data section; on the per-tensor path as they are read, a group of at most 256 MiB — or one larger
    tensor — at a time, which is all the option holds beyond the compression's own memory): load_file(..., verify=True) and ResidentCheckpoint.from_file check decodes against
    it.  Readers that do not know the key ignore it; with the default the file is byte for byte what it was without this option.
    base: write a DELTA file over it — a path to the base's `.safetensors` or `.znn.safetensors`, a ResidentCheckpoint on the device, or a mapping
    of names to device tensors: the file's tensors go to the device, become a variant store over the base (ResidentCheckpoint.from_state_dict(base=)) and that
    store is saved (ResidentCheckpoint.save_file).  A device is needed for it: with device="cpu" the current GPU is used.
    sparse=True (with base): tensors with few changed elements become "znp1" patches (from_state_dict(sparse=True)) and are written as such (save_file(sparse=True),
    DESIGN §3.11)."""
    from safetensors import safe_open
    from safetensors.torch import save_file
    assert filename.endswith(".safetensors")
    out_path = out_path or filename[: -len(".safetensors")] + SUFFIX
    if base is not None:
        return _compress_file_over_base(filename, out_path, device, method, digests, base, sparse)
    if torch.device(device).type == "cuda" and batched is not False:
        done = _compress_file_on_device(filename, out_path, torch.device(device), method, digests)
        if done is not None:
            return done
    tensors, infos = {}, {}
    batch = []                                        # (name, tensor, header, planes, bits, bytes, chunk)
    recorded, pending, pending_bytes = {}, [], 0      # digests=True: the tensors as read are digested in groups of at most _DIGEST_GROUP_BYTES (or one larger tensor) …

    def digest_pending():
        from . import codec
        recorded.update(zip([n for n, _ in pending], codec.digest_many([t for _, t in pending])))
        pending.clear()
    with safe_open(filename, "pt", device) as f:
        for name in f.keys():
            t = f.get_tensor(name)
            if digests:                               # (… so that no more than a group is held beyond what the compression itself keeps)
                if pending and pending_bytes + t.numel() * t.element_size() > _DIGEST_GROUP_BYTES:
                    digest_pending()
                    pending_bytes = 0
                pending.append((name, t))
                pending_bytes += t.numel() * t.element_size()
            if not torch.is_floating_point(t) or t.dtype == torch.float64 or t.numel() == 0:
                tensors[name] = t.cpu()
                continue
            znn = ZipNN(input_format="torch", bytearray_dtype=t.dtype, method=method or COMPRESSION_METHOD)
            if t.is_cuda if batched is None else batched:
                batch.append((name, t) + znn.torch_frame_plan(t) + (znn.compression_threshold,))
                continue
            frame = znn.compress(t)                       # our compress never modifies `t`
            if len(frame) >= t.element_size() * t.nelement():
                tensors[name] = t.cpu()
                continue
            tensors[name] = torch.frombuffer(bytearray(frame), dtype=COMPRESSED_DTYPE)
            infos[name] = build_compressed_tensor_info(t)
        metadata = dict(f.metadata() or {})
        if pending:
            digest_pending()
    if batch:
        # tensors staged in HBM: one batched compress for the whole file (zn_compress_batch_dev)
        from . import _capi, codec
        bodies = codec.compress_device_batch(_capi.lib(), [(codec.flat_bytes(t), P, bits, byts, chunk, th) for (_, t, _, P, bits, byts, chunk, th) in batch])
        for (name, t, hdr, *_), body in zip(batch, bodies):
            total = len(hdr) + body.numel()
            if total >= t.element_size() * t.nelement():
                tensors[name] = t.cpu()
                continue
            frame = codec.new_bytearray(total)
            frame[:len(hdr)] = hdr
            frame[24:32] = total.to_bytes(8, "little")     # what the core writes at zipnn_core.c:121
            codec.to_host(_capi.lib(), body, memoryview(frame)[len(hdr):])
            tensors[name] = torch.frombuffer(frame, dtype=COMPRESSED_DTYPE)
            infos[name] = build_compressed_tensor_info(t)
    if not metadata:
        metadata = {"format": "pt"}                       # the reference silently drops the list when a file has no metadata
    set_compressed_tensors_metadata(infos, metadata)
    if digests:
        _set_digests_metadata(metadata, list(recorded.keys()), list(recorded.values()))
    save_file(tensors, out_path, metadata)
    return out_path


def _base_store(base, dev):
    """`base` given as a path -> a resident store of that file (plain or compressed) on `dev`; anything else as it is."""
    if isinstance(base, (str, os.PathLike)):
        from .resident import ResidentCheckpoint
        return ResidentCheckpoint.from_file(os.fspath(base), dev)
    return base


def _compress_file_over_base(filename, out_path, device, method, digests, base, sparse=False):
    """compress_safetensors_file(base=): file -> delta file, through the store path (no second writer)."""
    from . import codec
    from .resident import ResidentCheckpoint
    dev = torch.device(device)
    if dev.type != "cuda" and torch.cuda.is_available():
        dev = torch.device("cuda", codec.current_device())
    dev = ResidentCheckpoint._work_device(dev)
    tensors = load_file(filename, dev)
    store = ResidentCheckpoint.from_state_dict(tensors, dev, method=method, base=_base_store(base, dev), digests=bool(digests), sparse=bool(sparse))
    del tensors
    return store.save_file(out_path, digests=bool(digests), metadata=read_metadata(filename) or None, sparse=bool(sparse))


def save_file(tensors, filename, device="cuda:0", base=None, digests=False, metadata=None, sparse=False):
    """safetensors.torch.save_file for live tensors, compressed: ResidentCheckpoint.from_state_dict(tensors, device, base=base, digests=digests, sparse=sparse)
    followed by its save_file — with `base` (a store on the device, a mapping of device tensors, a module) a DELTA file over it, with sparse=True
    one whose tensors with few changed elements are patches.  -> filename."""
    from .resident import ResidentCheckpoint
    store = ResidentCheckpoint.from_state_dict(tensors, device, base=base, digests=bool(digests), sparse=bool(sparse))
    return store.save_file(filename, digests=bool(digests), metadata=metadata, sparse=bool(sparse))


def _compress_file_on_device(filename, out_path, dev, method, digests=False):
    """compress_safetensors_file with the tensors staged in HBM, the way decode_file_on_device loads: the file's data section crosses PCIe ONCE
    (pinned multi-threaded upload of the mapping), ONE batched compress writes every body into one arena — each behind a 256-byte gap —, the
    arena comes back in ONE transfer and the frame headers are written into the gaps on the host: the frames handed to safetensors are views of that one
    buffer.  (Per tensor — safe_open + get_tensor in, one transfer per body out — the same file took 35 + 64 ms for these two legs; now ≈ 10 + 10.)
    -> out_path, or None when the container names a dtype this parser does not know (the caller falls back to the per-tensor path)."""
    import contextlib
    import mmap
    import threading
    from safetensors.torch import save_file
    from . import _capi, codec
    from .zipnn import dtype_from_user
    lay = _read_layout(filename)
    if lay is None:
        return None
    metadata, layout, data_start = lay
    metadata = dict(metadata)
    lib = _capi.lib()
    from safetensors import safe_open
    with safe_open(filename, "pt", "cpu") as f0:                  # (header only: the order the per-tensor path walks the names in — the metadata list keeps it)
        order = [n for n in f0.keys() if n in layout]
    if len(order) != len(layout):
        return None
    with open(filename, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if size else None
    view = memoryview(mm) if mm is not None else None
    tensors, infos, batch = {}, {}, []
    try:
        for name in order:
            dt, shape, lo, hi = layout[name]
            numel = 1
            for d in shape:
                numel *= int(d)
            if not dt.is_floating_point or dt == torch.float64 or numel == 0 or dtype_from_user(dt) is None:
                tensors[name] = torch.frombuffer(bytearray(view[data_start + lo: data_start + hi]), dtype=dt).reshape(shape) if hi > lo else torch.empty(shape, dtype=dt)
                continue
            znn = ZipNN(input_format="torch", bytearray_dtype=dt, method=method or COMPRESSION_METHOD)
            like = torch.empty(shape, dtype=dt, device="meta")                   # (dtype and shape are all the frame plan looks at)
            batch.append((name, lo, hi, like) + znn.torch_frame_plan(like) + (znn.compression_threshold,))
        blob = codec.to_device(lib, view[data_start:], dev) if (view is not None and size > data_start) else torch.empty(0, dtype=torch.uint8, device=dev)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
    finally:
        if view is not None:
            view.release()
        if mm is not None:
            def _close_mapping():
                with contextlib.suppress(BufferError):
                    mm.close()
            closer = threading.Thread(target=_close_mapping, daemon=True)      # (munmap behind the multi-threaded upload: 1.2 ms, see decode_file_on_device)
            closer.start()
            _PENDING_CLOSERS.append(closer)
    if batch:
        GAP = 256 * ((max(len(b[4]) for b in batch) + 255) // 256)              # room for the longest frame header in front of every body
        arena, offs, lens = codec.compress_device_batch(lib, [(blob[lo:hi], P, bits, byts, chunk, th) for (_, lo, hi, _, _, P, bits, byts, chunk, th) in batch],
                                                       gap=GAP, return_arena=True)
        end = max(o + n for o, n in zip(offs, lens))
        # one transfer: every body (and the unused tail of every slot in between), into a block of the library's pinned arena (one DMA, no page faults, nothing to munmap)
        host = codec.to_host(lib, arena[:end], out=lib.host_buffer(end))
        hv = memoryview(host).cast("B")
        for (name, lo, hi, like, hdr, *_), o, n in zip(batch, offs, lens):
            total = len(hdr) + n
            if total >= hi - lo:                                                   # did not shrink: stored as it was
                tensors[name] = blob[lo:hi].cpu().view(like.dtype).reshape(like.shape)
                continue
            s0 = o - len(hdr)
            hv[s0:o] = bytes(hdr)
            hv[s0 + 24: s0 + 32] = total.to_bytes(8, "little")                     # what the core writes at zipnn_core.c:121
            tensors[name] = torch.frombuffer(host, dtype=COMPRESSED_DTYPE, offset=s0, count=total)
            infos[name] = build_compressed_tensor_info(like)
    if not metadata:
        metadata = {"format": "pt"}                                                # the reference silently drops the list when a file has no metadata
    set_compressed_tensors_metadata(infos, metadata)
    if digests:
        # every tensor where the upload put it (safetensors aligns nothing: the kernel takes any byte address), one launch for the file
        flats = [blob[layout[name][2]:layout[name][3]] for name in order]
        _set_digests_metadata(metadata, order, codec.digests_to_ints(codec.digest_device_batch(lib, flats)) if flats else [])
    save_file({name: tensors[name] for name in order}, out_path, metadata)
    return out_path


def decompress_safetensors_file(filename, out_path=None, device="cpu"):
    """Inverse of compress_safetensors_file -> path of the plain .safetensors file."""
    from safetensors import safe_open
    from safetensors.torch import save_file
    assert filename.endswith(SUFFIX)
    out_path = out_path or filename[: -len(SUFFIX)] + ".safetensors"
    tensors = {}
    with safe_open(filename, "pt", "cpu") as f:
        metadata = dict(f.metadata() or {})
        infos = get_compressed_tensors_metadata(metadata)
        for name in f.keys():
            t = f.get_tensor(name)
            if name in infos:
                znn = ZipNN(input_format="torch", bytearray_dtype=COMPRESSED_DTYPE, method=COMPRESSION_METHOD)
                t = znn.decompress(t, decompress_cpu_gpu=device)
            tensors[name] = t.cpu() if isinstance(t, torch.Tensor) else t
    metadata.pop(METADATA_KEY, None)
    save_file(tensors, out_path, metadata or None)
    return out_path


_ST_DTYPES = {"F64": torch.float64, "F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16, "I64": torch.int64, "I32": torch.int32,
              "I16": torch.int16, "I8": torch.int8, "U8": torch.uint8, "BOOL": torch.bool, "F8_E4M3": getattr(torch, "float8_e4m3fn", None),
              "F8_E5M2": getattr(torch, "float8_e5m2", None), "U16": getattr(torch, "uint16", None), "U32": getattr(torch, "uint32", None),
              "U64": getattr(torch, "uint64", None)}


def _read_layout(filename):
    """The safetensors container itself: 8-byte little-endian header length, a JSON header {name: {dtype, shape, data_offsets}}
    (+ "__metadata__"), then the tensors' bytes back to back.  -> (metadata, {name: (dtype, shape, lo, hi)}, data_start), or None
    when the header names a dtype this loader does not know (the per-tensor path then reads the file through safetensors)."""
    import json
    with open(filename, "rb") as f:
        n = int.from_bytes(f.read(8), "little")
        hdr = json.loads(f.read(n))
    meta = hdr.pop("__metadata__", None) or {}
    layout = {}
    for name, e in hdr.items():
        dt = _ST_DTYPES.get(e["dtype"])
        if dt is None:
            return None
        layout[name] = (dt, tuple(e["shape"]), int(e["data_offsets"][0]), int(e["data_offsets"][1]))
    return meta, layout, 8 + n


def _contiguous_strides(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.append(acc)
        acc *= max(int(d), 1)
    return tuple(reversed(st))


_PENDING_CLOSERS = []      # helper threads still unmapping the file of an earlier decode_file_on_device call


def decode_file_on_device(filename, device, compressed_only=False, timings=None, use_arena=None):
    """The batched loader behind load_file and behind the plugin's read-ahead (SafeOpen.get_tensor): the file's data section
    crosses PCIe ONCE, as it lies on disk, through the library's pinned multi-threaded transfer; every compressed tensor is then
    decoded by ONE batched launch (zn_decompress_batch_dev) from where its frame landed in HBM into one output arena (every
    tensor at a 256-byte boundary of it).  All frame headers are parsed from the host mapping before anything moves — one pass over
    the mmap with zipnn.fast_frame_params, no ZipNN object and no device read-back per tensor — and the bodies and destinations
    go to the library as plain addresses.  -> {name: tensor} (with compressed_only: the compressed tensors alone), or None when the
    container names a dtype this parser does not know.
    The uncompressed tensors of the file are COPIED out of the uploaded section, so that nothing keeps the compressed bytes
    resident once the decode has run; the decoded tensors share the arena (they live and die together in a model load; set
    ZIPNN_AMD_LOAD_ARENA=0, or pass use_arena=False, for one allocation per tensor — what the plugin's read-ahead does, whose
    consumers may keep any subset of a shard)."""
    from . import _capi, codec
    up = _upload_file(filename, device)
    if up is None:
        return None
    if use_arena is None:                              # (load_file: everything is returned together; SafeOpen's read-ahead passes False)
        use_arena = os.environ.get("ZIPNN_AMD_LOAD_ARENA", "1") != "0"
    return _decode_uploaded(_capi.lib(), codec, up.device, up.layout, up.infos, up.frames, up.arena_bytes, up.blob, use_arena, compressed_only, timings, up.marks)


class _Uploaded:
    """A .znn.safetensors file whose data section is on the device (_upload_file)."""
    __slots__ = ("device", "layout", "infos", "frames", "arena_bytes", "blob", "marks", "metadata", "heads")

    def __init__(self, device, layout, infos, frames, arena_bytes, blob, marks, metadata=None, heads=None):
        self.device = device              # torch.device
        self.layout = layout              # {name: (dtype, shape, lo, hi)}: every tensor of the container, offsets into blob
        self.infos = infos                # the file's znn_compressed_vectors metadata
        self.frames = frames              # per compressed tensor: (name, offset of the frame BODY in blob, end of the frame, fast_frame_params, offset in a decode arena)
        self.arena_bytes = arena_bytes    # size of an arena that takes every decoded tensor at a 256-byte boundary
        self.blob = blob                  # the data section: a uint8 tensor on the device
        self.marks = marks                # perf_counter at start / headers parsed / upload done
        self.metadata = metadata or {}    # the file's __metadata__
        self.heads = heads or {}          # per compressed tensor: the first 16 bytes of its frame header (magic … dtype code)


def _upload_file(filename, device, delta=False, lay=None):
    """First half of decode_file_on_device, and how resident.ResidentCheckpoint.from_file gets its frames into HBM: every frame header parsed
    from the host mapping, then the file's data section to the device in ONE transfer.  -> _Uploaded, or None when the container names a dtype
    this parser does not know.  A delta file (znn_delta) is refused unless the caller says it brings the base (delta=True): its "same" and "sparse" entries hold no frame.
    lay: what _read_layout(filename) gave, where the caller has read it already."""
    import contextlib
    import mmap
    import threading
    import time
    from . import _capi, codec
    from .zipnn import fast_frame_params
    dev = torch.device(device)
    while _PENDING_CLOSERS:                            # mappings of earlier calls, unmapped on helper threads (below)
        _PENDING_CLOSERS.pop().join()
    lay = lay if lay is not None else _read_layout(filename)
    if lay is None:
        return None
    lib = _capi.lib()
    t0 = time.perf_counter()
    metadata, layout, data_start = lay
    infos = get_compressed_tensors_metadata(dict(metadata))
    kinds = file_delta(metadata)
    if kinds is not None and not delta:
        raise _needs_base(filename)
    skip = frozenset(n for n, k in kinds[0].items() if k in ("same", "sparse")) if kinds is not None else ()      # (no frame: nothing, or a patch)
    with open(filename, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if size else None
    view = memoryview(mm) if mm is not None else None
    head_len = 32 + 1 + 9 * 255                        # header + the largest shape extension (zipnn._frame_head)
    try:
        # ---- host side: one pass over the mapping ----
        plan, total, heads = [], 0, {}                 # (name, lo + body_off, hi, fp, arena offset)
        for name, (dt, shape, lo, hi) in layout.items():
            if name in infos and name not in skip:
                fp = fast_frame_params(view[data_start + lo: data_start + min(hi, lo + head_len)])
                heads[name] = bytes(view[data_start + lo: data_start + lo + 16])
                plan.append((name, lo + fp[0], hi, fp, total))
                total += (fp[5] + 255) & ~255
        t1 = time.perf_counter()
        blob = codec.to_device(lib, view[data_start:], dev) if (view is not None and size > data_start) else torch.empty(0, dtype=torch.uint8, device=dev)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
    finally:
        if view is not None:
            view.release()
        closer = None
        if mm is not None:
            # Unmapping a file that the upload's worker threads have just read costs ≈ 1.2 ms on a 256-CPU host (TLB shoot-downs) — as long as
            # the whole decode of a GPT-2 checkpoint.  mmap.close() drops the GIL around munmap, so it runs on a helper thread under the launches below
            # (measured: decode_s 1.65 -> 0.59 ms; process exit unmaps whatever a daemon thread has not).
            def _close_mapping():
                with contextlib.suppress(BufferError):     # (a traceback may still hold slices of the mapping: the real error must not be replaced by this one)
                    mm.close()
            closer = threading.Thread(target=_close_mapping, daemon=True)
            closer.start()
            _PENDING_CLOSERS.append(closer)                # (joined by the next call — by then long finished — not by this one: nothing below needs the mapping gone)
    return _Uploaded(dev, layout, infos, plan, total, blob, (t0, t1, t2), dict(metadata), heads)


def _decode_uploaded(lib, codec, dev, layout, infos, plan, total, blob, use_arena, compressed_only, timings, marks):
    """Second half of decode_file_on_device: the data section is in HBM (`blob`), `plan` holds every compressed tensor's frame parameters."""
    import time
    from . import _capi
    t0, t1, t2 = marks
    out = {}
    ta_ = tb_ = tc_ = t2
    if plan:
        arena = torch.empty(max(total, 16), dtype=torch.uint8, device=dev) if use_arena else None
        outs = [None] * len(plan) if use_arena else [torch.empty(fp[5], dtype=torch.uint8, device=dev) for (_, _, _, fp, _) in plan]
        base_in, base_out = blob.data_ptr(), (arena.data_ptr() if use_arena else 0)
        pack = struct.Struct(_capi.ZN_BATCH_ITEM_FMT).pack
        packed = b"".join([pack(base_in + b0, hi - b0, (((base_out + off) if use_arena else outs[i].data_ptr()) if fp[5] else 0), fp[5],
                                fp[1], fp[2], fp[3], fp[4], 0) for i, (_, b0, hi, fp, off) in enumerate(plan)])
        stream = codec._stream_handle(blob)
        with codec._device_of(dev):
            lib.decompress_batch_dev_packed(packed, len(plan), stream, check=False)      # asynchronous: the verdict is asked for below
        ta_ = time.perf_counter()
        # (views while the kernels run: one typed view of the arena per dtype, one as_strided per tensor)
        typed = {}
        for i, (name, _, _, fp, off) in enumerate(plan):
            n, dt, shape = fp[5], fp[6], tuple(fp[7]) if fp[7] is not None else None
            if n == 0:
                out[name] = torch.empty(shape if shape is not None else (0,), dtype=dt, device=dev)
                continue
            if use_arena:
                ta = typed.get(dt)
                if ta is None:
                    ta = typed[dt] = arena.view(dt)
                es = ta.element_size()
                shp = shape if shape is not None else (n // es,)
                out[name] = torch.as_strided(ta, shp, _contiguous_strides(shp), off // es)
            else:
                out[name] = outs[i].view(dt).reshape(shape) if shape is not None else outs[i].view(dt)
    tb_ = time.perf_counter()
    if plan:
        with codec._device_of(dev):
            lib.decode_status(stream)                  # waits for the decode; raises for a corrupt frame exactly as a checked call would
    tc_ = time.perf_counter()
    if not compressed_only:
        for name, (dt, shape, lo, hi) in layout.items():
            if name not in infos:
                # (a copy, not a view: one surviving int tensor would otherwise pin the whole uploaded section — all compressed frames — in HBM)
                out[name] = blob[lo:hi].clone().view(dt).reshape(shape) if hi > lo else torch.empty(shape, dtype=dt, device=dev)
    if timings is not None:
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        # (decode_s in parts: arena + item table + launch | views built while the kernels run | wait for the kernels' verdict | copies of the plain tensors + sync)
        timings.update(decode_launch_s=ta_ - t2, decode_views_s=tb_ - ta_, decode_wait_s=tc_ - tb_, decode_plain_s=t3 - tc_)
        timings.update(read_s=t1 - t0, h2d_s=t2 - t1, decode_s=t3 - t2, compressed_tensors=len(plan), h2d_bytes=int(blob.numel()),
                       compressed_bytes=int(sum(hi - b0 for (_, b0, hi, _, _) in plan)), decoded_bytes=int(sum(p[3][5] for p in plan)))
    return out


def load_file(filename, device="cuda:0", timings=None, verify=False, base=None, verify_base=True):
    """Load a (possibly ZipNN-compressed) safetensors file straight onto `device` -> {name: tensor}: one transfer of the file's data
    section, one batched decode (decode_file_on_device).  The batched counterpart of looping SafeOpen.get_tensor (reference
    zipnn.py:1592-1626, scripts/zipnn_decompress_safetensors.py:75-120) — and what SafeOpen itself uses behind get_tensor for a
    device target.  timings: an optional dict that receives the seconds spent mapping the file and parsing every header (`read_s`),
    moving the data section to the device (`h2d_s`) and decoding (`decode_s`), each ended by a device sync.
    verify=True: the decoded tensors are digested — on a GPU all of them by one batched launch, with device="cpu" by the host function — and compared with
    the file's `znn_digests` (compress_safetensors_file(..., digests=True)); DigestMismatch names the tensors that differ.  A file without digests is an
    error then, not a pass.
    base: what a DELTA file (znn_delta) was taken over — a ResidentCheckpoint on the device, a mapping of names to device tensors, a module, or
    a path to the base's file, plain or compressed.  The file becomes a variant store over it (ResidentCheckpoint.from_file(base=), which checks the base's
    digests against the file's unless verify_base=False) and every tensor is decoded once; plain tensors come back, none of them the base's own.  A delta
    file without `base` is a ValueError; a file that is no delta file does not look at `base`."""
    dev = torch.device(device)
    want = None
    meta = read_metadata(filename) if (verify or base is not None) else {}
    if verify:
        want = file_digests(meta)
        if want is None:
            raise ValueError(f"{filename}: the file carries no digests ({DIGESTS_KEY}): nothing to verify against")
    if base is not None and DELTA_KEY in meta:
        from .resident import ResidentCheckpoint
        dev = ResidentCheckpoint._work_device(dev)
        store = ResidentCheckpoint.from_file(filename, dev, base=_base_store(base, dev), verify_base=verify_base)
        got = store.get_tensors(store.keys())
        out = {n: (t if store._entries[n].decoded else t.clone()) for n, t in got.items()}      # (no view of the uploaded section, no tensor of the base)
        if want is not None:
            check_digests(out, want, filename)
        return out
    out = decode_file_on_device(filename, dev, timings=timings)
    if out is None:
        out = _load_file_per_tensor(filename, dev, timings)
    if want is not None:
        check_digests(out, want, filename)
    # (file order, as safetensors' own load_file returns it)
    return out


def _load_file_per_tensor(filename, dev, timings=None):
    """load_file through safetensors' own reader, tensor by tensor (CPU targets, dtypes the container parser above does not know)."""
    import time
    from safetensors import safe_open
    from . import _capi, codec

    def _sync():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out, host, meta = {}, [], []
    with safe_open(filename, "pt", "cpu") as f:
        infos = get_compressed_tensors_metadata(dict(f.metadata() or {}))
        for name in f.keys():
            host.append((name, f.get_tensor(name)))
    t1 = time.perf_counter()
    items = []
    for name, t in host:
        if name not in infos:
            out[name] = t.to(dev, non_blocking=True)
            continue
        znn = ZipNN(input_format="torch", bytearray_dtype=COMPRESSED_DTYPE, method=COMPRESSION_METHOD)
        fp = znn.frame_params(t)
        host_body = t.reshape(-1).view(torch.uint8)[fp["body_off"]:]
        # (large bodies through the library's pinned multi-threaded transfer; small ones are not worth its threads)
        body = codec.to_device(_capi.lib(), host_body.numpy(), dev) if host_body.numel() >= (2 << 20) and dev.type == "cuda" \
            else host_body.to(dev, non_blocking=True)
        items.append((body, fp["num_buf"], fp["bits_mode"], fp["bytes_mode"], fp["chunk"], fp["orig_size"]))
        meta.append((name, fp["torch_dtype"], fp["shape"]))
    if timings is not None:
        _sync()
    t2 = time.perf_counter()
    flats = codec.decompress_device_batch(_capi.lib(), items)
    for (name, dtype, shape), flat in zip(meta, flats):
        out[name] = flat.view(dtype).reshape(shape) if flat.numel() else torch.empty(shape, dtype=dtype, device=dev)
    if timings is not None:
        _sync()
        t3 = time.perf_counter()
        timings.update(read_s=t1 - t0, h2d_s=t2 - t1, decode_s=t3 - t2, compressed_tensors=len(items),
                       compressed_bytes=int(sum(it[0].numel() for it in items)), decoded_bytes=int(sum(it[5] for it in items)))
    return out
