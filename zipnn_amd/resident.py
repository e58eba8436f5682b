"""A checkpoint kept COMPRESSED in device memory, decoded a layer, a tensor or a row range at a time.

The decoder is fast enough (a 500 MB transformer block in a fraction of a millisecond) that a model can hold its weights as ZipNN frames
in HBM — about two thirds of their bf16 size — and decode what the next layer needs into a scratch buffer just before it runs.  This module
is the interface for that: `ResidentCheckpoint` owns the frames, `zn_decompress_window_batch_dev` / `zn_plan_*` (include/zipnn_hip.h) decode
chunk windows of them where they lie.  Nothing here moves compressed bytes again after they have been uploaded, and no decode reads anything
back to the host unless it is asked for the verdict (`status()`).

Without a GPU the module works on whatever library `zipnn_amd._capi.lib()` returns with CPU tensors as "device memory" — the way the CPU
test-suite drives the emulated kernels, exactly as `CompressedSlice` does.
"""
import torch

from . import _capi, codec
from .header import HEADER_LEN, EnumFormat, pack_shape
from .zipnn import (_ST_DTYPE_NAME, COMPRESSION_METHOD, ZipNN, build_compressed_tensor_info, dtype_from_user, index_rows,
                    set_compressed_tensors_metadata)

# (see ResidentCheckpoint.INDEX_DTYPES)
_INDEX_DTYPES = (torch.bfloat16, torch.float16, torch.float32) + tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e5m2") if hasattr(torch, n))

ALIGN = 256          # decode destinations inside a shared buffer start at multiples of this (the fused kernel wants 16-byte aligned destinations)


def _round_up(n):
    return (int(n) + ALIGN - 1) // ALIGN * ALIGN


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _patch_entries(n, elem, length):
    """-> T of a "znp1" patch of `length` bytes for a tensor of n bytes, elem bytes per element (include/zipnn_hip.h: L = round16(A1 + 2 T) + elem T, which
    grows strictly with T)."""
    nb = (n // elem + 65535) // 65536
    a1 = (32 + 4 * (nb + 1) + 15) // 16 * 16
    t = max((length - a1) // (2 + elem) - 16, 0)
    while (a1 + 2 * t + 15) // 16 * 16 + elem * t < length:
        t += 1
    if (a1 + 2 * t + 15) // 16 * 16 + elem * t != length:
        raise ValueError(f"{length} is not the length of a patch of a tensor of {n} bytes")
    return t


def _stream_of(dev, stream=None):
    """-> the raw stream handle to launch on: `stream` (a torch.cuda.Stream or a handle), else the device's current stream."""
    if stream is not None:
        return getattr(stream, "cuda_stream", stream)
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0


class _device_of:
    """torch.cuda.device(dev) for a GPU, nothing for the emulated library's CPU tensors."""

    def __init__(self, dev):
        self._ctx = torch.cuda.device(dev) if dev.type == "cuda" else None

    def __enter__(self):
        if self._ctx is not None:
            self._ctx.__enter__()
        return self

    def __exit__(self, *a):
        return self._ctx.__exit__(*a) if self._ctx is not None else False


class _Entry:
    """One tensor of the store: a frame body in device memory (`body`, with its codec parameters), or the tensor itself (`raw`).
    In a variant store (ResidentCheckpoint.from_state_dict(..., base=...)): `delta` is True where the body encodes tensor ^ base, "same" where the tensor's
    bytes are the base's (no body; `raw` is the base's own tensor where the base holds it plainly) and False otherwise; `base` is what a delta or "same" entry
    decodes over and `restore` what revert_ puts back — ("tensor", the base's tensor, held by reference) or ("entry", the base store, its entry) — or None.
    `head`: the first 16 bytes of the frame header the body was written behind or would be (magic … dtype code): what save_file writes in front of it again.
    A SPARSE entry (from_state_dict(..., base=..., sparse=True)): `delta` is "sparse", there is no body, `patch` is the "znp1" patch
    (include/zipnn_hip.h) that turns the base's bytes into the tensor's and `entries` its number of elements; reading it is the base's bytes with the patch
    XORed in.  Its frame parameters are those the tensor would be coded with: windows are counted in their chunks."""
    __slots__ = ("name", "dtype", "shape", "nbytes", "body", "raw", "P", "bits", "byts", "chunk", "hints", "delta", "base", "restore", "head", "patch", "entries")

    def __init__(self, name, dtype, shape, nbytes, body=None, raw=None, params=None):
        self.name, self.dtype, self.shape, self.nbytes, self.body, self.raw = name, dtype, tuple(int(d) for d in shape), int(nbytes), body, raw
        self.hints = None                      # the body's decode hints (ResidentCheckpoint.build_index): a uint8 tensor beside the body, or None
        self.P, self.bits, self.byts, self.chunk = params if params is not None else (0, 0, 0, 0)
        self.delta, self.base, self.restore = False, None, None
        self.head = None
        self.patch, self.entries = None, 0

    @property
    def compressed(self):
        return self.body is not None

    @property
    def decoded(self):
        """Whether reading the tensor runs a decode (a body of its own, or a "same" entry over a base that is compressed itself)."""
        return self.body is not None or self.patch is not None or (self.delta == "same" and self.raw is None)

    @property
    def chunks(self):
        return (self.nbytes + self.chunk - 1) // self.chunk if self.decoded else 0

    def window(self, lo, hi, dst_ptr, delta_ptr=None):
        """-> the item tuple of ZnLib.decompress_window_batch_dev / plan_create for chunks [lo, hi) of this tensor (delta_ptr: the WHOLE tensor's base)."""
        return (self.body.data_ptr(), self.body.numel(), self.P, self.bits, self.byts, self.chunk, self.nbytes, lo, hi, dst_ptr, delta_ptr)

    def hinted(self, lo, hi, dst_ptr, delta_ptr=None):
        """-> the item of ZnLib.decompress_hinted_batch_dev / plan_create_hinted: the window plus the body's index (None, 0 without one).  With a delta
        base the item names the index's kind as well: a delta body's index is of kind HINT_DELTA (build_index(deltas=True))."""
        h = self.hints
        item = (self.window(lo, hi, dst_ptr, delta_ptr), h.data_ptr() if h is not None else None, h.numel() if h is not None else 0)
        return item + (_capi.HINT_DELTA,) if delta_ptr is not None else item

    def patch_item(self, lo, hi, dst_ptr, base_ptr=None):
        """-> the item tuple of ZnLib.patch_apply_batch_dev / patch_plan_create for chunks [lo, hi) of this sparse entry: the patch's entries inside that byte
        window XORed into dst_ptr — over what lies there, or (base_ptr: the WHOLE tensor's base) over a copy of the base's window."""
        item = (self.patch.data_ptr(), self.patch.numel(), self.nbytes, self.P, lo * self.chunk, min(hi * self.chunk, self.nbytes), dst_ptr)
        return item + (base_ptr,) if base_ptr is not None else item

    def view(self, flat):
        """flat uint8 bytes of the whole tensor -> the tensor."""
        return flat.view(self.dtype).reshape(self.shape)


class ResidentCheckpoint:
    """The tensors of a checkpoint, resident in device memory in compressed form.

        store = ResidentCheckpoint.from_file("model.znn.safetensors", "cuda:0")      # or .from_state_dict(model.state_dict(), "cuda:0")
        w = store.get_tensor("h.0.mlp.c_fc.weight")                                  # decoded now, a new tensor
        rows = store.get_slice("wte.weight")[1000:1064]                              # only the chunks that hold those rows are decoded
        plan = store.plan(["h.0.attn.c_attn.weight", "h.0.attn.c_attn.bias"])        # prepared once …
        plan.run(); use(plan.tensors)                                                # … launched per step: no host wait, no copy
        handle = store.hook(model)                                                   # the model's own forward decodes layer by layer

    Tensors that a file stores uncompressed (integers, tensors that did not shrink) stay in the store as plain tensors.  Every decode runs on
    the current stream of the store's device.

    A VARIANT store holds a fine-tune as XOR deltas over a base that is already on the device:

        base = ResidentCheckpoint.from_state_dict(base_sd, "cuda:0", index=True)     # or from_file; or a {name: device tensor} mapping / an nn.Module
        ft = ResidentCheckpoint.from_state_dict(ft_sd, "cuda:0", base=base)          # bodies encode ft ^ base: a fraction of a plain store
        ft.get_tensor(n); ft.get_tensors(ns); ft.get_slice(n)[a:b]; ft.plan(ns).run(); ft.hook(model)     # all give the fine-tune's bytes
        ft.apply_(model)          # tensors that hold the base's values now hold the fine-tune's, in place (XOR is its own inverse) …
        ft.revert_(model)         # … and the base's again
        ft.info(n)["delta"]       # True, False or "same"
        ft = ResidentCheckpoint.from_state_dict(ft_sd, "cuda:0", base=base, sparse=True)      # tensors with few changed elements are kept as "znp1" patches
        ft.info(n)["delta"], ft.info(n)["patch_entries"]                                          # "sparse", the number of elements that differ
        flat = s3.rebased(base); sw = ft_b.rebased(ft_a)      # the same tensors over another store: a chain flattened, a sibling re-parented — by patch merges

    CONTENT DIGESTS ("zn64-1"; an error-detecting code, not a cryptographic hash) let a store answer whether what it decodes is still what it was built from:

        store = ResidentCheckpoint.from_state_dict(sd, "cuda:0", digests=True)       # or from_file(path, dev, digests=True, verify=True)
        store.digests(); store.info(n)["digest"]                                     # ints below 2^64
        store.verify()            # every tensor decoded into one scratch buffer and digested on the device -> {name: bool}, or DigestMismatch
        store.holds(model)        # do the live tensors hold this store's values?
        ft.apply_(model, guard=True); ft.revert_(model, guard=True)                  # raise before touching anything if they hold the wrong values
    """

    def __init__(self, device, entries, held_bytes, keep=()):
        self.device = torch.device(device)
        self._entries = {e.name: e for e in entries}
        self._held = int(held_bytes)
        self._keep = tuple(keep)              # the allocations the entries are views of
        self._index = None                     # the allocation the entries' hints are views of (build_index)
        self._index_bytes = 0
        self._digests = None                   # {name: "zn64-1" digest of the tensor's bytes} when the store was built with digests, else None
        self._metadata = None                  # from_file: the file's own metadata (without the keys this library writes), which save_file writes back

    # ---- constructors -------------------------------------------------------------------------------------------------------
    @staticmethod
    def _work_device(device):
        if isinstance(device, int):
            device = f"cuda:{device}"
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", codec.current_device())
        if dev.type != "cuda" and torch.cuda.is_available():
            raise ValueError("a resident checkpoint lives in GPU memory: device must be a cuda device")
        return dev

    @classmethod
    def from_file(cls, path, device="cuda:0", index=False, digests=False, verify=False, base=None, verify_base=True, check_patches=True):
        """A `.znn.safetensors` file (this library's or the reference's): its data section goes to `device` once, in one transfer, and stays.
        index=True: build_index() on the new store; index="deltas": build_index(deltas=True) — the delta bodies of a delta file get their index too.
        digests=True: the store records a content digest per tensor (digests(), verify(), holds()).  A file written with digests
        (compress_safetensors_file(..., digests=True)) brings them, and they are taken from it — they describe what the WRITER compressed.  A file
        without them is decoded once and the store records what it got: that only pins the state at load — damage that happened before is not seen.
        verify=True: the file's digests are checked against one decode of every tensor at load; DigestMismatch names the tensors that differ, and a file
        without digests is an error, not a pass.

        base: what a DELTA file (metadata key znn_delta; written by save_file of a variant store) was taken over — what from_state_dict accepts
        as `base`: a store on the device, a mapping of names to device tensors, a module.  The result is the variant store from_state_dict(ft_sd, base=base)
        would have built — the same info() for every tensor, the same bodies, now views of the uploaded data section — with no compression run and no tensor
        of the fine-tune materialised.  A delta file without `base` is a ValueError, and so is a base that lacks a tensor the file codes over it, holds it with
        another dtype or shape, or holds it compressed in chunks of another size (each names the tensor).  XOR over the wrong base decodes cleanly to garbage, so
        with verify_base=True (the default) the base's digests are compared with the file's `base_digests` before anything is uploaded or decoded: a base
        store's recorded digests are used as they are, a base without them is digested once, all its needed tensors in one batch (decoded, or where they lie);
        DigestMismatch names the tensors that differ.  verify=True keeps its meaning: the decoded fine-tune against `znn_digests`.  A file that is no delta file
        takes `base` only as what revert_ restores from.
        SPARSE entries (a file written by save_file(sparse=True)) become what from_state_dict(..., sparse=True) holds: the patch a 16-byte aligned
        view of the uploaded data section, info(n)["delta"] == "sparse".  A patch from a file is one this process did not build, so it is refused BY NAME AT LOAD
        instead of by the first apply that reads its damage (apply_ on live weights has written by then): before the upload every sparse entry's header is read
        from the file — a ValueError names the tensor whose entry is not the header's L + 15 bytes long, whose magic, element size or n is not its dtype's and
        shape's, or whose L is not zn_patch_len of its T — and with check_patches=True (the default) the slack around every patch must be zero and, after the
        upload and before anything is decoded, ONE zn_patch_check_batch_dev call validates every patch whole (header, first[], every entry, padding); a ValueError
        names every damaged tensor with its mask.  check_patches=False skips both; apply's own checks remain.  A well-formed patch of ANOTHER tensor passes:
        verify=True (the digests) is what catches that."""
        import json
        from . import safetensors_io
        dev = cls._work_device(device)
        meta = safetensors_io.read_metadata(path)
        recorded = safetensors_io.file_digests(meta) if (digests or verify) else None
        if verify and recorded is None:
            raise ValueError(f"{path}: the file carries no digests (znn_digests): nothing to verify against")
        delta = safetensors_io.file_delta(meta)
        if delta is not None and base is None:
            raise safetensors_io._needs_base(path)
        based = cls._base_items(base, dev)
        kinds, over = {}, {}                                           # {name: "delta" | "same" | "sparse"}, {name: (dtype, shape, what it is coded over)}
        if delta is not None:
            kinds, want = delta
            infos = safetensors_io.get_compressed_tensors_metadata(meta)
            for name in kinds:
                if name not in infos:
                    raise ValueError(f"{path}: {name!r} is listed under znn_delta but not under znn_compressed_vectors")
                dt, shape = getattr(torch, str(infos[name].get("dtype")), None), tuple(int(d) for d in json.loads(infos[name].get("shape", "[]")))
                if not isinstance(dt, torch.dtype):
                    raise ValueError(f"{path}: {name!r}: unknown dtype {infos[name].get('dtype')!r}")
                ref = based.get(name)
                if ref is None:
                    raise ValueError(f"{path}: the base has no tensor {name!r}, which the file codes over it")
                b = ref[1] if ref[0] == "tensor" else ref[2]
                if b.dtype != dt or tuple(b.shape) != shape:
                    raise ValueError(f"{path}: {name!r} is {dt} {list(shape)} over a base tensor of the same dtype and shape; the base holds {b.dtype} {list(b.shape)}")
                over[name] = (dt, shape, ref)
            if verify_base:
                got = cls._ref_digests({name: ref for name, (_, _, ref) in over.items()}, dev)
                bad = [name for name in kinds if got[name] != want[name]]
                if bad:
                    raise codec.DigestMismatch(bad, f"{path}: the base does not hold what the delta was taken over")
        patched = cls._file_patches(path, {n: over[n] for n, k in kinds.items() if k == "sparse"}, check_patches)      # {name: (offset in the data section, L, T, elem)}
        up = safetensors_io._upload_file(path, dev, delta=delta is not None)
        if up is None:
            raise ValueError(f"{path}: the container names a dtype this loader does not know")
        layout, plan, blob = up.layout, up.frames, up.blob
        entries, framed, extra = [], {}, 0
        for (name, b0, hi, fp, _) in plan:
            _, P, bits, byts, chunk, n, tdt, shape = fp
            head = up.heads.get(name)
            is_delta = kinds.get(name) == "delta"
            if head is not None and (head[9] != 0) != is_delta:
                raise ValueError(f"{path}: {name!r}: the frame header says {'delta' if head[9] else 'no delta'}, znn_delta says otherwise")
            if is_delta:
                tdt, shape, ref = over[name]
                if n != _numel(shape) * torch.empty(0, dtype=tdt).element_size():
                    raise ValueError(f"{path}: {name!r}: a frame of {n} bytes for {tdt} {list(shape)}")
                if ref[0] == "entry" and ref[2].chunk != chunk:
                    raise ValueError(f"{path}: {name!r} is coded in chunks of {chunk} bytes, the base holds it in chunks of {ref[2].chunk}")
            e = framed[name] = _Entry(name, tdt, shape if shape is not None else (n // max(torch.empty(0, dtype=tdt).element_size(), 1),), n,
                                      body=blob[b0:hi], params=(P, bits, byts, chunk))
            e.head = head
            if is_delta:
                e.delta, e.base = True, ref
        for name, (dt, shape, lo, hi) in layout.items():          # (file order)
            if name in framed:
                entries.append(framed[name])
                continue
            if kinds.get(name) == "same":                          # nothing of its own: the base's tensor itself, or a decode of the base's body
                tdt, tshape, ref = over[name]
                if hi != lo:
                    raise ValueError(f"{path}: {name!r} is listed as \"same\" but holds {hi - lo} bytes")
                if ref[0] == "tensor":
                    params = tuple(ZipNN(input_format="torch", bytearray_dtype=tdt, method=COMPRESSION_METHOD).torch_frame_plan(torch.empty(tshape, dtype=tdt, device="meta"))[1:])
                else:
                    params = (ref[2].P, ref[2].bits, ref[2].byts, ref[2].chunk)
                e = _Entry(name, tdt, tshape, _numel(tshape) * torch.empty(0, dtype=tdt).element_size(), raw=ref[1] if ref[0] == "tensor" else None, params=params)
                e.delta, e.base = "same", ref
                entries.append(e)
                continue
            if kinds.get(name) == "sparse":                        # the patch where the upload put it; the frame parameters the tensor would be coded with
                tdt, tshape, ref = over[name]
                at, L, T, elem = patched[name]
                if ref[0] == "tensor":
                    params = tuple(ZipNN(input_format="torch", bytearray_dtype=tdt, method=COMPRESSION_METHOD).torch_frame_plan(torch.empty(tshape, dtype=tdt, device="meta"))[1:])
                else:
                    params = (ref[2].P, ref[2].bits, ref[2].byts, ref[2].chunk)
                if params[0] != elem:
                    raise ValueError(f"{path}: {name!r}: {tdt} is not a dtype a patch describes")
                e = _Entry(name, tdt, tshape, _numel(tshape) * elem, params=params)
                e.patch, e.delta, e.base, e.entries = blob[at:at + L], "sparse", ref, T
                if e.patch.data_ptr() % 16:                        # (the upload's allocation is aligned far beyond 16 bytes; should one not be, the apply kernel still needs it)
                    e.patch = e.patch.clone()
                    extra += L
                entries.append(e)
                continue
            if hi > lo:
                es = torch.empty(0, dtype=dt).element_size()
                raw = blob[lo:hi]
                if (blob.data_ptr() + lo) % max(es, 1):            # (a view needs the element's alignment: safetensors does not promise it)
                    raw = raw.clone()
                    extra += hi - lo
                raw = raw.view(dt).reshape(shape)
            else:
                raw = torch.empty(shape, dtype=dt, device=dev)
            entries.append(_Entry(name, dt, shape, hi - lo, raw=raw))
        for e in entries:                                          # what revert_ restores from: the base's tensor of the same name, dtype and shape
            ref = based.get(e.name)
            if ref is not None:
                b = ref[1] if ref[0] == "tensor" else ref[2]
                if b.dtype == e.dtype and tuple(b.shape) == e.shape:
                    e.restore = ref
        store = cls(dev, entries, blob.numel() + extra, keep=(blob,) + ((base,) if base is not None else ()))
        store._metadata = {k: v for k, v in up.metadata.items() if k not in (safetensors_io.METADATA_KEY, safetensors_io.DIGESTS_KEY, safetensors_io.DELTA_KEY)}
        if patched and check_patches:                              # before anything is decoded: every patch whole, one launch, one read-back
            sp = [e for e in entries if e.patch is not None]
            verdicts, _ = codec.patch_check_device_batch(_capi.lib(), [(e.patch, e.nbytes, e.P) for e in sp], _stream_of(dev))
            bad = [(e.name, v) for e, v in zip(sp, verdicts) if v]
            if bad:
                raise ValueError(f"{path}: malformed patch (znp1) in " + ", ".join(f"{n!r}: {codec.patch_verdict_text(v)}" for n, v in bad))
        if index:
            store.build_index(deltas=(index == "deltas"))
        if recorded is not None:
            missing = [n for n in store.keys() if n not in recorded]
            if missing:
                raise ValueError(f"{path}: znn_digests lacks {missing[:3]}{' …' if len(missing) > 3 else ''}")
            store._digests = {n: recorded[n] for n in store.keys()}
            if verify:
                store.verify()
        elif digests:
            store._digests = store._decoded_digests(store.keys())
        return store

    @staticmethod
    def _file_patches(path, over, check_slack):
        """The "sparse" entries of a delta file, from the file alone, before anything is uploaded.  over: {name: (dtype, shape, _)} -> {name: (offset of the patch
        in the data section, L, T, elem)}.  The patch starts at the entry's first multiple of 16; its header must describe the tensor and give the
        entry's length; check_slack: the up to 15 bytes of the entry around the patch must be zero.  A ValueError names the tensor."""
        if not over:
            return {}
        from . import safetensors_io
        lay = safetensors_io._read_layout(path)
        if lay is None:
            raise ValueError(f"{path}: the container names a dtype this loader does not know")
        _, layout, data_start = lay
        lib, out = _capi.lib(), {}
        with open(path, "rb") as f:
            for name, (dt, shape, _) in over.items():
                fdt, _, lo, hi = layout[name]
                elem = torch.empty(0, dtype=dt).element_size()
                n = _numel(shape) * elem
                at = (lo + 15) // 16 * 16
                if fdt != torch.uint8 or hi - lo < 32 + safetensors_io.SPARSE_SLACK:
                    raise ValueError(f"{path}: {name!r} is listed as \"sparse\" but its entry of {hi - lo} bytes cannot hold a patch")
                f.seek(data_start + lo)
                head = f.read(at - lo + 32)
                magic, E, T, L = head[at - lo: at - lo + 4], head[at - lo + 4], int.from_bytes(head[at - lo + 16: at - lo + 24], "little"), int.from_bytes(head[at - lo + 24: at - lo + 32], "little")
                if magic != b"ZNP1" or E != elem or int.from_bytes(head[at - lo + 8: at - lo + 16], "little") != n:
                    raise ValueError(f"{path}: {name!r}: the patch's header does not describe a {dt} tensor of {n} bytes")
                if hi - lo != L + safetensors_io.SPARSE_SLACK:
                    raise ValueError(f"{path}: {name!r}: an entry of {hi - lo} bytes for a patch of {L} (the entry is the patch and {safetensors_io.SPARSE_SLACK} bytes)")
                if T > n // elem or lib.patch_len(n, elem, T) != L:
                    raise ValueError(f"{path}: {name!r}: {L} bytes is not the length of a patch of {T} elements")
                if check_slack:
                    f.seek(data_start + at + L)
                    if any(head[:at - lo]) or any(f.read(hi - at - L)):
                        raise ValueError(f"{path}: {name!r}: the bytes around the patch are not zero")
                out[name] = (at, L, T, elem)
        return out

    @staticmethod
    def _ref_digests(refs, dev):
        """{name: ("tensor", tensor) | ("entry", store, entry)} (_base_items) -> {name: digest of that base tensor's bytes}: a base store's recorded digest where
        it has one; otherwise the plain tensors digested where they lie, all in one batched launch, and a store's entries through one _decoded_digests call."""
        out, live, via = {}, [], {}
        for name, ref in refs.items():
            if ref[0] == "tensor":
                live.append((name, ref[1]))
            elif ref[1]._digests is not None:
                out[name] = ref[1]._digests[ref[2].name]
            else:
                via.setdefault(id(ref[1]), (ref[1], []))[1].append((name, ref[2].name))
        if live:
            with _device_of(dev):
                vals = codec.digests_to_ints(codec.digest_device_batch(_capi.lib(), [codec.flat_bytes(t) for _, t in live], _stream_of(dev)))
            out.update({name: v for (name, _), v in zip(live, vals)})
        for bstore, pairs in via.values():
            got = bstore._decoded_digests([bn for _, bn in pairs])
            out.update({name: got[bn] for name, bn in pairs})
        return out

    @staticmethod
    def _base_items(base, dev):
        """-> {name: ("tensor", tensor) | ("entry", store, entry)} for what from_state_dict accepts as `base`."""
        if base is None:
            return {}
        if isinstance(base, ResidentCheckpoint):
            if base.device != dev:
                raise ValueError(f"base: a store on {dev}, not on {base.device}")
            return {name: (("tensor", e.raw) if e.raw is not None else ("entry", base, e)) for name, e in base._entries.items()}
        if isinstance(base, torch.nn.Module):
            items = dict(base.named_parameters())
            items.update(dict(base.named_buffers()))
        else:
            items = dict(base)
        out = {}
        for name, t in items.items():
            t = t.detach()
            if t.device != dev or not t.is_contiguous():
                raise ValueError(f"base[{name!r}]: a contiguous tensor on {dev} (plain base tensors are read where they lie)")
            out[name] = ("tensor", t)
        return out

    #: from_state_dict(base=...): base tensors are taken (and a resident base decoded) in groups of at most this many bytes
    _BUILD_GROUP_BYTES = 1 << 30

    @classmethod
    def from_state_dict(cls, sd, device="cuda:0", threshold=0.95, method=None, index=False, base=None, digests=False, sparse=False):
        """Compress the tensors of a state dict on `device` (one batched call) and keep the bodies, trimmed to their lengths and packed at
        256-byte boundaries of one allocation.  A tensor whose body would not be smaller than the tensor itself — and every tensor the codec
        does not take: integers, float64, empty ones — is kept as it is.  index=True: build_index() on the new store; index="deltas":
        build_index(deltas=True), which indexes the delta bodies of a variant store as well.
        digests=True: the SOURCE tensors are digested on the device, all of them in one batched launch, before anything is compressed: the store then knows
        what it was built from (digests(), verify(), holds(), the guards of apply_ / revert_).

        base: the store becomes a VARIANT of it — another ResidentCheckpoint on the same device (compressed or not, a variant itself), a mapping of
        names to tensors on the device, or a module (its named parameters and buffers).  A tensor the base has under the same name with the same dtype,
        shape and frame parameters is also compressed as tensor ^ base (a second batched call) and the smaller of the two bodies is kept, the plain one
        on a tie; a tensor whose bytes ARE the base's is recorded as "same" and holds nothing.  Decodes combine delta and base on the way out; the
        variant keeps its base alive.  Plain base tensors are held BY REFERENCE and read at decode time: the caller keeps them at the base's values
        (apply_ on those very tensors changes what the variant decodes over until revert_).  resident_bytes counts the variant's own memory.
        sparse=True (with base): a delta candidate is also COUNTED against its base — one pass, no bytes written — and where the "znp1" patch (the changed
        elements with their XOR values, include/zipnn_hip.h) would be smaller than the best body so far it is built and kept instead:
        info(name)["delta"] == "sparse".  The smallest of plain body, delta body and patch wins, ties in that order, so nothing that is chosen without
        `sparse` changes.  Every read path serves such an entry (the base's bytes, then the patch applied in place); save_file(sparse=True) writes it down.
        Peak memory of the build, beside `sd` on the device: the plain pass's compress arena (as large as the tensors, as without `base`); then the
        plain bodies and, as they come, the delta bodies — each a trimmed copy out of its arena —, plus per group of at most 1 GiB of tensors (or one
        larger tensor) the decoded tensors of a resident base and one arena of the group's size; at the end the kept bodies are copied once more into
        the store's one allocation before the copies are dropped: about twice the bodies for a moment, never a whole second copy of the base."""
        dev = cls._work_device(device)
        lib = _capi.lib()
        based = cls._base_items(base, dev)
        todo, entries = [], {}
        coders = {}                            # one ZipNN per dtype: what decides a tensor's frame parameters

        heads = {}                             # {name: the first 16 bytes of the frame header that describes the tensor's body}

        def frame_plan(t):
            if t.dtype not in coders:
                coders[t.dtype] = ZipNN(input_format="torch", bytearray_dtype=t.dtype, method=method or COMPRESSION_METHOD)
            return coders[t.dtype].torch_frame_plan(t)

        def frame_params(t):
            return tuple(frame_plan(t)[1:])
        for name, t in sd.items():
            t = t.detach()
            if torch.is_floating_point(t) and t.dtype != torch.float64 and t.numel() > 0 and dtype_from_user(t.dtype) is not None:
                hdr, P, bits, byts, chunk = frame_plan(t)
                heads[name] = bytes(hdr[:16])
                todo.append((name, t.to(dev), (P, bits, byts, chunk)))
            else:
                entries[name] = _Entry(name, t.dtype, t.shape, t.numel() * t.element_size(), raw=t.to(dev).clone())

        def matches(name, t):                  # the base has this tensor: what revert_ restores from
            ref = based.get(name)
            if ref is None:
                return None
            b = ref[1] if ref[0] == "tensor" else ref[2]
            return ref if (b.dtype == t.dtype and tuple(b.shape) == tuple(t.shape)) else None

        def delta_ok(ref, t, prm):             # … with the same frame parameters: what a delta body can be coded over
            if ref[0] == "tensor":
                return frame_params(ref[1]) == tuple(prm)
            be = ref[2]
            return be.decoded and (be.P, be.bits, be.byts, be.chunk) == tuple(prm)

        def trimmed(bodies):                   # (out of the compress arena, which is as large as the tensors themselves)
            return [b.clone() for b in bodies]

        recorded = None
        if digests:                            # (the sources, before compression; raw entries are digested too)
            src = {name: t for name, t, _ in todo}
            src.update({name: e.raw for name, e in entries.items()})
            order = list(sd.keys())
            with _device_of(dev):
                recorded = dict(zip(order, codec.digests_to_ints(codec.digest_device_batch(lib, [codec.flat_bytes(src[n]) for n in order]))))
        keep, held = [], 0
        if todo:
            with _device_of(dev):
                plain = trimmed(codec.compress_device_batch(lib, [(codec.flat_bytes(t), P, bits, byts, chunk, float(threshold)) for (_, t, (P, bits, byts, chunk)) in todo]))
                refs = [matches(name, t) for (name, t, _) in todo]
                cand = [i for i, ((name, t, prm), ref) in enumerate(zip(todo, refs)) if ref is not None and delta_ok(ref, t, prm)]
                dbody, same, pbody = {}, set(), {}
                # in groups of at most _BUILD_GROUP_BYTES of base bytes: plain base tensors are read where they lie, a resident base's tensors are decoded
                # a group at a time (never the whole base at once), the group's "is it the base's bytes" flags come back in one read
                groups, cur, size = [], [], 0
                for i in cand:
                    nb = todo[i][1].numel() * todo[i][1].element_size()
                    if cur and size + nb > cls._BUILD_GROUP_BYTES:
                        groups.append(cur)
                        cur, size = [], 0
                    cur.append(i)
                    size += nb
                if cur:
                    groups.append(cur)
                for grp in groups:
                    via = [todo[i][0] for i in grp if refs[i][0] == "entry"]
                    decoded = base.get_tensors(via) if via else {}
                    flats = {i: codec.flat_bytes(refs[i][1] if refs[i][0] == "tensor" else decoded[todo[i][0]]) for i in grp}
                    eq = torch.stack([(codec.flat_bytes(todo[i][1]) == flats[i]).all() for i in grp]).tolist()
                    same.update(i for i, e in zip(grp, eq) if e)
                    rest = [i for i in grp if i not in same]
                    if rest:
                        got = trimmed(codec.compress_device_batch(lib, [(codec.flat_bytes(todo[i][1]),) + tuple(todo[i][2]) + (float(threshold), flats[i]) for i in rest]))
                        dbody.update(zip(rest, got))
                    if sparse and rest:                # the count pass gives every patch's length; only those below the best body so far are built
                        elig = [i for i in rest if codec.patch_elem(todo[i][1]) == todo[i][2][0]]
                        pairs = [(codec.flat_bytes(todo[i][1]), flats[i], todo[i][2][0]) for i in elig]
                        sizes = codec.patch_sizes_device_batch(lib, pairs)
                        take = [k for k, i in enumerate(elig) if 0 < sizes[k] < min(plain[i].numel(), dbody[i].numel(), flats[i].numel())]
                        built = codec.patch_build_device_batch(lib, [pairs[k] for k in take], [sizes[k] for k in take])
                        pbody.update({elig[k]: b.clone() for k, b in zip(take, built)})
                    del flats, decoded
            kept = []                              # (index, body, is a delta body)
            for i, (name, t, prm) in enumerate(todo):
                if i in same:
                    continue
                b, is_delta = plain[i], False
                if i in dbody and dbody[i].numel() < b.numel():        # (a tie goes to the plain body)
                    b, is_delta = dbody[i], True
                if i in pbody and pbody[i].numel() < min(b.numel(), t.numel() * t.element_size()):      # (… and the patch only when it is smaller than either)
                    b, is_delta = pbody[i], "sparse"
                if b.numel() < t.numel() * t.element_size():
                    kept.append((i, b, is_delta))
            offs, o = [], 0
            for (_, b, _) in kept:
                offs.append(o)
                o += _round_up(b.numel())
            packed = torch.empty(max(o, 1), dtype=torch.uint8, device=dev)
            for (i, b, is_delta), off in zip(kept, offs):
                name, t, prm = todo[i]
                packed[off:off + b.numel()].copy_(b)
                if is_delta == "sparse":
                    e = entries[name] = _Entry(name, t.dtype, t.shape, t.numel() * t.element_size(), params=prm)
                    e.patch, e.delta, e.base = packed[off:off + b.numel()], "sparse", refs[i]
                    e.entries = _patch_entries(e.nbytes, e.P, b.numel())
                    continue
                e = entries[name] = _Entry(name, t.dtype, t.shape, t.numel() * t.element_size(), body=packed[off:off + b.numel()], params=prm)
                if is_delta:
                    e.delta, e.base = True, refs[i]
            for i, (name, t, prm) in enumerate(todo):
                if i in same:                      # nothing of its own: the base's tensor itself, or a decode of the base's body
                    ref = refs[i]
                    e = entries[name] = _Entry(name, t.dtype, t.shape, t.numel() * t.element_size(), raw=ref[1] if ref[0] == "tensor" else None, params=prm)
                    e.delta, e.base = "same", ref
                elif name not in entries:
                    entries[name] = _Entry(name, t.dtype, t.shape, t.numel() * t.element_size(), raw=t.clone())
            for (name, t, _), ref in zip(todo, refs):
                entries[name].restore = ref
            keep.append(packed)
            held += o
            del plain, dbody, pbody            # (the bodies not kept go back to the allocator)
        for name, t in sd.items():
            if entries[name].restore is None:
                entries[name].restore = matches(name, t.detach())
        held += sum(e.nbytes for e in entries.values() if not e.compressed and e.delta not in ("same", "sparse"))
        if base is not None:
            keep.append(base)
        for name, h in heads.items():
            entries[name].head = h
        store = cls(dev, [entries[name] for name in sd.keys()], held, keep=keep)
        store._digests = recorded
        if index:
            store.build_index(deltas=(index == "deltas"))
        return store

    # ---- re-parenting a variant ------------------------------------------------------------------------------------
    @staticmethod
    def _node_key(ref):
        """What two walks compare: a plain tensor by its memory, an entry that holds its tensor plainly by that tensor, any other entry by itself."""
        if ref[0] == "entry" and ref[2].raw is not None and ref[2].delta is False:
            ref = ("tensor", ref[2].raw)
        if ref[0] == "tensor":
            return ("t", ref[1].data_ptr(), ref[1].numel() * ref[1].element_size())
        return ("e", id(ref[2]))

    @classmethod
    def _patch_path(cls, ref):
        """Walk base links from `ref` while the entry is "sparse" or "same" -> [(node key, the patches on the way there)]: the first element is `ref` itself with
        no patch, the last the first node that is neither (a plain tensor, or an entry with a body of its own)."""
        path, patches = [(cls._node_key(ref), ())], []
        while ref[0] == "entry" and ref[2].delta in ("sparse", "same"):
            e = ref[2]
            if e.delta == "sparse":
                patches.append(e.patch)
            ref = e.base
            path.append((cls._node_key(ref), tuple(patches)))
        return path

    def rebased(self, onto):
        """The same tensors as a NEW variant store whose base is `onto` — a ResidentCheckpoint on this store's device — without decoding what is kept as
        "znp1" patches: patches are XOR lists, so the patch of a tensor over `onto` is the XOR-merge (zn_patch_merge_batch_dev) of the patches
        that lie between the two.

            flat = s3.rebased(base)        # a chain s3 -> s2 -> s1 -> base becomes one store directly over base
            sw = ft_b.rebased(ft_a)        # siblings over one base: B as patches over A
            sw.apply_(model)               # live weights that hold A's values now hold B's: one sparse pass; sw.revert_(model) goes back

        Per tensor both stores' base links are walked while the entry is "sparse" or "same"; where the walks meet — the same entry, or the same plain base
        tensor — the new patch is the merge of every patch on both paths ("same" links bring nothing; `onto` lying on this store's own path has an empty
        side).  The pairwise merges of all tensors of a round are ONE batched call, intermediate results live in that round's scratch arena, the final patches
        are packed at 256-byte boundaries of one allocation.  An empty merge makes the entry "same" over `onto`; a patch shorter than the tensor makes it
        "sparse".  Every other tensor — no common node, a delta body or plain body on a path, a merged patch not smaller than the tensor, a tensor the codec
        does not take, a name `onto` lacks or has with another dtype or shape — is decoded from this store, in groups of at most _BUILD_GROUP_BYTES, and built
        by from_state_dict(..., base=onto, sparse=True): nothing is refused, the result is always complete.
        A merged patch does NOT compete with the delta body the tensor might also have over `onto`: rebased keeps patches as patches.
        The new store decodes exactly the bytes this one decodes, through every entry point; this store's recorded digests carry over unchanged.  It has no
        index (build_index on it behaves as on any variant), keeps `onto` alive and nothing else of the old chain, and changes neither store."""
        if not isinstance(onto, ResidentCheckpoint):
            raise ValueError("rebased: onto is a ResidentCheckpoint")
        if onto.device != self.device:
            raise ValueError(f"rebased: onto is a store on {self.device}, not on {onto.device}")
        dev, lib = self.device, _capi.lib()
        refs = self._base_items(onto, dev)
        lists, fallback, entries = {}, [], {}
        for name, e in self._entries.items():
            ref = refs.get(name)
            rb = None if ref is None else ref[1] if ref[0] == "tensor" else ref[2]
            ok = (rb is not None and rb.dtype == e.dtype and tuple(rb.shape) == e.shape and e.P in (1, 2, 4) and e.P == torch.empty(0, dtype=e.dtype).element_size()
                  and 0 < e.nbytes and e.nbytes // e.P < (1 << 32))
            if ok and ref[0] == "entry":           # (what a "same" or sparse entry can decode over: from_state_dict's delta_ok)
                ok = rb.decoded and (rb.P, rb.bits, rb.byts, rb.chunk) == (e.P, e.bits, e.byts, e.chunk)
            found = None
            if ok:
                mine, theirs = self._patch_path(("entry", self, e)), self._patch_path(("entry", onto, onto._entries[name]))
                at = {k: ps for k, ps in reversed(theirs)}      # (the nearest occurrence of a key wins)
                for k, ps in mine:
                    if k in at:
                        found = list(ps) + list(at[k])
                        break
            if found is None:
                fallback.append(name)
            else:
                lists[name] = found
        # rounds of pairwise merges, every tensor's in one call: a chain of depth d is d - 1 calls for the whole store
        scratch = []                               # the rounds' arenas: intermediate patches are views of them
        with _device_of(dev):
            while any(len(ps) > 1 for ps in lists.values()):
                todo = [name for name, ps in lists.items() if len(ps) > 1]
                got = codec.patch_merge_device_batch(lib, [(lists[n][0], lists[n][1], self._entries[n].nbytes, self._entries[n].P) for n in todo])
                scratch.append(got)
                for n, g in zip(todo, got):
                    lists[n] = ([g] if g is not None else []) + lists[n][2:]
        kept = []
        for name, ps in lists.items():
            if ps and ps[0].numel() >= self._entries[name].nbytes:
                fallback.append(name)              # a patch that is not smaller than the tensor: the build decides what it is kept as
            else:
                kept.append((name, ps[0] if ps else None))
        offs, o = {}, 0
        for name, p in kept:
            if p is not None:
                offs[name] = o
                o += _round_up(p.numel())
        packed = torch.empty(max(o, 1), dtype=torch.uint8, device=dev)
        for name, p in kept:
            e, ref = self._entries[name], refs[name]
            prm = (e.P, e.bits, e.byts, e.chunk)
            if p is None:
                ne = _Entry(name, e.dtype, e.shape, e.nbytes, raw=ref[1] if ref[0] == "tensor" else None, params=prm)
                ne.delta = "same"
            else:
                ne = _Entry(name, e.dtype, e.shape, e.nbytes, params=prm)
                ne.patch = packed[offs[name]:offs[name] + p.numel()]
                ne.patch.copy_(p)
                ne.delta, ne.entries = "sparse", _patch_entries(e.nbytes, e.P, p.numel())
            ne.base = ne.restore = ref
            ne.head = e.head
            entries[name] = ne
        del scratch, lists
        keep, held = [packed], o
        order = {n: i for i, n in enumerate(self._entries)}
        fallback.sort(key=order.__getitem__)
        groups, cur, size = [], [], 0
        for name in fallback:
            nb = self._entries[name].nbytes
            if cur and size + nb > self._BUILD_GROUP_BYTES:
                groups.append(cur)
                cur, size = [], 0
            cur.append(name)
            size += nb
        if cur:
            groups.append(cur)
        for grp in groups:
            sub = type(self).from_state_dict(self.get_tensors(grp), dev, base=onto, sparse=True)
            entries.update(sub._entries)
            keep += [k for k in sub._keep if k is not onto]
            held += sub._held
        keep.append(onto)
        store = type(self)(dev, [entries[name] for name in self._entries], held, keep=keep)
        store._digests = dict(self._digests) if self._digests is not None else None
        store._metadata = self._metadata
        return store

    # ---- the sync index ---------------------------------------------------------------------------------------------------------
    #: dtypes build_index() indexes by default; build_index(all_dtypes=True) indexes every compressed tensor.  The rule: a dtype whose hinted decode does
    #: not measure faster than the unhinted one by more than the run's own A/A spread (scripts/bench_resident.py --index) is taken out of this set.
    #: No dtype has been timed on a device yet, so none has been taken out.
    INDEX_DTYPES = frozenset(_INDEX_DTYPES)

    def build_index(self, names=None, all_dtypes=False, deltas=False):
        """Decode hints for the resident bodies (include/zipnn_hip.h): one pass over each body records where the decoder's sub-blocks
        start — about a byte per 16-24 bytes of Huffman-coded plane — so that every later decode of it (get_tensor, get_tensors, get_slice, plan,
        hook: no further arguments) starts them there instead of finding them by speculation.  The hints sit beside the bodies in device memory,
        never in them, and are advice: the decoded bytes are the same with and without.  names: the tensors to index (default: every compressed
        one); a dtype that measured no gain is left out unless all_dtypes is set.  Tensors already indexed keep their index; plans and hooks made
        before this call go on decoding without.
        deltas=True: the delta bodies of a variant store (info(n)["delta"] is True) get an index as well, of the kind the delta decode reads
        (ZN_HINT_DELTA: every Huffman-coded plane of a chunk has hints, valid for the delta instances' sub-block sizes) — built against the body where
        it lies; get_tensor(s), get_slice, plan, hook, verify, apply_ and revert_ then decode those bodies from it, with no further arguments.  A
        "same" entry holds no body and has nothing to index.  Without it (the default) delta bodies get none."""
        lib = _capi.lib()
        todo = []
        for name in (self.keys() if names is None else names):
            e = self._entries[name]
            if e.compressed and e.nbytes and e.hints is None and (all_dtypes or e.dtype in self.INDEX_DTYPES) and (e.delta is False or (deltas and e.delta is True)):
                todo.append(e)
        if not todo:
            return 0
        with _device_of(self.device):
            stream = _stream_of(self.device)

            def kind(e):                           # (None: the entry points without a kind, as ever)
                return _capi.HINT_DELTA if e.delta is True else None
            sizes = [lib.hint_size_dev(e.window(0, e.chunks, None), stream, kind(e)) for e in todo]
            offs, o = [], 0
            for n in sizes:
                offs.append(o)
                o += _round_up(n)
            buf = torch.empty(max(o, 1), dtype=torch.uint8, device=self.device)
            for e, n, off in zip(todo, sizes, offs):
                lib.hint_build_dev(e.window(0, e.chunks, None), buf.data_ptr() + off, n, stream, kind(e))
                e.hints = buf[off:off + n]
        self._index = (self._index or ()) + (buf,)
        self._index_bytes += o
        self._held += o
        return o

    def drop_index(self):
        """Free the hints.  Plans and hooks made while the index existed must be closed / removed first: they refer to it by address."""
        for e in self._entries.values():
            e.hints = None
        self._held -= self._index_bytes
        self._index, self._index_bytes = None, 0

    @property
    def index_bytes(self):
        """Bytes of device memory the index holds (part of resident_bytes)."""
        return self._index_bytes

    def _launch_sets(self, work, keep=None):
        """work: [(entry, chunk_lo, chunk_hi, flat uint8 destination of the window)] -> the batched calls that fill the destinations, in the order they
        must run on one stream: [("hinted" | "window", items)].  A plain entry: one window item.  A delta entry over a plain base tensor: the item with
        d_delta at that tensor (the library offsets it to the window).  Over a resident base: the BASE's own sets decode the same chunk window into the
        destination first — hinted if the base has an index, through its own base if it is a variant itself — and the delta's window then runs IN PLACE over
        it (d_dst == d_delta + chunk_lo * chunk, include/zipnn_hip.h).  A "same" entry is the base's decode alone.  A SPARSE entry adds a third kind of set,
        ("patch", items of zn_patch_apply_batch_dev), behind the others: over a plain base tensor the item has d_base at that tensor (the window's bytes are
        copied, then patched); over a resident base the base's own sets decode the window into the destination — hinted where it has an index, through its own
        patches if it is a sparse variant itself — and the patch's window is applied in place.  keep: a list that receives what the items refer to by address."""
        keep = keep if keep is not None else []

        def ptr(dst):                              # (a destination may also be given by its address)
            return dst if isinstance(dst, int) else dst.data_ptr()
        via, plain, delta, patch = {}, [], [], []      # (delta: (entry, lo, hi, destination address, base address); patch: items of the apply call)
        for e, lo, hi, dst in work:
            if e.delta is False:
                plain.append((e, lo, hi, dst))
                continue
            if e.delta == "sparse":
                keep.append(e.patch)
                if e.base[0] == "tensor":
                    bt = codec.flat_bytes(e.base[1])
                    keep.append(bt)
                    patch.append(e.patch_item(lo, hi, ptr(dst), bt.data_ptr()))
                else:
                    _, bstore, be = e.base
                    via.setdefault(id(bstore), (bstore, []))[1].append((be, lo, hi, dst))
                    patch.append(e.patch_item(lo, hi, ptr(dst)))
                continue
            if e.base[0] == "tensor":                  # (a delta entry: "same" over a plain tensor is that tensor, never work)
                bt = codec.flat_bytes(e.base[1])
                keep.append(bt)
                delta.append((e, lo, hi, ptr(dst), bt.data_ptr()))
            else:
                _, bstore, be = e.base
                via.setdefault(id(bstore), (bstore, []))[1].append((be, lo, hi, dst))
                if e.delta is True:
                    delta.append((e, lo, hi, ptr(dst), ptr(dst) - lo * e.chunk))
        sets = []
        for bstore, w in via.values():
            sets += bstore._launch_sets(w, keep)
        if plain:
            if any(e.hints is not None for e, _, _, _ in plain):
                keep += [e.hints for e, _, _, _ in plain if e.hints is not None]
                sets.append(("hinted", [e.hinted(lo, hi, ptr(dst)) for e, lo, hi, dst in plain]))
            else:
                sets.append(("window", [e.window(lo, hi, ptr(dst)) for e, lo, hi, dst in plain]))
        sets += self._delta_sets(delta, keep)
        if patch:
            sets.append(("patch", patch))
        keep += [dst for _, _, _, dst in work if not isinstance(dst, int)]
        return sets

    @staticmethod
    def _delta_sets(delta, keep=None):
        """delta: [(delta entry, chunk_lo, chunk_hi, destination address, address of the whole tensor's base)] -> their launch set: window items, or — where
        a body has an index (build_index(deltas=True)) — hinted items of kind HINT_DELTA, which the delta instances read."""
        if not delta:
            return []
        if any(e.hints is not None for e, _, _, _, _ in delta):
            if keep is not None:
                keep += [e.hints for e, _, _, _, _ in delta if e.hints is not None]
            return [("hinted", [e.hinted(lo, hi, d, b) for e, lo, hi, d, b in delta])]
        return [("window", [e.window(lo, hi, d, b) for e, lo, hi, d, b in delta])]

    def _run_sets(self, sets, check):
        """The calls of _launch_sets, in order, on the current stream.  check=False: the sets behind the first add their verdict to the first's
        (zn_decode_status_chain), so that status() speaks for all of them."""
        lib = _capi.lib()
        with _device_of(self.device):
            stream = _stream_of(self.device)
            try:
                for i, (kind, items) in enumerate(sets):
                    if i == 1 and not check:
                        lib.decode_status_chain(True)
                    if kind == "hinted":
                        lib.decompress_hinted_batch_dev(items, stream, check)
                    elif kind == "patch":
                        lib.patch_apply_batch_dev(items, stream, check)
                    else:
                        lib.decompress_window_batch_dev(items, stream, check)
            finally:
                if len(sets) > 1 and not check:
                    lib.decode_status_chain(False)

    def _decode(self, work, check):
        """work: [(entry, chunk_lo, chunk_hi, flat uint8 destination)] -> batched decodes on the current stream, hinted where an entry has an index; one
        launch set for a plain store, base + delta for a variant (_launch_sets)."""
        self._run_sets(self._launch_sets(work), check)

    # ---- introspection --------------------------------------------------------------------------------------------------------
    def keys(self):
        return list(self._entries.keys())

    def __contains__(self, name):
        return name in self._entries

    def __len__(self):
        return len(self._entries)

    def info(self, name):
        e = self._entries[name]
        return {"shape": list(e.shape), "dtype": e.dtype, "nbytes": e.nbytes, "compressed": e.compressed or e.patch is not None, "delta": e.delta,
                "resident_bytes": e.body.numel() if e.compressed else e.patch.numel() if e.patch is not None else (0 if e.delta == "same" else e.nbytes),
                "patch_entries": e.entries if e.patch is not None else None,
                "index_bytes": e.hints.numel() if e.hints is not None else 0,
                "digest": self._digests[name] if self._digests is not None else None}

    @property
    def nbytes(self):
        """Bytes of the tensors as a model would hold them."""
        return sum(e.nbytes for e in self._entries.values())

    @property
    def resident_bytes(self):
        """Bytes of device memory the store holds."""
        return self._held

    # ---- writing the store down -----------------------------------------------------------------------------------
    def _frame_header(self, e):
        """-> the frame header save_file writes in front of e's body: the torch-format header (with the shape extension) of a plain body — what
        compress_safetensors_file writes —, the BYTE-format header with the delta flag (byte 9 = 1, no shape extension) of a delta body: the form the
        reference's delta decode takes.  Bytes 0-15 are the entry's own (version, method, reorder modes, chunk exponent, dtype code)."""
        head = e.head
        if head is None:
            head = ZipNN(input_format="torch", bytearray_dtype=e.dtype, method=COMPRESSION_METHOD).torch_frame_plan(torch.empty(e.shape, dtype=e.dtype, device="meta"))[0][:16]
        h = bytearray(HEADER_LEN)
        h[:16] = head
        h[8], h[9] = (EnumFormat.BYTE.value, 1) if e.delta is True else (EnumFormat.TORCH.value, 0)
        ext = b"" if e.delta is True else pack_shape(e.shape)
        h[16:24] = e.nbytes.to_bytes(8, "little")
        h[24:32] = (HEADER_LEN + len(ext) + e.body.numel()).to_bytes(8, "little")      # (the total length, as the core writes it)
        return bytes(h) + ext

    def save_file(self, path, digests=None, metadata=None, sparse=False):
        """Write the store as a `.znn.safetensors` file -> path.  Any store: plain, indexed, a variant, a variant of a variant.  The bodies go out as they lie in
        device memory — one transfer to the host per allocation that holds them (one for a store from from_state_dict or from_file), never recompressed —,
        each behind the frame header that describes its parameters; a tensor whose header + body would not be smaller than the tensor is written as it is
        (the rule of compress_safetensors_file; it costs one decode of that tensor), and so is every tensor the store holds plainly.  A plain store's file is
        the file compress_safetensors_file writes for the same tensors, byte for byte.
        A VARIANT writes a delta file: the metadata key `znn_delta` lists the tensors coded over the base — "delta": the frame's body is tensor ^ base, its
        header the byte-format one with the delta flag; "same": a zero-length entry, the tensor is the base's — and `base_digests`, the content digests of the
        BASE's tensors: a base store's recorded ones, else one batched digest of the base's decoded or live tensors.  Read it back with
        from_file(path, device, base=...) / safetensors_io.load_file(path, device, base=...).
        digests: None writes `znn_digests` when the store has digests; True computes them (one decode of every tensor) where it has none; False omits them.
        metadata: the file's other metadata (default: what from_file found in the store's own file, else {"format": "pt"}).  The sync index is not saved:
        from_file(index=True) rebuilds it.
        sparse: a store with SPARSE entries is refused (ValueError naming them, before `path` is touched) unless sparse=True, which writes them:
        "sparse" under `znn_delta`, whose version is then 2 — earlier builds of this library refuse such a file by that number.  The entry is L + 15 bytes: the
        patch as it lies in device memory — it leaves in the same trip as the bodies — at the entry's first offset in the data section that is a multiple of 16,
        zero bytes around it, so that a loaded patch is a 16-byte aligned view of the uploaded data section.  safetensors decides where an entry lies: the file
        is written with zero-filled entries under a temporary name, the patches are put at their places, and the file is renamed to `path`.  A patch whose
        L + 15 bytes would not be smaller than the tensor is written as the tensor (one decode).  A store without sparse entries writes the same file either way."""
        import os
        from safetensors.torch import save_file as st_save_file
        from . import safetensors_io
        lib = _capi.lib()
        patched = [e.name for e in self._entries.values() if e.patch is not None]
        if patched and not sparse:
            raise ValueError(f"save_file: the store holds sparse entries (DESIGN §3.10): {', '.join(repr(n) for n in patched[:8])}{' …' if len(patched) > 8 else ''}"
                             " — pass sparse=True to write them as patches (DESIGN §3.11), or build the store without sparse=True")
        recorded = None
        if digests or (digests is None and self._digests is not None):
            recorded = self._digests if self._digests is not None else self._decoded_digests(self.keys())
        # which bodies go out as frames and which patches as they are, and the one trip of each allocation that holds them
        framed, roots = {}, {}
        for e in self._entries.values():
            hdr, held = (self._frame_header(e), e.body) if e.compressed else (b"", e.patch)
            if held is not None and len(hdr) + held.numel() + (safetensors_io.SPARSE_SLACK if e.patch is not None else 0) < e.nbytes:
                root = held._base if held._base is not None else held
                off = held.storage_offset() - root.storage_offset()
                key = (root.data_ptr(), root.numel())
                span = roots.setdefault(key, [root, off, off + held.numel()])
                span[1], span[2] = min(span[1], off), max(span[2], off + held.numel())
                framed[e.name] = (hdr, key, off)
        host = {}
        with _device_of(self.device):
            for key, (root, lo, hi) in roots.items():
                host[key] = (memoryview(codec.to_host(lib, root.reshape(-1)[lo:hi])), lo)
        tensors, infos, kinds, refs, patches = {}, {}, {}, {}, {}
        order = sorted(self._entries)                              # (the order safetensors walks a file's names in: the metadata lists keep it, as compress_safetensors_file's do)
        for name in order:
            e = self._entries[name]
            like = torch.empty(e.shape, dtype=e.dtype, device="meta")
            if name in framed and e.patch is not None:             # a placeholder: the patch goes in once safetensors has said where the entry lies
                hdr, key, off = framed[name]
                mv, lo = host[key]
                patches[name] = mv[off - lo: off - lo + e.patch.numel()]
                tensors[name] = torch.zeros(e.patch.numel() + safetensors_io.SPARSE_SLACK, dtype=torch.uint8)
                infos[name] = build_compressed_tensor_info(like)
                kinds[name], refs[name] = "sparse", e.base
            elif name in framed:
                hdr, key, off = framed[name]
                mv, lo = host[key]
                frame = codec.new_bytearray(len(hdr) + e.body.numel())
                frame[:len(hdr)] = hdr
                frame[len(hdr):] = mv[off - lo: off - lo + e.body.numel()]
                tensors[name] = torch.frombuffer(frame, dtype=torch.uint8)
                infos[name] = build_compressed_tensor_info(like)
                if e.delta is True:
                    kinds[name], refs[name] = "delta", e.base
            elif e.delta == "same":
                tensors[name] = torch.empty(0, dtype=torch.uint8)
                infos[name] = build_compressed_tensor_info(like)
                kinds[name], refs[name] = "same", e.base
            else:
                tensors[name] = (self.get_tensor(name) if e.decoded else e.raw).detach().cpu().contiguous()
        metadata = dict(metadata) if metadata is not None else dict(self._metadata or {})
        if not metadata:
            metadata = {"format": "pt"}
        set_compressed_tensors_metadata(infos, metadata)
        if recorded is not None:
            safetensors_io._set_digests_metadata(metadata, order, [recorded[n] for n in order])
        if kinds:
            safetensors_io._set_delta_metadata(metadata, kinds, self._ref_digests(refs, self.device))
        if not patches:
            st_save_file(tensors, path, metadata)
            return path
        tmp = f"{path}.tmp{os.getpid()}"
        try:
            st_save_file(tensors, tmp, metadata)
            _, layout, data_start = safetensors_io._read_layout(tmp)
            with open(tmp, "r+b") as f:
                for name, mv in patches.items():
                    lo, hi = layout[name][2], layout[name][3]
                    at = (lo + 15) // 16 * 16                      # (of the DATA SECTION: what a reader uploads to an aligned allocation)
                    assert hi - lo == len(mv) + safetensors_io.SPARSE_SLACK and at + len(mv) <= hi
                    f.seek(data_start + at)
                    f.write(mv)
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        return path

    # ---- decoding -------------------------------------------------------------------------------------------------------------
    def scratch_bytes(self, names):
        """Size of an `into` buffer for `names`: every compressed tensor at a multiple of 256 bytes."""
        return self._layout(names)[1]

    def _layout(self, names):
        offs, o = {}, 0
        for name in names:
            e = self._entries[name]
            if e.decoded and name not in offs:
                offs[name] = o
                o += _round_up(e.nbytes)
        return offs, o

    def _destinations(self, names, into):
        """-> ({name: tensor view}, [(entry, flat uint8 destination)]) — compressed tensors inside `into` (allocated when None), others as they are."""
        names = list(names)
        offs, total = self._layout(names)
        if into is None:
            into = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
        elif into.dtype != torch.uint8 or into.device != self.device or not into.is_contiguous() or into.numel() < total:
            raise ValueError(f"into: a contiguous uint8 tensor of at least {total} bytes on {self.device}")
        views, work = {}, []
        for name in names:
            e = self._entries[name]
            if not e.decoded:
                views[name] = e.raw
            elif name not in views:
                flat = into[offs[name]: offs[name] + e.nbytes]
                views[name] = e.view(flat)
                work.append((e, flat))
        return views, work

    def get_tensor(self, name, out=None, check=True):
        """The decoded tensor: a new one, or `out` (same dtype and shape, contiguous).  check=False leaves the verdict to status()."""
        e = self._entries[name]
        if out is not None and (out.dtype != e.dtype or tuple(out.shape) != e.shape or out.device != self.device or not out.is_contiguous()):
            raise ValueError(f"out: a contiguous {e.dtype} tensor of shape {list(e.shape)} on {self.device}")
        if not e.decoded:
            return e.raw.clone() if out is None else out.copy_(e.raw)
        if out is None:
            out = torch.empty(e.shape, dtype=e.dtype, device=self.device)
        if e.nbytes:
            self._decode([(e, 0, e.chunks, codec.flat_bytes(out))], check)
        return out

    def get_tensors(self, names, into=None, check=True):
        """Several tensors by ONE batched launch set -> {name: tensor}.  The decoded tensors are views of one buffer (`into`, a uint8 tensor of
        scratch_bytes(names) bytes, or a new allocation), each at a multiple of 256 bytes; tensors the store holds uncompressed are returned as
        they are (views of the store: do not write to them)."""
        views, work = self._destinations(names, into)
        if work:
            self._decode([(e, 0, e.chunks, flat) for e, flat in work], check)
        return views

    def get_slice(self, name):
        """An object with the protocol of safetensors' slices (and of `CompressedSlice`): get_shape(), get_dtype(), indexing."""
        return ResidentSlice(self, self._entries[name])

    def plan(self, names, into=None):
        """A prepared decode of `names` (zn_plan): see ResidentPlan."""
        return ResidentPlan(self, names, into)

    def status(self, stream=None):
        """Wait for the stream and raise what the last check=False decode on this device would have raised (zn_decode_status)."""
        with _device_of(self.device):
            _capi.lib().decode_status(_stream_of(self.device, stream))

    # ---- content digests ("zn64-1") ------------------------------------------------------------------------------
    @property
    def has_digests(self):
        return self._digests is not None

    def _need_digests(self):
        if self._digests is None:
            raise ValueError("the store has no digests: build it with digests=True")

    def digests(self):
        """{name: digest} of the tensors' bytes as the store recorded them (from_state_dict / from_file with digests=True): ints below 2^64.  An
        error-detecting code, not a cryptographic hash."""
        self._need_digests()
        return dict(self._digests)

    def _decoded_digests(self, names):
        """-> {name: digest of what the store decodes for it NOW}: every tensor through the store's normal path — hinted if indexed, base followed by an in-place
        delta for a variant — into ONE scratch buffer sized for the largest tensor (never a second copy of the model), as many tensors per group as fit;
        each group's tensors digested by one zn_digest_batch_dev call behind its decode on the current stream (the stream orders the buffer's reuse); tensors the
        store holds plainly are digested where they lie; one read-back at the end.  The decodes are unchecked: the digest is the verdict."""
        lib = _capi.lib()
        names = list(dict.fromkeys(names))
        ents = [self._entries[n] for n in names]
        plain = [e for e in ents if not (e.decoded and e.nbytes)]
        todo = [e for e in ents if e.decoded and e.nbytes]
        out = torch.empty(max(len(names), 1), dtype=torch.int64, device=self.device)      # slot order: the plain tensors, then the decoded ones group by group
        with _device_of(self.device):
            stream = _stream_of(self.device)
            if plain:
                nothing = torch.empty(0, dtype=torch.uint8, device=self.device)
                codec.digest_device_batch(lib, [codec.flat_bytes(e.raw) if e.raw is not None else nothing for e in plain], stream, out=out[:len(plain)])
            if todo:
                scratch = torch.empty(max(_round_up(e.nbytes) for e in todo), dtype=torch.uint8, device=self.device)
                groups, cur, o = [], [], 0
                for e in todo:
                    if cur and o + _round_up(e.nbytes) > scratch.numel():
                        groups.append(cur)
                        cur, o = [], 0
                    cur.append((e, scratch[o:o + e.nbytes]))
                    o += _round_up(e.nbytes)
                groups.append(cur)
                k = len(plain)
                for grp in groups:
                    self._decode([(e, 0, e.chunks, flat) for e, flat in grp], False)
                    codec.digest_device_batch(lib, [flat for _, flat in grp], stream, out=out[k:k + len(grp)])
                    k += len(grp)
            vals = codec.digests_to_ints(out[:len(names)])
        return dict(zip([e.name for e in plain + todo], vals))

    def verify(self, names=None, raise_=True):
        """Is what the store decodes still what it was built from?  Decodes every named tensor (default: all) through the store's normal path into a scratch
        buffer sized for the largest one, digests the decoded bytes on the device and compares with the recorded digests (_decoded_digests: one digest launch
        per group, one read-back).  -> {name: bool}; raise_=True: DigestMismatch (a ValueError) naming the tensors that differ."""
        self._need_digests()
        names = self.keys() if names is None else list(names)
        got = self._decoded_digests(names)
        res = {n: got[n] == self._digests[n] for n in names}
        bad = [n for n in names if not res[n]]
        if bad and raise_:
            raise codec.DigestMismatch(bad, "the store no longer decodes what it was built from")
        return res

    def _live_digests(self, pairs):
        """[(key, tensor)] -> {key: digest of the live tensor's bytes}: one batched launch, one read-back."""
        if not pairs:
            return {}
        with _device_of(self.device):
            vals = codec.digests_to_ints(codec.digest_device_batch(_capi.lib(), [codec.flat_bytes(t) for _, t in pairs], _stream_of(self.device)))
        return {k: v for (k, _), v in zip(pairs, vals)}

    def holds(self, target):
        """Do live tensors hold this store's values?  target: a module (named parameters and buffers) or a mapping of names to contiguous tensors on the
        store's device.  -> {name: bool} for the names the store has: the live tensors digested where they lie (one launch), compared with the recorded digests."""
        self._need_digests()
        tg = self._targets(target)
        live = self._live_digests([(e.name, t) for e, t in tg])
        return {e.name: live[e.name] == self._digests[e.name] for e, _ in tg}

    def _guard(self, target, want_base):
        """apply_ / revert_ with guard=True: raise DigestMismatch unless the target's tensors hold the base's values (want_base) or this store's.  The base's
        digests: a resident base's recorded ones; a base given as plain tensors has none recorded — what those tensors hold NOW is digested beside the target."""
        self._need_digests()
        tg = [(e, t) for e, t in self._targets(target) if e.nbytes]
        pairs, want = [(("live", e.name), t) for e, t in tg], {}
        for e, t in tg:
            if not want_base:
                want[e.name] = self._digests[e.name]
            elif e.restore is None:
                continue                           # (the base has no such tensor: apply_ overwrites whatever is there)
            elif e.restore[0] == "tensor":
                pairs.append((("base", e.name), e.restore[1]))
            else:
                bstore, be = e.restore[1], e.restore[2]
                if bstore._digests is None:
                    raise ValueError(f"guard: the base store has no digests (build it with digests=True) — {e.name}")
                want[e.name] = bstore._digests[be.name]
        got = self._live_digests(pairs)
        for (kind, name), _ in pairs:
            if kind == "base":
                want[name] = got[(kind, name)]
        bad = [e.name for e, _ in tg if e.name in want and got[("live", e.name)] != want[e.name]]
        if bad:
            raise codec.DigestMismatch(bad, "guard: the tensors do not hold the " + ("base's" if want_base else "variant's") + " values")

    # ---- a variant applied to live weights ------------------------------------------------------------------------------------
    def _targets(self, target):
        """target: a module (named parameters and buffers) or a mapping -> [(entry, tensor)] for the names the store has."""
        if isinstance(target, torch.nn.Module):
            items = dict(target.named_parameters())
            items.update(dict(target.named_buffers()))
        else:
            items = dict(target)
        out = []
        for name, t in items.items():
            e = self._entries.get(name)
            if e is None:
                continue
            t = t.detach()
            if t.dtype != e.dtype or tuple(t.shape) != e.shape or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{name}: a contiguous {e.dtype} tensor of shape {list(e.shape)} on {self.device}")
            out.append((e, t))
        return out

    def apply_(self, target, check=True, guard=False):
        """Turn live BASE weights into the fine-tune's, in place: `target` is a module or a mapping of names to contiguous tensors on the store's device that
        hold the base's values.  Delta entries are XORed over them by an in-place decode (d_dst == d_delta, include/zipnn_hip.h) — no second copy of the
        weights, no read of the base —, sparse entries are their patch applied in place (zn_patch_apply_batch_dev alone: only the changed elements are touched),
        plain entries are overwritten, "same" entries are left alone; one batched launch set on the current stream.
        Nothing is tracked: applying twice (or to tensors that do not hold the base) XORs the delta in twice and is the caller's mistake — unless guard=True
        (a store with digests): the live tensors are digested first and must hold the BASE's values, else DigestMismatch is raised before anything is touched.  If `target` is
        the very tensors this store holds as its plain base, the store decodes wrong values until revert_.  -> the names changed."""
        if guard:
            self._guard(target, True)
        work, inplace, done, patch = [], [], [], []
        for e, t in self._targets(target):
            if e.delta == "same" or not e.nbytes:
                continue
            if e.delta is True:
                inplace.append((e, 0, e.chunks, t.data_ptr(), t.data_ptr()))
            elif e.delta == "sparse":
                patch.append(e.patch_item(0, e.chunks, t.data_ptr()))
            elif e.compressed:
                work.append((e, 0, e.chunks, codec.flat_bytes(t)))
            else:
                t.copy_(e.raw)
            done.append(e.name)
        sets = self._launch_sets(work) + self._delta_sets(inplace) + ([("patch", patch)] if patch else [])
        self._run_sets(sets, check)
        return done

    def revert_(self, target, check=True, guard=False):
        """The inverse of apply_: delta and sparse entries by the same in-place call again (XOR is its own inverse), plain entries restored from the base — its
        tensor copied, or its resident body decoded — where the base has the tensor with the same dtype and shape.  -> the names that could NOT be
        reverted (plain entries with nothing to restore from: they stay as they are).  Reverting what was not applied is the caller's mistake — unless
        guard=True (a store with digests): the live tensors must hold THIS store's values, else DigestMismatch is raised before anything is touched."""
        if guard:
            self._guard(target, False)
        work, inplace, stay, via, patch = [], [], [], {}, []
        for e, t in self._targets(target):
            if e.delta == "same" or not e.nbytes:
                continue
            if e.delta is True:
                inplace.append((e, 0, e.chunks, t.data_ptr(), t.data_ptr()))
            elif e.delta == "sparse":
                patch.append(e.patch_item(0, e.chunks, t.data_ptr()))
            elif e.restore is None:
                stay.append(e.name)
            elif e.restore[0] == "tensor":
                if e.restore[1].data_ptr() == t.data_ptr():          # (the base's tensor IS the target: its values are gone)
                    stay.append(e.name)
                else:
                    t.copy_(e.restore[1])
            else:
                _, bstore, be = e.restore
                via.setdefault(id(bstore), (bstore, []))[1].append((be, 0, be.chunks, codec.flat_bytes(t)))
        sets = []
        for bstore, w in via.values():
            sets += bstore._launch_sets(w)
        sets += self._delta_sets(inplace) + ([("patch", patch)] if patch else [])
        self._run_sets(sets, check)
        return stay

    # ---- model integration ----------------------------------------------------------------------------------------------------
    def hook(self, model, modules=None):
        """Run `model` from the compressed store: see ResidentHook."""
        return ResidentHook(self, model, modules)


class ResidentSlice:
    """`ResidentCheckpoint.get_slice(name)`.  Rows a .. b-1 of a tensor are contiguous bytes of it, and the frame's chunks are independent: an
    index on the first dimension decodes only the chunks that cover its rows — a window decode from the resident body, on the device's current
    stream, with no host copy of anything and no synchronisation (ask `ResidentCheckpoint.status()` for the verdict).  Indices on later
    dimensions are applied to the decoded rows; an index on the first dimension that is not an int or a slice with a positive step decodes the
    whole tensor.  `last_chunk_range` is the (chunk_lo, chunk_hi) the last index operation decoded."""

    def __init__(self, store, entry):
        self._s, self._e = store, entry
        self.last_chunk_range = None

    def get_shape(self):
        return list(self._e.shape)

    def get_dtype(self):
        name = str(self._e.dtype).replace("torch.", "", 1)
        return _ST_DTYPE_NAME.get(name, name.upper())

    def __getitem__(self, idx):
        e, dev = self._e, self._s.device
        if not e.decoded:
            self.last_chunk_range = (0, 0)
            return e.raw[idx]
        n, shape, chunk = e.nbytes, e.shape, e.chunk
        a, b, sel, byte_lo, byte_hi, scalar = index_rows(idx, shape, n)
        if byte_hi <= byte_lo:
            self.last_chunk_range = (0, 0)
            t = torch.empty((max(b - a, 0),) + shape[1:], dtype=e.dtype, device=dev) if shape else torch.empty((), dtype=e.dtype, device=dev)
        else:
            c_lo, c_hi = byte_lo // chunk, (byte_hi + chunk - 1) // chunk
            self.last_chunk_range = (c_lo, c_hi)
            base = c_lo * chunk
            buf = torch.empty(min(c_hi * chunk, n) - base, dtype=torch.uint8, device=dev)      # (torch's allocator orders the block's reuse on the current stream: the decode runs there)
            self._s._decode([(e, c_lo, c_hi, buf)], False)
            t = buf[byte_lo - base: byte_hi - base].view(e.dtype).reshape(() if scalar else (b - a,) + shape[1:])
        return t[sel] if sel else t


class ResidentPlan:
    """`ResidentCheckpoint.plan(names, into=None)`: a zn_plan plus the buffer it decodes into.  Everything a batched decode works out on the
    host is done once, here; `run()` only launches — it neither waits for earlier device work nor copies anything to the device, so the decode
    of the next layer can be enqueued while this one still runs.  `tensors` are the views the runs fill; `status()` waits and raises what a
    checked decode would have raised; `close()` frees the plan (the store must outlive it).  The plan of a variant store over a resident base holds
    zn_plans of its own and of its base — the base's decode, then the delta windows in place over it —, launched back to back; their verdicts are
    chained (zn_decode_status_chain), so `status()` speaks for the whole run.  Sparse entries add a patch plan (zn_patch_plan) behind them: its table lives
    on the device too, and its run is launches only."""

    def __init__(self, store, names, into=None):
        self._store, self._lib = store, _capi.lib()
        self.tensors, work = store._destinations(names, into)
        self._keep = []
        self._stream = None
        self._hs = None
        sets = store._launch_sets([(e, 0, e.chunks, flat) for e, flat in work], self._keep)
        with _device_of(store.device):
            # (a plain store: one zn_plan, as ever; a variant over a resident base: the base's plan, then the plan of the delta windows that run in place over
            #  what it decoded — run() launches them back to back on one stream)
            hs = []
            try:
                for kind, items in (sets or [("window", [])]):
                    if kind == "patch":
                        hs.append((True, self._lib.patch_plan_create(items)))
                    else:
                        hs.append((False, self._lib.plan_create_hinted(items) if kind == "hinted" else self._lib.plan_create(items)))
            except Exception:
                self._destroy(hs)
                raise
            self._hs = hs

    def run(self, stream=None):
        if self._hs is None:
            raise RuntimeError("the plan is closed")
        self._stream = _stream_of(self._store.device, stream)
        with _device_of(self._store.device):
            try:
                for i, (is_patch, h) in enumerate(self._hs):
                    if i == 1:
                        self._lib.decode_status_chain(True)       # (the later plans add their verdict to the first one's: status() speaks for the whole run)
                    if is_patch:
                        self._lib.patch_plan_run(h, self._stream, False)
                    else:
                        self._lib.plan_run(h, self._stream, False)
            finally:
                if len(self._hs) > 1:
                    self._lib.decode_status_chain(False)
        return self.tensors

    def status(self):
        with _device_of(self._store.device):
            self._lib.decode_status(self._stream if self._stream is not None else _stream_of(self._store.device))

    def _destroy(self, hs):
        for is_patch, h in hs:
            if is_patch:
                self._lib.patch_plan_destroy(h)
            else:
                self._lib.plan_destroy(h)

    def close(self):
        if self._hs is not None:
            hs, self._hs = self._hs, None
            self._destroy(hs)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResidentHook:
    """`ResidentCheckpoint.hook(model, modules=None)`: the model computes from the compressed store.

    For each chosen sub-module (default: every module that directly owns parameters found in the store, by their names in
    `model.named_parameters()`) a forward pre-hook runs that module's plan into ONE scratch buffer shared by all of them — sized for the
    largest hooked module; where a hooked module contains hooked modules, for the largest sum along such a chain: a module decodes behind
    its hooked ancestors, whose parameters may be in use while it runs — and points the parameters' `.data` at the decoded views; a forward
    hook points them back at empty tensors.  A module whose forward is entered again while it is running (recursion) is not supported.  Both
    run on the current stream, so the stream orders the buffer's reuse: the next module's decode starts when this module's kernels are done.
    Between forwards the hooked parameters hold no storage.  `remove()` takes the hooks off and gives every parameter its own storage back,
    decoded once.

    Out of scope: a second scratch buffer to decode the next module while this one computes (prefetch), hipGraph capture of a hooked forward,
    and torch.compile — the hooks change `.data` from Python between modules.  Training is out of scope too: there is nothing to accumulate
    gradients into."""

    def __init__(self, store, model, modules=None):
        self._store = store
        chosen = None if modules is None else set(id(m) for m in modules)
        self._mods = []                        # (module, [(parameter, name)])
        for prefix, mod in model.named_modules():
            if chosen is not None and id(mod) not in chosen:
                continue
            own = [(p, (prefix + "." if prefix else "") + pname) for pname, p in mod.named_parameters(recurse=False)]
            own = [(p, name) for p, name in own if name in store]
            for p, name in own:
                i = store.info(name)
                if tuple(p.shape) != tuple(i["shape"]) or p.dtype != i["dtype"]:
                    raise ValueError(f"{name}: the model has {p.dtype} {list(p.shape)}, the store {i['dtype']} {i['shape']}")
            if own:
                self._mods.append((mod, own))
        # A hooked module's forward may call a hooked descendant while its own parameters are still in use (a block with a learned scale beside its Linear
        # children): along such a chain every module decodes into a region of its own — a module starts where its hooked ancestors end —, and modules that
        # are not nested share the buffer from the same offset.
        hooked = {id(mod): store.scratch_bytes([name for _, name in own]) for mod, own in self._mods}
        start = {}

        def walk(mod, off):
            if id(mod) in hooked:
                start[id(mod)] = max(start.get(id(mod), 0), off)      # (a module reachable along two paths: behind the longer chain)
                off = start[id(mod)] + hooked[id(mod)]
            for child in mod.children():
                walk(child, off)
        walk(model, 0)
        need = max([start[id(mod)] + hooked[id(mod)] for mod, _ in self._mods] + [1])
        self.scratch = torch.empty(need, dtype=torch.uint8, device=store.device)
        self._plans, self._handles = [], []
        for mod, own in self._mods:
            plan = store.plan([name for _, name in own], into=self.scratch[start[id(mod)]: start[id(mod)] + max(hooked[id(mod)], 1)])
            self._plans.append(plan)
            self._handles.append(mod.register_forward_pre_hook(self._pre(plan, own)))
            self._handles.append(mod.register_forward_hook(self._post(own)))
            self._release(own)

    @staticmethod
    def _release(own):
        for p, _ in own:
            p.data = torch.empty(0, dtype=p.dtype, device=p.device)

    def _pre(self, plan, own):
        def pre(module, args):
            views = plan.run()
            for p, name in own:
                p.data = views[name]
        return pre

    def _post(self, own):
        def post(module, args, output):
            self._release(own)
        return post

    def status(self):
        """Wait for the current stream; raise what the last decode would have raised as a checked call."""
        self._store.status()

    def remove(self):
        for h in self._handles:
            h.remove()
        self._handles = []
        for (mod, own) in self._mods:
            for p, name in own:
                p.data = self._store.get_tensor(name)
        for plan in self._plans:
            plan.close()
        self._plans, self._mods = [], []
