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


def _itemsize(dtype):
    return dtype.itemsize


def _frame_params_for(dtype, shape, method=None, coders=None, like=None):
    """Which frame would a tensor of this dtype and shape be coded with?  -> (the first 16 bytes of its frame header, (P, bits, byts, chunk)).
    coders: a dict that keeps one ZipNN per dtype — what decides both — over the calls of one build; like: a tensor of that dtype and shape, where the caller has one."""
    coders = coders if coders is not None else {}
    if dtype not in coders:
        coders[dtype] = ZipNN(input_format="torch", bytearray_dtype=dtype, method=method or COMPRESSION_METHOD)
    hdr, P, bits, byts, chunk = coders[dtype].torch_frame_plan(like if like is not None else torch.empty(shape, dtype=dtype, device="meta"))
    return bytes(hdr[:16]), (P, bits, byts, chunk)


def _groups(items, size_of, limit):
    """items, in order -> lists of them of at most `limit` bytes each by size_of(item) (a larger item makes a group of its own)."""
    groups, cur, size = [], [], 0
    for it in items:
        nb = size_of(it)
        if cur and size + nb > limit:
            groups.append(cur)
            cur, size = [], 0
        cur.append(it)
        size += nb
    if cur:
        groups.append(cur)
    return groups


def _packed(sizes):
    """-> ([offset of each], total): buffers of these sizes back to back in one allocation, each at a multiple of ALIGN."""
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += _round_up(n)
    return offs, o


def _named_tensors(target):
    """A module (its named parameters and buffers) or a mapping of names to tensors -> {name: tensor}."""
    if isinstance(target, torch.nn.Module):
        items = dict(target.named_parameters())
        items.update(dict(target.named_buffers()))
        return items
    return dict(target)


_stream_of, _device_of = codec._stream_of, codec._device_of

# The kinds of launch set (_launch_sets) and the ZnLib methods that serve each: (the batched call, plan create, plan run, plan destroy)
_KINDS = {"window": ("decompress_window_batch_dev", "plan_create", "plan_run", "plan_destroy"),
          "hinted": ("decompress_hinted_batch_dev", "plan_create_hinted", "plan_run", "plan_destroy"),
          "patch": ("patch_apply_batch_dev", "patch_plan_create", "patch_plan_run", "patch_plan_destroy"),
          "strided": ("patch_apply_strided_batch_dev", None, None, None)}      # sparse entries on non-contiguous live tensors: a batched call only


def _launch(lib, steps, stream, check):
    """steps: [(call, its items or plan handle, _)], launched in order on `stream`.  check=False: the steps behind the first add their verdict to the first's
    (zn_decode_status_chain), so that one decode_status speaks for the whole run."""
    chain = len(steps) > 1 and not check
    try:
        for i, (call, arg, _) in enumerate(steps):
            if i == 1 and chain:
                lib.decode_status_chain(True)
            call(arg, stream, check)
    finally:
        if chain:
            lib.decode_status_chain(False)


class _BaseRef:
    """One tensor of a variant's base — what an entry decodes over (_Entry.base) and what revert_ restores from (_Entry.restore): a tensor that lies plainly
    on the device (`tensor`, held by reference and read where it lies), or an entry of a resident store (`store`, `entry`) that is decoded through that store."""
    __slots__ = ("tensor", "store", "entry")

    def __init__(self, tensor=None, store=None, entry=None):
        self.tensor, self.store, self.entry = tensor, store, entry

    @property
    def dtype(self):
        return (self.tensor if self.tensor is not None else self.entry).dtype

    @property
    def shape(self):
        return tuple((self.tensor if self.tensor is not None else self.entry).shape)

    def fits(self, dtype, shape):
        """Does the base hold this tensor with this dtype and shape?"""
        return self.dtype == dtype and self.shape == tuple(shape)

    def params(self, coders=None):
        """-> the frame parameters (P, bits, byts, chunk) the base tensor is coded with, or would be (coders: see _frame_params_for)."""
        if self.entry is not None:
            return (self.entry.P, self.entry.bits, self.entry.byts, self.entry.chunk)
        return _frame_params_for(self.dtype, self.shape, coders=coders, like=self.tensor)[1]

    def decodes_under(self, params, coders=None):
        """Can a delta body, a "same" or a sparse entry with these frame parameters decode over it?  A resident base decodes in its own chunks."""
        return (self.entry is None or self.entry.decoded) and self.params(coders) == tuple(params)

    @property
    def key(self):
        """What two walks of base links compare: a plain tensor by its memory, an entry that holds its tensor plainly by that tensor, any other entry by itself."""
        t = self.tensor
        if t is None and self.entry.raw is not None and self.entry.delta is False:
            t = self.entry.raw
        return ("t", t.data_ptr(), t.numel() * t.element_size()) if t is not None else ("e", id(self.entry))

    def flat(self):
        """-> the plain tensor's bytes where they lie, or None: the base holds the tensor compressed and it must be decoded."""
        return codec.flat_bytes(self.tensor) if self.tensor is not None else None


class _Entry:
    """One tensor of the store: a frame body in device memory (`body`, with its codec parameters), or the tensor itself (`raw`).
    In a variant store (ResidentCheckpoint.from_state_dict(..., base=...)): `delta` is True where the body encodes tensor ^ base, "same" where the tensor's
    bytes are the base's (no body; `raw` is the base's own tensor where the base holds it plainly) and False otherwise; `base` is what a delta or "same" entry
    decodes over and `restore` what revert_ puts back — a _BaseRef (the base's tensor, held by reference, or the base store and its entry) — or None.
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

    # the four kinds of entry (head: see above; the constructors below are the only places that set delta, base, patch and entries)
    @classmethod
    def framed(cls, name, dtype, shape, nbytes, body, params, head=None, base=None):
        """A frame body of its own: the tensor's, or (base: a _BaseRef) that of tensor ^ base."""
        e = cls(name, dtype, shape, nbytes, body=body, params=params)
        e.head, e.delta, e.base = head, base is not None, base
        return e

    @classmethod
    def held(cls, name, raw, head=None):
        """The tensor itself."""
        e = cls(name, raw.dtype, raw.shape, raw.numel() * raw.element_size(), raw=raw)
        e.head = head
        return e

    @classmethod
    def same(cls, name, dtype, shape, ref, params, head=None):
        """Nothing of its own: the base's tensor itself, or a decode of the base's body."""
        e = cls(name, dtype, shape, _numel(shape) * _itemsize(dtype), raw=ref.tensor, params=params)
        e.head, e.delta, e.base = head, "same", ref
        return e

    @classmethod
    def sparse(cls, name, dtype, shape, ref, params, patch, head=None):
        """A "znp1" patch over the base's bytes; params: the frame parameters the tensor would be coded with."""
        e = cls(name, dtype, shape, _numel(shape) * _itemsize(dtype), params=params)
        e.head, e.delta, e.base, e.patch = head, "sparse", ref, patch
        e.entries = _patch_entries(e.nbytes, e.P, patch.numel())
        return e

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
        mine = ft.sharded(base_shards, {name: (dim, lo, hi)})     # one tensor-parallel rank's narrow() of every tensor, over its shard of the base — patches are selected, not decoded

        ft.apply_({"o_proj.weight": live.t(), "up_proj.weight": fused[:, a:b]})     # live tensors at any strides that pass the injectivity test; ft.patch(name) for other shapes

        cap = ResidentCheckpoint.from_live({"o_proj.weight": live.t(), "up_proj.weight": fused[:, a:b]}, base)      # … and the way back: live weights captured as a variant store, patches built where they lie

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
        from . import safetensors_io
        dev = cls._work_device(device)
        lay = safetensors_io._read_layout(path)                        # (the container's header, read once: the metadata, and what the patches' check and the upload go by)
        meta = lay[0] if lay is not None else safetensors_io.read_metadata(path)
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
            over = safetensors_io._delta_over_base(path, meta, kinds, based)
            if verify_base:
                got = cls._ref_digests({name: ref for name, (_, _, ref) in over.items()}, dev)
                bad = [name for name in kinds if got[name] != want[name]]
                if bad:
                    raise codec.DigestMismatch(bad, f"{path}: the base does not hold what the delta was taken over")
        if lay is None:
            raise ValueError(f"{path}: the container names a dtype this loader does not know")
        patched = safetensors_io._read_sparse_entries(path, lay, {n: over[n][:2] for n, k in kinds.items() if k == "sparse"}, check_patches)
        up = safetensors_io._upload_file(path, dev, delta=delta is not None, lay=lay)
        framed = cls._file_frames(path, up, kinds, over)
        entries, extra = cls._file_entries(path, up, framed, kinds, over, patched)
        cls._link_restore(entries, based)
        store = cls(dev, entries, up.blob.numel() + extra, keep=(up.blob,) + ((base,) if base is not None else ()))
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
    def _file_frames(path, up, kinds, over):
        """from_file, the frames of an uploaded file -> {name: entry}: bodies that are views of the data section; a delta body's against what it is coded over."""
        framed = {}
        for (name, b0, hi, fp, _) in up.frames:
            _, P, bits, byts, chunk, n, tdt, shape = fp
            head = up.heads.get(name)
            ref = None
            is_delta = kinds.get(name) == "delta"
            if head is not None and (head[9] != 0) != is_delta:
                raise ValueError(f"{path}: {name!r}: the frame header says {'delta' if head[9] else 'no delta'}, znn_delta says otherwise")
            if is_delta:
                tdt, shape, ref = over[name]
                if n != _numel(shape) * _itemsize(tdt):
                    raise ValueError(f"{path}: {name!r}: a frame of {n} bytes for {tdt} {list(shape)}")
                if ref.entry is not None and ref.entry.chunk != chunk:
                    raise ValueError(f"{path}: {name!r} is coded in chunks of {chunk} bytes, the base holds it in chunks of {ref.entry.chunk}")
            framed[name] = _Entry.framed(name, tdt, shape if shape is not None else (n // max(_itemsize(tdt), 1),), n, up.blob[b0:hi], (P, bits, byts, chunk),
                                         head=head, base=ref)
        return framed

    @staticmethod
    def _file_entries(path, up, framed, kinds, over, patched):
        """from_file, every tensor of an uploaded file in file order -> ([entry], bytes held beside the data section): the frames, the "same" and sparse entries of a
        delta file (patched: safetensors_io._read_sparse_entries), the plain tensors as views of the data section."""
        blob, entries, extra = up.blob, [], 0
        for name, (dt, shape, lo, hi) in up.layout.items():
            if name in framed:
                e = framed[name]
            elif kinds.get(name) == "same":
                tdt, tshape, ref = over[name]
                if hi != lo:
                    raise ValueError(f"{path}: {name!r} is listed as \"same\" but holds {hi - lo} bytes")
                e = _Entry.same(name, tdt, tshape, ref, ref.params())
            elif kinds.get(name) == "sparse":                      # the patch where the upload put it; the frame parameters the tensor would be coded with
                tdt, tshape, ref = over[name]
                at, L, elem = patched[name]
                params = ref.params()
                if params[0] != elem:
                    raise ValueError(f"{path}: {name!r}: {tdt} is not a dtype a patch describes")
                patch = blob[at:at + L]
                if patch.data_ptr() % 16:                          # (the upload's allocation is aligned far beyond 16 bytes; should one not be, the apply kernel still needs it)
                    patch = patch.clone()
                    extra += L
                e = _Entry.sparse(name, tdt, tshape, ref, params, patch)
            elif hi > lo:
                raw = blob[lo:hi]
                if (blob.data_ptr() + lo) % max(_itemsize(dt), 1):     # (a view needs the element's alignment: safetensors does not promise it)
                    raw = raw.clone()
                    extra += hi - lo
                e = _Entry.held(name, raw.view(dt).reshape(shape))
            else:
                e = _Entry.held(name, torch.empty(shape, dtype=dt, device=up.device))
            entries.append(e)
        return entries, extra

    @staticmethod
    def _link_restore(entries, based):
        """What revert_ restores each entry from: the base's tensor of the same name, dtype and shape.  based: _base_items."""
        for e in entries:
            ref = based.get(e.name)
            e.restore = ref if ref is not None and ref.fits(e.dtype, e.shape) else None

    @staticmethod
    def _ref_digests(refs, dev):
        """{name: _BaseRef} (_base_items) -> {name: digest of that base tensor's bytes}: a base store's recorded digest where it has one; otherwise the plain
        tensors digested where they lie, all in one batched launch, and a store's entries through one _decoded_digests call."""
        out, live, via = {}, [], {}
        for name, ref in refs.items():
            if ref.tensor is not None:
                live.append((name, ref.tensor))
            elif ref.store._digests is not None:
                out[name] = ref.store._digests[ref.entry.name]
            else:
                via.setdefault(id(ref.store), (ref.store, []))[1].append((name, ref.entry.name))
        out.update(zip([name for name, _ in live], codec.digests_of(_capi.lib(), [t for _, t in live], _stream_of(dev))))
        for bstore, pairs in via.values():
            got = bstore._decoded_digests([bn for _, bn in pairs])
            out.update({name: got[bn] for name, bn in pairs})
        return out

    @staticmethod
    def _base_items(base, dev):
        """-> {name: _BaseRef} for what from_state_dict accepts as `base`."""
        if base is None:
            return {}
        if isinstance(base, ResidentCheckpoint):
            if base.device != dev:
                raise ValueError(f"base: a store on {dev}, not on {base.device}")
            return {name: (_BaseRef(tensor=e.raw) if e.raw is not None else _BaseRef(store=base, entry=e)) for name, e in base._entries.items()}
        out = {}
        for name, t in _named_tensors(base).items():
            t = t.detach()
            if t.device != dev or not t.is_contiguous():
                raise ValueError(f"base[{name!r}]: a contiguous tensor on {dev} (plain base tensors are read where they lie)")
            out[name] = _BaseRef(tensor=t)
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
        coders = {}                            # one ZipNN per dtype: what decides a tensor's frame parameters
        todo, entries, heads = [], {}, {}      # [(name, the tensor on dev, its frame parameters)]: what the codec takes; {name: entry}; {name: _Entry.head}
        for name, t in sd.items():             # classify: what the codec takes, and what stays as it is
            t = t.detach()
            if torch.is_floating_point(t) and t.dtype != torch.float64 and t.numel() > 0 and dtype_from_user(t.dtype) is not None:
                heads[name], prm = _frame_params_for(t.dtype, t.shape, method, coders, like=t)
                todo.append((name, t.to(dev), prm))
            else:
                entries[name] = _Entry.held(name, t.to(dev).clone())
        recorded = None
        if digests:                            # (the sources, before compression; raw entries are digested too)
            src = {name: t for name, t, _ in todo}
            src.update({name: e.raw for name, e in entries.items()})
            recorded = dict(zip(sd.keys(), codec.digests_of(lib, [src[n] for n in sd.keys()])))
        keep, held = [], 0
        if todo:
            refs = [based.get(name) for name, _, _ in todo]        # the base has this tensor: what a delta can be coded over (and revert_ restores from)
            refs = [ref if ref is not None and ref.fits(t.dtype, t.shape) else None for ref, (_, t, _) in zip(refs, todo)]
            with _device_of(dev):                      # the plain pass, then the candidates over the base
                plain = [b.clone() for b in codec.compress_device_batch(lib, [(codec.flat_bytes(t),) + prm + (float(threshold),) for (_, t, prm) in todo])]      # (clones: out of the compress arena, which is as large as the tensors themselves)
                cand = [i for i, ((_, _, prm), ref) in enumerate(zip(todo, refs)) if ref is not None and ref.decodes_under(prm, coders)]
                dbody, same, pbody = cls._over_base(lib, todo, refs, cand, plain, base, float(threshold), sparse)
            kept = cls._choose(todo, plain, dbody, same, pbody)
            bodies, packed, o = cls._pack([b for _, b, _ in kept], dev)      # pack: the kept bodies and patches into the store's one allocation
            for (i, _, kind), body in zip(kept, bodies):
                name, t, prm = todo[i]
                if kind == "sparse":
                    entries[name] = _Entry.sparse(name, t.dtype, t.shape, refs[i], prm, body, head=heads[name])
                else:
                    entries[name] = _Entry.framed(name, t.dtype, t.shape, t.numel() * t.element_size(), body, prm, head=heads[name], base=refs[i] if kind else None)
            for i, (name, t, prm) in enumerate(todo):
                if i in same:
                    entries[name] = _Entry.same(name, t.dtype, t.shape, refs[i], prm, head=heads[name])
                elif name not in entries:
                    entries[name] = _Entry.held(name, t.clone(), head=heads[name])
            keep.append(packed)
            held += o
            del plain, dbody, pbody            # (the bodies not kept go back to the allocator)
        cls._link_restore(entries.values(), based)                     # finish: restore links, what the store holds, digests, index
        held += sum(e.nbytes for e in entries.values() if not e.compressed and e.delta not in ("same", "sparse"))
        if base is not None:
            keep.append(base)
        store = cls(dev, [entries[name] for name in sd.keys()], held, keep=keep)
        store._digests = recorded
        if index:
            store.build_index(deltas=(index == "deltas"))
        return store

    @classmethod
    def from_live(cls, live, base, ratio=1 / 8, digests=False):
        """CAPTURE live weights as a variant store over `base`: what a trainer or a policy update left in an engine's own layout, as the store
        whose patches the other replicas apply.  live: a mapping of names to tensors, or a module — tensors on the base's device in any layout
        zn_patch_build_strided_batch_dev accepts (transposed, a column slice of a fused buffer, a tile shuffle, at most 8 dimensions); base: whatever
        from_state_dict(base=...) accepts.  The device is the tensors'.

        Every tensor the base holds with the same dtype and shape, and whose elements a patch can describe, is COUNTED against its base where both lie — one
        batched strided size call per group of at most 1 GiB of tensors; a resident base is decoded a group at a time —: identical bytes give a "same" entry;
        a patch shorter than ratio x the tensor's bytes gives a sparse entry, built by one batched strided build call per group.  Such a tensor gets no plain
        body, no delta body and no contiguous copy.  Everything else — integers, tensors without a counterpart, patches at or above the ratio — goes, as a
        contiguous copy, through from_state_dict(..., base=base, sparse=True), and its entries are taken over.
        ratio is a POLICY, not from_state_dict's smallest-of-three rule: a huff0-coded plane spends at least one bit per byte, so a patch below
        1/8 of the tensor is below any delta body whose planes are all coded — but a tensor that is constant apart from a few elements can have a smaller plain
        body, which this constructor never looks for.
        The result is an ordinary variant store that keeps `base` alive: get_tensor(s), get_slice, plan, hook, verify, apply_ / revert_,
        save_file(sparse=True), rebased and sharded work on it.  digests=True: the sources are digested as from_state_dict does; a non-contiguous one
        goes through a contiguous copy, as in holds() — a group's at a time, so the copies alive at once are bounded by the same 1 GiB (or one larger tensor),
        but with digests the capture is no longer free of tensor-sized scratch."""
        live = {name: t.detach() for name, t in _named_tensors(live).items()}
        if not live:
            raise ValueError("from_live: no tensors")
        dev = next(iter(live.values())).device
        if any(t.device != dev for t in live.values()):
            raise ValueError("from_live: tensors on one device")
        lib = _capi.lib()
        based = cls._base_items(base, dev)
        coders, prms, heads, cand = {}, {}, {}, []
        for name, t in live.items():
            ref = based.get(name)
            if (ref is None or not ref.fits(t.dtype, t.shape) or t.dim() > _capi.PATCH_MAX_DIMS or t.numel() == 0 or not torch.is_floating_point(t)
                    or t.dtype == torch.float64 or dtype_from_user(t.dtype) is None):
                continue
            heads[name], prm = _frame_params_for(t.dtype, t.shape, None, coders)
            if codec.patch_elem(t) == prm[0] and ref.decodes_under(prm, coders):
                prms[name] = prm
                cand.append(name)
        recorded = {} if digests else None     # (filled a group at a time: a non-contiguous source is digested through a copy, and no more than a group's are alive at once)
        entries, keep, held = {}, [], 0
        with _device_of(dev):
            for grp in _groups(cand, lambda name: live[name].numel() * live[name].element_size(), cls._BUILD_GROUP_BYTES):
                via = [name for name in grp if based[name].tensor is None]
                decoded = base.get_tensors(via) if via else {}
                pairs = [(live[name], decoded[name] if based[name].tensor is None else based[name].tensor) for name in grp]
                if digests:
                    recorded.update(zip(grp, codec.digests_of(lib, [live[name] for name in grp])))
                sizes = codec.patch_sizes_strided_device_batch(lib, pairs)
                take = [k for k, name in enumerate(grp) if 0 < sizes[k] < ratio * live[name].numel() * live[name].element_size()]
                built, arena = codec.patch_build_strided_device_batch(lib, [pairs[k] for k in take], [sizes[k] for k in take], return_arena=True)
                for k, name in enumerate(grp):
                    if sizes[k] == 0:
                        entries[name] = _Entry.same(name, live[name].dtype, live[name].shape, based[name], prms[name], head=heads[name])
                for k, p in zip(take, built):
                    name = grp[k]
                    entries[name] = _Entry.sparse(name, live[name].dtype, live[name].shape, based[name], prms[name], p, head=heads[name])
                    held += _round_up(p.numel())
                if built:
                    keep.append(arena)         # the group's patches are views of it
                del decoded, pairs
        rest = {name: t.contiguous() for name, t in live.items() if name not in entries}
        if rest:                               # the chooser's entries, bodies and links are taken over as they are
            if digests:                        # (of the contiguous copies the chooser takes anyway)
                todo = [name for name in rest if name not in recorded]
                recorded.update(zip(todo, codec.digests_of(lib, [rest[name] for name in todo])))
            sub = cls.from_state_dict(rest, dev, base=base, sparse=True)
            entries.update(sub._entries)
            keep.extend(sub._keep)
            held += sub._held
        else:
            keep.append(base)
        cls._link_restore([entries[name] for name in cand if name in entries], based)
        store = cls(dev, [entries[name] for name in live.keys()], held, keep=keep)
        store._digests = {name: recorded[name] for name in live.keys()} if digests else None
        return store

    @classmethod
    def _over_base(cls, lib, todo, refs, cand, plain, base, threshold, sparse):
        """from_state_dict, the candidates over the base.  cand: the indices into todo whose refs[i] a delta can be coded over -> ({i: delta body}, {i: its bytes
        ARE the base's}, {i: patch}), every body a trimmed copy out of its arena.  In groups of at most _BUILD_GROUP_BYTES of base bytes: plain base tensors are
        read where they lie, a resident base's tensors are decoded a group at a time (never the whole base at once), the group's "is it the base's bytes" flags
        come back in one read."""
        dbody, same, pbody = {}, set(), {}
        for grp in _groups(cand, lambda i: todo[i][1].numel() * todo[i][1].element_size(), cls._BUILD_GROUP_BYTES):
            via = [todo[i][0] for i in grp if refs[i].tensor is None]
            decoded = base.get_tensors(via) if via else {}
            flats = {i: refs[i].flat() if refs[i].tensor is not None else codec.flat_bytes(decoded[todo[i][0]]) for i in grp}
            eq = torch.stack([(codec.flat_bytes(todo[i][1]) == flats[i]).all() for i in grp]).tolist()
            same.update(i for i, e in zip(grp, eq) if e)
            rest = [i for i in grp if i not in same]
            if rest:
                got = [b.clone() for b in codec.compress_device_batch(lib, [(codec.flat_bytes(todo[i][1]),) + tuple(todo[i][2]) + (threshold, flats[i]) for i in rest])]
                dbody.update(zip(rest, got))               # (clones: the group's compress arena goes back before the patches are built)
            if sparse and rest:                # the count pass gives every patch's length; only those below the best body so far are built
                elig = [i for i in rest if codec.patch_elem(todo[i][1]) == todo[i][2][0]]
                pairs = [(codec.flat_bytes(todo[i][1]), flats[i], todo[i][2][0]) for i in elig]
                sizes = codec.patch_sizes_device_batch(lib, pairs)
                take = [k for k, i in enumerate(elig) if 0 < sizes[k] < min(plain[i].numel(), dbody[i].numel(), flats[i].numel())]
                built = codec.patch_build_device_batch(lib, [pairs[k] for k in take], [sizes[k] for k in take])
                pbody.update({elig[k]: b.clone() for k, b in zip(take, built)})
            del flats, decoded
        return dbody, same, pbody

    @staticmethod
    def _choose(todo, plain, dbody, same, pbody):
        """from_state_dict, what each tensor is kept as -> [(index into todo, body, False | True: a delta body | "sparse": a patch)] for those that keep a body
        smaller than the tensor."""
        kept = []
        for i, (name, t, prm) in enumerate(todo):
            if i in same:
                continue
            b, kind = plain[i], False
            if i in dbody and dbody[i].numel() < b.numel():        # (a tie goes to the plain body)
                b, kind = dbody[i], True
            if i in pbody and pbody[i].numel() < min(b.numel(), t.numel() * t.element_size()):      # (… and the patch only when it is smaller than either)
                b, kind = pbody[i], "sparse"
            if b.numel() < t.numel() * t.element_size():
                kept.append((i, b, kind))
        return kept

    @staticmethod
    def _pack(bodies, dev):
        """-> ([copies of the bodies: views of the allocation], ONE new allocation that holds them at 256-byte boundaries, its bytes in use)."""
        offs, o = _packed(b.numel() for b in bodies)
        packed = torch.empty(max(o, 1), dtype=torch.uint8, device=dev)
        views = [packed[off:off + b.numel()] for off, b in zip(offs, bodies)]
        for v, b in zip(views, bodies):
            v.copy_(b)
        return views, packed, o

    # ---- re-parenting a variant ------------------------------------------------------------------------------------
    @staticmethod
    def _patch_path(ref):
        """Walk base links from `ref` (a _BaseRef) while the entry is "sparse" or "same" -> [(node key, the patches on the way there)]: the first element is
        `ref` itself with no patch, the last the first node that is neither (a plain tensor, or an entry with a body of its own)."""
        path, patches = [(ref.key, ())], []
        while ref.entry is not None and ref.entry.delta in ("sparse", "same"):
            if ref.entry.delta == "sparse":
                patches.append(ref.entry.patch)
            ref = ref.entry.base
            path.append((ref.key, tuple(patches)))
        return path

    def _patch_lists(self, onto, refs):
        """rebased, per tensor: where the walks from this store's entry and from onto's meet -> ({name: [the patches on both paths: their merge is the tensor's
        patch over `onto`]}, [the names without such a list]).  refs: _base_items(onto)."""
        lists, fallback = {}, []
        for name, e in self._entries.items():
            ref = refs.get(name)
            ok = (ref is not None and ref.fits(e.dtype, e.shape) and e.P in (1, 2, 4) and e.P == _itemsize(e.dtype) and 0 < e.nbytes and e.nbytes // e.P < (1 << 32)
                  and (ref.entry is None or ref.decodes_under((e.P, e.bits, e.byts, e.chunk))))      # (a resident base: what a "same" or sparse entry can decode over)
            found = None
            if ok:
                mine, theirs = self._patch_path(_BaseRef(store=self, entry=e)), self._patch_path(_BaseRef(store=onto, entry=onto._entries[name]))
                at = {k: ps for k, ps in reversed(theirs)}      # (the nearest occurrence of a key wins)
                for k, ps in mine:
                    if k in at:
                        found = list(ps) + list(at[k])
                        break
            if found is None:
                fallback.append(name)
            else:
                lists[name] = found
        return lists, fallback

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
        lists, fallback = self._patch_lists(onto, refs)
        # rounds of pairwise merges, every tensor's in one call: a chain of depth d is d - 1 calls for the whole store
        scratch = []                               # the rounds' arenas: intermediate patches are views of them
        with _device_of(dev):
            while any(len(ps) > 1 for ps in lists.values()):
                todo = [name for name, ps in lists.items() if len(ps) > 1]
                got = codec.patch_merge_device_batch(lib, [(lists[n][0], lists[n][1], self._entries[n].nbytes, self._entries[n].P) for n in todo])
                scratch.append(got)
                for n, g in zip(todo, got):
                    lists[n] = ([g] if g is not None else []) + lists[n][2:]
        merged = {}                                # {name: its one patch over `onto`, or None: the bytes are onto's}
        for name, ps in lists.items():
            if ps and ps[0].numel() >= self._entries[name].nbytes:
                fallback.append(name)              # a patch that is not smaller than the tensor: the build decides what it is kept as
            else:
                merged[name] = ps[0] if ps else None
        patched = [name for name, p in merged.items() if p is not None]
        views, packed, o = self._pack([merged[name] for name in patched], dev)
        mine, entries = dict(zip(patched, views)), {}
        for name in merged:
            e, ref = self._entries[name], refs[name]
            prm = (e.P, e.bits, e.byts, e.chunk)
            if name in mine:
                ne = _Entry.sparse(name, e.dtype, e.shape, ref, prm, mine[name], head=e.head)
            else:
                ne = _Entry.same(name, e.dtype, e.shape, ref, prm, head=e.head)
            ne.restore = ref
            entries[name] = ne
        del scratch, lists
        keep, held = [packed], o
        order = {n: i for i, n in enumerate(self._entries)}
        fallback.sort(key=order.__getitem__)
        for grp in _groups(fallback, lambda name: self._entries[name].nbytes, self._BUILD_GROUP_BYTES):
            sub = type(self).from_state_dict(self.get_tensors(grp), dev, base=onto, sparse=True)
            entries.update(sub._entries)
            keep += [k for k in sub._keep if k is not onto]
            held += sub._held
        keep.append(onto)
        store = type(self)(dev, [entries[name] for name in self._entries], held, keep=keep)
        store._digests = dict(self._digests) if self._digests is not None else None
        store._metadata = self._metadata
        return store

    # ---- sharding a variant ----------------------------------------------------------------------------------------
    def sharded(self, onto, spec):
        """One tensor-parallel rank's part of this store as a NEW variant store over `onto`, without decoding what is kept as "znp1" patches: a patch is a
        sorted list of element indices, so the patch of a narrow() of a tensor is a filter and a re-index of the tensor's patch (zn_patch_select_batch_dev,
        DESIGN §3.13).

            spec = {"q.weight": (0, 512, 1024), "o.weight": (1, 512, 1024)}      # {name: (dim, lo, hi)}; names absent from it are kept whole
            mine = ft.sharded(base_shards, spec)                                 # base_shards: what from_state_dict accepts as `base`, or None
            mine.get_tensor("q.weight")                                          # ft's q.weight.narrow(0, 512, 512)

        `onto` stands, for every tensor, for the same narrow of whatever this store's entry is coded over; keeping it at those values is the caller's contract,
        as with plain base tensors.  Its dtypes and shapes are checked against the shard shapes — a ValueError names every mismatch —, and so is `spec`: a name
        this store lacks, a dimension or range the tensor does not have.
        Every "sparse" entry whose name `onto` has goes through ONE batched select call and becomes "sparse" over onto's tensor, or "same" when nothing falls
        in the shard; a "same" entry becomes "same" over `onto`.  Every other tensor — a delta body, a plain body, a held tensor, a name `onto` lacks, a
        selected patch not smaller than the shard — is decoded from this store in groups of at most _BUILD_GROUP_BYTES, narrowed, made contiguous and built by
        from_state_dict(..., base=onto, sparse=True): nothing is refused, the result is always complete.
        The result has no index and no digests (its content is not the whole tensors'), keeps `onto` alive and nothing else of this store, and is served by
        every entry point; save_file(sparse=True) and from_file(path, dev, base=onto) round-trip it — shard a delta file once per rank, and each rank loads
        its own file over its own shard of the base, base digests verified as ever."""
        dev, lib = self.device, _capi.lib()
        if isinstance(onto, ResidentCheckpoint) and onto.device != dev:
            raise ValueError(f"sharded: onto is a store on {dev}, not on {onto.device}")
        rects, shapes, wrong = {}, {}, []
        for name, cut in spec.items():
            if name not in self._entries:
                wrong.append(f"{name!r}: the store has no such tensor")
                continue
            try:
                dim, lo, hi = cut
                shape = self._entries[name].shape
                rects[name] = codec.narrow_rect(shape, dim, lo, hi)
                dim %= len(shape)
                shapes[name] = shape[:dim] + (hi - lo,) + shape[dim + 1:]
            except (ValueError, TypeError) as err:
                wrong.append(f"{name!r}: {err}")
        if wrong:
            raise ValueError("sharded: " + "; ".join(wrong))
        refs = self._base_items(onto, dev)
        for name, e in self._entries.items():
            ref, shape = refs.get(name), shapes.get(name, e.shape)
            if ref is not None and not ref.fits(e.dtype, shape):
                wrong.append(f"{name!r}: onto holds {ref.dtype} {list(ref.shape)}, the shard is {e.dtype} {list(shape)}")
        if wrong:
            raise ValueError("sharded: " + "; ".join(wrong))
        coders, plans, select, fallback, entries = {}, {}, [], [], {}
        for name, e in self._entries.items():
            ref, shape = refs.get(name), shapes.get(name, e.shape)
            if ref is None or e.delta not in ("sparse", "same") or not e.nbytes:
                fallback.append(name)
                continue
            head, prm = _frame_params_for(e.dtype, shape, coders=coders)
            if not ref.decodes_under(prm, coders):                 # (a resident base that holds the shard in other chunks: the build decides)
                fallback.append(name)
            elif e.delta == "same":
                entries[name] = _Entry.same(name, e.dtype, shape, ref, prm, head=head)
            else:
                plans[name] = (head, prm)
                rows = _numel(e.shape)
                select.append((e.patch, e.P) + (rects[name] if name in rects else (1, rows, 0, 1, 0, rows)))
        with _device_of(dev):
            got = codec.patch_select_device_batch(lib, select)     # ONE call for the store
        small = [(name, p) for name, p in zip(plans, got) if p is not None and p.numel() < _numel(shapes.get(name, self._entries[name].shape)) * self._entries[name].P]
        views, packed, o = self._pack([p for _, p in small], dev)
        mine = dict(zip((name for name, _ in small), views))
        for name, p in zip(plans, got):
            e, ref, shape = self._entries[name], refs[name], shapes.get(name, self._entries[name].shape)
            head, prm = plans[name]
            if name in mine:
                entries[name] = _Entry.sparse(name, e.dtype, shape, ref, prm, mine[name], head=head)
            elif p is None:
                entries[name] = _Entry.same(name, e.dtype, shape, ref, prm, head=head)
            else:
                fallback.append(name)                              # a patch that is not smaller than the shard: the build decides what it is kept as
        for ne in entries.values():
            ne.restore = ne.base
        del got, small
        keep, held = [packed], o
        order = {n: i for i, n in enumerate(self._entries)}
        fallback.sort(key=order.__getitem__)
        for grp in _groups(fallback, lambda name: self._entries[name].nbytes, self._BUILD_GROUP_BYTES):
            whole = self.get_tensors(grp)
            part = {name: (whole[name].narrow(spec[name][0], spec[name][1], spec[name][2] - spec[name][1]).contiguous() if name in spec else whole[name]) for name in grp}
            del whole
            sub = type(self).from_state_dict(part, dev, base=onto, sparse=True)
            entries.update(sub._entries)
            keep += [k for k in sub._keep if k is not onto]
            held += sub._held
        if onto is not None:
            keep.append(onto)
        store = type(self)(dev, [entries[name] for name in self._entries], held, keep=keep)
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
            offs, o = _packed(sizes)
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
            bt = e.base.flat()                         # over a plain base tensor: read where it lies; over a resident base: its own sets decode the window first
            if bt is not None:
                keep.append(bt)
            else:
                via.setdefault(id(e.base.store), (e.base.store, []))[1].append((e.base.entry, lo, hi, dst))
            if e.delta == "sparse":
                keep.append(e.patch)
                patch.append(e.patch_item(lo, hi, ptr(dst), bt.data_ptr() if bt is not None else None))
            elif bt is not None:                       # (a delta entry: "same" over a plain tensor is that tensor, never work)
                delta.append((e, lo, hi, ptr(dst), bt.data_ptr()))
            elif e.delta is True:
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
        self._run_steps(self._set_steps(sets), check)

    @staticmethod
    def _set_steps(sets):
        """launch sets -> the steps of _launch: [(the batched call of the set's kind, its items, None)]"""
        lib = _capi.lib()
        return [(getattr(lib, _KINDS[kind][0]), items, None) for kind, items in sets]

    def _run_steps(self, steps, check):
        with _device_of(self.device):
            _launch(_capi.lib(), steps, _stream_of(self.device), check)

    def _scratch_steps(self, todo):
        """todo: [(store, entry of it, live tensor)] — non-contiguous live tensors that receive a decoded tensor -> the steps of _launch that
        decode each entry through its store's normal path into ONE scratch buffer and follow with a stride-aware copy_ into the live tensor, grouped as verify()
        groups: never more scratch than the largest such tensor, and the stream orders the buffer's reuse."""
        if not todo:
            return []
        scratch = torch.empty(max(_round_up(e.nbytes) for _, e, _ in todo), dtype=torch.uint8, device=self.device)
        steps = []
        for grp in _groups(todo, lambda it: _round_up(it[1].nbytes), scratch.numel()):
            flats = [scratch[o:o + e.nbytes] for (_, e, _), o in zip(grp, _packed(e.nbytes for _, e, _ in grp)[0])]
            via = {}
            for (store, e, _), flat in zip(grp, flats):
                via.setdefault(id(store), (store, []))[1].append((e, 0, e.chunks, flat))
            for store, w in via.values():
                steps += self._set_steps(store._launch_sets(w))
            steps.append((lambda pairs, stream, check: [t.copy_(e.view(flat)) for t, e, flat in pairs], [(t, e, flat) for (_, e, t), flat in zip(grp, flats)], None))
        return steps

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
        head = e.head if e.head is not None else _frame_params_for(e.dtype, e.shape)[0]
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
        return safetensors_io._save_with_sparse_entries(tensors, path, metadata, patches)

    # ---- decoding -------------------------------------------------------------------------------------------------------------
    def scratch_bytes(self, names):
        """Size of an `into` buffer for `names`: every compressed tensor at a multiple of 256 bytes."""
        return self._layout(names)[1]

    def _layout(self, names):
        names = [name for name in dict.fromkeys(names) if self._entries[name].decoded]
        offs, total = _packed(self._entries[name].nbytes for name in names)
        return dict(zip(names, offs)), total

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
                k = len(plain)
                for grp in _groups(todo, lambda e: _round_up(e.nbytes), scratch.numel()):
                    flats = [scratch[o:o + e.nbytes] for e, o in zip(grp, _packed(e.nbytes for e in grp)[0])]
                    self._decode([(e, 0, e.chunks, flat) for e, flat in zip(grp, flats)], False)
                    codec.digest_device_batch(lib, flats, stream, out=out[k:k + len(grp)])
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
        """[(key, tensor)] -> {key: digest of the live tensor's LOGICAL bytes}: contiguous tensors digested where they lie by one batched launch; non-contiguous
        ones through a contiguous copy — what zipnn_amd.digest does —, the copies grouped in one scratch buffer sized for the largest of them, one
        digest launch per group behind its copies on the current stream; one read-back."""
        lib = _capi.lib()
        here = [(k, t) for k, t in pairs if t.is_contiguous()]
        there = [(k, t) for k, t in pairs if not t.is_contiguous()]
        if not there:
            return dict(zip([k for k, _ in here], codec.digests_of(lib, [t for _, t in here], _stream_of(self.device))))

        def size(kt):
            return _round_up(kt[1].numel() * kt[1].element_size())
        out = torch.empty(len(pairs), dtype=torch.int64, device=self.device)
        with _device_of(self.device):
            stream = _stream_of(self.device)
            if here:
                codec.digest_device_batch(lib, [codec.flat_bytes(t) for _, t in here], stream, out=out[:len(here)])
            scratch = torch.empty(max(size(kt) for kt in there), dtype=torch.uint8, device=self.device)
            k = len(here)
            for grp in _groups(there, size, scratch.numel()):
                flats = [scratch[o:o + t.numel() * t.element_size()] for (_, t), o in zip(grp, _packed(t.numel() * t.element_size() for _, t in grp)[0])]
                for (_, t), flat in zip(grp, flats):
                    flat.view(t.dtype).reshape(t.shape).copy_(t)
                codec.digest_device_batch(lib, flats, stream, out=out[k:k + len(grp)])
                k += len(grp)
            vals = codec.digests_to_ints(out)
        return dict(zip([k for k, _ in here + there], vals))

    def holds(self, target):
        """Do live tensors hold this store's values?  target: a module (named parameters and buffers) or a mapping of names to tensors on the store's device, at
        any strides apply_ accepts.  -> {name: bool} for the names the store has: the live tensors digested where they lie (one launch; non-contiguous ones
        through grouped contiguous copies, _live_digests), compared with the recorded digests."""
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
            elif e.restore.tensor is not None:
                pairs.append((("base", e.name), e.restore.tensor))
            elif e.restore.store._digests is None:
                raise ValueError(f"guard: the base store has no digests (build it with digests=True) — {e.name}")
            else:
                want[e.name] = e.restore.store._digests[e.restore.entry.name]
        got = self._live_digests(pairs)
        for (kind, name), _ in pairs:
            if kind == "base":
                want[name] = got[(kind, name)]
        bad = [e.name for e, _ in tg if e.name in want and got[("live", e.name)] != want[e.name]]
        if bad:
            raise codec.DigestMismatch(bad, "guard: the tensors do not hold the " + ("base's" if want_base else "variant's") + " values")

    # ---- a variant applied to live weights ------------------------------------------------------------------------------------
    def _targets(self, target):
        """target: a module (named parameters and buffers) or a mapping -> [(entry, tensor)] for the names the store has.  A tensor has the entry's dtype and
        shape and lies on the store's device: contiguous, or a strided view of live memory — a transposed weight, a column slice of a fused buffer, a permuted
        layout — whose strides pass the injectivity test of zn_patch_apply_strided_batch_dev (expand()ed and overlapping views are refused)."""
        out = []
        for name, t in _named_tensors(target).items():
            e = self._entries.get(name)
            if e is None:
                continue
            t = t.detach()
            if t.dtype != e.dtype or tuple(t.shape) != e.shape or t.device != self.device:
                raise ValueError(f"{name}: a {e.dtype} tensor of shape {list(e.shape)} on {self.device}")
            why = None if t.is_contiguous() else codec.patch_layout_refusal(t)
            if why:
                raise ValueError(f"{name}: the view cannot be written in place: {why}")
            out.append((e, t))
        return out

    def _in_place_sets(self, target):
        """What apply_ and revert_ share: the target's tensors that differ from the base's ("same" and empty entries do not) -> (the launch sets that XOR delta
        bodies and patches into them IN PLACE — the same call both ways —, [(entry, tensor)] of the others: entries with a body or a tensor of their own, the
        names of all of them).  A sparse entry on a NON-CONTIGUOUS tensor is patched through its layout (a "strided" set) and is in place all the
        same; a delta entry on one has no in-place decode and joins the others: it is overwritten by a decode, not XORed."""
        inplace, patch, strided, rest, names = [], [], [], [], []
        for e, t in self._targets(target):
            if e.delta == "same" or not e.nbytes:
                continue
            if e.delta == "sparse":
                if t.is_contiguous():
                    patch.append(e.patch_item(0, e.chunks, t.data_ptr()))
                else:
                    strided.append(codec.patch_strided_item(t, e.patch))
            elif e.delta is True and t.is_contiguous():
                inplace.append((e, 0, e.chunks, t.data_ptr(), t.data_ptr()))
            else:
                rest.append((e, t))
            names.append(e.name)
        return self._delta_sets(inplace) + ([("patch", patch)] if patch else []) + ([("strided", strided)] if strided else []), rest, names

    def apply_(self, target, check=True, guard=False):
        """Turn live BASE weights into the fine-tune's, in place: `target` is a module or a mapping of names to contiguous tensors on the store's device that
        hold the base's values.  Delta entries are XORed over them by an in-place decode (d_dst == d_delta, include/zipnn_hip.h) — no second copy of the
        weights, no read of the base —, sparse entries are their patch applied in place (zn_patch_apply_batch_dev alone: only the changed elements are touched),
        plain entries are overwritten, "same" entries are left alone; one batched launch set on the current stream.
        Nothing is tracked: applying twice (or to tensors that do not hold the base) XORs the delta in twice and is the caller's mistake — unless guard=True
        (a store with digests): the live tensors are digested first and must hold the BASE's values, else DigestMismatch is raised before anything is touched.  If `target` is
        the very tensors this store holds as its plain base, the store decodes wrong values until revert_.  -> the names changed.
        NON-CONTIGUOUS targets — {"o_proj.weight": live.t(), "up_proj.weight": fused[:, a:b]}, any strided view of the entry's dtype and shape
        whose strides pass zn_patch_apply_strided_batch_dev's injectivity test: a sparse entry is patched through the view's layout, in place, by one more batched
        launch; a plain entry, and a DELTA entry, is decoded through the store's normal path into a scratch buffer (grouped: never more than the largest such
        tensor) and copied in by a stride-aware copy_ — for a delta entry that OVERWRITES instead of XORing, which is the same whenever the target held what
        apply_ requires, the base's values.  revert_ does the same with the base's tensors."""
        if guard:
            self._guard(target, True)
        sets, rest, done = self._in_place_sets(target)
        work, scratch = [], []
        for e, t in rest:
            if e.compressed and not t.is_contiguous():
                scratch.append((self, e, t))
            elif e.compressed:
                work.append((e, 0, e.chunks, codec.flat_bytes(t)))
            else:
                t.copy_(e.raw)
        self._run_steps(self._scratch_steps(scratch) + self._set_steps(self._launch_sets(work) + sets), check)
        return done

    def revert_(self, target, check=True, guard=False):
        """The inverse of apply_: delta and sparse entries by the same in-place call again (XOR is its own inverse), plain entries restored from the base — its
        tensor copied, or its resident body decoded — where the base has the tensor with the same dtype and shape.  -> the names that could NOT be
        reverted (plain entries with nothing to restore from: they stay as they are).  Reverting what was not applied is the caller's mistake — unless
        guard=True (a store with digests): the live tensors must hold THIS store's values, else DigestMismatch is raised before anything is touched."""
        if guard:
            self._guard(target, False)
        sets, rest, _ = self._in_place_sets(target)
        stay, via, scratch = [], {}, []
        for e, t in rest:
            ref = e.base if e.delta is True else e.restore      # (a delta entry is here with a non-contiguous target: what it decodes over is what it goes back to)
            if ref is None or (ref.tensor is not None and ref.tensor.data_ptr() == t.data_ptr()):      # (nothing to restore from, or the base's tensor IS the target: its values are gone)
                stay.append(e.name)
            elif ref.tensor is not None:
                t.copy_(ref.tensor)
            elif not t.is_contiguous():
                scratch.append((ref.store, ref.entry, t))
            else:
                via.setdefault(id(ref.store), (ref.store, []))[1].append((ref.entry, 0, ref.entry.chunks, codec.flat_bytes(t)))
        base_sets = []
        for bstore, w in via.values():
            base_sets += bstore._launch_sets(w)
        self._run_steps(self._scratch_steps(scratch) + self._set_steps(base_sets + sets), check)
        return stay

    def patch(self, name):
        """The "znp1" patch of a sparse entry: a uint8 view of the store's own memory — read it, do not write to it —, or None for a "same" entry (nothing
        differs from the base).  What zipnn_amd.patch_apply_ takes: through it a caller reaches live layouts with ANOTHER shape than the entry's (a tile-shuffled
        weight through the N-D view that undoes the shuffle).  KeyError: no such tensor; ValueError: the entry is neither sparse nor "same"."""
        e = self._entries[name]
        if e.delta == "same":
            return None
        if e.delta != "sparse":
            raise ValueError(f"{name}: not a sparse entry (delta: {e.delta!r})")
        return e.patch.detach()

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
            hs = []                                # per launch set: (the plan's run call, its handle, its destroy call)
            try:
                for kind, items in (sets or [("window", [])]):
                    _, create, run, destroy = _KINDS[kind]
                    hs.append((getattr(self._lib, run), getattr(self._lib, create)(items), getattr(self._lib, destroy)))
            except Exception:
                self._destroy(hs)
                raise
            self._hs = hs

    def run(self, stream=None):
        if self._hs is None:
            raise RuntimeError("the plan is closed")
        self._stream = _stream_of(self._store.device, stream)
        with _device_of(self._store.device):
            _launch(self._lib, self._hs, self._stream, False)      # (the later plans add their verdict to the first one's: status() speaks for the whole run)
        return self.tensors

    def status(self):
        with _device_of(self._store.device):
            self._lib.decode_status(self._stream if self._stream is not None else _stream_of(self._store.device))

    @staticmethod
    def _destroy(hs):
        for _, h, destroy in hs:
            destroy(h)

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
