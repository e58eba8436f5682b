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
from .zipnn import _ST_DTYPE_NAME, COMPRESSION_METHOD, ZipNN, dtype_from_user, index_rows

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
    """One tensor of the store: a frame body in device memory (`body`, with its codec parameters), or the tensor itself (`raw`)."""
    __slots__ = ("name", "dtype", "shape", "nbytes", "body", "raw", "P", "bits", "byts", "chunk", "hints")

    def __init__(self, name, dtype, shape, nbytes, body=None, raw=None, params=None):
        self.name, self.dtype, self.shape, self.nbytes, self.body, self.raw = name, dtype, tuple(int(d) for d in shape), int(nbytes), body, raw
        self.hints = None                      # the body's decode hints (ResidentCheckpoint.build_index): a uint8 tensor beside the body, or None
        self.P, self.bits, self.byts, self.chunk = params if params is not None else (0, 0, 0, 0)

    @property
    def compressed(self):
        return self.body is not None

    @property
    def chunks(self):
        return (self.nbytes + self.chunk - 1) // self.chunk if self.compressed else 0

    def window(self, lo, hi, dst_ptr):
        """-> the item tuple of ZnLib.decompress_window_batch_dev / plan_create for chunks [lo, hi) of this tensor."""
        return (self.body.data_ptr(), self.body.numel(), self.P, self.bits, self.byts, self.chunk, self.nbytes, lo, hi, dst_ptr)

    def hinted(self, lo, hi, dst_ptr):
        """-> the item of ZnLib.decompress_hinted_batch_dev / plan_create_hinted: the window plus the body's index (None, 0 without one)."""
        h = self.hints
        return (self.window(lo, hi, dst_ptr), h.data_ptr() if h is not None else None, h.numel() if h is not None else 0)

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
    the current stream of the store's device."""

    def __init__(self, device, entries, held_bytes, keep=()):
        self.device = torch.device(device)
        self._entries = {e.name: e for e in entries}
        self._held = int(held_bytes)
        self._keep = tuple(keep)              # the allocations the entries are views of
        self._index = None                     # the allocation the entries' hints are views of (build_index)
        self._index_bytes = 0

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
    def from_file(cls, path, device="cuda:0", index=False):
        """A `.znn.safetensors` file (this library's or the reference's): its data section goes to `device` once, in one transfer, and stays.
        index=True: build_index() on the new store."""
        from . import safetensors_io
        dev = cls._work_device(device)
        up = safetensors_io._upload_file(path, dev)
        if up is None:
            raise ValueError(f"{path}: the container names a dtype this loader does not know")
        layout, plan, blob = up.layout, up.frames, up.blob
        entries, framed, extra = [], {}, 0
        for (name, b0, hi, fp, _) in plan:
            _, P, bits, byts, chunk, n, tdt, shape = fp
            framed[name] = _Entry(name, tdt, shape if shape is not None else (n // max(torch.empty(0, dtype=tdt).element_size(), 1),), n,
                                  body=blob[b0:hi], params=(P, bits, byts, chunk))
        for name, (dt, shape, lo, hi) in layout.items():          # (file order)
            if name in framed:
                entries.append(framed[name])
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
        store = cls(dev, entries, blob.numel() + extra, keep=(blob,))
        if index:
            store.build_index()
        return store

    @classmethod
    def from_state_dict(cls, sd, device="cuda:0", threshold=0.95, method=None, index=False):
        """Compress the tensors of a state dict on `device` (one batched call) and keep the bodies, trimmed to their lengths and packed at
        256-byte boundaries of one allocation.  A tensor whose body would not be smaller than the tensor itself — and every tensor the codec
        does not take: integers, float64, empty ones — is kept as it is.  index=True: build_index() on the new store."""
        dev = cls._work_device(device)
        lib = _capi.lib()
        todo, entries = [], {}
        for name, t in sd.items():
            t = t.detach()
            if torch.is_floating_point(t) and t.dtype != torch.float64 and t.numel() > 0 and dtype_from_user(t.dtype) is not None:
                znn = ZipNN(input_format="torch", bytearray_dtype=t.dtype, method=method or COMPRESSION_METHOD)
                _, P, bits, byts, chunk = znn.torch_frame_plan(t)
                todo.append((name, t.to(dev), (P, bits, byts, chunk)))
            else:
                entries[name] = _Entry(name, t.dtype, t.shape, t.numel() * t.element_size(), raw=t.to(dev).clone())
        keep, held = [], 0
        if todo:
            with _device_of(dev):
                bodies = codec.compress_device_batch(lib, [(codec.flat_bytes(t), P, bits, byts, chunk, float(threshold)) for (_, t, (P, bits, byts, chunk)) in todo])
            kept = [(name, t, prm, b) for (name, t, prm), b in zip(todo, bodies) if b.numel() < t.numel() * t.element_size()]
            offs, o = [], 0
            for (_, _, _, b) in kept:
                offs.append(o)
                o += _round_up(b.numel())
            packed = torch.empty(max(o, 1), dtype=torch.uint8, device=dev)
            for (name, t, prm, b), off in zip(kept, offs):
                packed[off:off + b.numel()].copy_(b)
                entries[name] = _Entry(name, t.dtype, t.shape, t.numel() * t.element_size(), body=packed[off:off + b.numel()], params=prm)
            for (name, t, prm) in todo:
                if name not in entries:
                    entries[name] = _Entry(name, t.dtype, t.shape, t.numel() * t.element_size(), raw=t.clone())
            keep.append(packed)
            held += o
            del bodies                         # (the compress arena — as large as the tensors themselves — goes back to the allocator)
        held += sum(e.nbytes for e in entries.values() if not e.compressed)
        store = cls(dev, [entries[name] for name in sd.keys()], held, keep=keep)
        if index:
            store.build_index()
        return store

    # ---- the sync index ---------------------------------------------------------------------------------------------------------
    #: dtypes build_index() indexes by default; build_index(all_dtypes=True) indexes every compressed tensor.  The rule: a dtype whose hinted decode does
    #: not measure faster than the unhinted one by more than the run's own A/A spread (scripts/bench_resident.py --index) is taken out of this set.
    #: No dtype has been timed on a device yet, so none has been taken out.
    INDEX_DTYPES = frozenset(_INDEX_DTYPES)

    def build_index(self, names=None, all_dtypes=False):
        """Decode hints for the resident bodies (include/zipnn_hip.h): one pass over each body records where the decoder's sub-blocks
        start — about a byte per 16-24 bytes of Huffman-coded plane — so that every later decode of it (get_tensor, get_tensors, get_slice, plan,
        hook: no further arguments) starts them there instead of finding them by speculation.  The hints sit beside the bodies in device memory,
        never in them, and are advice: the decoded bytes are the same with and without.  names: the tensors to index (default: every compressed
        one); a dtype that measured no gain is left out unless all_dtypes is set.  Tensors already indexed keep their index; plans and hooks made
        before this call go on decoding without."""
        lib = _capi.lib()
        todo = []
        for name in (self.keys() if names is None else names):
            e = self._entries[name]
            if e.compressed and e.nbytes and e.hints is None and (all_dtypes or e.dtype in self.INDEX_DTYPES):
                todo.append(e)
        if not todo:
            return 0
        with _device_of(self.device):
            stream = _stream_of(self.device)
            sizes = [lib.hint_size_dev(e.window(0, e.chunks, None), stream) for e in todo]
            offs, o = [], 0
            for n in sizes:
                offs.append(o)
                o += _round_up(n)
            buf = torch.empty(max(o, 1), dtype=torch.uint8, device=self.device)
            for e, n, off in zip(todo, sizes, offs):
                lib.hint_build_dev(e.window(0, e.chunks, None), buf.data_ptr() + off, n, stream)
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

    def _decode(self, work, check):
        """work: [(entry, chunk_lo, chunk_hi, dst_ptr)] -> one batched decode on the current stream, hinted when an entry has an index."""
        lib = _capi.lib()
        with _device_of(self.device):
            if any(e.hints is not None for e, _, _, _ in work):
                lib.decompress_hinted_batch_dev([e.hinted(lo, hi, dp) for e, lo, hi, dp in work], _stream_of(self.device), check)
            else:
                lib.decompress_window_batch_dev([e.window(lo, hi, dp) for e, lo, hi, dp in work], _stream_of(self.device), check)

    # ---- introspection --------------------------------------------------------------------------------------------------------
    def keys(self):
        return list(self._entries.keys())

    def __contains__(self, name):
        return name in self._entries

    def __len__(self):
        return len(self._entries)

    def info(self, name):
        e = self._entries[name]
        return {"shape": list(e.shape), "dtype": e.dtype, "nbytes": e.nbytes, "compressed": e.compressed,
                "resident_bytes": e.body.numel() if e.compressed else e.nbytes, "index_bytes": e.hints.numel() if e.hints is not None else 0}

    @property
    def nbytes(self):
        """Bytes of the tensors as a model would hold them."""
        return sum(e.nbytes for e in self._entries.values())

    @property
    def resident_bytes(self):
        """Bytes of device memory the store holds."""
        return self._held

    # ---- decoding -------------------------------------------------------------------------------------------------------------
    def scratch_bytes(self, names):
        """Size of an `into` buffer for `names`: every compressed tensor at a multiple of 256 bytes."""
        return self._layout(names)[1]

    def _layout(self, names):
        offs, o = {}, 0
        for name in names:
            e = self._entries[name]
            if e.compressed and name not in offs:
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
            if not e.compressed:
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
        if not e.compressed:
            return e.raw.clone() if out is None else out.copy_(e.raw)
        if out is None:
            out = torch.empty(e.shape, dtype=e.dtype, device=self.device)
        if e.nbytes:
            self._decode([(e, 0, e.chunks, out.data_ptr())], check)
        return out

    def get_tensors(self, names, into=None, check=True):
        """Several tensors by ONE batched launch set -> {name: tensor}.  The decoded tensors are views of one buffer (`into`, a uint8 tensor of
        scratch_bytes(names) bytes, or a new allocation), each at a multiple of 256 bytes; tensors the store holds uncompressed are returned as
        they are (views of the store: do not write to them)."""
        views, work = self._destinations(names, into)
        if work:
            self._decode([(e, 0, e.chunks, flat.data_ptr()) for e, flat in work], check)
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
        if not e.compressed:
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
            self._s._decode([(e, c_lo, c_hi, buf.data_ptr())], False)
            t = buf[byte_lo - base: byte_hi - base].view(e.dtype).reshape(() if scalar else (b - a,) + shape[1:])
        return t[sel] if sel else t


class ResidentPlan:
    """`ResidentCheckpoint.plan(names, into=None)`: a zn_plan plus the buffer it decodes into.  Everything a batched decode works out on the
    host is done once, here; `run()` only launches — it neither waits for earlier device work nor copies anything to the device, so the decode
    of the next layer can be enqueued while this one still runs.  `tensors` are the views the runs fill; `status()` waits and raises what a
    checked decode would have raised; `close()` frees the plan (the store must outlive it)."""

    def __init__(self, store, names, into=None):
        self._store, self._lib = store, _capi.lib()
        self.tensors, work = store._destinations(names, into)
        self._keep = [flat for _, flat in work]
        self._stream = None
        self._h = None
        with _device_of(store.device):
            if any(e.hints is not None for e, _ in work):
                self._keep += [e.hints for e, _ in work if e.hints is not None]
                self._h = self._lib.plan_create_hinted([e.hinted(0, e.chunks, flat.data_ptr()) for e, flat in work])
            else:
                self._h = self._lib.plan_create([e.window(0, e.chunks, flat.data_ptr()) for e, flat in work])

    def run(self, stream=None):
        if self._h is None:
            raise RuntimeError("the plan is closed")
        self._stream = _stream_of(self._store.device, stream)
        with _device_of(self._store.device):
            self._lib.plan_run(self._h, self._stream, False)
        return self.tensors

    def status(self):
        with _device_of(self._store.device):
            self._lib.decode_status(self._stream if self._stream is not None else _stream_of(self._store.device))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.plan_destroy(h)

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
