"""torch <-> C-ABI glue for buffers that live in HBM.

torch is plumbing here (device memory, streams); the work is in libzipnn_hip.so.  The
functions take a `lib` (zipnn_amd._capi.ZnLib) so that the CPU test-suite can drive the
same code through the SIMT-emulated build of the kernels with CPU tensors.
"""
import torch


def current_device():
    return torch.cuda.current_device() if torch.cuda.is_available() else 0


def flat_bytes(t):
    """Contiguous 1-D uint8 view of a tensor's storage bytes (no copy when contiguous)."""
    t = t.contiguous()
    if t.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        return t.view(torch.uint8).reshape(-1)
    return t.reshape(-1).view(torch.uint8)


def to_device(lib, buf, dev):
    """bytes-like (pageable host memory) -> uint8 tensor on `dev`, through the library's pinned, multi-threaded
    transfer (zn_copy_to_device) instead of a pageable torch copy.  The copy runs on the library's own stream and
    is complete on return; torch's stream is drained first because the allocator may hand out a block that kernels
    queued earlier are still using."""
    mv = memoryview(buf).cast("B")
    t = torch.empty(mv.nbytes, dtype=torch.uint8, device=dev)
    if mv.nbytes:
        if t.is_cuda:
            with torch.cuda.device(t.device):
                torch.cuda.current_stream().synchronize()
                lib.copy_to_device(t.data_ptr(), mv)
        else:
            lib.copy_to_device(t.data_ptr(), mv)
    return t


def new_bytearray(n):
    """bytearray of n bytes WITHOUT the zero fill of bytearray(n) (128 ms for 256 MiB: every page touched by one
    thread before the data arrives) — the transfer that fills it touches the pages from several threads."""
    import ctypes
    try:
        f = ctypes.pythonapi.PyByteArray_FromStringAndSize
        f.restype = ctypes.py_object
        f.argtypes = [ctypes.c_char_p, ctypes.c_ssize_t]
        ba = f(None, n)
        if isinstance(ba, bytearray) and len(ba) == n:
            return ba
    except Exception:
        pass
    return bytearray(n)


def to_host(lib, t, out=None):
    """uint8 tensor (device) -> writable host buffer (a new bytearray unless `out` is given), the same way back."""
    t = t.contiguous()
    n = t.numel()
    if out is None:
        out = new_bytearray(n)
    if n:
        if t.is_cuda:
            with torch.cuda.device(t.device):
                torch.cuda.current_stream().synchronize()      # the kernels that produced `t` ran on torch's stream
                lib.copy_to_host(memoryview(out).cast("B")[:n], t.data_ptr())
        else:
            lib.copy_to_host(memoryview(out).cast("B")[:n], t.data_ptr())
    return out


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _device_of(dev):
    """torch.cuda.device(dev) for a GPU, nothing for the emulated library's CPU tensors."""
    return torch.cuda.device(dev) if dev.type == "cuda" else _nullctx()


def _stream_of(dev, stream=None):
    """-> the raw stream handle to launch on: `stream` (a torch.cuda.Stream or a handle), else the device's current stream."""
    if stream is not None:
        return getattr(stream, "cuda_stream", stream)
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0


def _stream_handle(t):
    return _stream_of(t.device)


def _delta_ptr(delta, like):
    """delta base: None, or a uint8 tensor of the same length on the same device (contiguous)."""
    if delta is None:
        return None, None
    delta = delta.contiguous()
    if delta.dtype != torch.uint8 or delta.numel() != like.numel() or delta.device != like.device:
        raise ValueError("delta base must be a uint8 tensor of the same length on the same device")
    return delta, (delta.data_ptr() if delta.numel() else None)


def compress_device(lib, flat, num_buf, bits_mode, bytes_mode, chunk, threshold, delta=None, body=None):
    """flat: uint8 tensor in HBM -> uint8 tensor (same device) holding the frame BODY
    (types ‖ cumSizes ‖ payload).  One 8-byte read-back for the length.
    delta: optional uint8 tensor of the same length — the body then encodes flat ^ delta, the XOR being fused
    into the kernels that read the tensor (the reference's delta step, zipnn/zipnn.py:625-640).
    body: optional preallocated uint8 buffer on the same device (>= zn_compress_bound bytes) the body is written into —
    a caller that compresses repeatedly (a checkpoint writer, bench.py) allocates it once; the result is a slice of it."""
    n = flat.numel()
    delta, dptr = _delta_ptr(delta, flat)
    cap = lib.compress_bound(n, num_buf, chunk, 0)
    if body is None:
        body = torch.empty(max(cap, 16), dtype=torch.uint8, device=flat.device)
    elif body.dtype != torch.uint8 or body.device != flat.device or body.numel() < max(cap, 16) or not body.is_contiguous():
        raise ValueError("body must be a contiguous uint8 tensor on the same device with at least zn_compress_bound bytes")
    with _device_of(flat.device):
        used = lib.compress_dev(flat.data_ptr() if n else 0, n, num_buf, bits_mode, bytes_mode, chunk, threshold,
                                body.data_ptr(), body.numel(), _stream_handle(flat), delta_ptr=dptr)
    return body[:used]


def compress_device_to_frame(lib, header, flat, num_buf, bits_mode, bytes_mode, chunk, threshold):
    """Device tensor -> host frame bytes (header ‖ body); only compressed bytes cross PCIe."""
    body = compress_device(lib, flat, num_buf, bits_mode, bytes_mode, chunk, threshold)
    hl = len(header)
    total = hl + body.numel()
    # (from 8 MiB up a block of the library's pinned arena — ZnLib.host_buffer —: the body then crosses PCIe as one DMA into memory that needs no page faults and
    #  goes back to the arena, not to munmap, when the caller drops the frame; the caller sees a memoryview either way, as from the reference's extension)
    frame = lib.host_buffer(total) if hasattr(lib, "host_buffer") and total >= getattr(lib, "HOST_ARENA_MIN", 1 << 62) else new_bytearray(total)
    fv = memoryview(frame).cast("B")
    fv[:hl] = bytes(header)
    if hl >= 32:
        fv[24:32] = total.to_bytes(8, "little")           # what the reference core writes at zipnn_core.c:121
    to_host(lib, body, fv[hl:])
    return frame


def decompress_device(lib, body, num_buf, bits_mode, bytes_mode, chunk, orig_size, out=None, check=True, delta=None):
    """body: uint8 tensor in HBM (frame minus header) -> uint8 tensor of orig_size bytes on
    the same device.  delta: optional uint8 tensor of orig_size bytes XORed into the output inside the
    kernels that write it (reference zipnn/zipnn.py:983-1004)."""
    if out is None:
        out = torch.empty(orig_size, dtype=torch.uint8, device=body.device)
    if orig_size == 0:
        return out
    body = body.contiguous()
    delta, dptr = _delta_ptr(delta, out)
    with _device_of(body.device):
        lib.decompress_dev(body.data_ptr(), body.numel(), num_buf, bits_mode, bytes_mode, chunk, orig_size,
                           out.data_ptr(), _stream_handle(body), check, delta_ptr=dptr)
    return out


def decompress_device_batch(lib, items, check=True, into=None):
    """Many tensors, one set of kernel launches (zn_decompress_batch_dev): small tensors fill the device together.
    items: iterable of (body, num_buf, bits_mode, bytes_mode, chunk, orig_size[, delta]) with `body` a uint8 tensor on
    the device (frame minus header) and `delta` an optional uint8 base of orig_size bytes.  Returns the list of
    decoded uint8 tensors (same device)."""
    items = list(items)
    deltas = [(it[6].contiguous() if len(it) > 6 and it[6] is not None else None) for it in items]
    items = [(it[0].contiguous(),) + tuple(it[1:6]) for it in items]
    if not items:
        return []
    for d, it in zip(deltas, items):
        if d is not None and (d.dtype != torch.uint8 or d.numel() != it[5] or d.device != it[0].device):
            raise ValueError("delta base must be a uint8 tensor of orig_size bytes on the same device")
    dev = items[0][0].device
    if into is not None:                       # one preallocated buffer: tensor i lands at the running offset
        assert into.numel() >= sum(n for (_, _, _, _, _, n) in items)
        offs, o = [], 0
        for (_, _, _, _, _, n) in items:
            offs.append(o); o += n
        outs = [into[o:o + n] for o, (_, _, _, _, _, n) in zip(offs, items)]
    else:
        outs = [torch.empty(n, dtype=torch.uint8, device=dev) for (_, _, _, _, _, n) in items]
    with _device_of(dev):
        lib.decompress_batch_dev(((b.data_ptr(), b.numel(), nb, bi, by, ch, n, o.data_ptr() if n else 0,
                                   d.data_ptr() if (d is not None and n) else None)
                                  for (b, nb, bi, by, ch, n), o, d in zip(items, outs, deltas)), _stream_handle(items[0][0]), check)
    return outs


def window_bytes(chunk, orig_size, chunk_lo, chunk_hi):
    """Bytes that chunks [chunk_lo, chunk_hi) of a tensor of orig_size bytes decode to."""
    return max(min(chunk_hi * chunk, orig_size) - chunk_lo * chunk, 0)


def decompress_device_windows(lib, items, check=True, outs=None):
    """Chunk windows of device-resident bodies, one set of kernel launches (zn_decompress_window_batch_dev): nothing is copied or re-based,
    the kernels read the window's rows of the WHOLE body's size tables.
    items: iterable of (body, num_buf, bits_mode, bytes_mode, chunk, orig_size, chunk_lo, chunk_hi[, delta]) with `body` the whole frame body
    (uint8 tensor on the device) and `delta` an optional uint8 base of the WHOLE tensor (orig_size bytes).  outs: optional list of uint8
    destinations (window_bytes(...) bytes each).  Returns the list of decoded uint8 tensors (same device)."""
    items = [(it[0].contiguous(),) + tuple(it[1:8]) + ((it[8].contiguous() if len(it) > 8 and it[8] is not None else None),) for it in items]
    if not items:
        return []
    dev = items[0][0].device
    for (b, _, _, _, _, n, _, _, d) in items:
        if d is not None and (d.dtype != torch.uint8 or d.numel() != n or d.device != b.device):
            raise ValueError("delta base must be a uint8 tensor of orig_size bytes on the same device")
    sizes = [window_bytes(ch, n, lo, hi) for (_, _, _, _, ch, n, lo, hi, _) in items]
    if outs is None:
        outs = [torch.empty(sz, dtype=torch.uint8, device=dev) for sz in sizes]
    elif len(outs) != len(items) or any(o.numel() < sz or o.dtype != torch.uint8 or not o.is_contiguous() for o, sz in zip(outs, sizes)):
        raise ValueError("outs: one contiguous uint8 destination of the window's size per item")
    with _device_of(dev):
        lib.decompress_window_batch_dev(((b.data_ptr(), b.numel(), nb, bi, by, ch, n, lo, hi, o.data_ptr() if sz else 0,
                                          d.data_ptr() if (d is not None and n) else None)
                                         for (b, nb, bi, by, ch, n, lo, hi, d), o, sz in zip(items, outs, sizes)), _stream_handle(items[0][0]), check)
    return outs


def compress_device_batch(lib, items, gap=0, return_arena=False):
    """Many tensors, one launch per stage (zn_compress_batch_dev), one read-back of all lengths.
    items: iterable of (flat_uint8_device_tensor, num_buf, bits_mode, bytes_mode, chunk, threshold[, delta]).
    Returns the list of body tensors (uint8, same device; slices of one arena).
    gap: bytes left free in FRONT of every body (a multiple of 256: the bodies stay 256-byte aligned) — room for the frame header when the arena goes
    to the host in one piece; return_arena: -> (arena, [offset of each body in it], [body lengths]) instead of the slices."""
    items = list(items)
    deltas = [(it[6].contiguous() if len(it) > 6 and it[6] is not None else None) for it in items]
    items = [(it[0].contiguous(),) + tuple(it[1:6]) for it in items]
    if not items:
        return []
    for d, it in zip(deltas, items):
        if d is not None and (d.dtype != torch.uint8 or d.numel() != it[0].numel() or d.device != it[0].device):
            raise ValueError("delta base must be a uint8 tensor of the same length on the same device")
    dev = items[0][0].device
    caps = [max(lib.compress_bound(f.numel(), nb, ch, 0), 16) for (f, nb, _, _, ch, _) in items]
    if gap % 256:
        raise ValueError("gap must be a multiple of 256")
    offs, o = [], 0
    for c in caps:
        o += gap
        offs.append(o); o += (c + 255) // 256 * 256
    arena = torch.empty(max(o, 16), dtype=torch.uint8, device=dev)
    base = arena.data_ptr()
    with _device_of(dev):
        lens = lib.compress_batch_dev(((f.data_ptr() if f.numel() else 0, f.numel(), nb, bi, by, ch, th, base + b0, c,
                                        d.data_ptr() if (d is not None and f.numel()) else None)
                                       for (f, nb, bi, by, ch, th), c, b0, d in zip(items, caps, offs, deltas)), _stream_handle(arena))
    if return_arena:
        return arena, offs, lens
    return [arena[b0:b0 + n] for b0, n in zip(offs, lens)]


def build_decode_hints(lib, items):
    """Decode hints (include/zipnn_hip.h) for bodies that stay where they are: items = window item tuples as for
    ZnLib.decompress_window_batch_dev (the window and the destination are ignored — an index covers the whole body).  -> one uint8 tensor
    per item, on the body's device (a CPU tensor for the emulated library), for ZnLib.decompress_hinted_batch_dev / plan_create_hinted.
    The hints hold for the body AT ITS ADDRESS: keep the body tensor alive and in place."""
    out = []
    for it in items:
        n = lib.hint_size_dev(it)
        dev = torch.device("cuda", current_device()) if torch.cuda.is_available() else torch.device("cpu")
        h = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
        lib.hint_build_dev(it, h.data_ptr(), n)
        out.append(h[:n])
    return out


# ---- changed-element patches ("znp1": include/zipnn_hip.h) -------------------------------------------------------------------
def patch_elem(t):
    """-> the element size a patch of tensor `t` is built with (1, 2 or 4), or None where a patch cannot describe it (other element sizes, 2^32 elements or more)."""
    es = t.element_size()
    return es if es in (1, 2, 4) and t.numel() < (1 << 32) else None


def patch_sizes_device_batch(lib, pairs):
    """pairs: [(flat uint8 source, flat uint8 base, elem)] on one device -> the lengths of their patches (0: identical bytes): the count pass alone, one read-back."""
    pairs = list(pairs)
    if not pairs:
        return []
    dev = pairs[0][0].device
    with _device_of(dev):
        return lib.patch_size_batch_dev([(s.data_ptr() if s.numel() else 0, b.data_ptr() if s.numel() else 0, s.numel(), el) for s, b, el in pairs], _stream_handle(pairs[0][0]))


def patch_build_device_batch(lib, pairs, sizes=None):
    """pairs: [(flat uint8 source, flat uint8 base, elem)] on one device -> their patches: uint8 tensors (views of one allocation, each at a multiple of 256
    bytes), None where the bytes are identical.  sizes: the lengths patch_sizes_device_batch gave for the same pairs (else they are counted here)."""
    pairs = list(pairs)
    if not pairs:
        return []
    for s, b, _ in pairs:
        if s.dtype != torch.uint8 or b.dtype != torch.uint8 or s.numel() != b.numel() or s.device != b.device or not s.is_contiguous() or not b.is_contiguous():
            raise ValueError("patch: contiguous uint8 views of the same length on one device")
    if sizes is None:
        sizes = patch_sizes_device_batch(lib, pairs)
    dev = pairs[0][0].device
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += (n + 255) // 256 * 256
    arena = torch.empty(max(o, 16), dtype=torch.uint8, device=dev)
    with _device_of(dev):
        lens = lib.patch_build_batch_dev([(s.data_ptr() if s.numel() else 0, b.data_ptr() if s.numel() else 0, s.numel(), el, arena.data_ptr() + off, n)
                                          for (s, b, el), off, n in zip(pairs, offs, sizes)], _stream_handle(arena))
    return [arena[off:off + n] if n else None for off, n in zip(offs, lens)]


def _patch_strided_pairs(pairs):
    """[(source view, base view)] -> the items of ZnLib.patch_size_strided_batch_dev: two tensors of one dtype and shape on one device, each in a layout of its own."""
    from . import _capi
    items = []
    for s, b in pairs:
        if s.dtype != b.dtype or tuple(s.shape) != tuple(b.shape) or s.device != b.device or patch_elem(s) is None:
            raise ValueError("patch: two tensors of the same dtype (1, 2 or 4 bytes per element) and shape on one device, fewer than 2^32 elements")
        if s.dim() > _capi.PATCH_MAX_DIMS:
            raise ValueError(f"patch: {s.dim()} dimensions (at most {_capi.PATCH_MAX_DIMS})")
        m, el = s.numel(), s.element_size()
        items.append((s.data_ptr() if m else 0, b.data_ptr() if m else 0, m * el, el, tuple(s.shape), tuple(s.stride()), tuple(b.stride())))
    return items


def patch_sizes_strided_device_batch(lib, pairs):
    """pairs: [(source, base)]: tensors in any layouts zn_patch_size_strided_batch_dev accepts (include/zipnn_hip.h) -> the lengths of their
    patches (0: identical bytes): the count pass alone, one read-back, no copy of either side."""
    pairs = [(s.detach(), b.detach()) for s, b in pairs]
    if not pairs:
        return []
    dev = pairs[0][0].device
    with _device_of(dev):
        return lib.patch_size_strided_batch_dev(_patch_strided_pairs(pairs), _stream_handle(pairs[0][0]))


def patch_build_strided_device_batch(lib, pairs, sizes=None, return_arena=False):
    """pairs: [(source, base)] as for patch_sizes_strided_device_batch -> their patches: uint8 tensors (views of one allocation, each at a multiple of 256
    bytes), None where the bytes are identical — by ONE zn_patch_build_strided_batch_dev call, byte for byte what patch_build_device_batch gives for contiguous
    copies of the views.  sizes: the lengths patch_sizes_strided_device_batch gave for the same pairs (else they are counted here).  return_arena: -> (the
    patches, the allocation they are views of, or None)."""
    pairs = [(s.detach(), b.detach()) for s, b in pairs]
    if not pairs:
        return ([], None) if return_arena else []
    items = _patch_strided_pairs(pairs)
    dev = pairs[0][0].device
    if sizes is None:
        with _device_of(dev):
            sizes = lib.patch_size_strided_batch_dev(items, _stream_handle(pairs[0][0]))
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += (n + 255) // 256 * 256
    arena = torch.empty(max(o, 16), dtype=torch.uint8, device=dev)
    with _device_of(dev):
        lens = lib.patch_build_strided_batch_dev([it + (arena.data_ptr() + off, n) for it, off, n in zip(items, offs, sizes)], _stream_handle(arena))
    out = [arena[off:off + n] if n else None for off, n in zip(offs, lens)]
    return (out, arena) if return_arena else out


def patch_build(t, base):
    """The "znp1" patch (include/zipnn_hip.h) that turns `base` into `t`: the elements whose bytes differ, with their XOR values — a uint8 tensor on the
    tensors' device, or None when the bytes are identical.  t and base: the same dtype (1, 2 or 4 bytes per element) and shape, on one device.  Either may be
    any strided view of at most 8 dimensions — a weight an engine keeps transposed, a column slice of a fused buffer, an expand()ed tensor —: both are read
    where they lie, through their layouts (zn_patch_build_strided_batch_dev), and no contiguous copy is made; the patch is the one their
    contiguous copies would give.  With p = patch_build(new, live.t()), patch_apply_(live.t(), p) leaves `new` in the live weight."""
    from . import _capi
    if t.dtype != base.dtype or tuple(t.shape) != tuple(base.shape) or t.device != base.device:
        raise ValueError("patch_build: two tensors of the same dtype and shape on one device")
    el = patch_elem(t)
    if el is None:
        raise ValueError(f"patch_build: {t.dtype} with {t.numel()} elements is not eligible (elements of 1, 2 or 4 bytes, fewer than 2^32 of them)")
    t, base = t.detach(), base.detach()
    if t.is_contiguous() and base.is_contiguous():
        return patch_build_device_batch(_capi.lib(), [(flat_bytes(t), flat_bytes(base), el)])[0]
    return patch_build_strided_device_batch(_capi.lib(), [(t, base)])[0]


def patch_layout_refusal(t):
    """Why zn_patch_apply_strided_batch_dev would refuse the strided view `t` (include/zipnn_hip.h; the library's own test, restated so that the error can say
    why), or None: more than 8 dimensions, a stride of 0 (expand()), or dimensions that overlap — sorted by stride, a stride that does not exceed the sum over
    the smaller ones of (size - 1) stride.  The test is sufficient, not necessary."""
    from . import _capi
    if t.dim() > _capi.PATCH_MAX_DIMS:
        return f"{t.dim()} dimensions (at most {_capi.PATCH_MAX_DIMS})"
    span = 0
    for st, sz in sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1):
        if st < 0:
            return "a negative stride"
        if st == 0:
            return "a stride of 0 (an expanded view: several elements share memory)"
        if st <= span:
            return f"strides {tuple(t.stride())} over sizes {tuple(t.shape)} may overlap (stride {st} does not step past the {span} elements the smaller strides span)"
        span += (sz - 1) * st
    return None


def patch_strided_item(t, patch):
    """-> the item of ZnLib.patch_apply_strided_batch_dev that applies `patch` (a uint8 tensor) through the strided view `t`; ValueError where the view is refused."""
    why = patch_layout_refusal(t) if t.numel() else None
    if why:
        raise ValueError(f"patch: the view cannot be patched in place: {why}")
    el = t.element_size()
    return (patch.data_ptr(), patch.numel(), t.numel() * el, el, t.data_ptr() if t.numel() else 0, tuple(t.shape), tuple(t.stride()))


def patch_apply_(t, patch, check=True):
    """t ^= patch, in place: a tensor that holds the base's values holds the fine-tune's afterwards, and the base's again after a second call.  patch: what
    patch_build returned (None: nothing to do).  `t` may have any shape and strides: only its numel and its LOGICAL row-major order matter — a transposed
    weight, a column slice of a fused buffer, the N-D view that undoes a tile shuffle.  A contiguous `t` takes zn_patch_apply_batch_dev; any other goes through
    its layout (zn_patch_apply_strided_batch_dev, DESIGN §3.15: an index map per entry, no pass over the tensor, no scratch copy), provided its strides pass the
    library's injectivity test — expand()ed and overlapping views raise a ValueError that says why.  A malformed patch raises (ZN_E_CORRUPT / ZN_E_ARG) and
    never writes outside the elements of `t`.  -> t"""
    from . import _capi
    if patch is None:
        return t
    d = t.detach()
    el = patch_elem(d)
    if el is None:
        raise ValueError("patch_apply_: a tensor with elements of 1, 2 or 4 bytes, fewer than 2^32 of them")
    if patch.dtype != torch.uint8 or patch.device != d.device or not patch.is_contiguous():
        raise ValueError("patch_apply_: the patch is a contiguous uint8 tensor on the tensor's device")
    n = d.numel() * el
    with _device_of(d.device):
        if d.is_contiguous():
            _capi.lib().patch_apply_batch_dev([(patch.data_ptr(), patch.numel(), n, el, 0, n, d.data_ptr() if n else 0)], _stream_handle(d), check)
        else:
            _capi.lib().patch_apply_strided_batch_dev([patch_strided_item(d, patch)], _stream_handle(d), check)
    return t


def _patch_merge_items(triples):
    triples = list(triples)
    for a, b, _, _ in triples:
        if (a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.device != triples[0][0].device or b.device != a.device
                or not a.is_contiguous() or not b.is_contiguous()):
            raise ValueError("patch merge: contiguous uint8 tensors on one device")
    return triples


def patch_merge_sizes_device_batch(lib, triples):
    """triples: [(patch a, patch b, n: the tensor's bytes, elem)] on one device, the patches contiguous uint8 tensors at 16-byte aligned addresses -> the
    lengths of their XOR-merges (0: everything cancels): the count pass alone, one read-back.  It validates both inputs whole (ZnError(ZN_E_CORRUPT))."""
    triples = _patch_merge_items(triples)
    if not triples:
        return []
    dev = triples[0][0].device
    with _device_of(dev):
        return lib.patch_merge_size_batch_dev([(a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), n, el) for a, b, n, el in triples], _stream_handle(triples[0][0]))


def patch_merge_device_batch(lib, triples, sizes=None, return_arena=False):
    """triples as for patch_merge_sizes_device_batch -> the merged patches: uint8 tensors (views of one allocation, each at a multiple of 256 bytes), None where
    everything cancels — by ONE zn_patch_merge_batch_dev call.  sizes: the lengths patch_merge_sizes_device_batch gave for the same triples (else they are
    counted here).  return_arena: (arena, offsets, lengths) instead."""
    triples = _patch_merge_items(triples)
    if not triples:
        return (None, [], []) if return_arena else []
    if sizes is None:
        sizes = patch_merge_sizes_device_batch(lib, triples)
    dev = triples[0][0].device
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += (n + 255) // 256 * 256
    arena = torch.empty(max(o, 16), dtype=torch.uint8, device=dev)
    with _device_of(dev):
        lens = lib.patch_merge_batch_dev([(a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), n, el, arena.data_ptr() + off if cap else 0, cap)
                                          for (a, b, n, el), off, cap in zip(triples, offs, sizes)], _stream_handle(arena))
    if return_arena:
        return arena, offs, lens
    return [arena[off:off + n] if n else None for off, n in zip(offs, lens)]


def _patch_header(p, what):
    import struct
    if p.dtype != torch.uint8 or not p.is_contiguous() or p.numel() < 32:
        raise ValueError(f"patch_merge: {what} is a contiguous uint8 tensor of at least 32 bytes")
    h = bytes(p[:32].cpu().numpy())
    if h[:4] != b"ZNP1":
        raise ValueError(f"patch_merge: {what} is not a znp1 patch")
    return h[4], struct.unpack_from("<Q", h, 8)[0]


def patch_merge(pa, pb):
    """The XOR-merge of two "znp1" patches of one tensor (include/zipnn_hip.h): the union of their elements, the XOR of the values where both have an entry, no
    entry where that is zero.  With pa = patch_build(A, base) and pb = patch_build(B, base) the result is patch_build(B, A), byte for byte, without A, B or the
    base: patch_apply_ of it turns a tensor that holds A into B, and back.  pa, pb: uint8 tensors on one device; the tensor's size and element size are read
    from their headers, which must agree (ValueError).  -> the merged patch, or None when they cancel.  Both inputs are validated whole on the way: a malformed
    one raises ZnError(ZN_E_CORRUPT)."""
    from . import _capi
    if pa.device != pb.device:
        raise ValueError("patch_merge: two patches on one device")
    (ea, na), (eb, nb) = _patch_header(pa, "the first patch"), _patch_header(pb, "the second patch")
    if (ea, na) != (eb, nb):
        raise ValueError(f"patch_merge: the patches describe different tensors ({na} bytes in elements of {ea} against {nb} in elements of {eb})")
    pa, pb = (p if p.data_ptr() % 16 == 0 else p.clone() for p in (pa, pb))
    return patch_merge_device_batch(_capi.lib(), [(pa, pb, na, ea)])[0]


def patch_select_device_batch(lib, items, place=False, sizes=None, return_arena=False):
    """items: [(patch, elem, rows, cols, row_lo, row_hi, col_lo, col_hi)] on one device, the patches contiguous uint8 tensors at 16-byte aligned addresses ->
    place=False: the patches of those rectangles of the tensors the inputs cover; place=True: the inputs cover the rectangles, the results the whole tensors
    (include/zipnn_hip.h, SHARDING PATCHES).  uint8 tensors (views of one allocation, each at a multiple of 256 bytes), None where no entry results — by ONE
    zn_patch_select_batch_dev / zn_patch_place_batch_dev call.  sizes: the lengths the size call gave for the same items (else they are counted here).
    return_arena: (arena, offsets, lengths) instead."""
    items = list(items)
    if not items:
        return (None, [], []) if return_arena else []
    dev = items[0][0].device
    for it in items:
        p = it[0]
        if p.dtype != torch.uint8 or p.device != dev or not p.is_contiguous():
            raise ValueError("patch select: contiguous uint8 tensors on one device")
    args = [(it[0].data_ptr(), it[0].numel()) + tuple(it[1:8]) for it in items]
    with _device_of(dev):
        if sizes is None:
            sizes = (lib.patch_place_size_batch_dev if place else lib.patch_select_size_batch_dev)(args, _stream_handle(items[0][0]))
        offs, o = [], 0
        for n in sizes:
            offs.append(o)
            o += (n + 255) // 256 * 256
        arena = torch.empty(max(o, 16), dtype=torch.uint8, device=dev)
        lens = (lib.patch_place_batch_dev if place else lib.patch_select_batch_dev)(
            [a + (arena.data_ptr() + off if cap else 0, cap) for a, off, cap in zip(args, offs, sizes)], _stream_handle(arena))
    if return_arena:
        return arena, offs, lens
    return [arena[off:off + n] if n else None for off, n in zip(offs, lens)]


def narrow_rect(shape, dim, lo, hi):
    """A narrow(dim, lo, hi - lo) of a tensor of `shape` as a rectangle of its elements -> (rows, cols, row_lo, row_hi, col_lo, col_hi): rows = prod(shape[:dim]),
    cols = shape[dim] * inner, all rows, cols [lo * inner, hi * inner).  ValueError for a dimension or a range the shape does not have."""
    shape = tuple(int(s) for s in shape)
    if not -len(shape) <= dim < len(shape):
        raise ValueError(f"dimension {dim} of a tensor of shape {shape}")
    dim %= len(shape)
    if not 0 <= lo < hi <= shape[dim]:
        raise ValueError(f"the range [{lo}, {hi}) of dimension {dim} of shape {shape} (a non-empty range inside the dimension)")
    rows = inner = 1
    for s in shape[:dim]:
        rows *= s
    for s in shape[dim + 1:]:
        inner *= s
    if rows == 0 or inner == 0:
        raise ValueError(f"a tensor of shape {shape} has no elements")
    return rows, shape[dim] * inner, 0, rows, lo * inner, hi * inner


def _patch_select_public(what, patch, shape, dim, lo, hi, place):
    from . import _capi
    try:
        E, n = _patch_header(patch, "the patch")
    except ValueError as e:
        raise ValueError(str(e).replace("patch_merge", what)) from None
    rect = narrow_rect(shape, dim, lo, hi)
    covered = (rect[3] - rect[2]) * (rect[5] - rect[4]) if place else rect[0] * rect[1]
    if E not in (1, 2, 4) or n != covered * E:
        raise ValueError(f"{what}: the patch covers {n} bytes in elements of {E}; {'the narrowed tensor' if place else 'a tensor of shape ' + str(tuple(shape))} has {covered} elements")
    if rect[0] * rect[1] >= 1 << 32:
        raise ValueError(f"{what}: patches cover fewer than 2^32 elements")
    if patch.data_ptr() % 16:
        patch = patch.clone()
    return patch_select_device_batch(_capi.lib(), [(patch, E) + rect], place=place)[0]


def patch_select(patch, shape, dim, lo, hi):
    """The "znp1" patch of a shard, from the patch of the whole tensor: with patch = patch_build(t, base), t and base of `shape`, the result is byte for byte
    patch_build(t.narrow(dim, lo, hi - lo).contiguous(), base.narrow(dim, lo, hi - lo).contiguous()) — without t or base — or None when nothing changed inside
    the shard.  The element size is read from the patch's header, whose n must be prod(shape) elements (ValueError).  The input is validated where the select
    reads it (the header, and the blocks that overlap the shard: ZnError(ZN_E_CORRUPT)); patch_check validates a whole patch."""
    return _patch_select_public("patch_select", patch, shape, dim, lo, hi, False)


def patch_place(patch, shape, dim, lo, hi):
    """The inverse of patch_select: `patch` covers the narrow(dim, lo, hi - lo) of a tensor of `shape`; the result covers the whole tensor and changes exactly
    those elements (None for a patch without entries).  patch_select(patch_place(p, ...), ...) is p, and patch_merge of the placed patches
    of disjoint shards that tile the tensor is the whole tensor's patch.  The input is validated whole on the way (ZnError(ZN_E_CORRUPT))."""
    return _patch_select_public("patch_place", patch, shape, dim, lo, hi, True)


PATCH_BAD_NAMES = ((1, "header"), (2, "first"), (4, "offset"), (8, "value"), (16, "padding"))      # the ZN_PATCH_BAD_* bits of a check verdict


def patch_verdict_text(mask):
    """A zn_patch_check_batch_dev verdict in words: 'offset+value (0x0c)'."""
    return "+".join(name for bit, name in PATCH_BAD_NAMES if mask & bit) + f" (0x{mask:02x})"


def patch_check_device_batch(lib, items, stream=None):
    """items: [(patch: a contiguous uint8 tensor at a 16-byte aligned address, n: the tensor's bytes, elem)] on one device -> ([verdict mask], [T]) by ONE
    zn_patch_check_batch_dev launch and one read-back: are the patches well-formed, the whole of each, for tensors of those sizes?  Nothing is written."""
    items = list(items)
    if not items:
        return [], []
    for p, _, _ in items:
        if p.dtype != torch.uint8 or not p.is_contiguous() or p.device != items[0][0].device:
            raise ValueError("patch: contiguous uint8 tensors on one device")
    dev = items[0][0].device
    with _device_of(dev):
        return lib.patch_check_batch_dev([(p.data_ptr(), p.numel(), n, el) for p, n, el in items], stream if stream is not None else _stream_handle(items[0][0]))


def patch_check(patch, t):
    """Is `patch` a well-formed "znp1" patch (include/zipnn_hip.h) for tensor `t` — what patch_build gives for a tensor of t's dtype and size?  Every field, every
    first[] pair, every entry and the padding are checked on the device, read-only, before anything is applied (patch_apply_ checks as it goes, and has written by
    then).  -> T, the number of elements the patch changes; a malformed patch raises ZnError(ZN_E_CORRUPT) whose `mask` holds the ZN_PATCH_BAD_* bits.  None
    (identical tensors) -> 0.  Well-formed is not RIGHT: a patch of another tensor of the same size passes; content digests tell those apart."""
    from . import _capi
    if patch is None:
        return 0
    d = t.detach()
    el = patch_elem(d)
    if el is None:
        raise ValueError("patch_check: a tensor with elements of 1, 2 or 4 bytes, fewer than 2^32 of them")
    if patch.dtype != torch.uint8 or patch.device != d.device or not patch.is_contiguous():
        raise ValueError("patch_check: the patch is a contiguous uint8 tensor on the tensor's device")
    verdicts, entries = patch_check_device_batch(_capi.lib(), [(patch, d.numel() * el, el)])
    if verdicts[0]:
        err = _capi.ZnError(_capi.ZN_E_CORRUPT, f"patch_check: the patch is malformed: {patch_verdict_text(verdicts[0])}")
        err.mask = verdicts[0]
        raise err
    return entries[0]


# ---- content digests ("zn64-1": include/zipnn_hip.h) -------------------------------------------------------------------------
DIGEST_ALGO = "zn64-1"


class DigestMismatch(ValueError):
    """Decoded or live bytes do not have the digest that was recorded for them.  `names`: the tensors concerned."""

    def __init__(self, names, what="digest mismatch"):
        self.names = list(names)
        super().__init__(f"{what}: {', '.join(repr(n) for n in self.names)}")


def digest_device_batch(lib, flats, stream=None, out=None):
    """flats: contiguous uint8 tensors on ONE device (any byte address, any length) -> an int64 tensor on that device with their digests' bit patterns, by
    one zn_digest_batch_dev launch on `stream` (a raw handle; default: the device's current stream).  Nothing waits: read the result behind the stream
    (digests_to_ints), and keep `flats` alive until then.  out: len(flats) contiguous int64 slots on the device to write to instead of a new tensor."""
    flats = list(flats)
    dev = flats[0].device if flats else (out.device if out is not None else torch.device("cpu"))
    if out is None:
        out = torch.empty(max(len(flats), 1), dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or out.device != dev or not out.is_contiguous() or out.numel() < len(flats):
        raise ValueError("digest: out must be a contiguous int64 tensor on the tensors' device, one slot per tensor")
    if flats:
        if any(f.dtype != torch.uint8 or f.device != dev or not f.is_contiguous() for f in flats):
            raise ValueError("digest: contiguous uint8 tensors on one device")
        with _device_of(dev):
            lib.digest_batch_dev([(f.data_ptr() if f.numel() else 0, f.numel()) for f in flats], out.data_ptr(),
                                 stream if stream is not None else _stream_handle(out))
    return out[:len(flats)]


def digests_to_ints(out):
    """The one read-back of a digest_device_batch result (8 bytes per item; waits for the stream) -> list of unsigned ints."""
    return [v & 0xFFFFFFFFFFFFFFFF for v in out.tolist()]


def digests_of(lib, tensors, stream=None):
    """Live tensors on ONE device -> their digests as ints, in order: digested where they lie by one batched launch, one read-back."""
    tensors = list(tensors)
    if not tensors:
        return []
    with _device_of(tensors[0].device):
        return digests_to_ints(digest_device_batch(lib, [flat_bytes(t) for t in tensors], stream))


def _host_bytes(x):
    """A CPU tensor, numpy array or bytes-like -> a bytes-like object of its contiguous bytes."""
    if isinstance(x, torch.Tensor):
        return memoryview(flat_bytes(x.detach()).numpy())
    import numpy as np
    if isinstance(x, np.ndarray):
        return memoryview(np.ascontiguousarray(x).reshape(-1).view(np.uint8))
    return memoryview(x).cast("B")


def digest_many(tensors):
    """Digests of many tensors -> list of ints, in order.  Device tensors: ONE launch (per device) for all of them and one read-back of 8 bytes each;
    CPU tensors, numpy arrays and bytes-like objects go through the host function (zn_digest_host).  The digest covers the contiguous bytes of each
    (a non-contiguous tensor is made contiguous first).  An error-detecting code, not a cryptographic hash."""
    from . import _capi
    lib = _capi.lib()
    tensors = list(tensors)
    res = [None] * len(tensors)
    by_dev = {}
    for i, x in enumerate(tensors):
        if isinstance(x, torch.Tensor) and x.is_cuda:
            by_dev.setdefault(x.device, []).append((i, flat_bytes(x.detach())))
        else:
            res[i] = lib.digest_host(_host_bytes(x))
    pending = [(items, digest_device_batch(lib, [f for _, f in items])) for items in by_dev.values()]
    for items, out in pending:
        for (i, _), v in zip(items, digests_to_ints(out)):
            res[i] = v
    return res


def digest(x):
    """The "zn64-1" content digest of a device tensor, a CPU tensor, a numpy array or a bytes-like object: an int below 2^64 (see digest_many)."""
    return digest_many([x])[0]
