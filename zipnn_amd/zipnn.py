"""ZipNN().compress()/decompress() and the zipnn_safetensors() plugin, on MI355X.

Drop-in for the reference's L3/L4 surface on the compress/decompress hot path
(reference zipnn/zipnn.py: class ZipNN :27-1218, SafeOpen/zipnn_safetensors :1584-1643):
same constructor keywords, same frame bytes, same return types, same exceptions — but
the two calls into the C extension (zipnn.py:714 `zipnn_core.zipnn_core`, :1143
`zipnn_core.combine_dtype`) go to the HIP library through `zipnn_amd._capi` instead.
There is no CPU code path here: without a GPU / the built extension the calls raise.

Additions the reference does not have (all optional):
  * tensors that already live on a GPU are compressed in place in HBM (no host round trip
    of the uncompressed bytes);
  * `decompress(..., decompress_cpu_gpu="cuda:0")` (the reference accepts and ignores this
    argument, zipnn.py:928) returns the tensor on that device, so a loader ships only the
    compressed bytes over PCIe.
"""
import json
import math
import multiprocessing

import numpy as np
import torch

from . import _capi, codec
from .header import (HEADER_LEN, VERSION, EnumFormat, EnumLossy, EnumMethod, dtype_from_code, dtype_from_user,
                     is_pow2, pack_shape, unpack_shape)

FP8_CHUNK_CAP = 128 * 1024   # huff0 block limit; fp8 has one plane per chunk (reference zipnn.py:721,1148)


def _delta_code(kind):
    return 1 if kind == "byte" else 2 if kind == "file" else 0


class ZipNN:
    def __init__(self, method: str = "AUTO", input_format: str = "byte", bytearray_dtype: str = "bfloat16",
                 is_monotonic: int = 0, threads: int = 0, compression_threshold=0.95, check_th_after_percent=10,
                 byte_reorder: int = 0, reorder_signbit: int = 0, delta_compressed_type: str = 0,
                 lossy_compressed_type: str = 0, lossy_compressed_factor=27, compression_chunk=256 * 1024,
                 is_streaming: bool = False, streaming_chunk: int = 1024 * 1024, input_file: str = None,
                 compressed_file: str = None, decompressed_file: str = None, zstd_level: int = 3,
                 lz4_compression_level: int = 0, *, devices=None):
        """Same keywords as the reference constructor (zipnn/zipnn.py:29-51), plus one keyword-only extension:
        `devices` — GPU ordinals; with more than one, host-buffer input is coded with its chunk ranges spread over them
        (zn_compress_multi / zn_decompress_multi: one host thread and stream per device, no collective, same bytes) —
        the role `threads` plays in the reference core.

        `method` only selects header byte 7: on this path the core always codes with huff0,
        exactly as the reference does (zipnn.py:658-668 never changes the codec when byte
        grouping is on).  `threads`, `check_th_after_percent`, `is_monotonic`, `byte_reorder`
        and `reorder_signbit` are accepted and recorded; the GPU path has no use for them
        (they are dead in the reference core too — SURVEY.md Appendix D).
        """
        self.method = EnumMethod(method).value
        self.input_format = EnumFormat(input_format).value
        self.bytearray_dtype = bytearray_dtype
        self.is_monotonic = is_monotonic
        self.threads = threads or min(multiprocessing.cpu_count(), 16)
        self.devices = [int(d) for d in devices] if devices else None
        self.compression_threshold = compression_threshold
        self.check_th_after_percent = check_th_after_percent
        self.byte_reorder = byte_reorder
        self.reorder_signbit = reorder_signbit
        self.delta_compressed_type = delta_compressed_type
        self.lossy_compressed_type = EnumLossy.NONE if lossy_compressed_type is None else EnumLossy(lossy_compressed_type)
        self.lossy_compressed_factor = lossy_compressed_factor
        if not is_pow2(compression_chunk):
            raise ValueError("compression_chunk must be a number that is a power of 2.")
        self.compression_chunk = compression_chunk
        if self.input_format != EnumFormat.BYTE.value and is_streaming:
            raise ValueError("Streaming is currently implemented only for bytes data type.")
        self.is_streaming = is_streaming
        if not is_pow2(streaming_chunk):
            raise ValueError("streaming_chunk must be a number that is a power of 2.")
        self.streaming_chunk = streaming_chunk
        self.input_file = input_file
        self.compressed_file = compressed_file
        self.decompressed_file = decompressed_file
        self.zstd_level = zstd_level
        self.lz4_compression_level = lz4_compression_level
        if self.lossy_compressed_type != EnumLossy.NONE and self.input_format != EnumFormat.TORCH.value:
            raise ValueError("When use lossy compression the input have to be torch.tensor")
        self._version_major, self._version_minor, self._version_tiny = VERSION
        self.header_length = HEADER_LEN
        self._header = bytearray(HEADER_LEN)
        self._ext_header = b""
        self._shape_size = 0
        self._update_header()

    # ------------------------------------------------------------------ header
    def _update_header(self):
        """Static header fields (reference zipnn.py:355-394)."""
        h = self._header
        h[0:2] = b"ZN"
        h[2], h[3], h[4] = VERSION
        h[7] = self.method
        h[8] = self.input_format
        h[9] = 0 if self.delta_compressed_type is None else _delta_code(self.delta_compressed_type)
        h[13] = 128 + int(math.log(self.streaming_chunk, 2)) if self.is_streaming else 0
        h[14] = int(math.log(self.compression_chunk, 2))

    def _retrieve_header(self, frame):
        """Parse a frame header into instance state (the reference overwrites its own
        configuration the same way, zipnn.py:396-438) and return the offset of the body."""
        mv = memoryview(frame)
        h = mv[:HEADER_LEN]
        if h[0:2].tobytes() != b"ZN":
            raise ValueError("Header should start with ZN")
        self.version_major, self.version_minor, self.version_tiny = int(h[2]), int(h[3]), int(h[4])
        self._byte_reorder = int(h[5])
        self._bit_reorder = int(h[6])
        self.method = int(h[7])
        self.input_format = int(h[8])
        d = self._header[9]   # sic: the reference reads its OWN header byte here (zipnn.py:420-422)
        self.delta_compressed_type = "byte" if d == 1 else "file" if d == 2 else 0
        self.lossy_compressed_type = int(h[10])
        self.lossy_compressed_factor = int(h[11])
        self._lossy_is_int = int(h[12])
        self.is_streaming = 1 if int(h[13]) > 127 else 0
        self.compression_chunk = 2 ** h[14]
        self.dtype = int(h[15])
        self.original_len = int.from_bytes(h[16:24], "little")
        if self.input_format in (EnumFormat.TORCH.value, EnumFormat.NUMPY.value):
            self.shape_bytes, self._shape_size = unpack_shape(mv[HEADER_LEN:])
        else:
            self._shape_size = 0
        return HEADER_LEN + self._shape_size

    def __metadata__(self):
        info = {
            "ZipNN version": ".".join(str(v) for v in VERSION),
            "Byte reorder": self.byte_reorder, "Bit reorder": self.reorder_signbit, "Method": self.method,
            "Input format": self.input_format, "Data type": self.bytearray_dtype, "Is monotonic": self.is_monotonic,
            "Threads": self.threads, "Compression threshold": self.compression_threshold,
            "Check threshold after percent": self.check_th_after_percent,
            "Delta compressed type": self.delta_compressed_type, "Lossy compressed type": self.lossy_compressed_type,
            "Lossy compressed factor": self.lossy_compressed_factor, "Compression chunk": self.compression_chunk,
            "Is streaming": self.is_streaming, "Streaming chunk": self.streaming_chunk,
            "Input file path": self.input_file, "Compressedfile path": self.compressed_file,
            "Decompressed file path": self.decompressed_file,
        }
        print(info)
        return info

    def __version__(self):
        print("ZipNN version: " + ".".join(str(v) for v in VERSION))

    def metadata(self, file, version=False):
        """Header fields of a compressed file / buffer as a dict (reference zipnn.py:497-553)."""
        if isinstance(file, str):
            with open(file, "rb") as f:
                mv = memoryview(f.read(HEADER_LEN + 1 + 9 * 255))    # header + the largest possible shape extension
        else:
            mv = memoryview(file)
        h = mv[:HEADER_LEN]
        if h[0:2].tobytes() != b"ZN":
            raise ValueError("Header should start with ZN")
        if version:
            print(f"ZipNN version: {h[2]}.{h[3]}.{h[4]}")
            return None
        info = {
            "zipnn version": f"{h[2]}.{h[3]}.{h[4]}", "byte_reorder": int(h[5]), "bit_reorder": int(h[6]),
            "method": EnumMethod(int(h[7])).name if int(h[7]) in EnumMethod._value2member_map_ else "UNKNOWN",
            "input_format": EnumFormat(int(h[8])).name if int(h[8]) in EnumFormat._value2member_map_ else "UNKNOWN",
            "delta_compressed_type": "byte" if h[9] == 1 else "file" if h[9] == 2 else 0,
            "lossy_compressed_type": EnumLossy(int(h[10])).name if int(h[10]) in EnumLossy._value2member_map_ else "NONE",
            "lossy_compressed_factor": int(h[11]), "lossy_is_int": int(h[12]), "is_streaming": int(h[13]) > 127,
            "compression_chunk": f"{2 ** h[14]} Bytes", "dtype": int(h[15]),
            "original_len": f"{int.from_bytes(h[16:24], 'little')} Bytes",
        }
        if int(h[8]) in (EnumFormat.TORCH.value, EnumFormat.NUMPY.value):
            info["shape_bytes"], info["shape_size"] = unpack_shape(mv[HEADER_LEN:])
        print(info)
        return info

    # ------------------------------------------------------------------ compress
    def compress(self, data, compress_cpu_gpu="cpu", delta_second_data=None, lossy_compressed_type: str = None,
                 lossy_compressed_factor: int = None):
        """Compress bytes / a torch tensor / a numpy array into one ZN frame (or, when
        streaming, a bytearray of back-to-back frames).  Reference: zipnn.py:560-643."""
        if self.delta_compressed_type == "byte":
            if len(data) != len(delta_second_data):
                raise ValueError("Length of delta file has to match the length of the original file.")
        elif self.delta_compressed_type == "file":
            try:
                with open(delta_second_data, "rb") as f:
                    delta_second_data = f.read()
            except Exception:
                raise FileNotFoundError("Encountered an error when reading the delta file")
            if len(data) != len(delta_second_data):
                raise ValueError("Length of delta file has to match the length of the original file.")
        elif delta_second_data is not None:
            raise ValueError("ZipNN isn't set for delta compression, but delta_second_data is not null.")
        delta_second_data = _delta_bytes(delta_second_data)      # (bytes view or None; never tested for truth as an array)

        if self.is_streaming and self.input_format == EnumFormat.BYTE.value:
            mv = memoryview(data).cast("B")
            mvd = delta_second_data
            batched = self._compress_stream_batched(mv, mvd)
            if batched is not None:
                return batched
            out = bytearray()
            for off in range(0, mv.nbytes, self.streaming_chunk):
                piece = mv[off:off + self.streaming_chunk]
                if mvd is not None:
                    piece = _xor(piece, mvd[off:off + self.streaming_chunk])
                out += self.compress_torch_numpy_byte(piece, lossy_compressed_type, lossy_compressed_factor)
            return out
        if delta_second_data is not None:
            if self.input_format == EnumFormat.BYTE.value:
                # the XOR with the second buffer happens inside the kernels that read the data (fused, no host pass)
                return self.compress_torch_numpy_byte(data, lossy_compressed_type, lossy_compressed_factor, delta=delta_second_data)
            data = _xor(data, delta_second_data)
        return self.compress_torch_numpy_byte(data, lossy_compressed_type, lossy_compressed_factor)

    def _compress_stream_batched(self, mv, mvd):
        """Streaming BYTE input (reference zipnn.py:612-635): the buffer crosses PCIe once, all `streaming_chunk`
        pieces are compressed by ONE batched call (zn_compress_batch_dev), one copy back; the frames are the ones
        the per-piece loop produces.  None = not applicable (the loop then raises the reference's errors for
        unsupported dtypes, or handles the single-piece case)."""
        dt = dtype_from_user(self.bytearray_dtype)
        is_float = self.bytearray_dtype in ("float64", "float32", "float16", "bfloat16", "float8_e4m3fn", "float8_e5m2")
        if dt is None or not is_float or mv.nbytes <= self.streaming_chunk:
            return None
        h = self._header
        h[5], h[6], h[15] = dt.byte_mode, dt.rotate, dt.code
        chunk = self.compression_chunk if dt.planes != 1 else min(FP8_CHUNK_CAP, self.compression_chunk)
        dev = torch.device("cuda", codec.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        flat = codec.to_device(_capi.lib(), mv, dev)
        base = codec.to_device(_capi.lib(), mvd[:mv.nbytes], dev) if mvd is not None else None
        offs = range(0, mv.nbytes, self.streaming_chunk)
        pieces = [flat[off:off + self.streaming_chunk] for off in offs]
        bases = [base[off:off + self.streaming_chunk] if base is not None else None for off in offs]   # XOR fused on the device
        bodies = codec.compress_device_batch(_capi.lib(), [(p, dt.planes, dt.rotate, dt.byte_mode, chunk, self.compression_threshold, b)
                                                           for p, b in zip(pieces, bases)])
        # frames assembled on the device (header ‖ body, back to back), one transfer back
        sizes = [b.numel() for b in bodies]
        total = sum(sizes) + HEADER_LEN * len(bodies)
        heads = bytearray()
        for p, nb in zip(pieces, sizes):
            h[16:24] = p.numel().to_bytes(8, "little")
            h[24:32] = (HEADER_LEN + nb).to_bytes(8, "little")           # what the core writes at zipnn_core.c:121
            heads += h
        heads_t = codec.to_device(_capi.lib(), heads, dev).view(len(bodies), HEADER_LEN)
        blob = torch.cat([x for i, b in enumerate(bodies) for x in (heads_t[i], b)])
        assert blob.numel() == total
        return codec.to_host(_capi.lib(), blob)

    def torch_frame_plan(self, t):
        """Header and core parameters for compressing torch tensor `t` (no data work): (header bytes incl. the shape
        extension and the length field, planes, bits_mode, bytes_mode, chunk) — what compress_torch_numpy_byte would use."""
        dt = dtype_from_user(t.dtype)
        if dt is None or not torch.is_floating_point(t):
            raise ValueError("Support only torch.dtype float32/bfloat16/float16")
        h = bytearray(self._header)
        h[5], h[6], h[15] = dt.byte_mode, dt.rotate, dt.code
        h[16:24] = (t.numel() * t.element_size()).to_bytes(8, "little")
        chunk = self.compression_chunk if dt.planes != 1 else min(FP8_CHUNK_CAP, self.compression_chunk)
        return bytes(h) + pack_shape(tuple(t.shape)), dt.planes, dt.rotate, dt.byte_mode, chunk

    def compress_torch_numpy_byte(self, data, lossy_compressed_type=None, lossy_compressed_factor=None, delta=None):
        """dtype -> (planes, rotate, byte mode), header, flat byte view, core call.
        Reference: zipnn.py:748-867 and compress_bin :670-746."""
        fmt = self.input_format
        if fmt == EnumFormat.BYTE.value:
            dt = dtype_from_user(self.bytearray_dtype)
            is_float = self.bytearray_dtype in ("float64", "float32", "float16", "bfloat16", "float8_e4m3fn", "float8_e5m2")
            shape = None
        elif fmt == EnumFormat.TORCH.value:
            dt = dtype_from_user(data.dtype)
            is_float = torch.is_floating_point(data)
            shape = tuple(data.shape)
        elif fmt == EnumFormat.NUMPY.value:
            dt = dtype_from_user(data.dtype)
            is_float = np.issubdtype(data.dtype, np.floating)
            shape = tuple(data.shape)
        else:
            raise ValueError("Unsupported input_format")
        if not is_float:
            if fmt == EnumFormat.NUMPY.value and np.dtype(data.dtype) == np.uint32:
                raise ValueError("Not support uint32 with NumPy format")
            raise ValueError("Support only uint32 with NumPy format")
        if dt is None:
            raise ValueError("Support only torch.dtype float32/bfloat16/float16")

        h = self._header
        h[5], h[6], h[15] = dt.byte_mode, dt.rotate, dt.code
        chunk = self.compression_chunk if dt.planes != 1 else min(FP8_CHUNK_CAP, self.compression_chunk)
        lib = _capi.lib()

        if fmt == EnumFormat.TORCH.value and data.is_cuda:
            flat = codec.flat_bytes(data)
            h[16:24] = flat.numel().to_bytes(8, "little")
            hdr = bytes(h) + pack_shape(shape)
            return memoryview(codec.compress_device_to_frame(lib, hdr, flat, dt.planes, dt.rotate, dt.byte_mode, chunk,
                                                             self.compression_threshold))
        if fmt == EnumFormat.TORCH.value:
            ba = memoryview(codec.flat_bytes(data).numpy())
        elif fmt == EnumFormat.NUMPY.value:
            ba = memoryview(np.ascontiguousarray(data).reshape(-1).view(np.uint8))
        else:
            ba = memoryview(data).cast("B")
        h[16:24] = ba.nbytes.to_bytes(8, "little")
        self._ext_header = pack_shape(shape) if shape is not None else self._ext_header
        hdr = bytes(h) + (pack_shape(shape) if shape is not None else b"")
        if self.devices and len(self.devices) > 1 and delta is None:
            frame = lib.compress_multi(hdr, ba, dt.planes, dt.rotate, dt.byte_mode, chunk, self.compression_threshold, self.devices)
        else:
            frame = lib.compress(hdr, ba, dt.planes, dt.rotate, dt.byte_mode, chunk, self.compression_threshold,
                                 device=self.devices[0] if self.devices else codec.current_device(), delta=delta)
        h[24:32] = frame[24:32]   # the core patches the total length into the caller's header (zipnn_core.c:121)
        return memoryview(frame)

    # ------------------------------------------------------------------ decompress
    def decompress(self, data, decompress_cpu_gpu="cpu", delta_second_data=None):
        """Inverse of compress (reference zipnn.py:928-1005).  `decompress_cpu_gpu` other than
        "cpu" (e.g. "gpu", "cuda", "cuda:1") keeps a TORCH-format result on that device."""
        if self.delta_compressed_type == "byte":
            if delta_second_data is None:
                raise ValueError("delta_second_data is None or not set for delta copression")
        elif self.delta_compressed_type == "file":
            try:
                with open(delta_second_data, "rb") as f:
                    delta_second_data = f.read()
            except Exception:
                raise FileNotFoundError("Encountered an error when reading the delta file")
        elif delta_second_data is not None:
            raise ValueError("ZipNN isn't set for delta compression, but delta_second_data is not null.")
        # the second buffer as bytes, whatever it came as (a tensor or an array has no truth value); an EMPTY one counts
        # as "no second buffer", which is what the reference's `if delta_second_data:` makes of it (zipnn.py:968,1000)
        delta_second_data = _delta_bytes(delta_second_data)

        if isinstance(data, torch.Tensor) and not (data.is_cuda and delta_second_data is None and self.input_format != EnumFormat.BYTE.value):
            # a frame handed over as a tensor: only the device-resident fast path (a CUDA frame, no second buffer, TORCH /
            # NUMPY result) works on the tensor itself; every other case (delta, streaming blobs of BYTE frames) takes the
            # host-bytes route — the reference only ever sees bytes here (zipnn.py:928-1005)
            data = data.detach().cpu().contiguous().view(torch.uint8).reshape(-1).numpy()
        if isinstance(data, torch.Tensor):
            mv = None
            was_delta, stream_byte = int(data[9]), int(data[13])
        else:
            mv = memoryview(data).cast("B") if not isinstance(data, memoryview) else data
            was_delta, stream_byte = mv[9], mv[13]
        if was_delta == 0 and self.delta_compressed_type != 0:
            raise ValueError("The data wasn't compressed using delta compression and you're trying to delta-decompress it.")
        if was_delta != 0 and self.delta_compressed_type == 0:
            raise ValueError("The data was compressed using delta compression and you're trying to decompress it normally.")
        target = _resolve_device(decompress_cpu_gpu)

        if self.input_format == EnumFormat.BYTE.value and stream_byte > 127 and mv is not None:
            batched = self._decompress_stream_batched(mv, delta_second_data)
            if batched is not None:
                return batched
            out = bytearray()
            off = od = 0
            mvd = delta_second_data
            while off < mv.nbytes:
                total = int.from_bytes(mv[off + 24:off + 32], "little")
                piece = self.decompress_bin(mv[off:off + total])
                if piece:
                    if mvd is not None:
                        if od + len(piece) > mvd.nbytes:
                            raise ValueError("Length of delta file has to match the length of the decompressed file.")
                        piece = _xor(piece, mvd[od:od + len(piece)])
                        od += len(piece)
                    out += piece
                off += total
            if mvd is not None and od != mvd.nbytes:
                raise ValueError("Length of delta file has to match the length of the decompressed file.")
            return out
        if delta_second_data is not None:
            if self.input_format == EnumFormat.BYTE.value and mv is not None:
                return self.decompress_bin(mv, delta=delta_second_data)     # XOR fused into the kernels that write the output
            plain = self.decompress_bin(mv)
            if len(plain) != delta_second_data.nbytes:
                raise ValueError("Length of delta file has to match the length of the decompressed file.")
            return _xor(plain, delta_second_data)
        return self.decompress_bin(data if mv is None else mv, target)

    def _decompress_stream_batched(self, mv, delta_second_data):
        """A streaming `.znn` blob = back-to-back frames of `streaming_chunk` bytes each (reference zipnn.py:971-995,
        scripts/zipnn_decompress_file.py:47-57).  All frame headers are parsed on the host, the blob crosses PCIe
        once, every frame's chunks are decoded by ONE batched launch, the result comes back once.
        None = not applicable (a single frame): the caller falls back to the per-frame loop."""
        frames, off, first16, first_ext = [], 0, None, 0
        while off < mv.nbytes:
            if off + HEADER_LEN > mv.nbytes:
                return None
            total = int.from_bytes(mv[off + 24:off + 32], "little")
            if total < HEADER_LEN or off + total > mv.nbytes:
                return None
            head16 = bytes(mv[off:off + 16])
            if frames and head16 == first16 and first_ext == 0:
                # same header as the first frame (the usual case: one writer, one configuration): only the length differs
                fp = dict(frames[0][2]); fp["orig_size"] = int.from_bytes(mv[off + 16:off + 24], "little")
            else:
                fp = self.frame_params(mv[off:off + total])
                if not frames:
                    first16, first_ext = head16, fp["body_off"] - HEADER_LEN
            frames.append((off + fp["body_off"], off + total, fp))
            off += total
        if len(frames) < 2:
            return None
        n_out = sum(fp["orig_size"] for (_, _, fp) in frames)
        dev = torch.device("cuda", codec.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        blob = codec.to_device(_capi.lib(), mv, dev)
        base = None
        if delta_second_data is not None:
            mvd = memoryview(delta_second_data).cast("B")
            if mvd.nbytes != n_out:
                raise ValueError("Length of delta file has to match the length of the decompressed file.")
            base = codec.to_device(_capi.lib(), mvd, dev) if n_out else None
        flat = torch.empty(n_out, dtype=torch.uint8, device=dev)
        items, o = [], 0
        for (b0, b1, fp) in frames:                  # frame i's slice of the second buffer: XOR fused on the device
            n = fp["orig_size"]
            items.append((blob[b0:b1], fp["num_buf"], fp["bits_mode"], fp["bytes_mode"], fp["chunk"], n,
                          base[o:o + n] if base is not None else None))
            o += n
        codec.decompress_device_batch(_capi.lib(), items, into=flat)
        return codec.to_host(_capi.lib(), flat)

    def frame_params(self, frame):
        """Parse one frame's header -> what the C ABI needs to decode its body (no data work):
        dict(body_off, num_buf, bits_mode, bytes_mode, chunk, orig_size, torch_dtype, shape)."""
        # header + shape extension: 1 byte ndim, then per dim a width byte and ≤ 8 bytes (header.pack_shape) — read what
        # this frame's ndim needs, not a fixed window (a 12-dimensional shape does not fit 80 bytes)
        body_off = self._retrieve_header(_frame_head(frame))
        dt = dtype_from_code(self.dtype)
        chunk = self.compression_chunk if dt.planes != 1 else min(FP8_CHUNK_CAP, self.compression_chunk)
        return dict(body_off=body_off, num_buf=dt.planes, bits_mode=self._bit_reorder, bytes_mode=self._byte_reorder,
                    chunk=chunk, orig_size=self.original_len, torch_dtype=dt.torch, shape=getattr(self, "shape_bytes", None))

    def decompress_bin(self, frame, target=None, delta=None):
        """One frame -> bytes / tensor / array (reference zipnn.py:1072-1198).  delta (BYTE format): second buffer
        of the original length, XORed into the output on the device."""
        on_device = isinstance(frame, torch.Tensor) and frame.is_cuda
        body_off = self._retrieve_header(_frame_head(frame))
        dt = dtype_from_code(self.dtype)
        if self.input_format == EnumFormat.NUMPY.value and dt.numpy is None:
            raise ValueError(f"Unsupported Dtype {self.dtype}")
        chunk = self.compression_chunk if dt.planes != 1 else min(FP8_CHUNK_CAP, self.compression_chunk)
        lib = _capi.lib()
        fmt = self.input_format

        if fmt == EnumFormat.TORCH.value and (on_device or target is not None):
            # device-resident result: only compressed bytes cross PCIe
            dev = target if target is not None else frame.device
            if isinstance(frame, torch.Tensor):
                body = frame.reshape(-1).view(torch.uint8)[body_off:]
                if not body.is_cuda and torch.device(dev).type == "cuda" and body.numel() >= (2 << 20):
                    body = codec.to_device(lib, body.contiguous().numpy(), dev)     # (pinned multi-threaded transfer)
                else:
                    body = body.to(dev, non_blocking=True)
            else:
                body = codec.to_device(lib, memoryview(frame)[body_off:], dev)
            flat = codec.decompress_device(lib, body, dt.planes, self._bit_reorder, self._byte_reorder, chunk,
                                           self.original_len)
            return flat.view(dt.torch).reshape(self.shape_bytes)

        if isinstance(frame, torch.Tensor):
            frame = memoryview(frame.cpu().contiguous().view(torch.uint8).reshape(-1).numpy())
        if delta is not None and memoryview(delta).nbytes != self.original_len:
            raise ValueError("Length of delta file has to match the length of the decompressed file.")
        if self.devices and len(self.devices) > 1 and delta is None:
            raw = lib.decompress_multi(memoryview(frame)[body_off:], dt.planes, self._bit_reorder, self._byte_reorder, chunk,
                                       self.original_len, self.devices)
        else:
            raw = lib.decompress(memoryview(frame)[body_off:], dt.planes, self._bit_reorder, self._byte_reorder, chunk,
                                 self.original_len, device=self.devices[0] if self.devices else codec.current_device(),
                                 delta=delta if self.original_len else None)
        if fmt == EnumFormat.BYTE.value:
            return memoryview(raw)
        if fmt == EnumFormat.TORCH.value:
            if self.original_len == 0:
                return torch.empty(self.shape_bytes, dtype=dt.torch)
            return torch.frombuffer(raw, dtype=torch.uint8).view(dt.torch).reshape(self.shape_bytes)
        if fmt == EnumFormat.NUMPY.value:
            return np.frombuffer(raw, dtype=dt.numpy).reshape(self.shape_bytes)
        raise ValueError(f"Unsupported input_format {self.input_format}")

    def decompress_read_file(self, data=None):
        import os
        filename = data if data is not None else self.compressed_file
        if not os.path.exists(filename):
            raise FileNotFoundError(f"The file at {filename} was not found.")
        with open(filename, "rb") as f:
            return self.decompress_bin(f.read())

    def write_bin(self, ba_decom):
        with open(self.decompressed_file, "wb") as f:
            f.write(ba_decom)
        return 0


_HEAD_WINDOW = HEADER_LEN + 1 + 9 * 8       # header + the shape extension of a tensor of up to 8 dimensions


def fast_frame_params(mv):
    """What ZipNN.frame_params returns, straight from the head of one frame (host bytes: header + shape extension) and without
    a ZipNN instance — the batched loaders parse hundreds of frames per file (same fields as ZipNN._retrieve_header,
    reference zipnn.py:396-438).  -> (body_off, num_buf, bits_mode, bytes_mode, chunk, orig_size, torch_dtype, shape).
    The bytes come from a file: anything that does not add up (a head shorter than the header, a chunk exponent no frame can
    carry, a shape whose bytes are not orig_size) raises ValueError — the callers fall back to, or report through, the
    per-tensor path."""
    if len(mv) < HEADER_LEN:
        raise ValueError("frame shorter than its header")
    if mv[0] != 0x5A or mv[1] != 0x4E:
        raise ValueError("Header should start with ZN")
    dt = dtype_from_code(mv[15])
    if mv[14] > 40:
        raise ValueError("compression chunk exponent out of range")
    chunk = 1 << mv[14]
    if dt.planes == 1 and chunk > FP8_CHUNK_CAP:
        chunk = FP8_CHUNK_CAP
    orig_size = int.from_bytes(mv[16:24], "little")
    shape, ext = None, 0
    if mv[8] in (EnumFormat.TORCH.value, EnumFormat.NUMPY.value):
        import struct
        try:
            shape, ext = unpack_shape(mv[HEADER_LEN:])
        except (IndexError, struct.error):
            raise ValueError("frame shorter than its shape extension")
        numel = 1
        for d in shape:
            numel *= int(d)
        if numel * dt.planes != orig_size:         # (a plane per byte of an element on every dtype this path codes)
            raise ValueError("frame shape does not match its original length")
    return (HEADER_LEN + ext, dt.planes, mv[6], mv[5], chunk, orig_size, dt.torch, shape)


def _frame_head(frame):
    """Header (+ shape extension) of one frame as host bytes.  A frame that lives in a tensor (possibly in HBM) is read
    with ONE small copy: a fixed window that holds the shape extension of up to 8 dimensions; the extension exists only in
    TORCH / NUMPY frames (header byte 8), and only a frame with more dimensions than that costs a second read."""
    if not isinstance(frame, torch.Tensor):
        mv = memoryview(frame)
        return mv[:HEADER_LEN + 1 + 9 * 255]
    flat = frame.reshape(-1)
    head = bytes(flat[:_HEAD_WINDOW].cpu().numpy())
    if len(head) > HEADER_LEN and head[8] in (EnumFormat.TORCH.value, EnumFormat.NUMPY.value):
        need = HEADER_LEN + 1 + 9 * head[HEADER_LEN]
        if need > len(head) and flat.numel() > len(head):
            head = bytes(flat[:need].cpu().numpy())
    return head


def _delta_bytes(delta):
    """The delta base as a flat byte view, or None for "no second buffer" (None or empty)."""
    if delta is None:
        return None
    if isinstance(delta, torch.Tensor):
        delta = delta.detach().cpu().contiguous().view(torch.uint8).reshape(-1).numpy()
    mv = memoryview(delta)
    if mv.nbytes == 0:
        return None
    return mv.cast("B") if mv.c_contiguous else memoryview(mv.tobytes())      # (cast() needs C order: a Fortran-ordered array is "contiguous" too)


def _xor(a, b):
    return np.bitwise_xor(np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)).tobytes()


def _resolve_device(spec):
    """"cpu" -> None; "gpu"/"cuda" -> current device; "cuda:N" / torch.device -> that device."""
    if spec is None or spec == "cpu":
        return None
    if isinstance(spec, torch.device):
        return None if spec.type == "cpu" else spec
    if spec in ("gpu", "cuda"):
        return torch.device("cuda", codec.current_device())
    return torch.device(spec)


# ---------------------------------------------------------------------------------------
# safetensors plugin (reference zipnn.py:1584-1643, util_safetensors.py, util_patch.py)
# ---------------------------------------------------------------------------------------
METADATA_KEY = "znn_compressed_vectors"     # reference util_safetensors.py:9
COMPRESSION_METHOD = "HUFFMAN"
COMPRESSED_DTYPE = torch.uint8


def build_compressed_tensor_info(uncompressed_tensor):
    """Per-tensor metadata stored under METADATA_KEY (reference util_safetensors.py:28-38)."""
    return {"dtype": str(uncompressed_tensor.dtype).replace("torch.", "", 1),
            "shape": str(list(uncompressed_tensor.shape))}


def set_compressed_tensors_metadata(compressed_tensor_infos, metadata):
    if metadata:
        metadata[METADATA_KEY] = json.dumps(compressed_tensor_infos)


def get_compressed_tensors_metadata(metadata):
    if metadata:
        return json.loads(metadata.get(METADATA_KEY) or "{}")
    return {}


def decompress_safetensors_tensor(tensor, device="cpu"):
    """One stored uint8 frame tensor -> the original tensor (reference zipnn.py:1584-1589).
    With a non-CPU `device` the frame is shipped compressed and decoded in HBM."""
    znn = ZipNN(input_format="torch", bytearray_dtype=COMPRESSED_DTYPE, method=COMPRESSION_METHOD)
    return znn.decompress(tensor.contiguous(), decompress_cpu_gpu=device if device is not None else "cpu")


_ST_DTYPE_NAME = {"float32": "F32", "float16": "F16", "bfloat16": "BF16", "float8_e4m3fn": "F8_E4M3", "float8_e5m2": "F8_E5M2"}


def index_rows(idx, shape, n):
    """The index arithmetic of a slice object over a tensor of `shape` stored as `n` contiguous bytes (CompressedSlice, resident.ResidentSlice): which rows
    [a, b) of the first dimension an index needs, as bytes [byte_lo, byte_hi) of the tensor, and the index `sel` to apply to those rows once they are decoded.
    -> (a, b, sel, byte_lo, byte_hi, scalar)."""
    if not isinstance(idx, tuple):
        idx = (idx,)
    rows = shape[0] if shape else 0
    first, rest = (idx[0], idx[1:]) if idx else (slice(None), ())
    a, b, lead = 0, rows, None              # decode rows [a, b); `lead` then indexes the first dimension of what was decoded
    if not shape or rows == 0 or n == 0:
        lead, rest = None, idx              # (a scalar or an empty tensor: nothing to range over)
    elif isinstance(first, bool) or first is None or first is Ellipsis or not isinstance(first, (int, slice)):
        rest = idx                          # (masks, lists, a leading Ellipsis / None: the whole tensor, the index as given)
    elif isinstance(first, int):
        r = first + rows if first < 0 else first
        if not 0 <= r < rows:
            raise IndexError(f"index {first} is out of bounds for dimension 0 with size {rows}")
        a, b, lead = r, r + 1, 0
    else:
        lo, hi, step = first.indices(rows)
        if step == 1:
            a, b, lead = lo, max(hi, lo), slice(None)
        elif step > 1 and hi > lo:
            a, b, lead = lo, hi, slice(None, None, step)
        else:
            rest = idx                      # (negative steps: the whole tensor, torch reports what it does not index)
    row_bytes = n // rows if rows else 0
    byte_lo, byte_hi = a * row_bytes, b * row_bytes
    scalar = not shape and n > 0             # a 0-dim tensor left compressed (no writer of ours or the reference's does that — the frame is larger than the
    if scalar:                               #  value — but a third party's file may): its one element is all the bytes, decoded and viewed as the scalar
        byte_lo, byte_hi = 0, n
    sel = (() if lead is None else (lead,)) + tuple(rest)
    return a, b, sel, byte_lo, byte_hi, scalar


class CompressedSlice:
    """`SafeOpen.get_slice(name)` of a compressed tensor: the protocol of safetensors' own slice object (`get_shape()`,
    `get_dtype()`, indexing), served by chunk-range decode.  Rows a .. b-1 of a tensor are the contiguous bytes
    [a, b) x row_bytes of the frame's original buffer; the frame's chunks are independent (own size-table entries, own huff0
    blocks: reference csrc/zipnn_core.c:929-1028 walks them one by one), so only the chunks that cover those bytes are uploaded
    and decoded (zn_decompress_range_dev: re-based size tables, that range's payload slices through the pinned pipe) and the
    result is a view of that range.  Indices on later dimensions are applied to the decoded rows; an index on the first
    dimension that is not an int or a step-1 slice decodes the whole tensor.  The reference answers NotImplementedError here
    (zipnn/zipnn.py:1615-1617); tensor-parallel loaders call exactly this."""

    def __init__(self, opener, name):
        self._o, self._name = opener, name
        info = opener.compressed_tensors_metadata[name]
        self._dtype_name = str(info.get("dtype", ""))
        self._shape = [int(d) for d in json.loads(info.get("shape", "[]"))]
        self._frame = self._keep = self._fp = None
        self.last_chunk_range = None           # (chunk_lo, chunk_hi) of the last index operation — what it decoded

    def get_shape(self):
        return list(self._shape)

    def get_dtype(self):
        return _ST_DTYPE_NAME.get(self._dtype_name, self._dtype_name.upper())

    def _load(self):
        if self._frame is None:
            t = self._o._host_reader().get_tensor(self._name)          # the frame: a 1-D uint8 tensor in host memory
            self._keep = t.contiguous().reshape(-1)
            self._frame = memoryview(self._keep.numpy())
            self._fp = fast_frame_params(self._frame[:HEADER_LEN + 1 + 9 * 255])

    def _device(self):
        d = self._o._device
        if isinstance(d, int):
            d = f"cuda:{d}"
        want = torch.device(d)
        if want.type == "cuda" or not torch.cuda.is_available():
            return want, want                   # (without a GPU the library is the emulated one and "device memory" is host memory: tests)
        return torch.device("cuda", codec.current_device()), want      # a CPU target: decoded in HBM, the rows come back

    def __getitem__(self, idx):
        self._load()
        body_off, P, bits, byts, chunk, n, tdt, shape = self._fp
        shape = tuple(int(d) for d in (shape if shape is not None else self._shape))
        work, want = self._device()
        a, b, sel, byte_lo, byte_hi, scalar = index_rows(idx, shape, n)
        if byte_hi <= byte_lo:
            self.last_chunk_range = (0, 0)
            t = torch.empty((max(b - a, 0),) + shape[1:], dtype=tdt, device=want) if shape else torch.empty((), dtype=tdt, device=want)
        else:
            c_lo, c_hi = byte_lo // chunk, (byte_hi + chunk - 1) // chunk
            self.last_chunk_range = (c_lo, c_hi)
            base = c_lo * chunk
            buf = torch.empty(min(c_hi * chunk, n) - base, dtype=torch.uint8, device=work)
            dev_index = work.index if (work.type == "cuda" and work.index is not None) else (codec.current_device() if work.type == "cuda" else 0)
            if work.type == "cuda":
                torch.cuda.current_stream(work).synchronize()      # (`buf` may be a block that kernels queued earlier still use)
            _capi.lib().decompress_range_dev(self._frame[body_off:], P, bits, byts, chunk, n, c_lo, c_hi, dev_index, buf.data_ptr())
            t = buf[byte_lo - base: byte_hi - base].view(tdt).reshape(() if scalar else (b - a,) + shape[1:])
            if want != work:
                t = t.to(want)
        return t[sel] if sel else t


class SafeOpen:
    """`safetensors.safe_open` wrapper that decompresses tensors named in the file's
    `znn_compressed_vectors` metadata on access (reference zipnn.py:1592-1626).  Unlike the
    reference it honours `device=` for compressed tensors and tolerates the extra keyword
    arguments newer safetensors releases pass (`backend=`)."""

    def __init__(self, filename, framework="pt", device="cpu", **kwargs):
        self._host = None
        # `device` as safetensors takes it — "cpu", "cuda:N", an ordinal — plus what torch users write: "cuda", torch.device
        if isinstance(device, torch.device):
            device = "cpu" if device.type == "cpu" else f"{device.type}:{device.index if device.index is not None else codec.current_device()}"
        elif device == "cuda":
            device = f"cuda:{codec.current_device()}"
        self._device = device
        # compressed tensors are read on the host and decoded on `device`
        self._f = _ORIGINAL_SAFE_OPEN(filename, framework=framework, device=device, **kwargs)
        self._host = None
        self._filename, self._framework, self._kwargs = filename, framework, kwargs
        if "znn_delta" in (self._f.metadata() or {}):
            # a delta file: its tensors are coded over a base this interface has no way to be given — refused at open, never decoded wrongly
            raise ValueError(f"{filename}: a delta file (znn_delta): its tensors are coded over a base — load it with zipnn_amd.safetensors_io.load_file(base=)")
        self.compressed_tensors_metadata = get_compressed_tensors_metadata(self._f.metadata())
        self._ahead = None                 # read-ahead cache {name: decoded tensor}; False = not applicable for this file

    def _read_ahead(self):
        """Device targets: the first get_tensor of a compressed name ships the file's data section to the device ONCE and decodes
        every compressed tensor of the file with ONE batched launch (safetensors_io.decode_file_on_device); get_tensor then
        serves from the cache, dropping each entry as it is handed out.  A consumer that walks the file through the reference's
        API (zipnn.py:1592-1626: one decompress per get_tensor) gets the batched path's speed.  Files larger than
        ZIPNN_AMD_READAHEAD_BYTES (default 32 GiB, and never more than half of the device's free memory; 0 switches it off) and
        containers the batched loader does not parse keep the per-tensor path.  Every tensor of the cache owns its allocation
        (no shared arena: a consumer that keeps one tensor of a shard does not pin the decoded bytes of all the others), and
        ANY failure of the read-ahead — a corrupt frame somewhere in the file, an allocation that does not fit — only switches
        it off: the per-tensor path then reports the error for the tensor that actually has it, as the reference does."""
        import os
        from . import safetensors_io
        self._ahead = False
        try:
            limit = int(os.environ.get("ZIPNN_AMD_READAHEAD_BYTES", str(32 << 30)))
            dev = self._device if not isinstance(self._device, int) else f"cuda:{self._device}"
            if limit > 0 and torch.device(dev).type == "cuda" and torch.cuda.is_available():
                limit = min(limit, torch.cuda.mem_get_info(torch.device(dev))[0] // 2)
            if limit <= 0 or os.path.getsize(self._filename) > limit:
                return
            got = safetensors_io.decode_file_on_device(self._filename, dev, compressed_only=True, use_arena=False)
            if got is not None:
                self._ahead = got
        except Exception as e:                 # noqa: BLE001 — (anything: the per-tensor path reports it properly, for the tensor it belongs to)
            self._ahead = False
            if isinstance(e, (MemoryError, getattr(torch.cuda, "OutOfMemoryError", MemoryError))) and torch.cuda.is_available():
                torch.cuda.empty_cache()

    def _host_reader(self):
        if str(self._device) == "cpu":
            return self._f
        if self._host is None:
            self._host = _ORIGINAL_SAFE_OPEN(self._filename, framework=self._framework, device="cpu", **self._kwargs)
            self._host.__enter__()
        return self._host

    def get_tensor(self, name):
        if name not in self.compressed_tensors_metadata:
            return self._f.get_tensor(name)
        dev = "cpu" if str(self._device) == "cpu" else (self._device if not isinstance(self._device, int) else f"cuda:{self._device}")
        if dev != "cpu":
            if self._ahead is None:
                self._read_ahead()
            if self._ahead:
                t = self._ahead.pop(name, None)
                if t is not None:
                    return t
        return decompress_safetensors_tensor(self._host_reader().get_tensor(name), device=dev)

    def get_slice(self, name):
        """A lazily indexed view of one tensor.  The reference has none for compressed tensors (it returns — does not raise —
        NotImplementedError, zipnn.py:1615-1617), which leaves a tensor-parallel loader, whose API this is, with nothing.  Chunks are
        independent, so here a compressed tensor is sliced by CHUNK RANGE: `f.get_slice(name)[a:b]` decodes only the chunks that
        hold rows a .. b-1 (CompressedSlice, zn_decompress_range_dev).  ZIPNN_AMD_REFERENCE_GET_SLICE=1 restores the reference's answer."""
        if name not in self.compressed_tensors_metadata:
            return self._f.get_slice(name)
        import os
        if os.environ.get("ZIPNN_AMD_REFERENCE_GET_SLICE", "0") == "1":
            return NotImplementedError   # sic: the reference returns (does not raise) it, zipnn.py:1617
        return CompressedSlice(self, name)

    def __enter__(self):
        self._f.__enter__()
        return self

    def _close_host(self, *exc):
        host, self._host = getattr(self, "_host", None), None
        if host is not None:
            try:
                host.__exit__(*(exc or (None, None, None)))
            except Exception:
                pass

    def __exit__(self, exc_type, exc_value, traceback):
        self._ahead = False                    # (what was not asked for goes back to the allocator)
        self._close_host(exc_type, exc_value, traceback)
        return self._f.__exit__(exc_type, exc_value, traceback)

    def __del__(self):          # (used without `with`: the second, host-side handle must not outlive the object)
        self._close_host()

    def __getattr__(self, name):
        if name.startswith("_"):          # (never delegate private names: `_f` itself is looked up here when __init__ failed early)
            raise AttributeError(name)
        return getattr(self._f, name)


def _capture_original_safe_open():
    import safetensors
    import safetensors.torch
    fn = getattr(safetensors.torch, "safe_open", None)
    if fn is None or isinstance(fn, type) and issubclass(fn, SafeOpen):
        fn = safetensors.safe_open
    return fn


_ORIGINAL_SAFE_OPEN = _capture_original_safe_open()
_patches_applied = {}


def multi_process_patcher(patch_func):
    """Apply patch_func here and in every process spawned from now on
    (reference util_patch.py:11-47)."""
    if patch_func in _patches_applied:
        return
    _patches_applied[patch_func] = None
    patch_func()
    from multiprocessing.process import BaseProcess
    start = BaseProcess.start

    def patched_start(self):
        self._target = _TargetWrapper(self._target, patch_func)
        return start(self)

    BaseProcess.start = patched_start


class _TargetWrapper:
    def __init__(self, target, patch_func):
        self.target, self.patch_func = target, patch_func

    def __call__(self, *args, **kwargs):
        multi_process_patcher(self.patch_func)
        return self.target(*args, **kwargs) if self.target is not None else None


def _zipnn_safetensors():
    import safetensors
    import safetensors.torch
    safetensors.torch.safe_open = SafeOpen      # what the reference patches (zipnn.py:1635)
    safetensors.safe_open = SafeOpen            # what transformers ≥ 5 imports


def zipnn_safetensors():
    """Plugin for the safetensors library to use ZipNN compression (reference zipnn.py:1638-1643)."""
    multi_process_patcher(_zipnn_safetensors)


def zipnn_hf(replace_local_file: bool = False):
    """Out of scope here (whole-file .znn path tied to private symbols of
    old transformers releases).  Use zipnn_safetensors()."""
    raise NotImplementedError("zipnn_hf is not part of the MI355X hot-path build; use zipnn_safetensors()")
