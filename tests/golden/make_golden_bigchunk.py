"""Generate tests/golden/golden_bigchunk_v1.npz from the REFERENCE itself: frames at compression_chunk 512 KiB, 1 MiB and 2 MiB.

Build container only (imports /root/reference/zipnn on top of oracle/_ref/zipnn_core.so, exactly as make_golden.py does; see its header).  No test in
tests/ and no older fixture carries a chunk above 256 KiB in a multi-plane frame; `compression_chunk` is a public argument of the reference's ZipNN(...)
(zipnn/zipnn.py) and travels in header byte 14.  Recorded per case: the frame (or streaming blob) `ZipNN(**ctor).compress(x)` returns, its sha256, and the
seeded RECIPE of the input with the input's sha256 — the inputs themselves are not stored: tests/bigchunk_util.golden_input rebuilds them (and the delta
base) from the recipe.  Data only: frames, seeds and parameter records.

    python tests/golden/make_golden_bigchunk.py          # rewrites golden_bigchunk_v1.npz, byte for byte

Inputs are compressible (1-bit-code `skew` bytes, constants, N(0, 0.02) float32 at 512 KiB, a sparse delta) so that the file stays small: from 1 MiB up every
plane of a full chunk is longer than huff0's 128 KiB block and is stored raw.
"""
import contextlib
import hashlib
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))   # zipnn_core (reference C ext)
sys.dont_write_bytecode = True                               # (nothing is written under /root/reference, not even __pycache__)
sys.path.insert(1, "/root/reference")                        # zipnn (reference Python)
sys.path.insert(2, os.path.join(ROOT, "tests"))              # bigchunk_util.golden_input: the recipes' one implementation
sys.path.insert(3, ROOT)

KB = 1024


def main():
    from zipnn import ZipNN  # the reference package
    import bigchunk_util as B

    cases = [
        # one full 512 KiB chunk of four 128 KiB planes — the largest huff0 blocks there are — and a 308-byte tail
        ("byte_fp32_normal_512k", dict(gen="normal_fp32", n=512 * KB + 308, seed=51), dict(bytearray_dtype="float32", compression_chunk=1 << 19), "byte", None),
        ("byte_fp32_skew_512k", dict(gen="gen2", kind="skew", n=512 * KB + 308, seed=52), dict(bytearray_dtype="float32", compression_chunk=1 << 19), "byte", None),
        # two full 1 MiB chunks (planes of 512 KiB: raw whatever they hold) and a tail whose planes are coded
        ("torch_bf16_const_1m", dict(gen="gen2", kind="const", n=2 * 1024 * KB + 300 * KB + 308, seed=53), dict(input_format="torch", compression_chunk=1 << 20), "torch", ("bfloat16", [-1, 10])),
        # one partial 2 MiB chunk whose four planes are exactly 131072 bytes
        ("torch_fp32_skew_2m_planes_at_the_block_limit", dict(gen="gen2", kind="skew", n=4 * 128 * KB, seed=54), dict(input_format="torch", compression_chunk=1 << 21), "torch", ("float32", [256, -1])),
        # streaming pieces of 256 KiB under a 1 MiB compression chunk: every frame is one partial chunk of two 128 KiB planes
        ("byte_bf16_skew_streaming_256k_under_1m", dict(gen="gen2", kind="skew", n=2 * 256 * KB + 10000, seed=55),
         dict(bytearray_dtype="bfloat16", is_streaming=True, streaming_chunk=1 << 18, compression_chunk=1 << 20), "byte", None),
        # a byte delta over a base with 3 % of the bytes perturbed, one full 1 MiB chunk and a tail
        ("delta_byte_bf16_1m", dict(gen="gen2", kind="bf16", n=1024 * KB + 200 * KB + 2, seed=56, base_seed=57),
         dict(bytearray_dtype="bfloat16", delta_compressed_type="byte", compression_chunk=1 << 20), "byte", None),
    ]
    out, meta = {}, []
    for name, recipe, ctor, kind, tspec in cases:
        raw, base = B.golden_input(recipe)
        extra = (lambda: dict(delta_second_data=bytearray(base))) if base is not None else dict
        if kind == "torch":
            dtype, shape = tspec
            x = torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(getattr(torch, dtype)).reshape(shape)
            src, shape = x.clone(), list(x.shape)          # the reference rotates its input in place
        else:
            dtype, shape, src = ctor.get("bytearray_dtype"), None, bytearray(raw)
        with contextlib.redirect_stdout(io.StringIO()):
            frame = bytes(ZipNN(**ctor).compress(src, **extra()))
            back = ZipNN(**ctor).decompress(frame, **extra())
        back_raw = back.contiguous().view(torch.uint8).numpy().tobytes() if kind == "torch" else bytes(back)
        assert back_raw == raw, f"reference round trip failed for {name}"
        e = ctor["compression_chunk"].bit_length() - 1
        assert frame[14] == e
        out[name + ".frame"] = np.frombuffer(frame, dtype=np.uint8)
        meta.append(dict(name=name, kind=kind, ctor=ctor, recipe=recipe, dtype=dtype, shape=shape, chunk_exponent=e, in_len=len(raw), frame_len=len(frame),
                         in_sha256=hashlib.sha256(raw).hexdigest(), frame_sha256=hashlib.sha256(frame).hexdigest()))
        print(f"{name:48s} in={len(raw):8d} frame={len(frame):8d} ratio={len(frame) / len(raw):.4f}")
    out["meta.json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "golden_bigchunk_v1.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:          # (np.savez_compressed stamps every entry with the time of day: this file is the same on every run)
        for key, arr in out.items():
            zi = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arr, allow_pickle=False)
            z.writestr(zi, buf.getvalue())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
