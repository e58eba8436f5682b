"""Reads a delta checkpoint file with the STOCK reference package (`/root/reference/zipnn` over its own compiled extension, oracle/_ref — both on
PYTHONPATH) and prints one JSON object.  argv: the delta file, the base's plain .safetensors file, a plain store's .znn.safetensors file.
  "delta":  per "delta" tensor, the sha256 of ZipNN(bytearray_dtype=<dtype>, delta_compressed_type="byte").decompress(frame, delta_second_data=<base bytes>),
            the frame cut out of the file's data section
  "plain":  per tensor of the plain store's file, dtype, shape and sha256 as the reference's SafeOpen returns it
  "opened": per tensor of the DELTA file through the reference's SafeOpen: [dtype, shape, sha256], or ["raised", the exception's text]
Called by tests/test_ref_delta_file.py in a subprocess (not a test module itself)."""
import contextlib
import hashlib
import io
import json
import sys

import torch


def _sha(t):
    return hashlib.sha256(t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    from safetensors.torch import load_file
    from zipnn import ZipNN                 # the reference package
    from zipnn.zipnn import SafeOpen
    delta_path, base_path, plain_path = sys.argv[1:4]
    raw = open(delta_path, "rb").read()
    n = int.from_bytes(raw[:8], "little")
    hdr = json.loads(raw[8:8 + n])
    data = raw[8 + n:]
    kinds = json.loads(hdr["__metadata__"]["znn_delta"])["tensors"]
    infos = json.loads(hdr["__metadata__"]["znn_compressed_vectors"])
    base = load_file(base_path)
    out = {"delta": {}, "plain": {}, "opened": {}}
    for name, kind in kinds.items():
        if kind != "delta":
            continue
        lo, hi = hdr[name]["data_offsets"]
        second = base[name].contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        with contextlib.redirect_stdout(io.StringIO()):
            back = ZipNN(bytearray_dtype=infos[name]["dtype"], delta_compressed_type="byte").decompress(bytearray(data[lo:hi]), delta_second_data=bytearray(second))
        out["delta"][name] = hashlib.sha256(bytes(back)).hexdigest()
    with SafeOpen(plain_path, "pt", "cpu") as f:
        for name in f.keys():
            t = f.get_tensor(name)
            out["plain"][name] = [str(t.dtype), list(t.shape), _sha(t)]
    with SafeOpen(delta_path, "pt", "cpu") as f:
        for name in f.keys():
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    t = f.get_tensor(name)
                out["opened"][name] = [str(t.dtype), list(t.shape), _sha(t)]
            except Exception as e:           # noqa: BLE001 — (whatever the reference raises: the test looks at it)
                out["opened"][name] = ["raised", f"{type(e).__name__}: {e}"]
    print("RESULT " + json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
