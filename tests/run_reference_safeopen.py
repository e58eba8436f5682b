"""Reads `.znn.safetensors` files with the STOCK reference package's SafeOpen (`/root/reference/zipnn` over its own compiled extension, oracle/_ref — both on
PYTHONPATH) and prints one JSON object: per file, per tensor, dtype, shape and the sha256 of its bytes.  Called by tests/test_ref_digest_files.py in a
subprocess (not a test module itself)."""
import hashlib
import json
import sys

import torch


def main():
    from zipnn.zipnn import SafeOpen      # the reference package
    out = {}
    for path in sys.argv[1:]:
        with SafeOpen(path, "pt", "cpu") as f:
            res = {}
            for name in f.keys():
                t = f.get_tensor(name)
                t = t if isinstance(t, torch.Tensor) else torch.as_tensor(t)
                res[name] = [str(t.dtype), list(t.shape), hashlib.sha256(t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()]
            out[path] = res
    print("RESULT " + json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
