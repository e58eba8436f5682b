"""CPU test (-m "not gpu"; skipped where /root/reference does not exist, i.e. on the GPU box): the delta checkpoint file against the STOCK
reference package, in a child process over its own compiled extension (oracle/_ref).  Every "delta" frame cut out of the file decodes, given the base tensor's
bytes, to the fine-tune's bytes with ZipNN(..., delta_compressed_type="byte").decompress(frame, delta_second_data=...); the reference's SafeOpen reads a plain
store's file (ResidentCheckpoint.save_file) whole, reads the tensors of a delta file that are not coded over the base, and RAISES on those that are — it never
returns wrong tensors."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import delta_file_util as D
import resident_delta_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_CORE = os.path.join(ROOT, "oracle", "_ref", "zipnn_core.so")
RUNNER = os.path.join(ROOT, "tests", "run_reference_delta_file.py")


def _sha(t):
    return hashlib.sha256(t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "zipnn")), reason="/root/reference is not on this machine")
def test_the_reference_decodes_delta_frames_and_refuses_them_unasked(use_simt, tmp_path):
    from safetensors.torch import save_file
    from zipnn_amd import ResidentCheckpoint
    if not os.path.exists(REF_CORE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True, capture_output=True)
    if not os.path.exists(REF_CORE):
        pytest.skip("oracle/_ref could not be built here")
    dev = torch.device("cpu")
    base_sd, ft_sd = R.state_dicts()
    base_path = str(tmp_path / "base.safetensors")
    save_file(base_sd, base_path, {"format": "pt"})
    base = ResidentCheckpoint.from_state_dict(base_sd, dev)
    delta_path = ResidentCheckpoint.from_state_dict(ft_sd, dev, base=base).save_file(str(tmp_path / "ft.delta.znn.safetensors"))
    plain_path = ResidentCheckpoint.from_state_dict(ft_sd, dev).save_file(str(tmp_path / "ft.znn.safetensors"))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "oracle", "_ref"), REF])
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    r = subprocess.run([sys.executable, RUNNER, delta_path, base_path, plain_path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    want = {k: [str(v.dtype), list(v.shape), _sha(v)] for k, v in ft_sd.items()}
    # every delta frame, decoded by the reference over the base tensor's bytes
    assert sorted(got["delta"]) == sorted(D.DELTA)
    assert got["delta"] == {k: want[k][2] for k in D.DELTA}
    # a plain store's file through the reference's SafeOpen
    assert got["plain"] == want
    # the delta file through it: what is not coded over the base is read, what is raises
    for k in ft_sd:
        if k in D.DELTA:
            assert got["opened"][k][0] == "raised" and "delta compression" in got["opened"][k][1], (k, got["opened"][k])
        elif k == "identical":
            assert got["opened"][k][0] == "raised", (k, got["opened"][k])          # (a zero-length entry is no frame: the reference fails on its header)
        else:
            assert got["opened"][k] == want[k], k
