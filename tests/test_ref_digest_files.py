"""CPU test (-m "not gpu"; skipped where /root/reference does not exist, i.e. on the GPU box): a `.znn.safetensors` file written with digests
(compress_safetensors_file(..., digests=True)) is still a file the STOCK reference package reads — its own SafeOpen, over its own compiled extension
(oracle/_ref), returns the same tensors as from the file written without: the extra metadata key is ignored by readers that do not know it."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import digest_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_CORE = os.path.join(ROOT, "oracle", "_ref", "zipnn_core.so")
RUNNER = os.path.join(ROOT, "tests", "run_reference_safeopen.py")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "zipnn")), reason="/root/reference is not on this machine")
def test_the_reference_s_safe_open_reads_a_file_with_digests(use_simt, tmp_path):
    from safetensors.torch import save_file
    from zipnn_amd import safetensors_io
    if not os.path.exists(REF_CORE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True, capture_output=True)
    if not os.path.exists(REF_CORE):
        pytest.skip("oracle/_ref could not be built here")
    sd = U.small_state_dict()
    src = str(tmp_path / "m.safetensors")
    save_file(sd, src, {"format": "pt"})
    with_d = safetensors_io.compress_safetensors_file(src, str(tmp_path / "with.znn.safetensors"), device="cpu", digests=True)
    without = safetensors_io.compress_safetensors_file(src, str(tmp_path / "without.znn.safetensors"), device="cpu")
    assert safetensors_io.DIGESTS_KEY in safetensors_io.read_metadata(with_d) and safetensors_io.DIGESTS_KEY not in safetensors_io.read_metadata(without)
    assert any(safetensors_io.get_compressed_tensors_metadata(safetensors_io.read_metadata(with_d)))      # some tensor IS compressed: the reference has to decode
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "oracle", "_ref"), REF])
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    r = subprocess.run([sys.executable, RUNNER, with_d, without], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    want = {k: [str(v.dtype), list(v.shape), hashlib.sha256(v.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()] for k, v in sd.items()}
    assert got[with_d] == got[without] == want
