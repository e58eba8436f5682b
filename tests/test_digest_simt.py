"""CPU tests (-m "not gpu"): the content digest "zn64-1" (include/zipnn_hip.h) on the emulated kernels — zn_k_digest against an independent numpy
restatement of the definition (tests/digest_ref.py) — and what is built on it: zipnn_amd.digest, resident stores with digests (verify, holds, guarded apply_ /
revert_) and `.znn.safetensors` files that carry them.  The cases live in tests/digest_util.py, shared with tests/test_gpu_digest.py."""
import numpy as np
import pytest
import torch

import digest_util as U
from digest_ref import KNOWN, digest_ref

CPU = torch.device("cpu")


def test_known_answers_and_argument_checks(use_simt):
    lib = use_simt
    for data, want in KNOWN.items():
        assert lib.digest_host(data) == want == digest_ref(data)
        assert U.device_digests(lib, [torch.frombuffer(bytearray(data), dtype=torch.uint8) if data else torch.empty(0, dtype=torch.uint8)]) == [want]
    assert U.device_digests(lib, []) == []                                   # count == 0
    out = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError):
        lib.digest_batch_dev([(0, 16)], out.data_ptr())                      # a null pointer with n > 0: an error status, never a fault
    with pytest.raises(ValueError):
        lib.digest_batch_dev([(out.data_ptr(), 8), (None, 1)], out.data_ptr())
    with pytest.raises(ValueError):
        lib.digest_batch_dev([(out.data_ptr(), 8)], 0)
    for n in (2 ** 64 - 1, 2 ** 64 - 262143, (0x7FFFFFFF << 18) + 1):         # sizes whose block count wraps or exceeds a grid: rejected before anything is launched
        with pytest.raises(ValueError):
            lib.digest_batch_dev([(out.data_ptr(), n)], out.data_ptr())
        with pytest.raises(ValueError):
            lib.digest_batch_dev([(out.data_ptr(), 8), (out.data_ptr(), n)], out.data_ptr())
    assert out.tolist() == [0, 0]
    assert lib._L.zn_abi_version() == 3


def test_size_alignment_content_matrix_in_one_launch(use_simt):
    """Every size x byte offset x content as one batch: each value == the reference; the items' neighbours in the shared allocation are random bytes."""
    U.check_matrix(use_simt, CPU)


def test_ragged_batch_equals_items_alone_and_reversed(use_simt):
    U.check_ragged(use_simt, CPU)


def test_small_damages_give_pairwise_different_digests(use_simt):
    U.check_sensitivity(use_simt, CPU)


def test_host_and_device_agree(use_simt):
    """zn_digest_host == the device value on the whole matrix; zipnn_amd.digest of a bf16 tensor, of a numpy view of it and of its bytes agree."""
    import zipnn_amd
    host, spans, want = U.matrix()
    assert [use_simt.digest_host(host[s:s + n]) for s, n in spans] == want
    x = (torch.randn(70001, generator=torch.Generator().manual_seed(2)) * 0.02).to(torch.bfloat16)
    d = zipnn_amd.digest(x)
    assert d == digest_ref(x) == zipnn_amd.digest(x.view(torch.int16).numpy()) == zipnn_amd.digest(x.view(torch.int16).numpy().tobytes())
    assert d == zipnn_amd.digest(bytearray(x.view(torch.uint8).numpy().tobytes())) == U.device_digests(use_simt, [x.view(torch.uint8)])[0]
    assert zipnn_amd.digest_many([x, b"", x[:5], np.arange(7, dtype=np.float64)]) == [d, KNOWN[b""], digest_ref(x[:5]), digest_ref(np.arange(7, dtype=np.float64))]
    assert zipnn_amd.digest(x[:70000].reshape(-1, 7)[:, :3]) == digest_ref(x[:70000].reshape(-1, 7)[:, :3].contiguous())      # the contiguous bytes


def test_store_on_the_reference_written_checkpoint(use_simt):
    from zipnn_amd import safetensors_io
    U.check_golden_store(CPU, safetensors_io.load_file(U.GOLDEN, "cpu"))
    assert "zn_k_digest" in use_simt.last_kernels()


def test_corruption_that_decodes_cleanly_is_seen_by_verify_alone(use_simt):
    U.check_clean_corruption(CPU)


def test_files_with_digests(use_simt, tmp_path, monkeypatch):
    from zipnn_amd import ResidentCheckpoint, DigestMismatch, safetensors_io
    with_d, without, sd = U.check_files(tmp_path, "cpu")
    # the per-tensor path digests the tensors as it reads them, a bounded group at a time: the same file whatever the bound
    monkeypatch.setattr(safetensors_io, "_DIGEST_GROUP_BYTES", 1000)
    again = safetensors_io.compress_safetensors_file(str(tmp_path / "m.safetensors"), str(tmp_path / "groups.znn.safetensors"), device="cpu", digests=True)
    assert U.read_container(again) == U.read_container(with_d)               # (header as parsed: the container does not order its metadata keys)
    with pytest.raises(ValueError, match="no digests"):
        safetensors_io.load_file(U.GOLDEN, "cpu", verify=True)               # the reference-written file has no key
    with pytest.raises(ValueError, match="no digests"):
        ResidentCheckpoint.from_file(U.GOLDEN, "cpu", verify=True)
    # a store from a file that carries digests takes them from it, and verify=True checks them at load
    store = ResidentCheckpoint.from_file(with_d, "cpu", digests=True, verify=True)
    assert store.digests() == {k: digest_ref(v) for k, v in sd.items()}
    with pytest.raises(DigestMismatch, match="noise"):
        ResidentCheckpoint.from_file(str(tmp_path / "damaged.znn.safetensors"), "cpu", verify=True)
    late = ResidentCheckpoint.from_file(str(tmp_path / "damaged.znn.safetensors"), "cpu", digests=True)      # the file's digests, unchecked at load …
    assert late.verify(raise_=False) == {k: k != "noise" for k in sd}                                         # … still tell later


def test_variant_stores_verify_holds_and_guards(use_simt):
    U.check_variant(CPU)
