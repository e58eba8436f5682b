"""GPU tests (-m gpu): the content digest "zn64-1" on the real libzipnn_hip.so — zn_k_digest against tests/digest_ref.py on the cases of
tests/test_digest_simt.py (tests/digest_util.py), a digest enqueued behind a plan run with no host sync, stores and files with digests on the device."""
import pytest
import torch

import digest_util as U
from digest_ref import digest_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    yield L
    L.release_workspace()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def test_size_alignment_content_matrix_in_one_launch_on_the_device(lib, dev):
    U.check_matrix(lib, dev)
    torch.cuda.synchronize()


def test_ragged_batch_equals_items_alone_and_reversed_on_the_device(lib, dev):
    U.check_ragged(lib, dev)
    torch.cuda.synchronize()


def test_small_damages_give_pairwise_different_digests_on_the_device(lib, dev):
    U.check_sensitivity(lib, dev)


def test_eight_mib_and_three_bytes_at_byte_offset_one(lib, dev):
    import zipnn_amd
    n = (8 << 20) + 3
    raw = torch.randint(0, 256, (n + 512,), dtype=torch.uint8, generator=torch.Generator().manual_seed(8))
    on = U.aligned_device_copy(raw.numpy(), dev)
    t = on[1:1 + n]
    assert t.data_ptr() % 16 == 1
    want = digest_ref(raw[1:1 + n].numpy())
    assert U.device_digests(lib, [t]) == [want] and zipnn_amd.digest(t) == want
    assert lib.digest_host(raw[1:1 + n].numpy()) == want
    assert zipnn_amd.digest_many([t, raw[1:1 + n], on[:4096]]) == [want, want, digest_ref(raw[:4096].numpy())]


def test_digest_behind_a_plan_run_on_a_side_stream_without_a_host_sync(lib, dev):
    """The digest is one more launch on the stream: enqueued right behind the decode it checks, it reads what the decode wrote."""
    from zipnn_amd import ResidentCheckpoint, codec
    x = (torch.randn(5 * U.K // 2 + 77, generator=torch.Generator().manual_seed(4)) * 0.02).to(torch.bfloat16)
    store = ResidentCheckpoint.from_state_dict({"x": x}, dev)
    assert store.info("x")["compressed"]
    plan = store.plan(["x"])
    flat = codec.flat_bytes(plan.tensors["x"])
    flat.fill_(0x5A)
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    plan.run(stream=side)
    codec.digest_device_batch(lib, [flat], stream=side.cuda_stream, out=out)
    side.synchronize()
    plan.status()
    assert codec.digests_to_ints(out) == [digest_ref(x)]
    plan.close()


def test_store_on_the_reference_written_checkpoint_on_the_device(lib, dev):
    """The expected tensors do not come from the device decode path the store uses: they are read on the host route (SafeOpen with device="cpu", the host-buffer
    entry points) and each must hash to what the REFERENCE recorded when it wrote the file (tests/golden/gpt2_small_ref.znn.safetensors.json)."""
    import hashlib
    import json
    from zipnn_amd import SafeOpen
    info = json.load(open(U.GOLDEN + ".json"))["tensors"]
    with SafeOpen(U.GOLDEN, "pt", device="cpu") as f:
        want = {k: f.get_tensor(k) for k in f.keys()}
    assert sorted(want) == sorted(info)
    for k, v in want.items():
        assert not v.is_cuda and hashlib.sha256(U._cpu_bytes(v).numpy().tobytes()).hexdigest() == info[k]["sha256"], k
    U.check_golden_store(dev, want)


def test_corruption_that_decodes_cleanly_is_seen_by_verify_alone_on_the_device(lib, dev):
    U.check_clean_corruption(dev)


def test_variant_stores_verify_holds_and_guards_on_the_device(lib, dev):
    U.check_variant(dev)


def test_files_with_digests_on_the_device(lib, dev, tmp_path):
    """compress_safetensors_file on the device (one digest launch over the uploaded data section) -> load_file(verify=True) on cuda:0 (one launch over the
    decoded tensors); a damaged stored-raw tensor is named."""
    from zipnn_amd import ResidentCheckpoint
    with_d, _, sd = U.check_files(tmp_path, "cuda:0")
    store = ResidentCheckpoint.from_file(with_d, dev, digests=True, verify=True)
    assert store.digests() == {k: digest_ref(v) for k, v in sd.items()}
