"""GPU tests (-m gpu): delta checkpoint files on the real libzipnn_hip.so — the cases of tests/test_delta_file_simt.py
(tests/delta_file_util.py) on cuda:0: round trips per kind of base, frames at odd addresses, sizes, the plain store's file, the guards, load_file(base=)
and SafeOpen's refusal."""
import pytest
import torch

import delta_file_util as D
import resident_delta_util as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from zipnn_amd import _capi
    L = _capi.lib()
    assert L.device_count() >= 1
    yield torch.device("cuda:0")
    L.release_workspace()


@pytest.fixture(scope="module")
def sds():
    return R.state_dicts()


@pytest.mark.parametrize("kind", R.BASES)
def test_a_saved_variant_loads_as_the_store_it_was_on_the_device(dev, sds, kind, tmp_path):
    D.check_round_trip(kind, *sds, dev, tmp_path)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", R.BASES)
def test_frames_at_odd_addresses_on_the_device(dev, sds, kind, tmp_path):
    D.check_round_trip(kind, *sds, dev, tmp_path, odd=True)
    torch.cuda.synchronize()


def test_the_delta_file_is_smaller_and_same_is_empty_on_the_device(dev, sds, tmp_path):
    D.check_sizes(*sds, dev, tmp_path)


def test_a_plain_store_s_file_is_compress_safetensors_file_s_on_the_device(dev, sds, tmp_path):
    D.check_plain_identity(sds[1], dev, tmp_path, "cuda:0")


def test_guards_on_the_device(dev, sds, tmp_path):
    D.check_guards(*sds, dev, tmp_path)
    torch.cuda.synchronize()


def test_a_damaged_delta_body_is_seen_by_verify_on_the_device(dev, sds, tmp_path):
    """One payload byte of a delta frame changed: the decoder rejects it or decodes other bytes, which the digest sees — as the damaged bodies of
    test_gpu_parity.py, never fatal: the undamaged file loads right after."""
    D.check_damaged_delta_body(*sds, dev, tmp_path)
    torch.cuda.synchronize()


def test_load_file_over_every_kind_of_base_and_safe_open_refuses_on_the_device(dev, sds, tmp_path):
    p = D.check_load_file(*sds, dev, tmp_path, "cuda:0")
    D.check_safe_open_refuses(p)
