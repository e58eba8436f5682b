"""GPU tests (-m gpu): ResidentCheckpoint.sharded on the real libzipnn_hip.so — the cases of tests/test_resident_shard_simt.py
(tests/resident_shard_util.py) at the same sizes: both shards of a two-way split decode the narrowed tensors of the state dict the store was built from
through every entry point, and their selected patches equal tests/patch_ref.py's patch of the shard pair byte for byte."""
import pytest
import torch

import resident_shard_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from zipnn_amd import _capi
    assert _capi.lib().device_count() >= 1
    yield torch.device("cuda:0")
    _capi.lib().release_workspace()


@pytest.mark.parametrize("onto_kind", ["dict", "store"])
def test_both_shards_of_a_two_way_split_decode_the_narrowed_tensors_on_the_device(dev, tmp_path, onto_kind):
    U.check_shards(dev, tmp_path, onto_kind)
    torch.cuda.synchronize()


def test_sharding_without_a_base_builds_a_plain_store_of_the_shards_on_the_device(dev):
    U.check_without_onto(dev)
    torch.cuda.synchronize()


def test_spec_and_onto_mismatches_are_refused_by_name_on_the_device(dev):
    U.check_errors(dev)
    torch.cuda.synchronize()


def test_a_chain_is_sharded_link_by_link_on_the_device(dev):
    U.check_chain(dev)
    torch.cuda.synchronize()


def test_sparse_and_same_entries_are_sharded_without_a_decode_by_one_select_call_on_the_device(dev, monkeypatch):
    from zipnn_amd import _capi
    U.check_no_decode_one_select(_capi.lib(), dev, monkeypatch)
    torch.cuda.synchronize()
