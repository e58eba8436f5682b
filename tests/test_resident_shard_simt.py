"""CPU tests (-m "not gpu"): ResidentCheckpoint.sharded on the emulated kernels — both shards of a two-way tensor-parallel split of a sparse
variant store, by one batched patch select per store; the cases live in tests/resident_shard_util.py, shared with tests/test_gpu_resident_shard.py."""
import pytest
import torch

import resident_shard_util as U

CPU = torch.device("cpu")


@pytest.mark.parametrize("onto_kind", ["dict", "store"])
def test_both_shards_of_a_two_way_split_decode_the_narrowed_tensors(use_simt, tmp_path, onto_kind):
    U.check_shards(CPU, tmp_path, onto_kind)


def test_sharding_without_a_base_builds_a_plain_store_of_the_shards(use_simt):
    U.check_without_onto(CPU)


def test_spec_and_onto_mismatches_are_refused_by_name(use_simt):
    U.check_errors(CPU)


def test_a_chain_is_sharded_link_by_link(use_simt):
    U.check_chain(CPU)


def test_sparse_and_same_entries_are_sharded_without_a_decode_by_one_select_call(use_simt, monkeypatch):
    U.check_no_decode_one_select(use_simt, CPU, monkeypatch)
