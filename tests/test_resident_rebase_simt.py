"""CPU tests (-m "not gpu"): ResidentCheckpoint.rebased on the emulated kernels — a chain of sparse variants flattened by batched patch merges, and
siblings re-parented onto each other; the cases live in tests/resident_rebase_util.py, shared with tests/test_gpu_resident_rebase.py."""
import torch

import resident_rebase_util as U

CPU = torch.device("cpu")


def test_a_chain_of_sparse_variants_flattens_onto_its_first_base(use_simt, tmp_path):
    U.check_chain(CPU, tmp_path)


def test_siblings_over_one_base_become_patches_over_each_other(use_simt):
    U.check_siblings(CPU)


def test_one_batched_merge_call_per_link_of_the_chain(use_simt, monkeypatch):
    """A chain of depth 3 costs two zn_patch_merge_batch_dev calls for the whole store, not per tensor."""
    from zipnn_amd import ResidentCheckpoint
    b_sd, s1_sd, s2_sd, s3_sd = U.chain_sds()
    stores = [ResidentCheckpoint.from_state_dict(b_sd, CPU)]
    for sd in (s1_sd, s2_sd, s3_sd):
        stores.append(ResidentCheckpoint.from_state_dict(sd, CPU, base=stores[-1], sparse=True))
    calls = []
    real = use_simt.patch_merge_batch_dev
    monkeypatch.setattr(use_simt, "patch_merge_batch_dev", lambda items, stream=0: calls.append(len(list(items))) or real(items, stream))
    stores[3].rebased(stores[0])
    assert calls == [3, 3]
