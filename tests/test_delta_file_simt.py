"""CPU tests (-m "not gpu"): delta checkpoint files on the emulated kernels, CPU tensors as device memory — a variant store written by
ResidentCheckpoint.save_file, read back by from_file(base=) and load_file(base=), refused by SafeOpen; a plain store's file is compress_safetensors_file's.
The checks are tests/delta_file_util.py's, the tensors tests/resident_delta_util.state_dicts()."""
import pytest
import torch

import delta_file_util as D
import resident_delta_util as R

DEV = torch.device("cpu")


@pytest.fixture(scope="module")
def sds():
    return R.state_dicts()


@pytest.mark.parametrize("kind", R.BASES)
def test_a_saved_variant_loads_as_the_store_it_was(use_simt, sds, kind, tmp_path):
    """Round trip per kind of base: the same info() and byte-equal bodies; get_tensor, get_tensors(into=), get_slice across the chunk boundaries,
    plan().run() twice and a hooked forward equal the fine-tune bit for bit; apply_ then revert_ restores the base; a variant of the loaded variant."""
    D.check_round_trip(kind, *sds, DEV, tmp_path)


def test_frames_at_odd_addresses(use_simt, sds, tmp_path):
    """The same with an int8 tensor of 3 elements in the file: the first frame — a delta frame — starts at an odd byte of the data section, and its body at
    an odd address of the uploaded section.  (Where the later frames start follows from the lengths the coder gave the earlier ones: the offsets are
    printed, and the first one, which the layout does fix, is asserted.)  On the emulator over the indexed resident base alone — the kind that runs the
    most kernels per decode; tests/test_gpu_delta_file.py runs all three."""
    D.check_round_trip("store+index", *sds, DEV, tmp_path, odd=True)


def test_the_delta_file_is_smaller_and_same_is_empty(use_simt, sds, tmp_path):
    D.check_sizes(*sds, DEV, tmp_path)


def test_a_plain_store_s_file_is_compress_safetensors_file_s(use_simt, sds, tmp_path):
    D.check_plain_identity(sds[1], DEV, tmp_path, "cpu")


def test_guards(use_simt, sds, tmp_path):
    """No base, a base that lacks a tensor or holds another shape: ValueError naming it.  One changed byte in one base tensor: DigestMismatch naming exactly
    that tensor, from recorded digests and from computed ones alike.  verify=True passes on a good file."""
    D.check_guards(*sds, DEV, tmp_path)


def test_a_damaged_delta_body_is_seen_by_verify(use_simt, sds, tmp_path):
    D.check_damaged_delta_body(*sds, DEV, tmp_path)


def test_load_file_over_every_kind_of_base_and_safe_open_refuses(use_simt, sds, tmp_path):
    p = D.check_load_file(*sds, DEV, tmp_path, "cpu")
    D.check_safe_open_refuses(p)
