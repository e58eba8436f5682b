"""CPU tests (-m "not gpu"): ResidentCheckpoint.from_live on the emulated kernels — live tensors kept transposed, narrowed, tile-shuffled and
contiguous captured as a variant store over a resident compressed base with an index and over a plain-tensor base.  The cases live in
tests/resident_capture_util.py, shared with tests/test_gpu_resident_capture.py."""
import pytest
import torch

import resident_capture_util as C

CPU = torch.device("cpu")


@pytest.mark.parametrize("kind", C.BASES)
def test_live_views_are_captured_as_patches_built_where_they_lie(use_simt, tmp_path, kind):
    C.check(kind, CPU, tmp_path)


def test_from_live_refuses_what_it_cannot_read(use_simt):
    from zipnn_amd import ResidentCheckpoint
    base_sd, new_sd = C.state_dicts(("w.t",))
    with pytest.raises(ValueError):
        ResidentCheckpoint.from_live({}, base_sd)
    # more than 8 dimensions: no patch can be built where it lies; the chooser takes the contiguous copy
    nine = torch.randn(2 ** 9).to(torch.bfloat16)
    live = {"w.nine": (nine.clone().view((2,) * 9).permute(8, 7, 6, 5, 4, 3, 2, 1, 0))}
    live["w.nine"].reshape(-1)[3] = 1.0
    cap = ResidentCheckpoint.from_live(live, {"w.nine": nine.view((2,) * 9).permute(8, 7, 6, 5, 4, 3, 2, 1, 0).contiguous()})
    assert torch.equal(cap.get_tensor("w.nine"), live["w.nine"])
