"""GPU tests (-m gpu): ResidentCheckpoint.from_live on the real libzipnn_hip.so — the cases of tests/test_resident_capture_simt.py
(tests/resident_capture_util.py) at the same shapes; the captured patches equal the emulated build's byte for byte; and the capture's peak device memory
against the workaround's.  No test here provokes a fault."""
import pytest
import torch

import resident_capture_util as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def release():
    yield
    from zipnn_amd import _capi
    _capi.lib().release_workspace()


@pytest.mark.parametrize("kind", C.BASES)
def test_live_views_are_captured_on_the_device_as_the_emulated_build_captures_them(simt_lib, tmp_path, dev, kind):
    from zipnn_amd import codec
    got = C.check(kind, dev, tmp_path)
    torch.cuda.synchronize()
    # the same views on the CPU through the emulated kernels: the captured patches, byte for byte
    base_sd, new_sd = C.state_dicts(C.SPARSE)
    _, live = C.lives(torch.device("cpu"), new_sd)
    emulated = codec.patch_build_strided_device_batch(simt_lib, [(live[n], base_sd[n]) for n in C.SPARSE])
    assert got == {n: p.numpy().tobytes() for n, p in zip(C.SPARSE, emulated)}


def test_a_capture_allocates_the_patches_and_no_copy_of_a_tensor(dev):
    """Every live tensor qualifies (2 % changed, a plain-tensor base), so the chooser receives nothing.  N: the largest source tensor's bytes.  During from_live
    peak allocated memory rises by less than N plus the patches' arena — there is no contiguous copy of any tensor, let alone plain or delta bodies —; the
    workaround, which starts with contiguous() on every view, rises by at least N."""
    from zipnn_amd import ResidentCheckpoint
    names = ("w.t", "w.narrow", "w.tile", "w.f32")
    base_sd, new_sd = C.state_dicts(names)
    base = C.make_base("dict", base_sd, dev)
    held, live = C.lives(dev, new_sd)
    N = max(t.numel() * t.element_size() for t in live.values())
    ResidentCheckpoint.from_live(live, base)                                      # (once before measuring: the library's workspace is allocated by now)
    torch.cuda.synchronize()

    def peak_rise(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        rest = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(dev) - rest, out

    rise, cap = peak_rise(lambda: ResidentCheckpoint.from_live(live, base))
    assert {cap.info(n)["delta"] for n in names} == {"sparse"}
    arena = sum((cap.info(n)["resident_bytes"] + 255) // 256 * 256 for n in names)
    print(f"from_live: peak rise {rise} bytes (N = {N}, the patches' arena {arena})")
    assert rise < N + arena
    around, ref = peak_rise(lambda: ResidentCheckpoint.from_state_dict({n: v.contiguous() for n, v in live.items()}, dev, base=base, sparse=True))
    print(f"workaround: peak rise {around} bytes")
    assert around >= N
    assert all(cap.patch(n).cpu().numpy().tobytes() == ref.patch(n).cpu().numpy().tobytes() for n in names)
    torch.cuda.synchronize()
