"""An independent numpy restatement of the "zn64-1" content digest, written from its definition (not from the kernel), for the digest tests.

    fmix32(x): x ^= x>>16; x *= 0x85EBCA6B; x ^= x>>13; x *= 0xC2B2AE35; x ^= x>>16          (mod 2^32)
    mix64(z):  z ^= z>>30; z *= 0xBF58476D1CE4E5B9; z ^= z>>27; z *= 0x94D049BB133111EB; z ^= z>>31   (mod 2^64)
    G = 0x9E3779B97F4A7C15
    bytes zero-padded to a multiple of 4; w_j = little-endian 32-bit word j, counted from the first byte; block c = words [65536 c, 65536 (c + 1))
    B_c = sum_i w_{65536 c + i} * fmix32(i + 1)  (mod 2^64);   D = mix64(n + G) + sum_c mix64(B_c + (c + 1) G)  (mod 2^64)
"""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
BLOCK_WORDS = 65536
KNOWN = {b"": 0xe220a8397b1dcdaf, b"\x01": 0x947511c5412f4857}


def _fmix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def _mix64(z):
    z &= M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    z ^= z >> 31
    return z


_KEYS = _fmix32(np.arange(1, BLOCK_WORDS + 1, dtype=np.uint64)).astype(np.uint64)


def as_bytes(x):
    """torch tensor / numpy array / bytes-like -> 1-D uint8 numpy array of its contiguous bytes."""
    if hasattr(x, "detach"):
        import torch
        x = x.detach().cpu().contiguous()
        x = (x.view(torch.uint8) if x.element_size() == 1 else x.reshape(-1).view(torch.uint8)).reshape(-1).numpy()
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    return np.frombuffer(bytes(x), dtype=np.uint8)


def digest_ref(x):
    b = as_bytes(x)
    n = int(b.size)
    padded = np.zeros((n + 3) // 4 * 4, dtype=np.uint8)
    padded[:n] = b
    words = padded.view("<u4").astype(np.uint64)
    d = _mix64(n + G)
    with np.errstate(over="ignore"):
        for c in range((words.size + BLOCK_WORDS - 1) // BLOCK_WORDS):
            w = words[c * BLOCK_WORDS:(c + 1) * BLOCK_WORDS]
            bc = int((w * _KEYS[:w.size]).sum(dtype=np.uint64))            # (uint64 products and sums wrap)
            d = (d + _mix64(bc + (c + 1) * G)) & M64
    return d


assert all(digest_ref(k) == v for k, v in KNOWN.items())
