// zn_patch_strided.hip — a "znp1" patch (include/zipnn_hip.h) applied IN PLACE through a strided layout: live weights an engine keeps
// transposed, as a column slice of a fused buffer, tile-shuffled or channels-last are strided views whose logical row-major order is the checkpoint tensor's.
// A patch is a list of (element index, XOR value): applying it through a layout is an index map per entry, not a pass over the tensor.
//
//   zn_k_patch_apply_strided   one workgroup per block of 65 536 elements of every item: dst[layout(e)] ^= val for the block's entries, after checking everything it reads
//
// zn_k_patch_apply's body with the address replaced: the same header, first[] and entry tests through zn_patch_format.hpp, the block's entries strided over the
// threads, one E-byte load / XOR / store each — at zn_patch_layout_offset(e), the one index map (zn_patch_format.hpp), whose divisions are 32-bit and whose
// result is 64-bit.  No atomics: a well-formed patch has distinct elements, and the host accepts only layouts it has shown to be injective (zn_patch.hip).
// Entries ascend inside a block, so neighbouring threads touch neighbouring elements of the innermost dimension: as coalesced as that dimension's stride allows.
// The kernel trusts nothing about the patch: it reads only inside [patch, patch + patch_len) and writes only the E bytes of elements of the view — an entry
// that fails its test is not applied and costs the verdict (ZN_DEV_CORRUPT).  The whole patch is always applied: every block is visited, so a call that returns
// clean has validated everything but the canonical padding.
#include "zn_patch_host.hpp"

template <uint32_t E>
__device__ __forceinline__ void zn_pl_apply_block(const ZnPatchLSeg& sg, uint32_t b, uint32_t* __restrict__ status) {
  typedef typename ZnPatchElem<E>::t T;
  const uint32_t tid = threadIdx.x;
  const uint8_t* p = ZN_GLOBAL_PTR(const uint8_t, sg.patch);
  const uint64_t n = sg.n, m = n / E, nb = zn_patch_blocks(m);                   // (the host has checked: n % E == 0, m < 2^32, patch_len >= 32, b < nb)
  uint64_t total;
  bool bad = !zn_patch_header_ok<E>(zn_patch_header(p), n, m, sg.patch_len, total);
  uint32_t f0 = 0, f1 = 0;
  if (!bad) {
    const uint32_t* first = (const uint32_t*)(p + 32);
    f0 = first[b]; f1 = first[b + 1u];
    bad = zn_patch_pair_bad(f0, f1, total, b, nb);
  }
  if (bad) {                                     // (workgroup-uniform)
    if (tid == 0) atomicOr(status, ZN_DEV_CORRUPT);
    return;
  }
  const uint16_t* off = (const uint16_t*)(p + zn_patch_a1(nb));
  const T* val = (const T*)(p + zn_patch_a2(nb, total));
  T* dst = (T*)ZN_GLOBAL_PTR(uint8_t, sg.dst);
  const uint64_t blk0 = (uint64_t)b * ZN_PATCH_BLOCK;
  bool wrong = false;
  for (uint32_t i = f0 + tid; i < f1; i += ZN_PATCH_THREADS) {
    const uint32_t o = off[i];
    const T v = val[i];
    const uint64_t el = blk0 + o;
    if (zn_patch_entry_bad(off, i, f0, o, v, el, m)) { wrong = true; continue; }
    dst[zn_patch_layout_offset(sg.ndim, sg.size, sg.stride, (uint32_t)el)] ^= v;         // (el < m < 2^32; the sizes' product is m: every coordinate lies inside its dimension)
  }
  if (wrong) atomicOr(status, ZN_DEV_CORRUPT);
}

__global__ void __launch_bounds__(ZN_PATCH_THREADS) zn_k_patch_apply_strided(const ZnPatchLSeg one, const ZnPatchLSeg* __restrict__ segs_, uint32_t nseg, uint32_t* __restrict__ status) {
  const ZnPatchLSeg* segs = ZN_GLOBAL_PTR(const ZnPatchLSeg, segs_);
  const ZnPatchLSeg sg = zn_patch_find(one, segs, nseg, blockIdx.x);
  const uint32_t b = blockIdx.x - sg.wg0;
  if (sg.E == 1u) zn_pl_apply_block<1>(sg, b, status);
  else if (sg.E == 2u) zn_pl_apply_block<2>(sg, b, status);
  else zn_pl_apply_block<4>(sg, b, status);
}

void zn_launch_patch_apply_strided(const ZnPatchLSeg& one, const ZnPatchLSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_status, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_apply_strided, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, d_status);
  zn_note_kernel("zn_k_patch_apply_strided");
}
