// zn_digest.hip — content digests ("zn64-1", include/zipnn_hip.h) of byte ranges in device memory.
//
//   zn_k_digest_init   one thread per item: D = mix64(n + G) into the item's slot
//   zn_k_digest        one workgroup per (item, 256 KiB block): B_c = Σ w_i · fmix32(i + 1) over the block's words, one wave-wide sum on the DPP network,
//                      one combine per workgroup through LDS, ONE 64-bit atomic add of mix64(B_c + (c + 1) G) to the item's slot.
//
// The two run behind each other on the caller's stream.  Blocks combine by a wrapping 64-bit sum, which commutes: no schedule changes a value, and
// a batch of hundreds of ragged tensors is one launch (a workgroup finds its item by binary search over the items' first workgroups, as the batched decode does).
//
// Loads are 16 bytes per lane, non-temporal (a pure streaming read: nothing is read twice), 1 KiB per wave instruction, and always ALIGNED: an item may
// start at any byte address, and its words are counted from its first byte, so a misaligned item reads the two aligned granules its four words straddle and
// funnel-shifts (v_alignbyte) them into place.  A granule is read only if it holds a byte of the item; bytes of it outside the item are masked away.
// The keys are computed in registers from the word index (a table of them would be the block's size): two 32-bit multiplies per word beside the 32 x 32 + 64
// multiply-add that uses them.
#include "zn_internal.hpp"
#include <string.h>

#define ZN_DG_THREADS 256u
#define ZN_DG_BLOCK_WORDS 65536u                                   // 256 KiB of data per block c — part of the digest's DEFINITION, not a tuning knob
#define ZN_DG_STEP_WORDS (ZN_DG_THREADS * 4u)                      // words per workgroup step: 16 bytes per lane
#define ZN_DG_STEPS (ZN_DG_BLOCK_WORDS / ZN_DG_STEP_WORDS)
#define ZN_DG_G 0x9E3779B97F4A7C15ull

__host__ __device__ __forceinline__ uint32_t zn_dg_fmix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ uint64_t zn_dg_mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
  return z;
}

#if !defined(ZN_SIMT_EMULATOR)
typedef uint32_t zn_dg_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 zn_dg_ld128(const uint8_t* p) { const zn_dg_v4u v = __builtin_nontemporal_load((const zn_dg_v4u*)p); return make_uint4(v.x, v.y, v.z, v.w); }
#else
__device__ __forceinline__ uint4 zn_dg_ld128(const uint8_t* p) { return *(const uint4*)p; }
#endif

// wave-wide wrapping 64-bit sum, in lane 63: the two halves go through the DPP network (row_shr 1/2/4/8, row_bcast15, row_bcast31) as 32-bit moves
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t zn_dg_dpp_add(uint64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xF, false);
  return v + (((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ uint64_t zn_dg_wave_sum(uint64_t v) {
  v = zn_dg_dpp_add<0x111, 0xF>(v);
  v = zn_dg_dpp_add<0x112, 0xF>(v);
  v = zn_dg_dpp_add<0x114, 0xF>(v);
  v = zn_dg_dpp_add<0x118, 0xF>(v);
  v = zn_dg_dpp_add<0x142, 0xA>(v);
  v = zn_dg_dpp_add<0x143, 0xC>(v);
  return v;                                                        // (lane 63 holds the wave's sum)
}

__device__ __forceinline__ ZnDigSeg zn_dg_find(const ZnDigSeg& one, const ZnDigSeg* __restrict__ segs, uint32_t nseg, uint32_t b) {
  if (segs == nullptr) return one;
  uint32_t lo = 0, hi = nseg;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (segs[mid].wg0 <= b) lo = mid; else hi = mid; }
  return segs[lo];
}

// Four words of the item from byte offset `off` of it (off % 16 == 0): with SHIFT the item starts `a` bytes (1..15) into an aligned granule.
// MASKED: the words may reach past the item's last byte (n_left = bytes of the item from `off` on, may be <= 0): nothing outside is read or counted.
template <bool SHIFT, bool MASKED>
__device__ __forceinline__ void zn_dg_words(const uint8_t* __restrict__ base, uint64_t off, uint32_t a, int64_t n_left, uint32_t (&w)[4]) {
  // base = the item's first byte rounded DOWN to 16: the granule at base + off holds the item's bytes [off - a, off - a + 16)
  const uint8_t* p = base + off;
  uint32_t d[8];
  if (!MASKED) {
    const uint4 g0 = zn_dg_ld128(p);
    d[0] = g0.x; d[1] = g0.y; d[2] = g0.z; d[3] = g0.w;
    if (SHIFT) { const uint4 g1 = zn_dg_ld128(p + 16); d[4] = g1.x; d[5] = g1.y; d[6] = g1.z; d[7] = g1.w; }
  } else {
    // granule 0 holds item bytes from off - a (it always holds byte `off` of the item when n_left > 0), granule 1 from off - a + 16
    uint4 g0 = make_uint4(0, 0, 0, 0), g1 = make_uint4(0, 0, 0, 0);
    if (n_left > 0) g0 = zn_dg_ld128(p);
    if (SHIFT && n_left + (int64_t)a > 16) g1 = zn_dg_ld128(p + 16);
    d[0] = g0.x; d[1] = g0.y; d[2] = g0.z; d[3] = g0.w; d[4] = g1.x; d[5] = g1.y; d[6] = g1.z; d[7] = g1.w;
  }
  if (SHIFT) {
    const uint32_t q = a >> 2, r = a & 3u;                         // (wave-uniform: per item)
    uint32_t e[5];
#pragma unroll
    for (int k = 0; k < 5; k++) e[k] = q == 0 ? d[k] : q == 1 ? d[k + 1] : q == 2 ? d[k + 2] : d[k + 3];
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = __builtin_amdgcn_alignbyte(e[k + 1], e[k], r);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = d[k];
  }
  if (MASKED) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int64_t left = n_left - 4 * k;                         // bytes of the item in word k and behind it
      if (left <= 0) w[k] = 0;
      else if (left < 4) w[k] &= 0xFFFFFFFFu >> (8u * (uint32_t)(4 - left));
    }
  }
}

template <bool SHIFT, bool MASKED>
__device__ __forceinline__ uint64_t zn_dg_step(const uint8_t* __restrict__ base, uint64_t off, uint32_t a, int64_t n_left, uint32_t i0, uint64_t acc) {
  uint32_t w[4];
  zn_dg_words<SHIFT, MASKED>(base, off, a, n_left, w);
#pragma unroll
  for (int k = 0; k < 4; k++) acc += (uint64_t)w[k] * (uint64_t)zn_dg_fmix32(i0 + (uint32_t)k + 1u);      // v_mad_u64_u32
  return acc;
}

template <bool SHIFT>
__device__ __forceinline__ uint64_t zn_dg_block(const uint8_t* __restrict__ base, uint32_t a, uint64_t n, uint64_t c) {
  const uint32_t tid = threadIdx.x;
  const uint64_t blk_off = c * (uint64_t)(ZN_DG_BLOCK_WORDS * 4u);        // the block's first byte of the item
  const uint64_t left = n - blk_off;                                       // > 0: the grid has no workgroup for a block without bytes
  // steps whose 4 KiB lie wholly inside the item need no masks (the second granule of a shifted lane then also holds a byte of the item)
  const uint32_t full = left >= (uint64_t)(ZN_DG_BLOCK_WORDS * 4u) ? ZN_DG_STEPS : (uint32_t)(left / (ZN_DG_STEP_WORDS * 4u));
  uint64_t acc = 0;
  uint32_t s = 0;
#pragma unroll 4
  for (; s < full; s++) {
    const uint32_t i0 = s * ZN_DG_STEP_WORDS + tid * 4u;
    acc = zn_dg_step<SHIFT, false>(base, blk_off + (uint64_t)i0 * 4u, a, 0, i0, acc);
  }
  if (full < ZN_DG_STEPS) {
    const uint32_t steps = (uint32_t)((left + ZN_DG_STEP_WORDS * 4u - 1u) / (ZN_DG_STEP_WORDS * 4u));      // ≤ ZN_DG_STEPS here
    for (; s < steps; s++) {
      const uint32_t i0 = s * ZN_DG_STEP_WORDS + tid * 4u;
      acc = zn_dg_step<SHIFT, true>(base, blk_off + (uint64_t)i0 * 4u, a, (int64_t)left - (int64_t)i0 * 4, i0, acc);
    }
  }
  return acc;
}

__global__ void __launch_bounds__(256) zn_k_digest_init(const ZnDigSeg one, const ZnDigSeg* __restrict__ segs, uint32_t nseg, unsigned long long* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nseg) return;
  const uint64_t n = segs ? segs[i].n : one.n;
  out[i] = zn_dg_mix64(n + ZN_DG_G);
}

__global__ void __launch_bounds__(ZN_DG_THREADS) zn_k_digest(const ZnDigSeg one, const ZnDigSeg* __restrict__ segs_, uint32_t nseg, unsigned long long* __restrict__ out) {
  __shared__ uint64_t part[ZN_DG_THREADS / 64u];
  const ZnDigSeg* segs = ZN_GLOBAL_PTR(const ZnDigSeg, segs_);
  const ZnDigSeg sg = zn_dg_find(one, segs, nseg, blockIdx.x);
  const uint64_t c = blockIdx.x - sg.wg0;
  const uint8_t* src = ZN_GLOBAL_PTR(const uint8_t, sg.src);
  const uint32_t a = (uint32_t)((uintptr_t)src & 15u);
  const uint8_t* base = src - a;
  const uint64_t acc = a ? zn_dg_block<true>(base, a, sg.n, c) : zn_dg_block<false>(base, 0, sg.n, c);
  const uint64_t wsum = zn_dg_wave_sum(acc);
  if ((threadIdx.x & 63u) == 63u) part[threadIdx.x >> 6] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t B = 0;
    for (uint32_t i = 0; i < ZN_DG_THREADS / 64u; i++) B += part[i];
    // (a device-wide atomic: the item's blocks run on every XCD)
    atomicAdd(&out[sg.slot], (unsigned long long)zn_dg_mix64(B + (c + 1u) * ZN_DG_G));
  }
}

void zn_launch_digest(const ZnDigSeg& one, const ZnDigSeg* d_segs, uint32_t nseg, uint32_t total_wg, unsigned long long* d_out, hipStream_t stream) {
  if (nseg == 0) return;
  hipLaunchKernelGGL(zn_k_digest_init, dim3((nseg + 255u) / 256u), dim3(256), 0, stream, one, d_segs, nseg, d_out);
  zn_note_kernel("zn_k_digest_init");
  if (total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_digest, dim3(total_wg), dim3(ZN_DG_THREADS), 0, stream, one, d_segs, nseg, d_out);
  zn_note_kernel("zn_k_digest");
}

// the scalar restatement for host buffers and files (zn_digest_host): the definition, word by word
uint64_t zn_digest_scalar(const uint8_t* b, size_t n) {
  uint64_t D = zn_dg_mix64((uint64_t)n + ZN_DG_G), B = 0, c = 0;
  const size_t words = (n + 3u) / 4u;
  for (size_t j = 0; j < words; j++) {
    uint32_t w = 0;
    const size_t left = n - 4u * j;
    if (left >= 4u) memcpy(&w, b + 4u * j, 4);                     // (little-endian hosts: the ABI's only kind)
    else for (size_t k = 0; k < left; k++) w |= (uint32_t)b[4u * j + k] << (8u * k);
    const uint32_t i = (uint32_t)(j % ZN_DG_BLOCK_WORDS);
    B += (uint64_t)w * (uint64_t)zn_dg_fmix32(i + 1u);
    if (i == ZN_DG_BLOCK_WORDS - 1u || j == words - 1u) { D += zn_dg_mix64(B + (c + 1u) * ZN_DG_G); B = 0; c++; }
  }
  return D;
}
