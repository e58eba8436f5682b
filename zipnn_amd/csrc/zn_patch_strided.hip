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

// ---- zn_k_patch_count_strided / zn_k_patch_emit_strided: the patch of a strided source over a strided base ----
// zn_k_patch_count / zn_k_patch_emit (zn_patch.hip) with both tensors read through layouts of their own over one logical shape.  The order in which a block's
// elements are LOADED is free; the order in which its entries are EMITTED is the format's, logical and ascending.  The two are separated as the merge does it
// (zn_patch_merge.hip): the emit pass sets the bit of every differing element, at its logical offset, in a bitmap of the block in LDS (8 KiB), a popcount prefix
// per word (zn_pm_prefix, 4 KiB) turns a bit into a rank, and each thread walks bitmap words and loads the two elements of every set bit AGAIN through the
// layouts — only changed elements are read twice — to write off / val at first[b] + rank.  Never at or beyond first[b + 1]: if the source changed between or
// during the passes the patch is wrong, not the memory around it.  The count pass sums popcounts and needs no bitmap.
// The load order (zn_pg_walk).  Where the innermost dimension has stride 1 on both sides a thread takes 16 consecutive bytes per step as zn_pa_diff
// does, decided per step: one 16-byte load of each side when the 16 / E elements lie inside one innermost row and both addresses are 16-byte aligned, element
// loads that step along the row otherwise.  Where `fast` — the dimension of the smallest source stride — is NOT the last one and fewer than 65 536 elements
// lie behind it (inner), the block is walked along memory instead: e = hi inner + lo with hi fastest over the block's range of hi, the e outside the block
// skipped, so that neighbouring lanes step along `fast`: several times the logical order's rate on a transposed Llama-3-8B block, inside the spread elsewhere
// (profiles/patch_build_strided.txt has the figures and the decision).  The bits are the same.  -DZN_PATCH_BUILD_LOGICAL_ORDER builds the baseline the measurement compares with: element
// e = blk0 + s 256 + tid for every layout without a stride-1 innermost dimension.

// the word whose bit k says that element k of x's 16 / E differs
template <uint32_t E>
__device__ __forceinline__ uint32_t zn_pg_mask(const uint4 a, const uint4 b) {
  const uint32_t x[4] = {a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w};
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t k = 0; k < 16u / E; k++) {
    const uint32_t d = (x[(k * E) >> 2] >> (8u * ((k * E) & 3u))) & (E == 4u ? 0xFFFFFFFFu : (1u << (8u * (E & 3u))) - 1u);
    if (d) mask |= 1u << k;
  }
  return mask;
}

// The `left` elements of the block at element e0, each exactly once, in the load order -> f(o0, mask): bit k of mask says that element o0 + k OF THE BLOCK
// differs from the base (o0 a multiple of the elements a step takes, which divide 32: the bits of one call lie in one bitmap word).
template <uint32_t E, typename F>
__device__ __forceinline__ void zn_pg_walk(const ZnPatchGSeg& sg, uint32_t e0, uint32_t left, F f) {
  typedef typename ZnPatchElem<E>::t T;
  constexpr uint32_t V = 16u / E, STEP = ZN_PATCH_THREADS * V;
  const uint32_t tid = threadIdx.x, nd = sg.ndim;
  const T* src = (const T*)ZN_GLOBAL_PTR(const uint8_t, sg.src);
  const T* base = (const T*)ZN_GLOBAL_PTR(const uint8_t, sg.base);
  uint32_t row = 0;                              // the innermost row's length where both sides have stride 1 along it, else 0   (constant indices: see zn_patch_layout_offset)
#pragma unroll
  for (uint32_t d = 0; d < ZN_PATCH_LAYOUT_DIMS; d++)
    if (d + 1u == nd && sg.sstride[d] == 1u && sg.bstride[d] == 1u) row = sg.size[d];
#ifndef ZN_PATCH_BUILD_LOGICAL_ORDER
  uint32_t inner = 1;                            // the product of the sizes behind `fast` (<= m < 2^32)
#pragma unroll
  for (uint32_t d = 1; d < ZN_PATCH_LAYOUT_DIMS; d++)
    if (d > sg.fast && d < nd) inner *= sg.size[d];
  if (nd && sg.fast + 1u < nd && inner < ZN_PATCH_BLOCK) {                       // (workgroup-uniform)
    const uint32_t h0 = e0 / inner, H = (e0 + (left - 1u)) / inner - h0 + 1u, all = inner * H;      // H <= 65 536 / inner + 2: all < 3 * 65 536
    for (uint32_t i = tid; i < all; i += ZN_PATCH_THREADS) {
      const uint32_t lo = i / H;
      const uint64_t e = (uint64_t)(h0 + (i - lo * H)) * inner + lo;
      if (e < e0 || e >= (uint64_t)e0 + left) continue;
      const T d = (T)(src[zn_patch_layout_offset(nd, sg.size, sg.sstride, (uint32_t)e)] ^ base[zn_patch_layout_offset(nd, sg.size, sg.bstride, (uint32_t)e)]);
      f((uint32_t)e - e0, d != (T)0 ? 1u : 0u);
    }
    return;
  }
#endif
  if (row == 0) {                                // (workgroup-uniform)
    for (uint32_t o = tid; o < left; o += ZN_PATCH_THREADS) {
      const T d = (T)(src[zn_patch_layout_offset(nd, sg.size, sg.sstride, e0 + o)] ^ base[zn_patch_layout_offset(nd, sg.size, sg.bstride, e0 + o)]);
      f(o, d != (T)0 ? 1u : 0u);
    }
    return;
  }
  for (uint32_t o0 = tid * V; o0 < left; o0 += STEP) {
    const uint32_t e = e0 + o0;
    uint32_t c = e % row;                        // the column of the step's first element
    uint64_t as = zn_patch_layout_offset(nd, sg.size, sg.sstride, e), ab = zn_patch_layout_offset(nd, sg.size, sg.bstride, e);
    uint32_t mask = 0;
    if (o0 + V <= left && c + V <= row && ((((uintptr_t)(src + as)) | ((uintptr_t)(base + ab))) & 15u) == 0u)
      mask = zn_pg_mask<E>(*(const uint4*)(src + as), *(const uint4*)(base + ab));
    else {
      for (uint32_t k = 0; k < V && o0 + k < left; k++) {
        if ((T)(src[as] ^ base[ab]) != (T)0) mask |= 1u << k;
        as++; ab++; c++;
        if (c == row && k + 1u < V && o0 + k + 1u < left) {        // the next element opens a row
          c = 0;
          as = zn_patch_layout_offset(nd, sg.size, sg.sstride, e + k + 1u); ab = zn_patch_layout_offset(nd, sg.size, sg.bstride, e + k + 1u);
        }
      }
    }
    f(o0, mask);
  }
}

struct ZnPgLds { uint32_t bm[ZN_PM_WORDS]; uint16_t pref[ZN_PM_WORDS]; uint32_t part[ZN_PATCH_WAVES]; };

template <uint32_t E>
__device__ __forceinline__ void zn_pg_count_block(const ZnPatchGSeg& sg, uint32_t b, uint32_t* __restrict__ words, uint32_t* part) {
  const uint32_t tid = threadIdx.x;
  const uint64_t m = sg.m, blk0 = (uint64_t)b * ZN_PATCH_BLOCK;
  const uint32_t left = m - blk0 >= (uint64_t)ZN_PATCH_BLOCK ? ZN_PATCH_BLOCK : (uint32_t)(m - blk0);      // > 0: the grid has no workgroup for a block without elements
  uint32_t v = 0;
  zn_pg_walk<E>(sg, (uint32_t)blk0, left, [&](uint32_t, uint32_t mask) { v += (uint32_t)__popc(mask); });
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  if ((tid & 63u) == 0) part[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) { uint32_t c = 0; for (uint32_t w = 0; w < ZN_PATCH_WAVES; w++) c += part[w]; words[b] = c; }
}

template <uint32_t E>
__device__ __forceinline__ void zn_pg_emit_block(const ZnPatchGSeg& sg, uint32_t b, const uint32_t* __restrict__ words, ZnPgLds& s) {
  typedef typename ZnPatchElem<E>::t T;
  const uint32_t tid = threadIdx.x, nd = sg.ndim;
  const uint64_t m = sg.m, nb = zn_patch_blocks(m), blk0 = (uint64_t)b * ZN_PATCH_BLOCK, total = words[nb];
  const uint32_t left = m - blk0 >= (uint64_t)ZN_PATCH_BLOCK ? ZN_PATCH_BLOCK : (uint32_t)(m - blk0);
  const uint32_t lo = words[b], hi = words[b + 1u];
  uint8_t* p = ZN_GLOBAL_PTR(uint8_t, sg.patch);
  if (tid == 0) zn_patch_emit_head<E>(p, m, nb, total, b, lo);
  if (hi <= lo) return;                          // (workgroup-uniform) nothing of this block differs
  uint16_t* off = (uint16_t*)(p + zn_patch_a1(nb));
  T* val = (T*)(p + zn_patch_a2(nb, total));
  for (uint32_t i = tid; i < ZN_PM_WORDS; i += ZN_PATCH_THREADS) s.bm[i] = 0u;
  __syncthreads();
  // (a) every differing element sets the bit of its logical offset
  zn_pg_walk<E>(sg, (uint32_t)blk0, left, [&](uint32_t o0, uint32_t mask) { if (mask) atomicOr(&s.bm[o0 >> 5], mask << (o0 & 31u)); });
  __syncthreads();
  // (b) every word's rank
  (void)zn_pm_prefix(s.bm, s.pref, s.part);
  // (c) the entries, in the order of their bits; neighbouring threads take neighbouring words
  const T* src = (const T*)ZN_GLOBAL_PTR(const uint8_t, sg.src);
  const T* base = (const T*)ZN_GLOBAL_PTR(const uint8_t, sg.base);
  for (uint32_t w = tid; w < ZN_PM_WORDS; w += ZN_PATCH_THREADS) {
    uint32_t bits = s.bm[w], pos = lo + (uint32_t)s.pref[w];
    while (bits) {
      const uint32_t o = w * 32u + (uint32_t)__ffsll((unsigned long long)bits) - 1u, e = (uint32_t)blk0 + o;
      bits &= bits - 1u;
      const T v = (T)(src[zn_patch_layout_offset(nd, sg.size, sg.sstride, e)] ^ base[zn_patch_layout_offset(nd, sg.size, sg.bstride, e)]);
      if (pos < hi) { off[pos] = (uint16_t)o; val[pos] = v; }        // never outside the block's own range, whatever the source holds by now
      pos++;
    }
  }
}

__global__ void __launch_bounds__(ZN_PATCH_THREADS) zn_k_patch_count_strided(const ZnPatchGSeg one, const ZnPatchGSeg* __restrict__ segs_, uint32_t nseg, uint32_t* __restrict__ words_) {
  __shared__ uint32_t part[ZN_PATCH_WAVES];
  const ZnPatchGSeg* segs = ZN_GLOBAL_PTR(const ZnPatchGSeg, segs_);
  const ZnPatchGSeg sg = zn_patch_find(one, segs, nseg, blockIdx.x);
  uint32_t* words = ZN_GLOBAL_PTR(uint32_t, words_) + sg.w0;
  const uint32_t b = blockIdx.x - sg.wg0;
  if (sg.E == 1u) zn_pg_count_block<1>(sg, b, words, part);
  else if (sg.E == 2u) zn_pg_count_block<2>(sg, b, words, part);
  else zn_pg_count_block<4>(sg, b, words, part);
}

__global__ void __launch_bounds__(ZN_PATCH_THREADS) zn_k_patch_emit_strided(const ZnPatchGSeg one, const ZnPatchGSeg* __restrict__ segs_, uint32_t nseg, const uint32_t* __restrict__ words_) {
  __shared__ ZnPgLds s;
  const ZnPatchGSeg* segs = ZN_GLOBAL_PTR(const ZnPatchGSeg, segs_);
  const ZnPatchGSeg sg = zn_patch_find(one, segs, nseg, blockIdx.x);
  const uint32_t* words = ZN_GLOBAL_PTR(const uint32_t, words_) + sg.w0;
  const uint32_t b = blockIdx.x - sg.wg0;
  if (sg.E == 1u) zn_pg_emit_block<1>(sg, b, words, s);
  else if (sg.E == 2u) zn_pg_emit_block<2>(sg, b, words, s);
  else zn_pg_emit_block<4>(sg, b, words, s);
}

void zn_launch_patch_count_strided(const ZnPatchGSeg& one, const ZnPatchGSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_count_strided, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, d_words);
  zn_note_kernel("zn_k_patch_count_strided");
}
void zn_launch_patch_emit_strided(const ZnPatchGSeg& one, const ZnPatchGSeg* d_segs, uint32_t nseg, uint32_t total_wg, const uint32_t* d_words, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_emit_strided, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, d_words);
  zn_note_kernel("zn_k_patch_emit_strided");
}
