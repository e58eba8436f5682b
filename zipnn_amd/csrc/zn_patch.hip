// zn_patch.hip — changed-element patches ("znp1", include/zipnn_hip.h): the elements of a tensor that differ from a base, with their XOR values.
//
//   zn_k_patch_count   one workgroup per block of 65 536 elements: how many of them differ (one word per block)
//   zn_k_patch_scan    one workgroup per item: the block counts become first[] (an exclusive prefix sum, in place), the item's T goes to its total
//   zn_k_patch_emit    one workgroup per block again: off / val of the block's differing elements at first[b] + rank, in ascending order; block 0 writes the header
//   zn_k_patch_apply   one workgroup per block of the window: dst[e] ^= val for the block's entries inside the window, after checking everything it reads
//   zn_k_patch_check   one workgroup per block of the tensor: the whole patch against the format, read-only — a mask of findings per item
//
// Count and emit are ONE body (zn_pa_block<E, EMIT>): the same loads, the same comparison, the same order of elements.  The emit instance never writes outside
// [first[b], first[b + 1]) of off / val: if the source changed between the two passes the patch is wrong, not the memory around it.  A thread takes 16 consecutive
// bytes per step (one 16-byte load each of source and base when both are 16-byte aligned and the bytes lie inside the tensor; element loads otherwise), so that
// ranks ascend with the thread index: a wave-exclusive scan of the per-thread counts, the waves' sums through LDS, a running total in a register.
// The apply kernel trusts nothing: a patch may come from anywhere.  It reads only inside [patch, patch + patch_len) — the header first, whose L must be patch_len
// and the formula's value for its T, which bounds every later index — and writes only elements of the window; what is wrong costs the verdict (ZN_DEV_CORRUPT).
#include "zn_patch_host.hpp"

#include <algorithm>
#include <memory>

// zn_patch_wave_incl, skipped where no lane of the wave brings anything
__device__ __forceinline__ uint32_t zn_pa_wave_incl(uint32_t v, uint32_t lane) {
  if (__ballot(v != 0u) == 0ull) return 0u;
  return zn_patch_wave_incl(v, lane);
}

// src ^ base of the 16 / E elements from element e0 on, as the four little-endian words they occupy (elements at or behind m: zero) -> the mask of those that differ
template <uint32_t E>
__device__ __forceinline__ uint32_t zn_pa_diff(const uint8_t* __restrict__ src, const uint8_t* __restrict__ base, uint64_t e0, uint64_t m, bool fast, uint32_t (&x)[4]) {
  typedef typename ZnPatchElem<E>::t T;
  constexpr uint32_t V = 16u / E;
  if (fast && e0 + V <= m) {
    const uint4 a = *(const uint4*)(src + e0 * E), b = *(const uint4*)(base + e0 * E);
    x[0] = a.x ^ b.x; x[1] = a.y ^ b.y; x[2] = a.z ^ b.z; x[3] = a.w ^ b.w;
  } else {
    x[0] = x[1] = x[2] = x[3] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < V; k++)
      if (e0 + k < m) {
        const T d = (T)(((const T*)src)[e0 + k] ^ ((const T*)base)[e0 + k]);
        x[(k * E) >> 2] |= (uint32_t)d << (8u * ((k * E) & 3u));
      }
  }
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t k = 0; k < V; k++) {
    const uint32_t d = (x[(k * E) >> 2] >> (8u * ((k * E) & 3u))) & (E == 4u ? 0xFFFFFFFFu : (1u << (8u * (E & 3u))) - 1u);
    if (d) mask |= 1u << k;
  }
  return mask;
}

// Block b of one item.  !EMIT: words[b] = its number of differing elements.  EMIT: words[] is first[]; the block's entries go to off / val of the patch.
template <uint32_t E, bool EMIT>
__device__ __forceinline__ void zn_pa_block(const ZnPatchBSeg& sg, uint32_t b, uint32_t* __restrict__ words, uint32_t (*part)[ZN_PATCH_WAVES]) {
  typedef typename ZnPatchElem<E>::t T;
  constexpr uint32_t V = 16u / E, STEP = ZN_PATCH_THREADS * V;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint8_t* src = ZN_GLOBAL_PTR(const uint8_t, sg.src);
  const uint8_t* base = ZN_GLOBAL_PTR(const uint8_t, sg.base);
  const uint64_t m = sg.m, blk0 = (uint64_t)b * ZN_PATCH_BLOCK;
  const uint32_t left = m - blk0 >= (uint64_t)ZN_PATCH_BLOCK ? ZN_PATCH_BLOCK : (uint32_t)(m - blk0);      // > 0: the grid has no workgroup for a block without elements
  const uint32_t steps = (left + STEP - 1u) / STEP;
  const bool fast = ((((uintptr_t)src) | ((uintptr_t)base)) & 15u) == 0u;        // (per item: wave-uniform)
  uint32_t lo = 0, hi = 0;
  uint16_t* off = nullptr; T* val = nullptr;
  if (EMIT) {
    const uint64_t nb = zn_patch_blocks(m), total = words[nb];
    uint8_t* p = ZN_GLOBAL_PTR(uint8_t, sg.patch);
    lo = words[b]; hi = words[b + 1u];
    if (tid == 0) zn_patch_emit_head<E>(p, m, nb, total, b, lo);
    if (hi <= lo) return;                        // (workgroup-uniform) nothing of this block differs
    off = (uint16_t*)(p + zn_patch_a1(nb)); val = (T*)(p + zn_patch_a2(nb, total));
  }
  uint32_t run = 0;                              // count: this thread's differing elements; emit: the block's entries in front of this step
  for (uint32_t s = 0; s < steps; s++) {
    const uint32_t o0 = s * STEP + tid * V;      // offset of the thread's first element inside the block
    uint32_t x[4];
    const uint32_t mask = zn_pa_diff<E>(src, base, blk0 + o0, m, fast, x);
    const uint32_t cnt = (uint32_t)__popc(mask);
    if (!EMIT) { run += cnt; continue; }
    const uint32_t incl = zn_pa_wave_incl(cnt, lane);
    if (lane == 63u) part[s & 1u][wave] = incl;  // (two sets of slots: one barrier per step is enough)
    __syncthreads();
    uint32_t before, all;
    zn_patch_wave_sums(part[s & 1u], wave, before, all);
    if (cnt) {
      uint32_t pos = lo + run + before + incl - cnt;
#pragma unroll
      for (uint32_t k = 0; k < V; k++)
        if ((mask >> k) & 1u) {
          if (pos < hi) {                        // never outside the block's own range, whatever the source holds by now
            off[pos] = (uint16_t)(o0 + k);
            val[pos] = (T)(x[(k * E) >> 2] >> (8u * ((k * E) & 3u)));
          }
          pos++;
        }
    }
    run += all;
  }
  if (!EMIT) {
    uint32_t v = run;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) part[0][wave] = v;
    __syncthreads();
    if (tid == 0) { uint32_t c = 0; for (uint32_t w = 0; w < ZN_PATCH_WAVES; w++) c += part[0][w]; words[b] = c; }
  }
}

template <bool EMIT>
__device__ __forceinline__ void zn_pa_dispatch(const ZnPatchBSeg& one, const ZnPatchBSeg* __restrict__ segs_, uint32_t nseg, uint32_t* words_, uint32_t (*part)[ZN_PATCH_WAVES]) {
  const ZnPatchBSeg* segs = ZN_GLOBAL_PTR(const ZnPatchBSeg, segs_);
  const ZnPatchBSeg sg = zn_patch_find(one, segs, nseg, blockIdx.x);
  uint32_t* words = ZN_GLOBAL_PTR(uint32_t, words_) + sg.w0;
  const uint32_t b = blockIdx.x - sg.wg0;
  if (sg.E == 1u) zn_pa_block<1, EMIT>(sg, b, words, part);
  else if (sg.E == 2u) zn_pa_block<2, EMIT>(sg, b, words, part);
  else zn_pa_block<4, EMIT>(sg, b, words, part);
}

__global__ void __launch_bounds__(ZN_PATCH_THREADS) zn_k_patch_count(const ZnPatchBSeg one, const ZnPatchBSeg* __restrict__ segs, uint32_t nseg, uint32_t* __restrict__ words) {
  __shared__ uint32_t part[2][ZN_PATCH_WAVES];
  zn_pa_dispatch<false>(one, segs, nseg, words, part);
}

__global__ void __launch_bounds__(ZN_PATCH_THREADS) zn_k_patch_emit(const ZnPatchBSeg one, const ZnPatchBSeg* __restrict__ segs, uint32_t nseg, uint32_t* __restrict__ words) {
  __shared__ uint32_t part[2][ZN_PATCH_WAVES];
  zn_pa_dispatch<true>(one, segs, nseg, words, part);
}

// one workgroup per item: its block counts -> first[] (in place), first[NB] = T, totals[item] = T
__global__ void __launch_bounds__(ZN_PATCH_THREADS) zn_k_patch_scan(const ZnPatchBSeg one, const ZnPatchBSeg* __restrict__ segs_, uint32_t* __restrict__ words_, uint64_t* __restrict__ totals) {
  __shared__ uint32_t part[ZN_PATCH_WAVES];
  const ZnPatchBSeg* segs = ZN_GLOBAL_PTR(const ZnPatchBSeg, segs_);
  const ZnPatchBSeg sg = segs ? segs[blockIdx.x] : one;
  uint32_t* words = ZN_GLOBAL_PTR(uint32_t, words_) + sg.w0;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t nb = (uint32_t)zn_patch_blocks(sg.m);
  uint32_t run = 0;
  for (uint32_t i0 = 0; i0 < nb; i0 += ZN_PATCH_THREADS) {
    const uint32_t i = i0 + tid;
    const uint32_t c = i < nb ? words[i] : 0u;
    const uint32_t incl = zn_pa_wave_incl(c, lane);
    if (lane == 63u) part[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;                // (zn_patch_wave_sums, written out: through the helper this kernel takes a 29th vector register)
#pragma unroll
    for (uint32_t w = 0; w < ZN_PATCH_WAVES; w++) { const uint32_t q = part[w]; if (w < wave) before += q; all += q; }
    if (i < nb) words[i] = run + before + incl - c;
    run += all;
    __syncthreads();
  }
  if (tid == 0) { words[nb] = run; totals[blockIdx.x] = run; }
}

template <uint32_t E>
__device__ __forceinline__ void zn_pa_apply_block(const ZnPatchASeg& sg, uint32_t b, uint32_t* __restrict__ status) {
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
  const uint64_t e_lo = sg.byte_lo / E, e_hi = sg.byte_hi / E, blk0 = (uint64_t)b * ZN_PATCH_BLOCK;
  bool wrong = false;
  for (uint32_t i = f0 + tid; i < f1; i += ZN_PATCH_THREADS) {
    const uint32_t o = off[i];
    const T v = val[i];
    const uint64_t el = blk0 + o;
    if (zn_patch_entry_bad(off, i, f0, o, v, el, m)) { wrong = true; continue; }
    if (el >= e_lo && el < e_hi) dst[el - e_lo] ^= v;
  }
  if (wrong) atomicOr(status, ZN_DEV_CORRUPT);
}

__global__ void __launch_bounds__(ZN_PATCH_THREADS) zn_k_patch_apply(const ZnPatchASeg one, const ZnPatchASeg* __restrict__ segs_, uint32_t nseg, uint32_t* __restrict__ status) {
  const ZnPatchASeg* segs = ZN_GLOBAL_PTR(const ZnPatchASeg, segs_);
  const ZnPatchASeg sg = zn_patch_find(one, segs, nseg, blockIdx.x);
  const uint32_t b = sg.b_lo + (blockIdx.x - sg.wg0);
  if (sg.E == 1u) zn_pa_apply_block<1>(sg, b, status);
  else if (sg.E == 2u) zn_pa_apply_block<2>(sg, b, status);
  else zn_pa_apply_block<4>(sg, b, status);
}

// ---- zn_k_patch_check: is the WHOLE patch well-formed?  Apply's header test (written out, below) and first[] test (zn_patch_format.hpp) for every block, its entry rules for
// every entry with a finding of their own each, and the canonical form apply never reads.  Reads [patch, patch + patch_len) — the header first, which bounds every later index, as in apply — and writes verdict words.
// A thread takes 8 consecutive entries per step: one 16-byte load of off[] (groups start at multiples of 8 entries; off[] is padded to a multiple of 16 bytes, so
// a group that holds an entry lies inside the patch) and the 8 E bytes of val[] in 8- or 16-byte loads where all 8 are entries (val[] has no padding behind it).
struct alignas(16) ZnPcOffs { uint16_t o[8]; };
template <uint32_t E> struct alignas(E == 1u ? 8 : 16) ZnPcVals { typename ZnPatchElem<E>::t v[8]; };

template <uint32_t E>
__device__ __forceinline__ void zn_pc_block(const ZnPatchCSeg& sg, uint32_t b, uint32_t* __restrict__ words) {
  typedef typename ZnPatchElem<E>::t T;
  const uint32_t tid = threadIdx.x;
  const uint8_t* p = ZN_GLOBAL_PTR(const uint8_t, sg.patch);
  uint32_t* verdict = words + 2u * sg.slot;
  const uint64_t n = sg.n, m = n / E, nb = zn_patch_blocks(m);                   // (the host has checked: n % E == 0, m < 2^32, patch_len >= 32, b < max(nb, 1))
  // zn_patch_header_ok's test, written out: E is the byte p[4] here — what lies in bytes 5 - 7 is a finding about the padding (below), not about the header —, and
  // through zn_patch_header this kernel takes 52 vector registers instead of 50
  const uint32_t magic = *(const uint32_t*)p, e = p[4];
  const uint64_t hn = *(const uint64_t*)(p + 8), total = *(const uint64_t*)(p + 16), len = *(const uint64_t*)(p + 24);
  bool bad = magic != ZN_PATCH_MAGIC || e != E || hn != n || total > m || len != sg.patch_len;
  if (!bad) bad = zn_patch_total(m, E, total) != len;
  if (bad) {                                     // (workgroup-uniform) nothing behind the header is read
    if (tid == 0) atomicOr(verdict, ZN_PATCH_BAD_HEADER);
    return;
  }
  const uint64_t a1 = zn_patch_a1(nb), a2 = zn_patch_a2(nb, total);
  uint32_t found = 0;
  if (b == 0) {                                  // the item's T, and the canonical form: three runs of fewer than 16 bytes
    if (tid == 0) verdict[1] = (uint32_t)total;  // (total <= m < 2^32)
    if (tid < 16u) {
      const uint64_t i1 = 32u + 4u * (nb + 1u) + tid, i2 = a1 + 2u * total + tid;
      if ((tid >= 5u && tid < 8u && p[tid]) || (i1 < a1 && p[i1]) || (i2 < a2 && p[i2])) found |= ZN_PATCH_BAD_PADDING;
    }
  }
  const uint32_t* first = (const uint32_t*)(p + 32);
  const uint32_t f0 = first[b], f1 = nb ? first[b + 1u] : f0;                    // (a tensor without elements: first[0] alone, and T == 0)
  if (zn_patch_pair_bad(f0, f1, total, b, nb)) found |= ZN_PATCH_BAD_FIRST;      // (workgroup-uniform; nb == 0: T == 0 behind the header test, and f1 is f0, which must be 0)
  else {
    const uint16_t* off = (const uint16_t*)(p + a1);
    const T* val = (const T*)(p + a2);
    const uint64_t blk0 = (uint64_t)b * ZN_PATCH_BLOCK;
    for (uint64_t g = (uint64_t)(f0 & ~7u) + 8u * tid; g < f1; g += 8u * ZN_PATCH_THREADS) {
      const ZnPcOffs og = *(const ZnPcOffs*)(off + g);
      ZnPcVals<E> vg;
      if (g + 8u <= total) vg = *(const ZnPcVals<E>*)(val + g);
      else {
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) vg.v[k] = g + k < total ? val[g + k] : (T)1;
      }
      bool have = g > f0;                        // is there an entry of this block in front of the one looked at?
      uint32_t prev = have ? (uint32_t)off[g - 1u] : 0u;
#pragma unroll
      for (uint32_t k = 0; k < 8u; k++) {
        const uint64_t i = g + k;
        if (i < f0) continue;
        const uint32_t o = og.o[k];
        if (i < f1) {
          if (blk0 + o >= m || (have && prev >= o)) found |= ZN_PATCH_BAD_OFFSET;
          if (vg.v[k] == (T)0) found |= ZN_PATCH_BAD_VALUE;
        }
        prev = o; have = true;
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) found |= __shfl_xor(found, d);
  if ((tid & 63u) == 0 && found) atomicOr(verdict, found);                       // (at most one per wave)
}

__global__ void __launch_bounds__(ZN_PATCH_THREADS) zn_k_patch_check(const ZnPatchCSeg one, const ZnPatchCSeg* __restrict__ segs_, uint32_t nseg, uint32_t* __restrict__ words_) {
  const ZnPatchCSeg* segs = ZN_GLOBAL_PTR(const ZnPatchCSeg, segs_);
  const ZnPatchCSeg sg = zn_patch_find(one, segs, nseg, blockIdx.x);
  uint32_t* words = ZN_GLOBAL_PTR(uint32_t, words_);
  const uint32_t b = blockIdx.x - sg.wg0;
  if (sg.E == 1u) zn_pc_block<1>(sg, b, words);
  else if (sg.E == 2u) zn_pc_block<2>(sg, b, words);
  else zn_pc_block<4>(sg, b, words);
}

void zn_launch_patch_count(const ZnPatchBSeg& one, const ZnPatchBSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_count, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, d_words);
  zn_note_kernel("zn_k_patch_count");
}
void zn_launch_patch_scan(const ZnPatchBSeg& one, const ZnPatchBSeg* d_segs, uint32_t nseg, uint32_t* d_words, uint64_t* d_totals, hipStream_t stream) {
  if (nseg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_scan, dim3(nseg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, d_words, d_totals);
  zn_note_kernel("zn_k_patch_scan");
}
void zn_launch_patch_emit(const ZnPatchBSeg& one, const ZnPatchBSeg* d_segs, uint32_t nseg, uint32_t total_wg, const uint32_t* d_words, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_emit, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, const_cast<uint32_t*>(d_words));
  zn_note_kernel("zn_k_patch_emit");
}
void zn_launch_patch_apply(const ZnPatchASeg& one, const ZnPatchASeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_status, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_apply, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, d_status);
  zn_note_kernel("zn_k_patch_apply");
}
void zn_launch_patch_check(const ZnPatchCSeg& one, const ZnPatchCSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_check, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, d_words);
  zn_note_kernel("zn_k_patch_check");
}

// ---- the C ABI of the patches (host side: checks, tables, launches) ----
namespace {

bool patch_aligned(const void* p, int elem) { return (((uintptr_t)p) & (uintptr_t)(elem - 1)) == 0; }

// The sizes of the patches of `items` against their bases; with `emit`: … and the patches, where every capacity suffices (zn_patch_two_pass).  An item without
// elements gets no workgroup; lens[i] == 0: the tensor's bytes are the base's.
struct PatchSrc { const void* d_src; const void* d_base; size_t n; int elem; void* d_patch; size_t cap; };
int patch_build(const std::vector<PatchSrc>& items, std::vector<uint64_t>& lens, bool emit, hipStream_t stream) {
  const size_t count = items.size();
  lens.assign(count, 0);
  if (count == 0) return ZN_OK;
  if (count > 0x7FFFFFFFull) return ZN_E_ARG;
  std::vector<ZnPatchBSeg> segs(count);
  std::vector<size_t> caps(count);
  uint64_t wg = 0, words = 0;
  for (size_t i = 0; i < count; i++) {
    const PatchSrc& it = items[i];
    if (!zn_patch_elem_ok(it.n, it.elem)) return ZN_E_ARG;
    if (it.n && (!it.d_src || !it.d_base || !patch_aligned(it.d_src, it.elem) || !patch_aligned(it.d_base, it.elem))) return ZN_E_ARG;
    if (emit && it.cap && !zn_patch_out_ok(it.d_patch)) return ZN_E_ARG;
    const uint64_t m = it.n / (size_t)it.elem;
    segs[i] = ZnPatchBSeg{(const uint8_t*)it.d_src, (const uint8_t*)it.d_base, (uint8_t*)it.d_patch, m, (uint32_t)wg, (uint32_t)words, (uint32_t)it.elem, 0u};
    caps[i] = it.cap;
    wg += zn_patch_blocks(m); words += zn_patch_blocks(m) + 1u;
    if (wg > 0x7FFFFFFFull || words > 0x7FFFFFFFull) return ZN_E_ARG;
  }
  return zn_patch_two_pass(segs, segs.data(), wg, words, emit ? caps.data() : nullptr, lens, stream,
                           [](const ZnPatchBSeg& one, const ZnPatchBSeg* d, uint32_t n, uint32_t g, uint32_t* wd, uint32_t*, hipStream_t st) { zn_launch_patch_count(one, d, n, g, wd, st); },
                           [](const ZnPatchBSeg& one, const ZnPatchBSeg* d, uint32_t n, uint32_t g, uint32_t* wd, uint32_t*, hipStream_t st) { zn_launch_patch_emit(one, d, n, g, wd, st); });
}

// what an apply call or plan works out before its first launch (S: ZnPatchASeg, or ZnPatchLSeg for the strided call, which has no copies)
template <typename S>
struct PatchSet {
  std::vector<S> segs;
  struct Copy { void* dst; const void* src; size_t n; };
  std::vector<Copy> copies;                      // items with d_base: the window's bytes of the base go to the destination first
  uint64_t total_wg = 0;
};
typedef PatchSet<ZnPatchASeg> PatchApplySet;
void patch_launch_kernel(const ZnPatchASeg& one, const ZnPatchASeg* d, uint32_t n, uint32_t wg, uint32_t* st, hipStream_t s) { zn_launch_patch_apply(one, d, n, wg, st, s); }
void patch_launch_kernel(const ZnPatchLSeg& one, const ZnPatchLSeg* d, uint32_t n, uint32_t wg, uint32_t* st, hipStream_t s) { zn_launch_patch_apply_strided(one, d, n, wg, st, s); }
int patch_apply_segments(const zn_patch_apply_item* items, size_t count, PatchApplySet& A) {
  if (count && !items) return ZN_E_ARG;
  if (count > 0x7FFFFFFFull) return ZN_E_ARG;
  A.segs.resize(count);
  for (size_t i = 0; i < count; i++) {
    const zn_patch_apply_item& it = items[i];
    if (!zn_patch_elem_ok(it.n, it.elem)) return ZN_E_ARG;
    const size_t E = (size_t)it.elem;
    if (!zn_patch_input_ok(it.d_patch, it.patch_len)) return ZN_E_ARG;
    if (it.byte_lo > it.byte_hi || it.byte_hi > it.n || it.byte_lo % E || it.byte_hi % E) return ZN_E_ARG;
    const bool empty = it.byte_lo == it.byte_hi;
    if (!empty && (!it.d_dst || !patch_aligned(it.d_dst, it.elem))) return ZN_E_ARG;
    const uint64_t b_lo = (it.byte_lo / E) / ZN_PATCH_BLOCK, b_hi = empty ? b_lo : zn_patch_blocks(it.byte_hi / E);
    A.segs[i] = ZnPatchASeg{(const uint8_t*)it.d_patch, it.patch_len, it.n, (uint8_t*)it.d_dst, it.byte_lo, it.byte_hi, (uint32_t)A.total_wg, (uint32_t)it.elem, (uint32_t)b_lo, 0u};
    A.total_wg += b_hi - b_lo;
    if (A.total_wg > 0x7FFFFFFFull) return ZN_E_ARG;
    if (!empty && it.d_base) A.copies.push_back({it.d_dst, (const uint8_t*)it.d_base + it.byte_lo, it.byte_hi - it.byte_lo});
  }
  return ZN_OK;
}

// the launches of an apply: d_table null = the table is staged through the pinned buffer (or, for one item, travels as the kernel's argument)
template <typename S>
int patch_apply_launch(const PatchSet<S>& A, const S* d_table, hipStream_t stream, int check) {
  if (A.total_wg == 0 && A.copies.empty()) return ZN_OK;
  WsLease L;
  if (L.rc) return L.rc;
  Workspace& w = *L.w;
  t_kernels.clear();
  int rc;
  const bool staged = A.segs.size() > 1 && !d_table && A.total_wg;
  const size_t table_bytes = A.segs.size() * sizeof(S);
  if ((rc = w.reserve(WS_WORDS, ZN_WORDS_BYTES))) return rc;
  if ((rc = w.host_words())) return rc;
  if (staged && (rc = w.reserve(WS_SEGS, table_bytes))) return rc;
  if ((rc = L.acquire(stream))) return rc;
  L.mark = staged;
  bool chain;
  uint32_t* d_status = zn_take_status_slot(w, L.dev, check, &chain);
  if (!chain) ZN_HIP(hipMemsetAsync(d_status, 0, 4 * sizeof(uint32_t), stream));      // (chained: the status word is the sequence's)
  for (const typename PatchSet<S>::Copy& c : A.copies)
    if (c.dst != c.src) ZN_HIP(hipMemcpyAsync(c.dst, c.src, c.n, hipMemcpyDeviceToDevice, stream));
  if (staged) {
    ZN_HIP(hipEventSynchronize(w.busy));         // the previous batched call may still be reading the pinned staging
    if ((rc = w.h_segs.reserve(table_bytes))) return rc;
    if ((rc = zn_patch_stage(w, A.segs.data(), table_bytes, 0, stream))) return rc;
    d_table = (const S*)w.buf[WS_SEGS];
  }
  if (A.total_wg) patch_launch_kernel(A.segs[0], A.segs.size() > 1 ? d_table : nullptr, (uint32_t)A.segs.size(), (uint32_t)A.total_wg, d_status, stream);
  if (launch_failed()) return ZN_E_HIP;
  if (check) {
    ZN_HIP(hipMemcpyAsync(w.h_status, d_status, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    ZN_HIP(hipStreamSynchronize(stream));
    return status_to_rc(*w.h_status);
  }
  return ZN_OK;
}

// One item of the strided call -> its segment, the layout CANONICAL (zn_patch_layout_canon: dimensions of size 1 dropped, neighbours merged where
// stride[i] == size[i + 1] stride[i + 1]; a contiguous tensor becomes one dimension of stride 1, a single element none).  What remains must be INJECTIVE by the sufficient test: sorted by stride,
// every stride exceeds the sum over the smaller ones of (size - 1) stride — each dimension steps past everything the smaller ones span —, and no stride is 0.
// That refuses expand() and overlapping as_strided views, and some injective layouts too (interleaved ones).  The largest offset stays below 2^62 elements.
int patch_strided_segment(const zn_patch_apply_strided_item& it, ZnPatchLSeg& sg, bool& contiguous) {
  if (it.ndim < 0 || it.ndim > (int)ZN_PATCH_LAYOUT_DIMS || !zn_patch_elem_ok(it.n, it.elem)) return ZN_E_ARG;
  if (!zn_patch_input_ok(it.d_patch, it.patch_len)) return ZN_E_ARG;
  if (it.n && (!it.d_dst || !patch_aligned(it.d_dst, it.elem))) return ZN_E_ARG;
  const uint64_t m = it.n / (size_t)it.elem;
  uint64_t prod = 1;
  unsigned __int128 reach = 0;                   // the last element's offset
  for (int d = 0; d < it.ndim; d++) {
    const uint64_t sz = it.size[d];
    if (it.stride[d] < 0) return ZN_E_ARG;
    if (prod && sz && prod > ~0ull / sz) return ZN_E_ARG;
    prod *= sz;
    if (sz) reach += (unsigned __int128)(sz - 1u) * (uint64_t)it.stride[d];
  }
  if (prod != m) return ZN_E_ARG;
  sg = ZnPatchLSeg{(const uint8_t*)it.d_patch, it.patch_len, it.n, (uint8_t*)it.d_dst, {}, {}, 0u, (uint32_t)it.elem, 0u, 0u};
  contiguous = true;
  if (m == 0) return ZN_OK;                      // (no element, no workgroup: nothing is written)
  if (reach >> 62) return ZN_E_ARG;
  uint64_t none[ZN_PATCH_LAYOUT_DIMS];
  const uint32_t k = zn_patch_layout_canon(it.ndim, it.size, it.stride, nullptr, sg.size, sg.stride, none);      // (every size <= m < 2^32; size stride <= 2 reach)
  sg.ndim = k;
  uint32_t order[ZN_PATCH_LAYOUT_DIMS];
  for (uint32_t i = 0; i < k; i++) order[i] = i;
  std::sort(order, order + k, [&](uint32_t a, uint32_t b) { return sg.stride[a] < sg.stride[b]; });
  uint64_t span = 0;
  for (uint32_t i = 0; i < k; i++) {
    const uint32_t d = order[i];
    if (sg.stride[d] <= span) return ZN_E_ARG;
    span += (uint64_t)(sg.size[d] - 1u) * sg.stride[d];
  }
  contiguous = k == 0 || (k == 1u && sg.stride[0] == 1u);
  return ZN_OK;
}

// The strided build: the checks of one side of an item — its strides over the item's sizes — -> the offset of its last element, in elements.
// false: a negative stride, or a last element 2^62 elements or more away.
bool patch_view_reach(const zn_patch_build_strided_item& it, const long long* stride, uint64_t& reach_out) {
  unsigned __int128 reach = 0;
  for (int d = 0; d < it.ndim; d++) {
    if (stride[d] < 0) return false;
    if (it.size[d]) reach += (unsigned __int128)(it.size[d] - 1u) * (uint64_t)stride[d];
  }
  if (it.n && (reach >> 62)) return false;
  reach_out = it.n ? (uint64_t)reach : 0u;
  return true;
}

// The sizes of the patches of strided sources against strided bases; with `emit`: … and the patches (patch_build's counterpart).  Sources are only read: a
// stride of 0 and overlapping views are accepted.  A batch whose items all collapse to contiguous tensors on both sides takes patch_build's launches.
int patch_build_strided(const zn_patch_build_strided_item* items, size_t count, std::vector<uint64_t>& lens, bool emit, hipStream_t stream) {
  lens.assign(count, 0);
  if (count == 0) return ZN_OK;
  if (count > 0x7FFFFFFFull) return ZN_E_ARG;
  std::vector<ZnPatchGSeg> segs(count);
  std::vector<ZnPatchBSeg> scan(count);
  std::vector<size_t> caps(count);
  uint64_t wg = 0, words = 0;
  bool all_contiguous = true;
  for (size_t i = 0; i < count; i++) {
    const zn_patch_build_strided_item& it = items[i];
    if (it.ndim < 0 || it.ndim > (int)ZN_PATCH_LAYOUT_DIMS || !zn_patch_elem_ok(it.n, it.elem)) return ZN_E_ARG;
    const uint64_t m = it.n / (size_t)it.elem;
    uint64_t prod = 1, sreach, breach;
    for (int d = 0; d < it.ndim; d++) {
      const uint64_t sz = it.size[d];
      if (prod && sz && prod > ~0ull / sz) return ZN_E_ARG;
      prod *= sz;
    }
    if (prod != m) return ZN_E_ARG;
    if (!patch_view_reach(it, it.src_stride, sreach) || !patch_view_reach(it, it.base_stride, breach)) return ZN_E_ARG;
    if (it.n && (!it.d_src || !it.d_base || !patch_aligned(it.d_src, it.elem) || !patch_aligned(it.d_base, it.elem))) return ZN_E_ARG;
    if (emit && it.patch_cap) {
      if (!zn_patch_out_ok(it.d_patch)) return ZN_E_ARG;
      if (it.n && (zn_patch_overlap(it.d_patch, it.patch_cap, it.d_src, (size_t)(sreach + 1u) * (size_t)it.elem) ||
                   zn_patch_overlap(it.d_patch, it.patch_cap, it.d_base, (size_t)(breach + 1u) * (size_t)it.elem))) return ZN_E_ARG;
    }
    ZnPatchGSeg& sg = segs[i];
    sg = ZnPatchGSeg{(const uint8_t*)it.d_src, (const uint8_t*)it.d_base, (uint8_t*)it.d_patch, m, {}, {}, {}, (uint32_t)wg, (uint32_t)words, (uint32_t)it.elem, 0u, 0u, 0u};
    if (m) {                                     // (every size is in 1 .. m < 2^32)
      sg.ndim = zn_patch_layout_canon(it.ndim, it.size, it.src_stride, it.base_stride, sg.size, sg.sstride, sg.bstride);
      for (uint32_t d = 0; d < sg.ndim; d++) {   // the dimension memory is followed along: the smallest non-zero source stride, ties by the base's
        const uint64_t ks = sg.sstride[d] ? sg.sstride[d] : ~0ull, kb = sg.bstride[d] ? sg.bstride[d] : ~0ull;
        const uint64_t fs = sg.sstride[sg.fast] ? sg.sstride[sg.fast] : ~0ull, fb = sg.bstride[sg.fast] ? sg.bstride[sg.fast] : ~0ull;
        if (ks < fs || (ks == fs && kb < fb)) sg.fast = d;
      }
      all_contiguous = all_contiguous && (sg.ndim == 0 || (sg.ndim == 1u && sg.sstride[0] == 1u && sg.bstride[0] == 1u));
    }
    scan[i] = ZnPatchBSeg{nullptr, nullptr, nullptr, m, 0u, (uint32_t)words, (uint32_t)it.elem, 0u};
    caps[i] = it.patch_cap;
    wg += zn_patch_blocks(m); words += zn_patch_blocks(m) + 1u;
    if (wg > 0x7FFFFFFFull || words > 0x7FFFFFFFull) return ZN_E_ARG;
  }
  if (all_contiguous) {                          // every layout collapsed to the tensor itself: the contiguous launches
    std::vector<PatchSrc> plain(count);
    for (size_t i = 0; i < count; i++) plain[i] = PatchSrc{items[i].d_src, items[i].d_base, items[i].n, items[i].elem, items[i].d_patch, items[i].patch_cap};
    return patch_build(plain, lens, emit, stream);
  }
  return zn_patch_two_pass(segs, scan.data(), wg, words, emit ? caps.data() : nullptr, lens, stream,
                           [](const ZnPatchGSeg& one, const ZnPatchGSeg* d, uint32_t n, uint32_t g, uint32_t* wd, uint32_t*, hipStream_t st) { zn_launch_patch_count_strided(one, d, n, g, wd, st); },
                           [](const ZnPatchGSeg& one, const ZnPatchGSeg* d, uint32_t n, uint32_t g, uint32_t* wd, uint32_t*, hipStream_t st) { zn_launch_patch_emit_strided(one, d, n, g, wd, st); });
}

}  // namespace

// A prepared apply: the segments, the base copies, and the table in device memory of its own (zn_plan's counterpart for patches).
struct zn_patch_plan {
  PatchApplySet A;
  ZnPatchASeg* d_table = nullptr;
  hipEvent_t last = nullptr;
  bool ran = false;
  int dev = 0;
  ~zn_patch_plan() {
    if (d_table) (void)hipFree(d_table);
    if (last) (void)hipEventDestroy(last);
  }
};

extern "C" {

size_t zn_patch_len(size_t n, int elem, size_t entries) {
  if (!zn_patch_elem_ok(n, elem) || entries > n / (size_t)elem) return 0;
  return (size_t)zn_patch_total(n / (size_t)elem, (uint32_t)elem, entries);
}

int zn_patch_size_batch_dev(const zn_patch_size_item* items, size_t count, size_t* sizes_out, void* stream_) {
  try {
    if (count == 0) return ZN_OK;
    if (!items || !sizes_out) return ZN_E_ARG;
    std::vector<PatchSrc> src(count);
    for (size_t i = 0; i < count; i++) src[i] = PatchSrc{items[i].d_src, items[i].d_base, items[i].n, items[i].elem, nullptr, 0};
    std::vector<uint64_t> lens;
    const int rc = patch_build(src, lens, false, (hipStream_t)stream_);
    if (rc) return rc;
    for (size_t i = 0; i < count; i++) sizes_out[i] = (size_t)lens[i];
    return ZN_OK;
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_patch_build_batch_dev(zn_patch_build_item* items, size_t count, void* stream_) {
  try {
    if (count == 0) return ZN_OK;
    if (!items) return ZN_E_ARG;
    std::vector<PatchSrc> src(count);
    for (size_t i = 0; i < count; i++) { src[i] = PatchSrc{items[i].d_src, items[i].d_base, items[i].n, items[i].elem, items[i].d_patch, items[i].patch_cap}; items[i].patch_len = 0; }
    std::vector<uint64_t> lens;
    const int rc = patch_build(src, lens, true, (hipStream_t)stream_);
    if (rc == ZN_OK || rc == ZN_E_CAP) for (size_t i = 0; i < count; i++) items[i].patch_len = (size_t)lens[i];      // (ZN_E_CAP: the lengths that were needed; nothing was written)
    return rc;
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_patch_apply_batch_dev(const zn_patch_apply_item* items, size_t count, void* stream_, int check) {
  try {
    PatchApplySet A;
    const int rc = patch_apply_segments(items, count, A);
    return rc ? rc : patch_apply_launch<ZnPatchASeg>(A, nullptr, (hipStream_t)stream_, check);
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_patch_apply_strided_batch_dev(const zn_patch_apply_strided_item* items, size_t count, void* stream_, int check) {
  try {
    if (count && !items) return ZN_E_ARG;
    if (count > 0x7FFFFFFFull) return ZN_E_ARG;
    PatchSet<ZnPatchLSeg> A;
    A.segs.resize(count);
    bool all_contiguous = true;
    for (size_t i = 0; i < count; i++) {
      bool contiguous;
      const int rc = patch_strided_segment(items[i], A.segs[i], contiguous);
      if (rc) return rc;
      all_contiguous = all_contiguous && contiguous;
      A.segs[i].wg0 = (uint32_t)A.total_wg;
      A.total_wg += zn_patch_blocks(items[i].n / (size_t)items[i].elem);
      if (A.total_wg > 0x7FFFFFFFull) return ZN_E_ARG;
    }
    if (!all_contiguous) return patch_apply_launch<ZnPatchLSeg>(A, nullptr, (hipStream_t)stream_, check);
    // every layout collapsed to the tensor itself: the contiguous launch, whole windows in place
    std::vector<zn_patch_apply_item> plain(count);
    for (size_t i = 0; i < count; i++) plain[i] = zn_patch_apply_item{items[i].d_patch, items[i].patch_len, items[i].n, items[i].elem, 0u, items[i].n, items[i].d_dst, nullptr};
    PatchApplySet P;
    const int rc = patch_apply_segments(plain.data(), count, P);
    return rc ? rc : patch_apply_launch<ZnPatchASeg>(P, nullptr, (hipStream_t)stream_, check);
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_patch_size_strided_batch_dev(const zn_patch_build_strided_item* items, size_t count, size_t* sizes_out, void* stream_) {
  try {
    if (count == 0) return ZN_OK;
    if (!items || !sizes_out) return ZN_E_ARG;
    std::vector<uint64_t> lens;
    const int rc = patch_build_strided(items, count, lens, false, (hipStream_t)stream_);
    if (rc) return rc;
    for (size_t i = 0; i < count; i++) sizes_out[i] = (size_t)lens[i];
    return ZN_OK;
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_patch_build_strided_batch_dev(zn_patch_build_strided_item* items, size_t count, void* stream_) {
  try {
    if (count == 0) return ZN_OK;
    if (!items) return ZN_E_ARG;
    for (size_t i = 0; i < count; i++) items[i].patch_len = 0;
    std::vector<uint64_t> lens;
    const int rc = patch_build_strided(items, count, lens, true, (hipStream_t)stream_);
    if (rc == ZN_OK || rc == ZN_E_CAP) for (size_t i = 0; i < count; i++) items[i].patch_len = (size_t)lens[i];      // (ZN_E_CAP: the lengths that were needed; nothing was written)
    return rc;
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_patch_check_batch_dev(const zn_patch_check_item* items, size_t count, unsigned int* verdicts_out, unsigned long long* entries_out, void* stream_) {
  try {
    if (count == 0) return ZN_OK;
    if (!items || !verdicts_out || count > 0x7FFFFFFFull) return ZN_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<ZnPatchCSeg> segs(count);
    uint64_t wg = 0;
    for (size_t i = 0; i < count; i++) {
      const zn_patch_check_item& it = items[i];
      if (!zn_patch_elem_ok(it.n, it.elem)) return ZN_E_ARG;
      if (!zn_patch_input_ok(it.d_patch, it.patch_len)) return ZN_E_ARG;
      const uint64_t nb = zn_patch_blocks(it.n / (size_t)it.elem);
      segs[i] = ZnPatchCSeg{(const uint8_t*)it.d_patch, it.patch_len, it.n, (uint32_t)wg, (uint32_t)it.elem, (uint32_t)i, 0u};
      wg += nb ? nb : 1u;                        // (a tensor without elements still has a header and first[0])
      if (wg > 0x7FFFFFFFull) return ZN_E_ARG;
    }
    WsLease L;
    if (L.rc) return L.rc;
    Workspace& w = *L.w;
    t_kernels.clear();
    int rc;
    const bool table = count > 1;
    const size_t table_bytes = table ? count * sizeof(ZnPatchCSeg) : 0u, word_bytes = count * 2u * sizeof(uint32_t);
    if ((rc = w.reserve(WS_TOTALS, word_bytes))) return rc;
    if ((rc = w.h_totals.reserve(word_bytes))) return rc;
    if (table && (rc = w.reserve(WS_SEGS, table_bytes))) return rc;
    if ((rc = L.acquire(stream))) return rc;
    L.mark = table;
    uint32_t* d_words = (uint32_t*)w.buf[WS_TOTALS];
    ZN_HIP(hipMemsetAsync(d_words, 0, word_bytes, stream));
    if (table) {
      ZN_HIP(hipEventSynchronize(w.busy));       // the previous batched call may still be reading the pinned staging
      if ((rc = w.h_segs.reserve(table_bytes))) return rc;
      if ((rc = zn_patch_stage(w, segs.data(), table_bytes, 0, stream))) return rc;
    }
    zn_launch_patch_check(segs[0], table ? (const ZnPatchCSeg*)w.buf[WS_SEGS] : nullptr, (uint32_t)count, (uint32_t)wg, d_words, stream);
    if (launch_failed()) return ZN_E_HIP;
    ZN_HIP(hipMemcpyAsync(w.h_totals.p, d_words, word_bytes, hipMemcpyDeviceToHost, stream));
    ZN_HIP(hipStreamSynchronize(stream));
    const uint32_t* got = (const uint32_t*)w.h_totals.p;
    for (size_t i = 0; i < count; i++) {
      verdicts_out[i] = got[2u * i];
      if (entries_out) entries_out[i] = got[2u * i] ? 0ull : (unsigned long long)got[2u * i + 1u];
    }
    return ZN_OK;
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_patch_plan_create(const zn_patch_apply_item* items, size_t count, zn_patch_plan** plan) {
  if (!plan) return ZN_E_ARG;
  *plan = nullptr;
  try {
    int dev = 0, rc = zn_current_dev(&dev);
    if (rc) return rc;
    std::unique_ptr<zn_patch_plan> pl(new zn_patch_plan());
    pl->dev = dev;
    if ((rc = patch_apply_segments(items, count, pl->A))) return rc;
    if (pl->A.segs.size() > 1) {
      const size_t bytes = pl->A.segs.size() * sizeof(ZnPatchASeg);
      hipError_t e = hipMalloc((void**)&pl->d_table, bytes);
      if (e != hipSuccess) { pl->d_table = nullptr; t_hip_err = std::string("hipMalloc: ") + hipGetErrorString(e); (void)hipGetLastError(); return ZN_E_ALLOC; }
      ZN_HIP(hipMemcpy(pl->d_table, pl->A.segs.data(), bytes, hipMemcpyHostToDevice));
    }
    ZN_HIP(hipEventCreateWithFlags(&pl->last, hipEventDisableTiming));
    *plan = pl.release();
    return ZN_OK;
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_patch_plan_run(zn_patch_plan* plan, void* stream_, int check) {
  if (!plan) return ZN_E_ARG;
  try {
    int dev = 0;
    ZN_HIP(hipGetDevice(&dev));
    if (dev != plan->dev) return ZN_E_ARG;
    const int rc = patch_apply_launch(plan->A, plan->d_table, (hipStream_t)stream_, check);
    if (plan->d_table) { if (hipEventRecord(plan->last, (hipStream_t)stream_) == hipSuccess) plan->ran = true; else { (void)hipGetLastError(); (void)hipDeviceSynchronize(); } }
    return rc;
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_patch_plan_destroy(zn_patch_plan* plan) {
  if (!plan) return ZN_OK;
  int rc = ZN_OK;
  {
    DeviceScope scope(plan->dev);
    if (!scope.ok || (plan->ran && hipEventSynchronize(plan->last) != hipSuccess)) { t_hip_err = "zn_patch_plan_destroy"; (void)hipGetLastError(); (void)hipDeviceSynchronize(); rc = ZN_E_HIP; }
    delete plan;
  }
  return rc;
}

}  // extern "C"
