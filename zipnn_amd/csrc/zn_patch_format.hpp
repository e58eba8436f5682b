// zn_patch_format.hpp — the "znp1" patch format (include/zipnn_hip.h) in ONE place: its constants and layout, the items of the patch launches, and
// the device-side tests every kernel that reads or writes a patch goes through.  Included by the four patch units (zn_patch.hip, zn_patch_merge.hip,
// zn_patch_select.hip, zn_patch_strided.hip) and nobody else; the host side of their entry points is zn_patch_host.hpp.
#pragma once

#include "zn_common.hpp"

#define ZN_PATCH_BLOCK 65536u                // elements per block — part of the format's DEFINITION
#define ZN_PATCH_MAGIC 0x31504E5Au           // "ZNP1", little-endian
#define ZN_PATCH_THREADS 256u                // every patch kernel's workgroup
#define ZN_PATCH_WAVES (ZN_PATCH_THREADS / 64u)
// header (32 bytes: magic, E, n, T, L), first[NB + 1], padding to 16, off[T], padding to 16, val[T]
__host__ __device__ static inline uint64_t zn_patch_blocks(uint64_t m) { return (m + ZN_PATCH_BLOCK - 1u) / ZN_PATCH_BLOCK; }
__host__ __device__ static inline uint64_t zn_patch_a1(uint64_t nb) { return (32u + 4u * (nb + 1u) + 15u) & ~15ull; }
__host__ __device__ static inline uint64_t zn_patch_a2(uint64_t nb, uint64_t T) { return (zn_patch_a1(nb) + 2u * T + 15u) & ~15ull; }
__host__ __device__ static inline uint64_t zn_patch_total(uint64_t m, uint32_t E, uint64_t T) { return zn_patch_a2(zn_patch_blocks(m), T) + (uint64_t)E * T; }

// ---- build, apply, check : zn_patch.hip ----
// One item of a count / emit launch: m elements of E bytes at src against base; its first workgroup (one per block, none for an empty item); where its NB + 1
// words start in the launch's scratch words (count: entries of block b; behind the scan: first[]).  patch: where the emit pass writes (16-byte aligned).
struct ZnPatchBSeg { const uint8_t* src; const uint8_t* base; uint8_t* patch; uint64_t m; uint32_t wg0; uint32_t w0; uint32_t E; uint32_t pad_; };
// One item of an apply launch: the patch, the tensor it describes (n bytes, E per element), the byte window [byte_lo, byte_hi) and where the window's first byte
// lies (dst); its first workgroup — one per block the window touches, the first of them block b_lo.
struct ZnPatchASeg { const uint8_t* patch; uint64_t patch_len; uint64_t n; uint8_t* dst; uint64_t byte_lo, byte_hi; uint32_t wg0; uint32_t E; uint32_t b_lo; uint32_t pad_; };
// `one` when d_segs == nullptr, else the table (a workgroup finds its item by binary search over wg0).  d_words: the launch's scratch words.
void zn_launch_patch_count(const ZnPatchBSeg& one, const ZnPatchBSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, hipStream_t stream);
void zn_launch_patch_scan(const ZnPatchBSeg& one, const ZnPatchBSeg* d_segs, uint32_t nseg, uint32_t* d_words, uint64_t* d_totals, hipStream_t stream);    // d_totals[i] = T of item i
void zn_launch_patch_emit(const ZnPatchBSeg& one, const ZnPatchBSeg* d_segs, uint32_t nseg, uint32_t total_wg, const uint32_t* d_words, hipStream_t stream);
void zn_launch_patch_apply(const ZnPatchASeg& one, const ZnPatchASeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_status, hipStream_t stream);
// One item of a check launch (zn_k_patch_check): the patch and the tensor it claims to describe; its first workgroup — one per block, one for a tensor without
// elements — and its slot of the launch's verdict words: d_words[2 slot] collects the ZN_PATCH_BAD_* bits, d_words[2 slot + 1] receives the header's T.
struct ZnPatchCSeg { const uint8_t* patch; uint64_t patch_len; uint64_t n; uint32_t wg0; uint32_t E; uint32_t slot; uint32_t pad_; };
void zn_launch_patch_check(const ZnPatchCSeg& one, const ZnPatchCSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, hipStream_t stream);
// ---- the XOR-merge of two patches : zn_patch_merge.hip ----
// One item of a merge launch: the two patches of one tensor of m elements of E bytes, where the emit pass writes (16-byte aligned); its first workgroup — one per
// block, one for a tensor without elements — and where its NB + 1 words start in the launch's scratch words (as ZnPatchBSeg's: the scan between the passes is
// zn_k_patch_scan, over a ZnPatchBSeg table with the same m and w0).  d_status: one word, ZN_DEV_CORRUPT when an input is malformed.
struct ZnPatchMSeg { const uint8_t* a; uint64_t a_len; const uint8_t* b; uint64_t b_len; uint8_t* out; uint64_t m; uint32_t wg0; uint32_t w0; uint32_t E; uint32_t pad_; };
void zn_launch_patch_merge_count(const ZnPatchMSeg& one, const ZnPatchMSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, uint32_t* d_status, hipStream_t stream);
void zn_launch_patch_merge_emit(const ZnPatchMSeg& one, const ZnPatchMSeg* d_segs, uint32_t nseg, uint32_t total_wg, const uint32_t* d_words, uint32_t* d_status, hipStream_t stream);
// ---- a patch restricted to a rectangle of its tensor, and embedded back : zn_patch_select.hip ----
// One item of a select / place launch: the input patch, where the emit pass writes (16-byte aligned), the WHOLE tensor as R x C elements of E bytes and the
// rectangle rows [r0, r1) x cols [c0, c1) of it (not empty, inside, R C < 2^32).  SELECT: the input covers the tensor, the output the rectangle; PLACE: the other
// way round.  Its first workgroup — one per OUTPUT block — and where the output's NB + 1 words start in the launch's scratch words (the scan between the passes is
// zn_k_patch_scan, over a ZnPatchBSeg table with the output's m and the same w0).  d_status: one word, ZN_DEV_CORRUPT when an input is malformed.
struct ZnPatchSSeg { const uint8_t* in; uint64_t in_len; uint8_t* out; uint32_t R, C, r0, r1, c0, c1; uint32_t wg0; uint32_t w0; uint32_t E; uint32_t pad_; };
void zn_launch_patch_select_count(bool place, const ZnPatchSSeg& one, const ZnPatchSSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, uint32_t* d_status, hipStream_t stream);
void zn_launch_patch_select_emit(bool place, const ZnPatchSSeg& one, const ZnPatchSSeg* d_segs, uint32_t nseg, uint32_t total_wg, const uint32_t* d_words, uint32_t* d_status, hipStream_t stream);
// ---- a patch applied through a strided layout : zn_patch_strided.hip ----
#define ZN_PATCH_LAYOUT_DIMS 8u              // ZN_PATCH_MAX_DIMS of include/zipnn_hip.h
// Where element e of the logical row-major order lies, in elements from logical element 0: e unravelled over size[0 .. ndim) (the last dimension fastest) and
// dotted with the strides.  e < the product of the sizes, which is below 2^32, so every quotient fits 32 bits and the divisions are 32-bit ones (there is no
// hardware integer divide: a 64-bit one costs several times a 32-bit one); only the products with the strides are 64-bit — a view of a large buffer spans more
// than 2^32 elements.  Dimension 0 needs no division: what is left of e is its coordinate.  The loop is unrolled over constant indices, so that sizes and
// strides — wave-uniform in the kernel — stay in registers.  Touches no memory: the stand-alone host test calls it with layouts that have none behind them.
__host__ __device__ static inline uint64_t zn_patch_layout_offset(uint32_t ndim, const uint32_t (&size)[ZN_PATCH_LAYOUT_DIMS], const uint64_t (&stride)[ZN_PATCH_LAYOUT_DIMS], uint32_t e) {
  uint64_t at = 0;
#pragma unroll
  for (uint32_t d = ZN_PATCH_LAYOUT_DIMS - 1u; d >= 1u; d--)
    if (d < ndim) {
      const uint32_t q = e / size[d];
      at += (uint64_t)(e - q * size[d]) * stride[d];
      e = q;
    }
  if (ndim) at += (uint64_t)e * stride[0];
  return at;
}
// One item of a strided apply launch: the patch, the tensor it describes (n bytes, E per element), where LOGICAL element 0 lies (dst) and the layout as the host
// has collapsed it (ndim <= 8 dimensions, no size 1, no stride 0, injective; the sizes' product is n / E); its first workgroup — one per block of the tensor.
struct ZnPatchLSeg { const uint8_t* patch; uint64_t patch_len; uint64_t n; uint8_t* dst; uint64_t stride[ZN_PATCH_LAYOUT_DIMS]; uint32_t size[ZN_PATCH_LAYOUT_DIMS]; uint32_t wg0; uint32_t E; uint32_t ndim; uint32_t pad_; };
void zn_launch_patch_apply_strided(const ZnPatchLSeg& one, const ZnPatchLSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_status, hipStream_t stream);
// Two layouts over ONE logical shape made canonical together (the strided apply has one: sb == nullptr): dimensions of size 1 dropped, neighbours merged where
// stride[i] == size[i + 1] stride[i + 1] in BOTH lists.  The caller has checked: ndim <= 8, no stride negative, every size in 1 .. 2^32 - 1.  -> the number of
// dimensions left (a contiguous tensor: one, of stride 1; a single element: none).  Touches no memory.
static inline uint32_t zn_patch_layout_canon(int ndim, const unsigned long long* size, const long long* sa, const long long* sb, uint32_t (&osize)[ZN_PATCH_LAYOUT_DIMS],
                                             uint64_t (&osa)[ZN_PATCH_LAYOUT_DIMS], uint64_t (&osb)[ZN_PATCH_LAYOUT_DIMS]) {
  uint32_t k = 0;
  for (int d = 0; d < ndim; d++) {
    const uint64_t sz = size[d], a = (uint64_t)sa[d], b = sb ? (uint64_t)sb[d] : 0u;
    if (sz == 1u) continue;
    if (k && osa[k - 1u] == sz * a && (!sb || osb[k - 1u] == sz * b)) { osize[k - 1u] *= (uint32_t)sz; osa[k - 1u] = a; osb[k - 1u] = b; }
    else { osize[k] = (uint32_t)sz; osa[k] = a; osb[k] = b; k++; }
  }
  return k;
}
// ---- a patch built from strided sources : zn_patch_strided.hip ----
// One item of a strided count / emit launch: ZnPatchBSeg's fields, the logical shape as the host has made it canonical jointly for both sides (ndim <= 8, no
// size 1; a stride may be 0: sources are only read) with the source's and the base's strides over it, and `fast`: the dimension along which memory is followed
// (the smallest non-zero source stride, ties by the base's).  src / base: where LOGICAL element 0 of each lies.
struct ZnPatchGSeg {
  const uint8_t* src; const uint8_t* base; uint8_t* patch; uint64_t m;
  uint64_t sstride[ZN_PATCH_LAYOUT_DIMS], bstride[ZN_PATCH_LAYOUT_DIMS]; uint32_t size[ZN_PATCH_LAYOUT_DIMS];
  uint32_t wg0; uint32_t w0; uint32_t E; uint32_t ndim; uint32_t fast; uint32_t pad_;
};
void zn_launch_patch_count_strided(const ZnPatchGSeg& one, const ZnPatchGSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, hipStream_t stream);
void zn_launch_patch_emit_strided(const ZnPatchGSeg& one, const ZnPatchGSeg* d_segs, uint32_t nseg, uint32_t total_wg, const uint32_t* d_words, hipStream_t stream);
// What zn_patch_two_pass (zn_patch_host.hpp) asks of a segment type.  reads_patches: its inputs are patches, which may be malformed — the passes get a verdict
// word.  The builds read tensors: none.
template <typename S> struct ZnPatchSegTraits { static constexpr bool reads_patches = true; };
template <> struct ZnPatchSegTraits<ZnPatchBSeg> { static constexpr bool reads_patches = false; };
template <> struct ZnPatchSegTraits<ZnPatchGSeg> { static constexpr bool reads_patches = false; };

#if defined(__HIPCC__) || defined(ZN_SIMT_EMULATOR)
template <uint32_t E> struct ZnPatchElem;
template <> struct ZnPatchElem<1> { typedef uint8_t t; };
template <> struct ZnPatchElem<2> { typedef uint16_t t; };
template <> struct ZnPatchElem<4> { typedef uint32_t t; };

// which item of a batched launch does workgroup `b` belong to?  (last segment with wg0 <= b; wave-uniform)
template <typename S>
__device__ __forceinline__ S zn_patch_find(const S& one, const S* __restrict__ segs, uint32_t nseg, uint32_t b) {
  if (segs == nullptr) return one;
  uint32_t lo = 0, hi = nseg;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (segs[mid].wg0 <= b) lo = mid; else hi = mid; }
  return segs[lo];
}

// inclusive sum over the lanes of a wave (lane 63 holds the wave's total)
__device__ __forceinline__ uint32_t zn_patch_wave_incl(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t t = __shfl_up(v, d); if (lane >= d) v += t; }
  return v;
}
// … and across the workgroup: part[w] = wave w's total (visible: a barrier lies behind the writes) -> the sum of the waves in front of `wave`, and of all
// (zn_k_patch_scan has the loop written out: through this helper it takes a 29th vector register)
__device__ __forceinline__ void zn_patch_wave_sums(const uint32_t* part, uint32_t wave, uint32_t& before, uint32_t& all) {
  before = 0; all = 0;
#pragma unroll
  for (uint32_t w = 0; w < ZN_PATCH_WAVES; w++) { const uint32_t q = part[w]; if (w < wave) before += q; all += q; }
}

// A block's 65 536 possible offsets as a bitmap in LDS (the merge; the strided build, §3.16): 2 048 words, 8 per thread of a prefix pass
#define ZN_PM_WORDS (ZN_PATCH_BLOCK / 32u)
#define ZN_PM_PER (ZN_PM_WORDS / ZN_PATCH_THREADS)      // bitmap words per thread of a prefix pass
// pref[w] = the set bits of bm[0 .. w) -> the set bits of the whole bitmap.  Every thread of the workgroup; the bitmap is complete and visible on entry, pref
// is on return.
__device__ __forceinline__ uint32_t zn_pm_prefix(const uint32_t* bm, uint16_t* pref, uint32_t* part) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t c[ZN_PM_PER], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < ZN_PM_PER; k++) { c[k] = (uint32_t)__popc(bm[tid * ZN_PM_PER + k]); sum += c[k]; }
  const uint32_t incl = zn_patch_wave_incl(sum, lane);
  if (lane == 63u) part[wave] = incl;
  __syncthreads();
  uint32_t before, all;
  zn_patch_wave_sums(part, wave, before, all);
  uint32_t run = before + incl - sum;
#pragma unroll
  for (uint32_t k = 0; k < ZN_PM_PER; k++) { pref[tid * ZN_PM_PER + k] = (uint16_t)run; run += c[k]; }      // (run <= 65 504 at a word's start)
  __syncthreads();
  return all;
}

// The 32 header bytes as they lie there.  (zn_k_patch_check reads them itself: to it E is the byte at offset 4, and the three above it are padding with a finding of its own.)
struct ZnPatchHdr { uint32_t magic, e; uint64_t n, total, len; };
__device__ __forceinline__ ZnPatchHdr zn_patch_header(const uint8_t* p) {
  return ZnPatchHdr{*(const uint32_t*)p, *(const uint32_t*)(p + 4), *(const uint64_t*)(p + 8), *(const uint64_t*)(p + 16), *(const uint64_t*)(p + 24)};
}
// The header must describe the item (n bytes, m elements of E), and its L — the formula's value for its T — must be the length we were given: every index below
// T then lies inside [p, p + len).  -> false: nothing behind the header may be read.  (workgroup-uniform)
template <uint32_t E>
__device__ __forceinline__ bool zn_patch_header_ok(const ZnPatchHdr h, uint64_t n, uint64_t m, uint64_t len, uint64_t& T) {
  T = h.total;
  if (h.magic != ZN_PATCH_MAGIC || h.e != E || h.n != n || h.total > m || h.len != len) return false;
  return zn_patch_total(m, E, h.total) == h.len;
}
// first[b], first[b + 1] of a patch of nb blocks and T entries: ascending, inside T, first[0] == 0, first[nb] == T.  (nb == 0, the check's tensor without elements, whose one
// word the caller passes twice: the last clause cannot fire and need not — T is 0 behind the header test, and the word must be 0.)
__device__ __forceinline__ bool zn_patch_pair_bad(uint32_t f0, uint32_t f1, uint64_t T, uint32_t b, uint64_t nb) {
  return f0 > f1 || (uint64_t)f1 > T || (b == 0 && f0 != 0u) || ((uint64_t)b + 1u == nb && (uint64_t)f1 != T);
}
// entry i of a block whose entries start at f0: offset o (element el of m), value v — inside the tensor, not zero, strictly above its predecessor
template <typename V, typename I>
__device__ __forceinline__ bool zn_patch_entry_bad(const uint16_t* off, I i, uint32_t f0, uint32_t o, V v, uint64_t el, uint64_t m) {
  return el >= m || v == (V)0 || (i > f0 && (uint32_t)off[i - 1u] >= o);
}

// What ONE thread of the workgroup of output block b writes beside the block's entries: first[b] = lo, the closing first[nb] = T; block 0: the header, and
// the zero padding in front of off[] and of val[]
template <uint32_t E>
__device__ __forceinline__ void zn_patch_emit_head(uint8_t* p, uint64_t m, uint64_t nb, uint64_t T, uint32_t b, uint32_t lo) {
  const uint64_t a1 = zn_patch_a1(nb), a2 = zn_patch_a2(nb, T);
  uint32_t* first = (uint32_t*)(p + 32);
  first[b] = lo;
  if ((uint64_t)b + 1u == nb) first[nb] = (uint32_t)T;
  if (b == 0) {
    *(uint32_t*)p = ZN_PATCH_MAGIC; *(uint32_t*)(p + 4) = E;
    *(uint64_t*)(p + 8) = m * E; *(uint64_t*)(p + 16) = T; *(uint64_t*)(p + 24) = a2 + (uint64_t)E * T;
    for (uint64_t i = 32u + 4u * (nb + 1u); i < a1; i++) p[i] = 0;
    for (uint64_t i = a1 + 2u * T; i < a2; i++) p[i] = 0;
  }
}
#endif
