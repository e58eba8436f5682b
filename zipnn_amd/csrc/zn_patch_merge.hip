// zn_patch_merge.hip — the XOR-merge of two "znp1" patches over one tensor (include/zipnn_hip.h): the union of their entries, the values XORed
// where both have one, what cancels to zero dropped.  merge(patch(A, base), patch(B, base)) is patch(B, A), byte for byte, without either tensor.
//
//   zn_k_patch_merge_count   one workgroup per block of 65 536 elements: how many entries the merged block keeps (one word per block)
//   zn_k_patch_scan          (zn_patch.hip, as it is) the block counts become first[], the item's T goes to its total
//   zn_k_patch_merge_emit    one workgroup per block again: off / val of the kept entries at first[b] + rank, in ascending order; block 0 writes the header
//
// Count and emit are ONE body (zn_pm_block<E, EMIT>).  A block's 65 536 possible offsets are 2 048 words of bitmap in LDS: every entry of A and of B sets its
// bit (bmA, bmB); keep = bmA | bmB less the bits of entries whose values cancel; an exclusive popcount prefix per word (u16: a word starts at rank <= 65 504)
// turns a bit into a rank — of an offset among B's entries (where its value lies) and among the kept ones (where it goes).  Ranks ascend with the offset, so the
// output is in element order without a sort.  LDS: three bitmaps of 8 KiB and two prefix arrays of 4 KiB, 32 KiB per workgroup.
// The kernels trust nothing: an input may come from anywhere.  They read only inside [x, x + x_len) — the header first, whose L must be x_len and the formula's
// value for its T, which bounds every later index — and every block of both inputs is visited by the count pass, so a merge that returns ZN_OK has seen both
// inputs whole: offsets inside the tensor and strictly ascending, no zero value.  The emit instance never writes outside [first[b], first[b + 1]) of off / val:
// if an input changed between the two passes the result is wrong, not the memory around it.
#include "zn_workspace.hpp"

#include <vector>

#define ZN_PM_THREADS 256u
#define ZN_PM_WAVES (ZN_PM_THREADS / 64u)
#define ZN_PM_WORDS (ZN_PATCH_BLOCK / 32u)
#define ZN_PM_PER (ZN_PM_WORDS / ZN_PM_THREADS)      // bitmap words per thread of a prefix pass

template <uint32_t E> struct ZnPmElem;
template <> struct ZnPmElem<1> { typedef uint8_t t; };
template <> struct ZnPmElem<2> { typedef uint16_t t; };
template <> struct ZnPmElem<4> { typedef uint32_t t; };

struct ZnPmLds {
  uint32_t bmA[ZN_PM_WORDS], bmB[ZN_PM_WORDS], keep[ZN_PM_WORDS];
  uint16_t prefB[ZN_PM_WORDS], prefK[ZN_PM_WORDS];
  uint32_t part[ZN_PM_WAVES];
  uint32_t wrong;
};

// one input's part of a block: its entries [f0, f1) of off[] / val[]
template <typename T> struct ZnPmIn { const uint16_t* off; const T* val; uint32_t f0, f1; };

// The header must describe the item, and its L — the formula's value for its T — must be the length we were given: every index below T then lies inside.
// Then the block's pair of first[]; more entries than the block has elements cannot ascend.  (workgroup-uniform)
template <uint32_t E>
__device__ __forceinline__ bool zn_pm_open(const uint8_t* __restrict__ p, uint64_t len, uint64_t m, uint64_t nb, uint32_t b, uint32_t left, ZnPmIn<typename ZnPmElem<E>::t>& in) {
  typedef typename ZnPmElem<E>::t T;
  in.off = nullptr; in.val = nullptr; in.f0 = in.f1 = 0;
  const uint32_t magic = *(const uint32_t*)p, e = *(const uint32_t*)(p + 4);
  const uint64_t hn = *(const uint64_t*)(p + 8), total = *(const uint64_t*)(p + 16), L = *(const uint64_t*)(p + 24);
  if (magic != ZN_PATCH_MAGIC || e != E || hn != m * E || total > m || L != len) return false;
  if (zn_patch_total(m, E, total) != L) return false;
  const uint32_t* first = (const uint32_t*)(p + 32);
  if (nb == 0) return first[0] == 0u;            // a tensor without elements: first[0] alone (and T == 0: total <= m)
  const uint32_t f0 = first[b], f1 = first[b + 1u];
  if (f0 > f1 || (uint64_t)f1 > total || (b == 0 && f0 != 0u) || ((uint64_t)b + 1u == nb && (uint64_t)f1 != total)) return false;
  if (f1 - f0 > left) return false;
  in.off = (const uint16_t*)(p + zn_patch_a1(nb)); in.val = (const T*)(p + zn_patch_a2(nb, total)); in.f0 = f0; in.f1 = f1;
  return true;
}

// inclusive sum over the lanes of a wave (lane 63 holds the wave's total)
__device__ __forceinline__ uint32_t zn_pm_wave_incl(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t t = __shfl_up(v, d); if (lane >= d) v += t; }
  return v;
}

// pref[w] = the set bits of bm[0 .. w) -> the set bits of the whole bitmap.  Every thread of the workgroup; the bitmap is complete and visible on entry, pref
// is on return.
__device__ __forceinline__ uint32_t zn_pm_prefix(const uint32_t* bm, uint16_t* pref, uint32_t* part) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t c[ZN_PM_PER], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < ZN_PM_PER; k++) { c[k] = (uint32_t)__popc(bm[tid * ZN_PM_PER + k]); sum += c[k]; }
  const uint32_t incl = zn_pm_wave_incl(sum, lane);
  if (lane == 63u) part[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < ZN_PM_WAVES; w++) { const uint32_t q = part[w]; if (w < wave) before += q; all += q; }
  uint32_t run = before + incl - sum;
#pragma unroll
  for (uint32_t k = 0; k < ZN_PM_PER; k++) { pref[tid * ZN_PM_PER + k] = (uint16_t)run; run += c[k]; }      // (run <= 65 504 at a word's start)
  __syncthreads();
  return all;
}

// entries of one input into its bitmap; -> something is wrong with them (an offset beyond the tensor's last element, not above its predecessor, or seen twice;
// a zero value)
template <typename T>
__device__ __forceinline__ bool zn_pm_mark(const ZnPmIn<T>& in, uint32_t* bm, uint64_t blk0, uint64_t m) {
  bool bad = false;
  for (uint32_t i = in.f0 + threadIdx.x; i < in.f1; i += ZN_PM_THREADS) {
    const uint32_t o = in.off[i];
    const T v = in.val[i];
    if (blk0 + o >= m || v == (T)0 || (i > in.f0 && (uint32_t)in.off[i - 1u] >= o)) { bad = true; continue; }
    const uint32_t bit = 1u << (o & 31u);
    if (atomicOr(&bm[o >> 5], bit) & bit) bad = true;
  }
  return bad;
}

// Block b of one item.  !EMIT: words[b] = the entries the merged block keeps.  EMIT: words[] is first[] of the result; the block's entries go to its off / val.
template <uint32_t E, bool EMIT>
__device__ __forceinline__ void zn_pm_block(const ZnPatchMSeg& sg, uint32_t b, uint32_t* __restrict__ words, uint32_t* __restrict__ status, ZnPmLds& s) {
  typedef typename ZnPmElem<E>::t T;
  const uint32_t tid = threadIdx.x;
  const uint64_t m = sg.m, nb = zn_patch_blocks(m), blk0 = (uint64_t)b * ZN_PATCH_BLOCK;
  const uint32_t left = (uint64_t)b >= nb ? 0u : (m - blk0 >= (uint64_t)ZN_PATCH_BLOCK ? ZN_PATCH_BLOCK : (uint32_t)(m - blk0));
  ZnPmIn<T> A, B;
  const bool okA = zn_pm_open<E>(ZN_GLOBAL_PTR(const uint8_t, sg.a), sg.a_len, m, nb, b, left, A);
  const bool okB = zn_pm_open<E>(ZN_GLOBAL_PTR(const uint8_t, sg.b), sg.b_len, m, nb, b, left, B);
  if (!okA || !okB) {                            // (workgroup-uniform) nothing behind a wrong header is read
    if (tid == 0) { atomicOr(status, ZN_DEV_CORRUPT); if (!EMIT && (uint64_t)b < nb) words[b] = 0u; }
    return;
  }
  if ((uint64_t)b >= nb) return;                 // a tensor without elements: its one workgroup has looked at the two headers
  uint32_t lo = 0, hi = 0;
  uint16_t* off = nullptr; T* val = nullptr;
  if (EMIT) {
    const uint64_t total = words[nb];
    uint8_t* p = ZN_GLOBAL_PTR(uint8_t, sg.out);
    const uint64_t a1 = zn_patch_a1(nb), a2 = zn_patch_a2(nb, total);
    lo = words[b]; hi = words[b + 1u];
    if (tid == 0) {
      uint32_t* first = (uint32_t*)(p + 32);
      first[b] = lo;
      if ((uint64_t)b + 1u == nb) first[nb] = (uint32_t)total;
      if (b == 0) {                              // the header, and the zero padding in front of off[] and of val[]
        *(uint32_t*)p = ZN_PATCH_MAGIC; *(uint32_t*)(p + 4) = E;
        *(uint64_t*)(p + 8) = m * E; *(uint64_t*)(p + 16) = total; *(uint64_t*)(p + 24) = a2 + (uint64_t)E * total;
        for (uint64_t i = 32u + 4u * (nb + 1u); i < a1; i++) p[i] = 0;
        for (uint64_t i = a1 + 2u * total; i < a2; i++) p[i] = 0;
      }
    }
    if (hi <= lo) return;                        // (workgroup-uniform) the merged block keeps nothing
    off = (uint16_t*)(p + a1); val = (T*)(p + a2);
  }
  const bool haveA = A.f1 > A.f0, haveB = B.f1 > B.f0;
  if (!haveA && !haveB) {                        // (workgroup-uniform) empty in both inputs
    if (!EMIT && tid == 0) words[b] = 0u;
    return;
  }
  for (uint32_t i = tid; i < ZN_PM_WORDS; i += ZN_PM_THREADS) { s.bmA[i] = 0u; s.bmB[i] = 0u; }
  if (tid == 0) s.wrong = 0u;
  __syncthreads();
  // 1. every entry sets its bit
  const bool badA = zn_pm_mark<T>(A, s.bmA, blk0, m), badB = zn_pm_mark<T>(B, s.bmB, blk0, m);
  if (badA || badB) s.wrong = 1u;
  __syncthreads();
  if (s.wrong) {                                 // (workgroup-uniform)
    if (tid == 0) { atomicOr(status, ZN_DEV_CORRUPT); if (!EMIT) words[b] = 0u; }
    return;
  }
  for (uint32_t i = tid; i < ZN_PM_WORDS; i += ZN_PM_THREADS) s.keep[i] = s.bmA[i] | s.bmB[i];
  const bool both = haveA && haveB;
  if (both) {
    // 2. where B's value for an offset lies (… and the barrier that makes keep visible)
    (void)zn_pm_prefix(s.bmB, s.prefB, s.part);
    // 3. an A entry that meets a B entry of the same value leaves nothing
    for (uint32_t i = A.f0 + tid; i < A.f1; i += ZN_PM_THREADS) {
      const uint32_t o = A.off[i], w = o >> 5, bit = 1u << (o & 31u);
      const uint32_t wb = s.bmB[w];
      if (!(wb & bit)) continue;
      const uint32_t j = B.f0 + (uint32_t)s.prefB[w] + (uint32_t)__popc(wb & (bit - 1u));
      if (j < B.f1 && (T)(A.val[i] ^ B.val[j]) == (T)0) atomicAnd(&s.keep[w], ~bit);
    }
  }
  __syncthreads();
  // 4. the block's count, and every kept offset's rank
  const uint32_t kept = zn_pm_prefix(s.keep, s.prefK, s.part);
  if (!EMIT) {
    if (tid == 0) words[b] = kept;
    return;
  }
  // 5. A's side: its kept entries, XORed with B's value where the element has one
  for (uint32_t i = A.f0 + tid; i < A.f1; i += ZN_PM_THREADS) {
    const uint32_t o = A.off[i], w = o >> 5, bit = 1u << (o & 31u);
    const uint32_t wk = s.keep[w];
    if (!(wk & bit)) continue;
    T v = A.val[i];
    const uint32_t wb = s.bmB[w];
    if (both && (wb & bit)) {
      const uint32_t j = B.f0 + (uint32_t)s.prefB[w] + (uint32_t)__popc(wb & (bit - 1u));
      if (j < B.f1) v = (T)(v ^ B.val[j]);
    }
    const uint32_t pos = lo + (uint32_t)s.prefK[w] + (uint32_t)__popc(wk & (bit - 1u));
    if (pos < hi) { off[pos] = (uint16_t)o; val[pos] = v; }      // never outside the block's own range, whatever the inputs hold by now
  }
  // 6. B's side: the entries of elements A has none for
  for (uint32_t i = B.f0 + tid; i < B.f1; i += ZN_PM_THREADS) {
    const uint32_t o = B.off[i], w = o >> 5, bit = 1u << (o & 31u);
    const uint32_t wk = s.keep[w];
    if ((s.bmA[w] & bit) || !(wk & bit)) continue;
    const uint32_t pos = lo + (uint32_t)s.prefK[w] + (uint32_t)__popc(wk & (bit - 1u));
    if (pos < hi) { off[pos] = (uint16_t)o; val[pos] = B.val[i]; }
  }
}

__device__ __forceinline__ ZnPatchMSeg zn_pm_find(const ZnPatchMSeg& one, const ZnPatchMSeg* __restrict__ segs, uint32_t nseg, uint32_t b) {
  if (segs == nullptr) return one;
  uint32_t lo = 0, hi = nseg;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (segs[mid].wg0 <= b) lo = mid; else hi = mid; }
  return segs[lo];
}

template <bool EMIT>
__device__ __forceinline__ void zn_pm_dispatch(const ZnPatchMSeg& one, const ZnPatchMSeg* __restrict__ segs_, uint32_t nseg, uint32_t* words_, uint32_t* status_, ZnPmLds& s) {
  const ZnPatchMSeg* segs = ZN_GLOBAL_PTR(const ZnPatchMSeg, segs_);
  const ZnPatchMSeg sg = zn_pm_find(one, segs, nseg, blockIdx.x);
  uint32_t* words = ZN_GLOBAL_PTR(uint32_t, words_) + sg.w0;
  uint32_t* status = ZN_GLOBAL_PTR(uint32_t, status_);
  const uint32_t b = blockIdx.x - sg.wg0;
  if (sg.E == 1u) zn_pm_block<1, EMIT>(sg, b, words, status, s);
  else if (sg.E == 2u) zn_pm_block<2, EMIT>(sg, b, words, status, s);
  else zn_pm_block<4, EMIT>(sg, b, words, status, s);
}

__global__ void __launch_bounds__(ZN_PM_THREADS) zn_k_patch_merge_count(const ZnPatchMSeg one, const ZnPatchMSeg* __restrict__ segs, uint32_t nseg, uint32_t* __restrict__ words,
                                                                        uint32_t* __restrict__ status) {
  __shared__ ZnPmLds s;
  zn_pm_dispatch<false>(one, segs, nseg, words, status, s);
}

__global__ void __launch_bounds__(ZN_PM_THREADS) zn_k_patch_merge_emit(const ZnPatchMSeg one, const ZnPatchMSeg* __restrict__ segs, uint32_t nseg, uint32_t* __restrict__ words,
                                                                       uint32_t* __restrict__ status) {
  __shared__ ZnPmLds s;
  zn_pm_dispatch<true>(one, segs, nseg, words, status, s);
}

void zn_launch_patch_merge_count(const ZnPatchMSeg& one, const ZnPatchMSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, uint32_t* d_status, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_merge_count, dim3(total_wg), dim3(ZN_PM_THREADS), 0, stream, one, d_segs, nseg, d_words, d_status);
  zn_note_kernel("zn_k_patch_merge_count");
}
void zn_launch_patch_merge_emit(const ZnPatchMSeg& one, const ZnPatchMSeg* d_segs, uint32_t nseg, uint32_t total_wg, const uint32_t* d_words, uint32_t* d_status, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_merge_emit, dim3(total_wg), dim3(ZN_PM_THREADS), 0, stream, one, d_segs, nseg, const_cast<uint32_t*>(d_words), d_status);
  zn_note_kernel("zn_k_patch_merge_emit");
}

// ---- the C ABI of the merge (host side: checks, tables, launches) ----
namespace {

bool merge_elem_ok(size_t n, int elem) { return (elem == 1 || elem == 2 || elem == 4) && n % (size_t)elem == 0 && (uint64_t)(n / (size_t)elem) < (1ull << 32); }
bool merge_input_ok(const void* p, size_t len) { return p && (((uintptr_t)p) & 15u) == 0 && len >= 32u; }
bool merge_overlap(const void* p, size_t pn, const void* q, size_t qn) { return (uintptr_t)p < (uintptr_t)q + qn && (uintptr_t)q < (uintptr_t)p + pn; }

// `bytes` of a table through the pinned staging buffer into WS_SEGS at byte offset `at`; the caller has synchronised with the buffer's last reader
int merge_stage(Workspace& w, const void* table, size_t bytes, size_t at, hipStream_t stream) {
  memcpy((uint8_t*)w.h_segs.p + at, table, bytes);
  ZN_HIP(hipMemcpyAsync((uint8_t*)w.buf[WS_SEGS] + at, (uint8_t*)w.h_segs.p + at, bytes, hipMemcpyHostToDevice, stream));
  return ZN_OK;
}

// Count, scan, one read-back of every item's T and of the verdict; with `emit`: capacity check, then the emit pass for the items that keep entries.  Synchronous.
int patch_merge(const zn_patch_merge_item* items, size_t count, std::vector<uint64_t>& lens, bool emit, hipStream_t stream) {
  lens.assign(count, 0);
  if (count == 0) return ZN_OK;
  if (count > 0x7FFFFFFFull) return ZN_E_ARG;
  std::vector<ZnPatchMSeg> segs(count);
  std::vector<ZnPatchBSeg> scan(count);          // the scan kernel's view of the same items: m and w0
  uint64_t wg = 0, words = 0;
  for (size_t i = 0; i < count; i++) {
    const zn_patch_merge_item& it = items[i];
    if (!merge_elem_ok(it.n, it.elem)) return ZN_E_ARG;
    if (!merge_input_ok(it.d_a, it.a_len) || !merge_input_ok(it.d_b, it.b_len)) return ZN_E_ARG;
    if (emit && it.out_cap) {
      if (!it.d_out || (((uintptr_t)it.d_out) & 15u) != 0) return ZN_E_ARG;
      if (merge_overlap(it.d_out, it.out_cap, it.d_a, it.a_len) || merge_overlap(it.d_out, it.out_cap, it.d_b, it.b_len)) return ZN_E_ARG;
    }
    const uint64_t m = it.n / (size_t)it.elem, nb = zn_patch_blocks(m);
    segs[i] = ZnPatchMSeg{(const uint8_t*)it.d_a, it.a_len, (const uint8_t*)it.d_b, it.b_len, (uint8_t*)it.d_out, m, (uint32_t)wg, (uint32_t)words, (uint32_t)it.elem, 0u};
    scan[i] = ZnPatchBSeg{nullptr, nullptr, nullptr, m, 0u, (uint32_t)words, (uint32_t)it.elem, 0u};
    wg += nb ? nb : 1u;                          // (a tensor without elements still has two headers to look at)
    words += nb + 1u;
    if (wg > 0x7FFFFFFFull || words > 0x7FFFFFFFull) return ZN_E_ARG;
  }
  WsLease L;
  if (L.rc) return L.rc;
  Workspace& w = *L.w;
  t_kernels.clear();
  int rc;
  const bool table = count > 1;
  const size_t mseg_bytes = table ? count * sizeof(ZnPatchMSeg) : 0u, bseg_bytes = table ? count * sizeof(ZnPatchBSeg) : 0u;
  const size_t table_bytes = 2u * mseg_bytes + bseg_bytes;                       // count table, scan table, emit table (the emit pass has a grid of its own)
  const size_t back_bytes = (count + 1u) * sizeof(uint64_t);                     // every item's T, and the verdict word behind them
  if ((rc = w.reserve(WS_META_A, words * sizeof(uint32_t)))) return rc;
  if ((rc = w.reserve(WS_TOTALS, back_bytes))) return rc;
  if ((rc = w.h_totals.reserve(back_bytes))) return rc;
  if (table && (rc = w.reserve(WS_SEGS, table_bytes))) return rc;
  if ((rc = L.acquire(stream))) return rc;
  L.mark = table;
  uint32_t* d_words = (uint32_t*)w.buf[WS_META_A];
  uint64_t* d_totals = (uint64_t*)w.buf[WS_TOTALS];
  uint32_t* d_status = (uint32_t*)(d_totals + count);
  ZN_HIP(hipMemsetAsync(d_status, 0, sizeof(uint64_t), stream));
  if (table) {
    ZN_HIP(hipEventSynchronize(w.busy));         // the previous batched call may still be reading the pinned staging
    if ((rc = w.h_segs.reserve(table_bytes))) return rc;
    if ((rc = merge_stage(w, segs.data(), mseg_bytes, 0, stream))) return rc;
    if ((rc = merge_stage(w, scan.data(), bseg_bytes, mseg_bytes, stream))) return rc;
  }
  const uint8_t* d_tab = (const uint8_t*)w.buf[WS_SEGS];
  zn_launch_patch_merge_count(segs[0], table ? (const ZnPatchMSeg*)d_tab : nullptr, (uint32_t)count, (uint32_t)wg, d_words, d_status, stream);
  zn_launch_patch_scan(scan[0], table ? (const ZnPatchBSeg*)(d_tab + mseg_bytes) : nullptr, (uint32_t)count, d_words, d_totals, stream);
  if (launch_failed()) return ZN_E_HIP;
  ZN_HIP(hipMemcpyAsync(w.h_totals.p, d_totals, back_bytes, hipMemcpyDeviceToHost, stream));
  ZN_HIP(hipStreamSynchronize(stream));
  const uint64_t* T = (const uint64_t*)w.h_totals.p;
  if ((uint32_t)T[count] & ZN_DEV_CORRUPT) return ZN_E_CORRUPT;
  bool short_cap = false;
  for (size_t i = 0; i < count; i++) {
    lens[i] = T[i] ? zn_patch_total(segs[i].m, segs[i].E, T[i]) : 0u;           // (0: everything cancels)
    if (emit && lens[i] > items[i].out_cap) short_cap = true;
  }
  if (!emit) return ZN_OK;
  if (short_cap) return ZN_E_CAP;
  uint64_t ewg = 0;
  for (size_t i = 0; i < count; i++) { segs[i].wg0 = (uint32_t)ewg; if (T[i]) ewg += zn_patch_blocks(segs[i].m); }
  if (ewg == 0) return ZN_OK;
  // (the first tables' copies are over — the stream was synchronised —; the emit table goes behind them)
  if (table && (rc = merge_stage(w, segs.data(), mseg_bytes, mseg_bytes + bseg_bytes, stream))) return rc;
  zn_launch_patch_merge_emit(segs[0], table ? (const ZnPatchMSeg*)(d_tab + mseg_bytes + bseg_bytes) : nullptr, (uint32_t)count, (uint32_t)ewg, d_words, d_status, stream);
  if (launch_failed()) return ZN_E_HIP;
  ZN_HIP(hipMemcpyAsync(w.h_totals.p, d_status, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));      // an input that changed under the call
  ZN_HIP(hipStreamSynchronize(stream));
  return ((uint32_t)T[0] & ZN_DEV_CORRUPT) ? ZN_E_CORRUPT : ZN_OK;
}

}  // namespace

extern "C" {

int zn_patch_merge_size_batch_dev(const zn_patch_merge_item* items, size_t count, size_t* sizes_out, void* stream_) {
  try {
    if (count == 0) return ZN_OK;
    if (!items || !sizes_out) return ZN_E_ARG;
    std::vector<uint64_t> lens;
    const int rc = patch_merge(items, count, lens, false, (hipStream_t)stream_);
    if (rc) return rc;
    for (size_t i = 0; i < count; i++) sizes_out[i] = (size_t)lens[i];
    return ZN_OK;
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_patch_merge_batch_dev(zn_patch_merge_item* items, size_t count, void* stream_) {
  try {
    if (count == 0) return ZN_OK;
    if (!items) return ZN_E_ARG;
    for (size_t i = 0; i < count; i++) items[i].out_len = 0;
    std::vector<uint64_t> lens;
    const int rc = patch_merge(items, count, lens, true, (hipStream_t)stream_);
    if (rc == ZN_OK || rc == ZN_E_CAP) for (size_t i = 0; i < count; i++) items[i].out_len = (size_t)lens[i];       // (ZN_E_CAP: the lengths that were needed; nothing was written)
    return rc;
  } catch (...) { return ZN_E_ALLOC; }
}

}  // extern "C"
