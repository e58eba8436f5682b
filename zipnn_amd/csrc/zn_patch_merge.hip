// zn_patch_merge.hip — the XOR-merge of two "znp1" patches over one tensor (include/zipnn_hip.h): the union of their entries, the values XORed
// where both have one, what cancels to zero dropped.  merge(patch(A, base), patch(B, base)) is patch(B, A), byte for byte, without either tensor.
//
//   zn_k_patch_merge_count   one workgroup per block of 65 536 elements: how many entries the merged block keeps (one word per block)
//   zn_k_patch_scan          (zn_patch.hip) the block counts become first[], the item's T goes to its total
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
#include "zn_patch_host.hpp"

struct ZnPmLds {
  uint32_t bmA[ZN_PM_WORDS], bmB[ZN_PM_WORDS], keep[ZN_PM_WORDS];
  uint16_t prefB[ZN_PM_WORDS], prefK[ZN_PM_WORDS];
  uint32_t part[ZN_PATCH_WAVES];
  uint32_t wrong;
};

// one input's part of a block: its entries [f0, f1) of off[] / val[]
template <typename T> struct ZnPmIn { const uint16_t* off; const T* val; uint32_t f0, f1; };

// The header test, then the block's pair of first[] (zn_patch_format.hpp); here also: more entries than the block has elements cannot ascend.  (workgroup-uniform)
template <uint32_t E>
__device__ __forceinline__ bool zn_pm_open(const uint8_t* __restrict__ p, uint64_t len, uint64_t m, uint64_t nb, uint32_t b, uint32_t left, ZnPmIn<typename ZnPatchElem<E>::t>& in) {
  typedef typename ZnPatchElem<E>::t T;
  in.off = nullptr; in.val = nullptr; in.f0 = in.f1 = 0;
  uint64_t total;
  if (!zn_patch_header_ok<E>(zn_patch_header(p), m * E, m, len, total)) return false;
  const uint32_t* first = (const uint32_t*)(p + 32);
  if (nb == 0) return first[0] == 0u;            // a tensor without elements: first[0] alone (and T == 0: total <= m)
  const uint32_t f0 = first[b], f1 = first[b + 1u];
  if (zn_patch_pair_bad(f0, f1, total, b, nb) || f1 - f0 > left) return false;
  in.off = (const uint16_t*)(p + zn_patch_a1(nb)); in.val = (const T*)(p + zn_patch_a2(nb, total)); in.f0 = f0; in.f1 = f1;
  return true;
}

// entries of one input into its bitmap; -> something is wrong with them (an offset beyond the tensor's last element, not above its predecessor, or seen twice;
// a zero value)
template <typename T>
__device__ __forceinline__ bool zn_pm_mark(const ZnPmIn<T>& in, uint32_t* bm, uint64_t blk0, uint64_t m) {
  bool bad = false;
  for (uint32_t i = in.f0 + threadIdx.x; i < in.f1; i += ZN_PATCH_THREADS) {
    const uint32_t o = in.off[i];
    const T v = in.val[i];
    if (zn_patch_entry_bad(in.off, i, in.f0, o, v, blk0 + o, m)) { bad = true; continue; }
    const uint32_t bit = 1u << (o & 31u);
    if (atomicOr(&bm[o >> 5], bit) & bit) bad = true;
  }
  return bad;
}

// Block b of one item.  !EMIT: words[b] = the entries the merged block keeps.  EMIT: words[] is first[] of the result; the block's entries go to its off / val.
template <uint32_t E, bool EMIT>
__device__ __forceinline__ void zn_pm_block(const ZnPatchMSeg& sg, uint32_t b, uint32_t* __restrict__ words, uint32_t* __restrict__ status, ZnPmLds& s) {
  typedef typename ZnPatchElem<E>::t T;
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
    lo = words[b]; hi = words[b + 1u];
    if (tid == 0) zn_patch_emit_head<E>(p, m, nb, total, b, lo);
    if (hi <= lo) return;                        // (workgroup-uniform) the merged block keeps nothing
    off = (uint16_t*)(p + zn_patch_a1(nb)); val = (T*)(p + zn_patch_a2(nb, total));
  }
  const bool haveA = A.f1 > A.f0, haveB = B.f1 > B.f0;
  if (!haveA && !haveB) {                        // (workgroup-uniform) empty in both inputs
    if (!EMIT && tid == 0) words[b] = 0u;
    return;
  }
  for (uint32_t i = tid; i < ZN_PM_WORDS; i += ZN_PATCH_THREADS) { s.bmA[i] = 0u; s.bmB[i] = 0u; }
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
  for (uint32_t i = tid; i < ZN_PM_WORDS; i += ZN_PATCH_THREADS) s.keep[i] = s.bmA[i] | s.bmB[i];
  const bool both = haveA && haveB;
  if (both) {
    // 2. where B's value for an offset lies (… and the barrier that makes keep visible)
    (void)zn_pm_prefix(s.bmB, s.prefB, s.part);
    // 3. an A entry that meets a B entry of the same value leaves nothing
    for (uint32_t i = A.f0 + tid; i < A.f1; i += ZN_PATCH_THREADS) {
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
  for (uint32_t i = A.f0 + tid; i < A.f1; i += ZN_PATCH_THREADS) {
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
  for (uint32_t i = B.f0 + tid; i < B.f1; i += ZN_PATCH_THREADS) {
    const uint32_t o = B.off[i], w = o >> 5, bit = 1u << (o & 31u);
    const uint32_t wk = s.keep[w];
    if ((s.bmA[w] & bit) || !(wk & bit)) continue;
    const uint32_t pos = lo + (uint32_t)s.prefK[w] + (uint32_t)__popc(wk & (bit - 1u));
    if (pos < hi) { off[pos] = (uint16_t)o; val[pos] = B.val[i]; }
  }
}

template <bool EMIT>
__device__ __forceinline__ void zn_pm_dispatch(const ZnPatchMSeg& one, const ZnPatchMSeg* __restrict__ segs_, uint32_t nseg, uint32_t* words_, uint32_t* status_, ZnPmLds& s) {
  const ZnPatchMSeg* segs = ZN_GLOBAL_PTR(const ZnPatchMSeg, segs_);
  const ZnPatchMSeg sg = zn_patch_find(one, segs, nseg, blockIdx.x);
  uint32_t* words = ZN_GLOBAL_PTR(uint32_t, words_) + sg.w0;
  uint32_t* status = ZN_GLOBAL_PTR(uint32_t, status_);
  const uint32_t b = blockIdx.x - sg.wg0;
  if (sg.E == 1u) zn_pm_block<1, EMIT>(sg, b, words, status, s);
  else if (sg.E == 2u) zn_pm_block<2, EMIT>(sg, b, words, status, s);
  else zn_pm_block<4, EMIT>(sg, b, words, status, s);
}

__global__ void __launch_bounds__(ZN_PATCH_THREADS) zn_k_patch_merge_count(const ZnPatchMSeg one, const ZnPatchMSeg* __restrict__ segs, uint32_t nseg, uint32_t* __restrict__ words,
                                                                        uint32_t* __restrict__ status) {
  __shared__ ZnPmLds s;
  zn_pm_dispatch<false>(one, segs, nseg, words, status, s);
}

__global__ void __launch_bounds__(ZN_PATCH_THREADS) zn_k_patch_merge_emit(const ZnPatchMSeg one, const ZnPatchMSeg* __restrict__ segs, uint32_t nseg, uint32_t* __restrict__ words,
                                                                       uint32_t* __restrict__ status) {
  __shared__ ZnPmLds s;
  zn_pm_dispatch<true>(one, segs, nseg, words, status, s);
}

void zn_launch_patch_merge_count(const ZnPatchMSeg& one, const ZnPatchMSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, uint32_t* d_status, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_merge_count, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, d_words, d_status);
  zn_note_kernel("zn_k_patch_merge_count");
}
void zn_launch_patch_merge_emit(const ZnPatchMSeg& one, const ZnPatchMSeg* d_segs, uint32_t nseg, uint32_t total_wg, const uint32_t* d_words, uint32_t* d_status, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  hipLaunchKernelGGL(zn_k_patch_merge_emit, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, const_cast<uint32_t*>(d_words), d_status);
  zn_note_kernel("zn_k_patch_merge_emit");
}

// ---- the C ABI of the merge (host side: checks, tables, launches) ----
namespace {

// The sizes of the merged patches; with `emit`: … and the patches, where every capacity suffices (zn_patch_two_pass).  An item without elements still has two
// headers to look at: one workgroup; lens[i] == 0: everything cancels.
int patch_merge(const zn_patch_merge_item* items, size_t count, std::vector<uint64_t>& lens, bool emit, hipStream_t stream) {
  lens.assign(count, 0);
  if (count == 0) return ZN_OK;
  if (count > 0x7FFFFFFFull) return ZN_E_ARG;
  std::vector<ZnPatchMSeg> segs(count);
  std::vector<ZnPatchBSeg> scan(count);
  std::vector<size_t> caps(count);
  uint64_t wg = 0, words = 0;
  for (size_t i = 0; i < count; i++) {
    const zn_patch_merge_item& it = items[i];
    if (!zn_patch_elem_ok(it.n, it.elem)) return ZN_E_ARG;
    if (!zn_patch_input_ok(it.d_a, it.a_len) || !zn_patch_input_ok(it.d_b, it.b_len)) return ZN_E_ARG;
    if (emit && it.out_cap) {
      if (!zn_patch_out_ok(it.d_out)) return ZN_E_ARG;
      if (zn_patch_overlap(it.d_out, it.out_cap, it.d_a, it.a_len) || zn_patch_overlap(it.d_out, it.out_cap, it.d_b, it.b_len)) return ZN_E_ARG;
    }
    const uint64_t m = it.n / (size_t)it.elem, nb = zn_patch_blocks(m);
    segs[i] = ZnPatchMSeg{(const uint8_t*)it.d_a, it.a_len, (const uint8_t*)it.d_b, it.b_len, (uint8_t*)it.d_out, m, (uint32_t)wg, (uint32_t)words, (uint32_t)it.elem, 0u};
    scan[i] = ZnPatchBSeg{nullptr, nullptr, nullptr, m, 0u, (uint32_t)words, (uint32_t)it.elem, 0u};
    caps[i] = it.out_cap;
    wg += nb ? nb : 1u;
    words += nb + 1u;
    if (wg > 0x7FFFFFFFull || words > 0x7FFFFFFFull) return ZN_E_ARG;
  }
  return zn_patch_two_pass(segs, scan.data(), wg, words, emit ? caps.data() : nullptr, lens, stream, zn_launch_patch_merge_count, zn_launch_patch_merge_emit);
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
