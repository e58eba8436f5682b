// zn_patch_select.hip — "znp1" patches restricted to a rectangle of their tensor and embedded back (include/zipnn_hip.h): what a tensor-parallel
// rank needs, which holds a narrow() of every weight.  View the tensor as R x C elements and take rows [r0, r1), cols [c0, c1), w = c1 - c0.  The map from the
// rectangle's row-major index j to the tensor's, phi(j) = (r0 + j / w) C + c0 + j % w, is strictly increasing: SELECT keeps the entries inside the rectangle and
// re-indexes them by phi^-1, PLACE re-indexes a rectangle's entries by phi — no tensor, no sort, and the result is byte for byte the patch zn_patch_build_batch_dev
// builds from the sliced tensors.
//
//   zn_k_patch_select_count / zn_k_patch_place_count   one workgroup per OUTPUT block of 65 536 elements: how many entries it keeps (one word per block)
//   zn_k_patch_scan                                     (zn_patch.hip) the block counts become first[], the item's T goes to its total
//   zn_k_patch_select_emit / zn_k_patch_place_emit     one workgroup per output block again: off / val of the kept entries at first[ob] + rank; block 0 writes the header
//
// All four are ONE body (zn_ps_block<E, PLACE, EMIT>).  An output block's elements lie in a range of input indices — SELECT: [phi(j_lo), phi(j_hi - 1)], about
// C / w input blocks; PLACE: the j with phi(j) inside the block, one contiguous range whose ends cost a division each, at most two input blocks.  The workgroup
// looks at the first[] pairs of that range 256 at a time (a narrow w over a wide C spans thousands of blocks, most of them empty), and walks the entries of the
// blocks that have any 256 at a time, in order: keep flag, ballot, the set bits below the lane, the four waves' sums through two alternating sets of LDS slots,
// a running total in a register (zn_pa_block's emit scheme) — kept entries leave in input order, which is output order.
// The kernels trust nothing: an input may come from anywhere.  Every workgroup checks the header first (magic, E, n against the item, T <= m, L against the
// length given and against the formula's value for T: that bounds every later index), then the first[] pair and EVERY entry of every input block it visits.
// PLACE visits every input block from some workgroup, so a place that returns ZN_OK has validated its input whole; SELECT validates the header and the input
// blocks that overlap the rectangle's rows — the rest is zn_patch_check_batch_dev's job.  The emit instances never write outside [first[ob], first[ob + 1]) of
// off / val: if the input changed between the two passes the result is wrong, not the memory around it.
#include "zn_patch_host.hpp"

struct ZnPsLds {
  uint32_t f0[ZN_PATCH_THREADS], f1[ZN_PATCH_THREADS];   // the first[] pairs of the 256 input blocks being looked at
  unsigned long long some[ZN_PATCH_WAVES];            // … which of them have entries, one mask per wave
  uint32_t part[2][ZN_PATCH_WAVES];
  uint32_t wrong;
};

// the smallest j with phi(j) >= i (h w when there is none): i's place in the rectangle's order
__device__ __forceinline__ uint64_t zn_ps_lower(const ZnPatchSSeg& sg, uint64_t i) {
  const uint32_t w = sg.c1 - sg.c0;
  const uint64_t row = i / sg.C, col = i - row * sg.C;
  if (row < sg.r0) return 0u;
  if (row >= sg.r1) return (uint64_t)(sg.r1 - sg.r0) * w;
  const uint64_t rr = row - sg.r0;
  return col <= sg.c0 ? rr * w : col >= sg.c1 ? (rr + 1u) * w : rr * w + (col - sg.c0);
}

// Output block ob of one item.  !EMIT: words[ob] = the entries it keeps.  EMIT: words[] is first[] of the result; the block's entries go to its off / val.
template <uint32_t E, bool PLACE, bool EMIT>
__device__ __forceinline__ void zn_ps_block(const ZnPatchSSeg& sg, uint32_t ob, uint32_t* __restrict__ words, uint32_t* __restrict__ status, ZnPsLds& s) {
  typedef typename ZnPatchElem<E>::t T;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t C = sg.C, w = sg.c1 - sg.c0;
  const uint64_t m_all = (uint64_t)sg.R * C, m_rect = (uint64_t)(sg.r1 - sg.r0) * w;
  const uint64_t m_in = PLACE ? m_rect : m_all, m_out = PLACE ? m_all : m_rect;     // (the host has checked: a non-empty rectangle inside the tensor, m_all < 2^32)
  const uint64_t nb_in = zn_patch_blocks(m_in), nb_out = zn_patch_blocks(m_out);
  const uint8_t* p = ZN_GLOBAL_PTR(const uint8_t, sg.in);
  uint64_t total;
  bool bad = !zn_patch_header_ok<E>(zn_patch_header(p), m_in * E, m_in, sg.in_len, total);
  if (bad) {                                     // (workgroup-uniform) nothing behind a wrong header is read
    if (tid == 0) { atomicOr(status, ZN_DEV_CORRUPT); if (!EMIT) words[ob] = 0u; }
    return;
  }
  const uint64_t o_lo = (uint64_t)ob * ZN_PATCH_BLOCK, o_hi = o_lo + ZN_PATCH_BLOCK < m_out ? o_lo + ZN_PATCH_BLOCK : m_out;      // the output indices this block owns
  // the input entries that can land in it: indices [in_lo, in_hi) of the input's numbering
  uint64_t in_lo, in_hi;
  if (PLACE) { in_lo = zn_ps_lower(sg, o_lo); in_hi = zn_ps_lower(sg, o_hi); }
  else {
    const uint64_t ja = o_lo, jb = o_hi - 1u;
    in_lo = (sg.r0 + ja / w) * C + sg.c0 + ja % w;
    in_hi = (sg.r0 + jb / w) * C + sg.c0 + jb % w + 1u;
  }
  uint32_t lo = 0, hi = 0;
  uint16_t* off_out = nullptr; T* val_out = nullptr;
  if (EMIT) {
    const uint64_t tout = words[nb_out];
    uint8_t* q = ZN_GLOBAL_PTR(uint8_t, sg.out);
    lo = words[ob]; hi = words[ob + 1u];
    if (tid == 0) zn_patch_emit_head<E>(q, m_out, nb_out, tout, ob, lo);
    if (hi <= lo) return;                        // (workgroup-uniform) this block keeps nothing
    off_out = (uint16_t*)(q + zn_patch_a1(nb_out)); val_out = (T*)(q + zn_patch_a2(nb_out, tout));
  }
  if (in_hi <= in_lo) {                          // (workgroup-uniform; PLACE) no element of the rectangle lies in this block
    if (!EMIT && tid == 0) words[ob] = 0u;
    return;
  }
  const uint32_t* first = (const uint32_t*)(p + 32);
  const uint16_t* off = (const uint16_t*)(p + zn_patch_a1(nb_in));
  const T* val = (const T*)(p + zn_patch_a2(nb_in, total));
  const uint32_t ib_lo = (uint32_t)(in_lo / ZN_PATCH_BLOCK), ib_hi = (uint32_t)((in_hi - 1u) / ZN_PATCH_BLOCK);      // (in_hi <= m_in: ib_hi < nb_in)
  if (tid == 0) s.wrong = 0u;
  uint32_t run = 0, step = 0;                    // count: this wave's kept entries; emit: the block's entries in front of this step
  for (uint32_t ib0 = ib_lo; ib0 <= ib_hi; ib0 += ZN_PATCH_THREADS) {
    // the first[] pairs of up to 256 input blocks, one per thread
    const uint32_t ib = ib0 + tid;
    uint32_t f0 = 0, f1 = 0;
    if (ib <= ib_hi) {                           // (a tensor has at most 65 536 blocks: the sum does not wrap)
      f0 = first[ib]; f1 = first[ib + 1u];
      const uint64_t blk0 = (uint64_t)ib * ZN_PATCH_BLOCK;
      const uint64_t left = m_in - blk0 >= (uint64_t)ZN_PATCH_BLOCK ? ZN_PATCH_BLOCK : m_in - blk0;
      if (zn_patch_pair_bad(f0, f1, total, ib, nb_in) || (uint64_t)(f1 - f0) > left) { bad = true; f0 = f1 = 0; }      // (more entries than elements cannot ascend)
    }
    s.f0[tid] = f0; s.f1[tid] = f1;
    const unsigned long long some = __ballot(f1 > f0);
    if (lane == 0) s.some[wave] = some;
    __syncthreads();
    for (uint32_t wv = 0; wv < ZN_PATCH_WAVES; wv++) {
      unsigned long long mask = s.some[wv];      // (workgroup-uniform: every thread walks the same blocks in the same order)
      while (mask) {
        const uint32_t k = wv * 64u + (uint32_t)__ffsll(mask) - 1u;
        mask &= mask - 1ull;
        const uint32_t g0 = s.f0[k], g1 = s.f1[k];
        const uint64_t blk0 = (uint64_t)(ib0 + k) * ZN_PATCH_BLOCK;
        for (uint64_t i0 = g0; i0 < g1; i0 += ZN_PATCH_THREADS) {      // (64 bits: g1 may lie within 256 of 2^32)
          const uint64_t i = i0 + tid;
          bool keep = false;
          uint32_t oo = 0; T v = (T)0;
          if (i < g1) {
            const uint32_t o = off[i];
            v = val[i];
            const uint64_t x = blk0 + o;         // the entry's index in the input's numbering
            if (zn_patch_entry_bad(off, i, g0, o, v, x, m_in)) bad = true;
            else if (PLACE) {
              if (x >= in_lo && x < in_hi) {
                const uint32_t rr = (uint32_t)x / w, cc = (uint32_t)x - rr * w;
                oo = (uint32_t)(((uint64_t)(sg.r0 + rr) * C + sg.c0 + cc) - o_lo);
                keep = true;
              }
            } else {
              const uint32_t row = (uint32_t)x / C, col = (uint32_t)x - row * C;
              if (row >= sg.r0 && row < sg.r1 && col >= sg.c0 && col < sg.c1) {
                const uint64_t j = (uint64_t)(row - sg.r0) * w + (col - sg.c0);
                if (j >= o_lo && j < o_hi) { oo = (uint32_t)(j - o_lo); keep = true; }
              }
            }
          }
          const unsigned long long kept = __ballot(keep);
          if (!EMIT) { run += (uint32_t)__popcll(kept); continue; }
          if (lane == 0) s.part[step & 1u][wave] = (uint32_t)__popcll(kept);      // (two sets of slots: one barrier per step is enough)
          __syncthreads();
          uint32_t before, all;
          zn_patch_wave_sums(s.part[step & 1u], wave, before, all);
          if (keep) {
            const uint32_t pos = lo + run + before + (uint32_t)__popcll(kept & ((1ull << lane) - 1ull));
            if (pos < hi) { off_out[pos] = (uint16_t)oo; val_out[pos] = v; }      // never outside the block's own range, whatever the input holds by now
          }
          run += all;
          step++;
        }
      }
    }
    __syncthreads();                             // (the pairs and masks are overwritten by the next round)
  }
  if (bad) s.wrong = 1u;
  if (!EMIT && lane == 0) s.part[0][wave] = run;
  __syncthreads();
  if (tid == 0) {
    const bool wrong = s.wrong != 0u;
    if (wrong) atomicOr(status, ZN_DEV_CORRUPT);
    if (!EMIT) { uint32_t c = 0; for (uint32_t q = 0; q < ZN_PATCH_WAVES; q++) c += s.part[0][q]; words[ob] = wrong ? 0u : c; }
  }
}

template <bool PLACE, bool EMIT>
__device__ __forceinline__ void zn_ps_dispatch(const ZnPatchSSeg& one, const ZnPatchSSeg* __restrict__ segs_, uint32_t nseg, uint32_t* words_, uint32_t* status_, ZnPsLds& s) {
  const ZnPatchSSeg* segs = ZN_GLOBAL_PTR(const ZnPatchSSeg, segs_);
  const ZnPatchSSeg sg = zn_patch_find(one, segs, nseg, blockIdx.x);
  uint32_t* words = ZN_GLOBAL_PTR(uint32_t, words_) + sg.w0;
  uint32_t* status = ZN_GLOBAL_PTR(uint32_t, status_);
  const uint32_t ob = blockIdx.x - sg.wg0;
  if (sg.E == 1u) zn_ps_block<1, PLACE, EMIT>(sg, ob, words, status, s);
  else if (sg.E == 2u) zn_ps_block<2, PLACE, EMIT>(sg, ob, words, status, s);
  else zn_ps_block<4, PLACE, EMIT>(sg, ob, words, status, s);
}

#define ZN_PS_KERNEL(NAME, PLACE, EMIT)                                                                                                                          \
  __global__ void __launch_bounds__(ZN_PATCH_THREADS) NAME(const ZnPatchSSeg one, const ZnPatchSSeg* __restrict__ segs, uint32_t nseg, uint32_t* __restrict__ words, \
                                                        uint32_t* __restrict__ status) {                                                                         \
    __shared__ ZnPsLds s;                                                                                                                                        \
    zn_ps_dispatch<PLACE, EMIT>(one, segs, nseg, words, status, s);                                                                                              \
  }
ZN_PS_KERNEL(zn_k_patch_select_count, false, false)
ZN_PS_KERNEL(zn_k_patch_select_emit, false, true)
ZN_PS_KERNEL(zn_k_patch_place_count, true, false)
ZN_PS_KERNEL(zn_k_patch_place_emit, true, true)
#undef ZN_PS_KERNEL

void zn_launch_patch_select_count(bool place, const ZnPatchSSeg& one, const ZnPatchSSeg* d_segs, uint32_t nseg, uint32_t total_wg, uint32_t* d_words, uint32_t* d_status, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  if (place) hipLaunchKernelGGL(zn_k_patch_place_count, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, d_words, d_status);
  else hipLaunchKernelGGL(zn_k_patch_select_count, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, d_words, d_status);
  zn_note_kernel(place ? "zn_k_patch_place_count" : "zn_k_patch_select_count");
}
void zn_launch_patch_select_emit(bool place, const ZnPatchSSeg& one, const ZnPatchSSeg* d_segs, uint32_t nseg, uint32_t total_wg, const uint32_t* d_words, uint32_t* d_status, hipStream_t stream) {
  if (nseg == 0 || total_wg == 0) return;
  if (place) hipLaunchKernelGGL(zn_k_patch_place_emit, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, const_cast<uint32_t*>(d_words), d_status);
  else hipLaunchKernelGGL(zn_k_patch_select_emit, dim3(total_wg), dim3(ZN_PATCH_THREADS), 0, stream, one, d_segs, nseg, const_cast<uint32_t*>(d_words), d_status);
  zn_note_kernel(place ? "zn_k_patch_place_emit" : "zn_k_patch_select_emit");
}

// ---- the C ABI of select and place (host side: checks, tables, launches) ----
namespace {

// The sizes of the selected / placed patches; with `emit`: … and the patches, where every capacity suffices (zn_patch_two_pass).  Every item has at least one
// output block: the rectangle is not empty; lens[i] == 0: no entry results.
int patch_select(const zn_patch_select_item* items, size_t count, std::vector<uint64_t>& lens, bool place, bool emit, hipStream_t stream) {
  lens.assign(count, 0);
  if (count == 0) return ZN_OK;
  if (count > 0x7FFFFFFFull) return ZN_E_ARG;
  std::vector<ZnPatchSSeg> segs(count);
  std::vector<ZnPatchBSeg> scan(count);
  std::vector<size_t> caps(count);
  uint64_t wg = 0, words = 0;
  for (size_t i = 0; i < count; i++) {
    const zn_patch_select_item& it = items[i];
    if (it.rows == 0 || it.cols == 0 || it.rows >= (1ull << 32) || it.cols >= (1ull << 32) || !zn_patch_count_ok(it.elem, (uint64_t)it.rows * (uint64_t)it.cols)) return ZN_E_ARG;
    if (it.row_lo >= it.row_hi || it.row_hi > it.rows || it.col_lo >= it.col_hi || it.col_hi > it.cols) return ZN_E_ARG;
    if (!zn_patch_input_ok(it.d_patch, it.patch_len)) return ZN_E_ARG;
    if (emit && it.out_cap && (!zn_patch_out_ok(it.d_out) || zn_patch_overlap(it.d_out, it.out_cap, it.d_patch, it.patch_len))) return ZN_E_ARG;
    const uint64_t m_all = (uint64_t)it.rows * it.cols, m_rect = (uint64_t)(it.row_hi - it.row_lo) * (it.col_hi - it.col_lo);
    const uint64_t m_out = place ? m_all : m_rect, nb = zn_patch_blocks(m_out);
    segs[i] = ZnPatchSSeg{(const uint8_t*)it.d_patch, it.patch_len, (uint8_t*)it.d_out, (uint32_t)it.rows, (uint32_t)it.cols, (uint32_t)it.row_lo, (uint32_t)it.row_hi,
                          (uint32_t)it.col_lo, (uint32_t)it.col_hi, (uint32_t)wg, (uint32_t)words, (uint32_t)it.elem, 0u};
    scan[i] = ZnPatchBSeg{nullptr, nullptr, nullptr, m_out, 0u, (uint32_t)words, (uint32_t)it.elem, 0u};
    caps[i] = it.out_cap;
    wg += nb;
    words += nb + 1u;
    if (wg > 0x7FFFFFFFull || words > 0x7FFFFFFFull) return ZN_E_ARG;
  }
  return zn_patch_two_pass(segs, scan.data(), wg, words, emit ? caps.data() : nullptr, lens, stream,
                           [place](const ZnPatchSSeg& one, const ZnPatchSSeg* d, uint32_t n, uint32_t g, uint32_t* wd, uint32_t* st, hipStream_t q) { zn_launch_patch_select_count(place, one, d, n, g, wd, st, q); },
                           [place](const ZnPatchSSeg& one, const ZnPatchSSeg* d, uint32_t n, uint32_t g, uint32_t* wd, uint32_t* st, hipStream_t q) { zn_launch_patch_select_emit(place, one, d, n, g, wd, st, q); });
}

int select_sizes(const zn_patch_select_item* items, size_t count, size_t* sizes_out, bool place, void* stream_) {
  try {
    if (count == 0) return ZN_OK;
    if (!items || !sizes_out) return ZN_E_ARG;
    std::vector<uint64_t> lens;
    const int rc = patch_select(items, count, lens, place, false, (hipStream_t)stream_);
    if (rc) return rc;
    for (size_t i = 0; i < count; i++) sizes_out[i] = (size_t)lens[i];
    return ZN_OK;
  } catch (...) { return ZN_E_ALLOC; }
}

int select_run(zn_patch_select_item* items, size_t count, bool place, void* stream_) {
  try {
    if (count == 0) return ZN_OK;
    if (!items) return ZN_E_ARG;
    for (size_t i = 0; i < count; i++) items[i].out_len = 0;
    std::vector<uint64_t> lens;
    const int rc = patch_select(items, count, lens, place, true, (hipStream_t)stream_);
    if (rc == ZN_OK || rc == ZN_E_CAP) for (size_t i = 0; i < count; i++) items[i].out_len = (size_t)lens[i];       // (ZN_E_CAP: the lengths that were needed; nothing was written)
    return rc;
  } catch (...) { return ZN_E_ALLOC; }
}

}  // namespace

extern "C" {

int zn_patch_select_size_batch_dev(const zn_patch_select_item* items, size_t count, size_t* sizes_out, void* stream) { return select_sizes(items, count, sizes_out, false, stream); }
int zn_patch_select_batch_dev(zn_patch_select_item* items, size_t count, void* stream) { return select_run(items, count, false, stream); }
int zn_patch_place_size_batch_dev(const zn_patch_select_item* items, size_t count, size_t* sizes_out, void* stream) { return select_sizes(items, count, sizes_out, true, stream); }
int zn_patch_place_batch_dev(zn_patch_select_item* items, size_t count, void* stream) { return select_run(items, count, true, stream); }

}  // extern "C"
