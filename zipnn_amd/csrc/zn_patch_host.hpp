// zn_patch_host.hpp — what the host side of every "znp1" entry point shares (zn_patch.hip, zn_patch_merge.hip, zn_patch_select.hip): the argument checks, the
// staging of a launch's table, and the two-pass driver of the operations that produce patches.
#pragma once

#include "zn_workspace.hpp"
#include "zn_patch_format.hpp"

#include <type_traits>
#include <vector>

// an element size of the format and fewer than 2^32 elements; … as n bytes, which are whole elements
static inline bool zn_patch_count_ok(int elem, uint64_t m) { return (elem == 1 || elem == 2 || elem == 4) && m < (1ull << 32); }
static inline bool zn_patch_elem_ok(size_t n, int elem) { return zn_patch_count_ok(elem, elem > 0 ? n / (size_t)elem : 0u) && n % (size_t)elem == 0; }
// where a patch is written: 16-byte aligned; where one is read: … and a header's worth of bytes
static inline bool zn_patch_out_ok(const void* p) { return p && (((uintptr_t)p) & 15u) == 0; }
static inline bool zn_patch_input_ok(const void* p, size_t len) { return zn_patch_out_ok(p) && len >= 32u; }
static inline bool zn_patch_overlap(const void* p, size_t pn, const void* q, size_t qn) { return (uintptr_t)p < (uintptr_t)q + qn && (uintptr_t)q < (uintptr_t)p + pn; }

// `bytes` of a table through the pinned staging buffer into WS_SEGS at byte offset `at`; the caller has synchronised with the buffer's last reader
static inline int zn_patch_stage(Workspace& w, const void* table, size_t bytes, size_t at, hipStream_t stream) {
  memcpy((uint8_t*)w.h_segs.p + at, table, bytes);
  ZN_HIP(hipMemcpyAsync((uint8_t*)w.buf[WS_SEGS] + at, (uint8_t*)w.h_segs.p + at, bytes, hipMemcpyHostToDevice, stream));
  return ZN_OK;
}

// The two passes of an operation that produces patches: count, scan, one read-back of every item's T; with `caps` (the items' output capacities; null = a size
// call): capacity check, then the emit pass for the items that keep entries.  Synchronous.  lens[i] = the length of item i's output, 0 where it has no entry.
//   segs    the operation's items, wg0 / w0 filled for the count grid of `wg` workgroups over `words` scratch words; the driver renumbers wg0 for the emit grid
//   scan    zn_k_patch_scan's view of the same items: the OUTPUT's m and E, and w0.  The build's items are that view themselves (S = ZnPatchBSeg, scan =
//           segs.data()): one table serves count and scan.  Every other segment type has a table of its own for the scan.  Those that read patches, which may
//           be malformed (ZnPatchSegTraits<S>::reads_patches), also have a verdict word behind the totals that both passes may raise (ZN_E_CORRUPT; after the
//           count pass before any capacity is looked at); the strided build reads tensors and has none (its launchers receive a null d_status).
//   launch_count / launch_emit (one, d_segs, nseg, total_wg, d_words, d_status, stream)
template <typename S, typename Count, typename Emit>
int zn_patch_two_pass(std::vector<S>& segs, const ZnPatchBSeg* scan, uint64_t wg, uint64_t words, const size_t* caps, std::vector<uint64_t>& lens, hipStream_t stream,
                      Count launch_count, Emit launch_emit) {
  constexpr bool reads = ZnPatchSegTraits<S>::reads_patches, own_scan = !std::is_same<S, ZnPatchBSeg>::value;
  const size_t count = segs.size();
  WsLease L;
  if (L.rc) return L.rc;
  Workspace& w = *L.w;
  t_kernels.clear();
  int rc;
  const bool table = count > 1;
  const size_t seg_bytes = table ? count * sizeof(S) : 0u, scan_bytes = table && own_scan ? count * sizeof(ZnPatchBSeg) : 0u;
  const size_t table_bytes = 2u * seg_bytes + scan_bytes;                        // count table, scan table, emit table (the emit pass has a grid of its own)
  const size_t back_bytes = (count + (reads ? 1u : 0u)) * sizeof(uint64_t);      // every item's T, and the verdict word behind them
  if ((rc = w.reserve(WS_META_A, words * sizeof(uint32_t)))) return rc;
  if ((rc = w.reserve(WS_TOTALS, back_bytes))) return rc;
  if ((rc = w.h_totals.reserve(back_bytes))) return rc;
  if (table && (rc = w.reserve(WS_SEGS, table_bytes))) return rc;
  if ((rc = L.acquire(stream))) return rc;
  L.mark = table;
  uint32_t* d_words = (uint32_t*)w.buf[WS_META_A];
  uint64_t* d_totals = (uint64_t*)w.buf[WS_TOTALS];
  uint32_t* d_status = reads ? (uint32_t*)(d_totals + count) : nullptr;
  if (reads) ZN_HIP(hipMemsetAsync(d_status, 0, sizeof(uint64_t), stream));
  if (table) {
    ZN_HIP(hipEventSynchronize(w.busy));         // the previous batched call may still be reading the pinned staging
    if ((rc = w.h_segs.reserve(table_bytes))) return rc;
    if ((rc = zn_patch_stage(w, segs.data(), seg_bytes, 0, stream))) return rc;
    if (own_scan && (rc = zn_patch_stage(w, scan, scan_bytes, seg_bytes, stream))) return rc;
  }
  const uint8_t* d_tab = (const uint8_t*)w.buf[WS_SEGS];
  launch_count(segs[0], table ? (const S*)d_tab : nullptr, (uint32_t)count, (uint32_t)wg, d_words, d_status, stream);
  zn_launch_patch_scan(scan[0], table ? (const ZnPatchBSeg*)(d_tab + (own_scan ? seg_bytes : 0u)) : nullptr, (uint32_t)count, d_words, d_totals, stream);
  if (launch_failed()) return ZN_E_HIP;
  ZN_HIP(hipMemcpyAsync(w.h_totals.p, d_totals, back_bytes, hipMemcpyDeviceToHost, stream));
  ZN_HIP(hipStreamSynchronize(stream));
  const uint64_t* T = (const uint64_t*)w.h_totals.p;
  if (reads && ((uint32_t)T[count] & ZN_DEV_CORRUPT)) return ZN_E_CORRUPT;
  bool short_cap = false;
  for (size_t i = 0; i < count; i++) {
    lens[i] = T[i] ? zn_patch_total(scan[i].m, scan[i].E, T[i]) : 0u;
    if (caps && lens[i] > caps[i]) short_cap = true;
  }
  if (!caps) return ZN_OK;
  if (short_cap) return ZN_E_CAP;
  uint64_t ewg = 0;
  for (size_t i = 0; i < count; i++) { segs[i].wg0 = (uint32_t)ewg; if (T[i]) ewg += zn_patch_blocks(scan[i].m); }
  if (ewg == 0) return ZN_OK;
  // (the first tables' copies are over — the stream was synchronised —; the emit table goes behind them)
  if (table && (rc = zn_patch_stage(w, segs.data(), seg_bytes, seg_bytes + scan_bytes, stream))) return rc;
  launch_emit(segs[0], table ? (const S*)(d_tab + seg_bytes + scan_bytes) : nullptr, (uint32_t)count, (uint32_t)ewg, d_words, d_status, stream);
  if (launch_failed()) return ZN_E_HIP;
  if (reads) ZN_HIP(hipMemcpyAsync(w.h_totals.p, d_status, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));      // an input that changed under the call
  ZN_HIP(hipStreamSynchronize(stream));
  return reads && ((uint32_t)T[0] & ZN_DEV_CORRUPT) ? ZN_E_CORRUPT : ZN_OK;
}
