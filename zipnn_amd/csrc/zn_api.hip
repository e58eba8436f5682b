// zn_api.hip — the C ABI of libzipnn_hip.so (include/zipnn_hip.h).
//
// Host-side control only: argument checks, per-device workspace cache, kernel launches,
// the one 8-byte read-back of the compressed length.  All data work is in the kernels.
#include "zn_workspace.hpp"

#include <memory>
#include <atomic>
#include <thread>
#include <chrono>
#include <vector>
#include <unordered_map>

thread_local std::string t_hip_err;
thread_local std::string t_kernels;
std::mutex g_dev_mu[64];
Workspace g_ws[64];
std::mutex g_host_mu[64];
HostPath g_host[64];

namespace {

// which status slot the calling thread's last check = 0 decode used (zn_decode_status): device, slot, the slot's generation at that call
thread_local int t_status_dev = -1;
thread_local uint32_t t_status_slot = 0;
thread_local uint64_t t_status_gen = 0;
thread_local int t_status_chain = 0;          // zn_decode_status_chain: this thread's unchecked decode calls add to the status slot of its previous one

int check_geom(size_t n, int num_buf, int bytes_mode, size_t chunk, ZnGeom* g, int bits_mode) {
  if (!(num_buf == 1 || num_buf == 2 || num_buf == 4)) return ZN_E_ARG;
  if ((num_buf == 4 && bytes_mode != 220) || (num_buf != 4 && bytes_mode != 10)) return ZN_E_ARG;
  if (chunk == 0 || (chunk % (size_t)num_buf) != 0 || chunk > (1ull << 31)) return ZN_E_ARG;
  g->n = n; g->chunk = chunk; g->K = (n + chunk - 1) / chunk; g->P = (uint32_t)num_buf;
  g->rot = (bits_mode == 1 && num_buf > 1) ? 1u : 0u;
  if (g->K * (uint64_t)num_buf > 0x7FFFFFFFull) return ZN_E_ARG;
  return ZN_OK;
}

}  // namespace

void zn_note_kernel(const char* name) { if (!t_kernels.empty()) t_kernels += ";"; t_kernels += name; }

extern "C" {

int zn_abi_version(void) { return 3; }

const char* zn_strerror(int s) {
  switch (s) {
    case ZN_OK: return "ok";
    case ZN_E_ARG: return "bad argument";
    case ZN_E_HIP: return "HIP runtime call failed";
    case ZN_E_CAP: return "destination capacity too small";
    case ZN_E_CORRUPT: return "compressed data is corrupt";
    case ZN_E_TYPE: return "Compress Type is not correct in Decompression function";
    case ZN_E_NODEV: return "no HIP device";
    case ZN_E_ALLOC: return "allocation failed";
    case ZN_E_TIMEOUT: return "a device-side wait between workgroups timed out";
    default: return "unknown status";
  }
}

const char* zn_last_hip_error(void) { return t_hip_err.c_str(); }
const char* zn_last_kernels(void) { return t_kernels.c_str(); }

int zn_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

size_t zn_num_chunks(size_t n, size_t chunk) { return chunk ? (n + chunk - 1) / chunk : 0; }

size_t zn_compress_bound(size_t n, int num_buf, size_t chunk, size_t hdr_len) {
  return hdr_len + 9u * (size_t)num_buf * zn_num_chunks(n, chunk) + n;
}

// Which of the two huff0 forms of a tree description the encoder writes (both decode with every huff0): 0 = zstd >= 1.4.7's (the
// default; what the oracle's pin and the reference built against a current libzstd write), 1 = the FiniteStateEntropy library's, which
// the reference's PyPI wheels bundle: weight counts that round below one FSE cell as -1 markers.  Process-wide.
static std::atomic<int> g_legacy_weights{0};
int zn_set_legacy_tree_descriptions(int on) {
  if (on != 0 && on != 1) return ZN_E_ARG;
  g_legacy_weights.store(on, std::memory_order_relaxed);
  return ZN_OK;
}

// The one-pass encoder (zn_k_encode_onepass): 0 = never (the four-kernel encoder only), 1 (default) = automatic — where it has measured faster: calls whose
// two-plane, sign-rotated tensors (bf16) bring at least ZN_ONEPASS_MIN_CHUNKS full chunks (profiles/r05_encoder_onepass.txt: 4 GiB 2.17 vs 2.27 ms,
// 2 GiB 1.145 vs 1.183, 1 GiB 0.633 vs 0.625; fp16 / fp32 / fp8 lose 9-30 % to it: longer table builds inside the workgroup) —, 2 = every call with
// full chunks (tests).  ZIPNN_AMD_ONEPASS=0/1/2 in the environment sets the default of a process.  The four-kernel encoder takes over whenever the
// one-pass kernel's layout speculation fails.  (Developer / test knob.)
#define ZN_ONEPASS_MIN_CHUNKS 6144u
static std::atomic<int> g_encode_onepass{-1};
static int zn_encode_onepass_mode() {
  int v = g_encode_onepass.load(std::memory_order_relaxed);
  if (v < 0) { const char* e = getenv("ZIPNN_AMD_ONEPASS"); v = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 1; g_encode_onepass.store(v, std::memory_order_relaxed); }
  return v;
}
extern "C" int zn_set_encode_onepass(int mode) {
  if (mode < 0 || mode > 2) return ZN_E_ARG;
  g_encode_onepass.store(mode, std::memory_order_relaxed);
  return ZN_OK;
}

// Compress `count` tensors: one launch per stage and plane count over all of them (a single tensor travels to the
// kernels as an argument, a batch as a segment table), one read-back of all body lengths.
struct EncodeSet {                               // what a compress call launches: the segments of its tensors by plane count, and the grid totals
  std::vector<ZnESeg> segs[3];                   // by plane count: 1, 2, 4
  uint64_t pc_all = 0, slot_all = 0; size_t slot = 0, count = 0;
  uint64_t chunks_of[3] = {0, 0, 0}, jobs_of[3] = {0, 0, 0}, tails_of[3] = {0, 0, 0}, ptails_of[3] = {0, 0, 0}, scan_of[3] = {0, 0, 0};
  bool delta_of[3] = {false, false, false};
  size_t nseg() const { return segs[0].size() + segs[1].size() + segs[2].size(); }
};
static int build_encode_set(zn_cbatch_item* items, size_t count, EncodeSet& E) {
  if (count && !items) return ZN_E_ARG;
  E.count = count;
  for (size_t i = 0; i < count; i++) {
    zn_cbatch_item& it = items[i];
    ZnESeg sg; memset(&sg, 0, sizeof(sg));
    int rc = check_geom(it.n, it.num_buf, it.bytes_mode, it.chunk, &sg.g, it.bits_mode);
    if (rc) return rc;
    if (it.n && (!it.d_src || !it.d_body)) return ZN_E_ARG;
    if (it.body_cap < zn_compress_bound(it.n, it.num_buf, it.chunk, 0)) return ZN_E_CAP;
    it.body_len = 0;
    const int q = zn_class_of(sg.g.P);
    const uint64_t PK = (uint64_t)sg.g.P * sg.g.K;
    sg.src = (const uint8_t*)it.d_src; sg.body = (uint8_t*)it.d_body; sg.threshold = it.threshold;
    sg.legacy_weights = g_legacy_weights.load(std::memory_order_relaxed) ? 1u : 0u;
    sg.xr = it.n ? (const uint8_t*)it.d_delta : nullptr;
    if (sg.xr) E.delta_of[q] = true;
    // full chunks go through the fused encoder, the partial tail (or everything, for geometries the fused
    // kernels do not take) through the generic one
    sg.nfull = zn_encode_fused_ok(sg.g, it.d_src, sg.xr) ? (uint64_t)(it.n / it.chunk) : 0;
    const uint64_t KL = sg.g.K - sg.nfull;
    sg.pc0 = E.pc_all; sg.slot0 = E.slot_all; sg.total_idx = i;
    uint32_t blocks = 0; zn_scan_geometry(PK, &sg.T, &blocks);
    sg.chunk0 = (uint32_t)E.chunks_of[q]; sg.job0 = (uint32_t)E.jobs_of[q]; sg.tail0 = (uint32_t)E.tails_of[q];
    sg.ptail0 = (uint32_t)E.ptails_of[q]; sg.scan0 = (uint32_t)E.scan_of[q];
    E.chunks_of[q] += sg.nfull; E.jobs_of[q] += sg.nfull * sg.g.P; E.tails_of[q] += KL; E.ptails_of[q] += KL * sg.g.P; E.scan_of[q] += blocks;
    E.pc_all += PK; E.slot_all += KL * sg.g.P;
    const size_t sl = zn_plane_slot(it.chunk, it.num_buf);
    if (sl > E.slot) E.slot = sl;                // one slot stride for the whole launch
    if (E.jobs_of[q] > 0x7FFFFFFFull || E.ptails_of[q] > 0x7FFFFFFFull || E.pc_all > 0x7FFFFFFFFFull) return ZN_E_ARG;
    E.segs[q].push_back(sg);
  }
  return ZN_OK;
}
// Which plane counts' full chunks go through the one-pass kernel in this call (op_of, by plane count); counts the device's back-off down.
// The one-pass encoder takes the full chunks of the call when every tensor's prefix sums fit its look-back words (40 bits)
static bool onepass_choice(const EncodeSet& E, Workspace& w, bool op_of[3]) {
  const int op_mode = zn_encode_onepass_mode();
  for (int q = 0; q < 3; q++) {
    op_of[q] = false;
    if (op_mode == 0 || E.chunks_of[q] == 0) continue;
    bool ok = true, rot = true;
    for (const ZnESeg& sg : E.segs[q]) { if (sg.g.n >= (1ull << 38)) ok = false; if (sg.nfull && !sg.g.rot) rot = false; }
    // automatic mode: plain weights only.  A call with a delta base (XOR of a fine-tuned checkpoint: both planes compress) breaks the layout speculation almost
    // always, and a misspeculation costs the whole call twice — so delta calls never take it, and after a misspeculated call the device sits out
    // `op_backoff` automatic calls (8, doubling up to 1 024 while misspeculations keep coming; a call that speculated right halves the penalty)
    const bool auto_ok = q == 1 && rot && !E.delta_of[q] && E.chunks_of[q] >= ZN_ONEPASS_MIN_CHUNKS;
    if (op_mode == 1 && auto_ok && w.op_backoff > 0) { w.op_backoff--; continue; }
    op_of[q] = ok && (op_mode == 2 || auto_ok);
  }
  return op_of[0] || op_of[1] || op_of[2];
}
// One pass over the launches; `op`: the full chunks of the plane counts in op_of through the one-pass encoder (their ragged planes, if any, through the ragged
// workgroups of the three fused launches), else everything through the four-kernel encoder.  Ends with the copy of the body lengths + the status word.
static int launch_encode(const EncodeSet& E, Workspace& w, bool op, const bool op_of[3], hipStream_t stream) {
  const size_t count = E.count;
  const bool table = E.nseg() > 1;
  uint64_t* d_totals = (uint64_t*)w.buf[WS_TOTALS];
  uint32_t* d_status = (uint32_t*)(d_totals + count);
  uint32_t* d_csize = (uint32_t*)w.buf[WS_META_A]; uint8_t* d_type = (uint8_t*)w.buf[WS_META_B]; uint64_t* d_offs = (uint64_t*)w.buf[WS_META_C];
  bool status_zeroed = false;                    // (by the first table kernel of the call; a memset only when none is launched — or in front of the one-pass kernel, which may set bits)
  if (op) {
    ZN_HIP(hipMemsetAsync(d_status, 0, 4 * sizeof(uint64_t), stream));      // the status word and the three ticket counters behind it
    status_zeroed = true;
  }
  uint64_t lb_base = 0;
  for (int stage = 0; stage < 3; stage++) {      // stats (fused + generic) for every plane count, then the scans, then emit / gather
    size_t seg_base = 0;
    if (stage == 1 && !status_zeroed) { ZN_HIP(hipMemsetAsync(d_status, 0, sizeof(uint32_t), stream)); status_zeroed = true; }
    for (int q = 0; q < 3; q++) {
      if (E.segs[q].empty()) continue;
      const int P = zn_planes_of(q);
      const ZnESeg* d_segs = table ? (const ZnESeg*)w.buf[WS_SEGS] + seg_base : nullptr;
      const uint32_t nseg = (uint32_t)E.segs[q].size();
      const ZnESeg& one = E.segs[q][0];
      const bool opq = op && op_of[q];
      if (stage == 0) {
        if (zn_launch_encode_fused_stats(P, one, d_segs, nseg, opq ? 0u : (uint32_t)E.chunks_of[q], opq ? 0u : (uint32_t)E.jobs_of[q], (uint32_t)E.ptails_of[q], (uint8_t*)w.buf[WS_PLANES], E.slot,
                                         d_csize, d_type, (ZnEncDesc*)w.buf[WS_DESC], E.delta_of[q], status_zeroed ? nullptr : d_status, stream)) status_zeroed = true;
        if (opq) {
          w.lb_gen = (w.lb_gen + 1u) & 0x3FFFFFu;
          if (w.lb_gen == 0) { ZN_HIP(hipMemsetAsync(w.buf[WS_LB], 0, w.cap[WS_LB], stream)); w.lb_gen = 1; }       // (the tag has wrapped: forget every older word)
          zn_launch_encode_onepass(P, one, d_segs, nseg, (uint32_t)E.chunks_of[q], d_csize, d_type, (uint64_t*)w.buf[WS_LB] + lb_base,
                                   (uint32_t*)(d_totals + count + 1 + q), d_status, w.lb_gen, E.delta_of[q], stream);
          lb_base += E.chunks_of[q];
        }
      } else if (stage == 1) {
        zn_launch_scan_sizes(one, d_segs, nseg, (uint32_t)E.scan_of[q], d_csize, d_type, d_offs, d_totals, opq ? d_status : nullptr, stream);
      } else {
        zn_launch_encode_fused_emit(P, one, d_segs, nseg, opq ? 0u : (uint32_t)E.chunks_of[q], (uint32_t)E.ptails_of[q], (const uint8_t*)w.buf[WS_PLANES], E.slot,
                                    d_csize, d_type, d_offs, (const ZnEncDesc*)w.buf[WS_DESC], d_status, E.delta_of[q], stream);
      }
      seg_base += nseg;
    }
  }
  if (launch_failed()) return ZN_E_HIP;
  ZN_HIP(hipMemcpyAsync(w.h_totals.p, d_totals, (count + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));     // body lengths + the status word
  return ZN_OK;
}
static int compress_items(zn_cbatch_item* items, size_t count, hipStream_t stream) {
  EncodeSet E;
  int rc = build_encode_set(items, count, E);
  if (rc || count == 0) return rc;
  WsLease L;
  if (L.rc) return L.rc;
  Workspace& w = *L.w;
  t_kernels.clear();
  const size_t nseg_all = E.nseg(), pc_all = E.pc_all;
  const bool table = nseg_all > 1;
  if ((rc = w.reserve(WS_PLANES, E.slot_all * E.slot))) return rc;
  if ((rc = w.reserve(WS_META_A, pc_all * sizeof(uint32_t)))) return rc;   // stored sizes
  if ((rc = w.reserve(WS_META_B, pc_all))) return rc;                      // types
  if ((rc = w.reserve(WS_META_C, pc_all * sizeof(uint64_t)))) return rc;   // payload offsets
  if ((rc = w.reserve(WS_DESC, pc_all * sizeof(ZnEncDesc)))) return rc;
  if ((rc = w.reserve(WS_WORDS, ZN_WORDS_BYTES))) return rc;
  // (one slot more than there are tensors: the call's status word rides behind the body lengths, so that both come back in ONE copy)
  if ((rc = w.reserve(WS_TOTALS, (count + 4) * sizeof(uint64_t)))) return rc;      // (… and the one-pass encoder's three ticket counters behind that)
  if ((rc = w.host_words())) return rc;
  if ((rc = w.h_totals.reserve((count + 1) * sizeof(uint64_t)))) return rc;
  if (table) {
    if ((rc = w.reserve(WS_SEGS, nseg_all * sizeof(ZnESeg)))) return rc;
    if ((rc = w.h_segs.reserve(nseg_all * sizeof(ZnESeg)))) return rc;
  }
  bool op_of[3];                                 // by plane count: this call's full chunks of that plane count go through the one-pass kernel
  const bool onepass = onepass_choice(E, w, op_of);
  if (onepass) {
    const size_t had = w.cap[WS_LB];
    if ((rc = w.reserve(WS_LB, (E.chunks_of[0] + E.chunks_of[1] + E.chunks_of[2]) * sizeof(uint64_t)))) return rc;
    if (w.cap[WS_LB] != had) { ZN_HIP(hipMemset(w.buf[WS_LB], 0, w.cap[WS_LB])); w.lb_gen = 0; }      // (a fresh array: no word of any generation)
  }
  if ((rc = L.acquire(stream))) return rc;
  L.mark = table;
  if (table) {
    ZN_HIP(hipEventSynchronize(w.busy));         // the previous batched call may still be reading the pinned staging
    ZnESeg* hs = (ZnESeg*)w.h_segs.p; size_t o = 0;
    for (int q = 0; q < 3; q++) for (const ZnESeg& sg : E.segs[q]) hs[o++] = sg;
    ZN_HIP(hipMemcpyAsync(w.buf[WS_SEGS], hs, nseg_all * sizeof(ZnESeg), hipMemcpyHostToDevice, stream));
  }
  const uint64_t* h_totals = (const uint64_t*)w.h_totals.p;
  if ((rc = launch_encode(E, w, onepass, op_of, stream))) return rc;
  if (onepass) {
    ZN_HIP(hipStreamSynchronize(stream));
    if ((uint32_t)h_totals[count] & (ZN_DEV_MISSPEC | ZN_DEV_SYNC_TIMEOUT)) {    // a tensor that does not look like weights: its bytes are where a decoder would not look for them
      const bool timed_out = ((uint32_t)h_totals[count] & ZN_DEV_SYNC_TIMEOUT) != 0;      // (… or a look-back that gave up waiting: the four-kernel encoder waits for nobody)
      w.op_penalty = w.op_penalty ? (w.op_penalty < 1024u ? 2u * w.op_penalty : 1024u) : 8u;
      w.op_backoff = w.op_penalty;
      if ((rc = launch_encode(E, w, false, op_of, stream))) return rc;
      zn_note_kernel(timed_out ? "(one-pass look-back timed out: four-kernel encoder)" : "(one-pass speculation failed: four-kernel encoder)");
    } else if (w.op_penalty) w.op_penalty >>= 1;
  }
  ZN_HIP(hipStreamSynchronize(stream));
  for (size_t i = 0; i < count; i++) items[i].body_len = (size_t)h_totals[i];
  if ((uint32_t)h_totals[count]) return ZN_E_CORRUPT;   // internal consistency check of the encoder failed
  return ZN_OK;
}

int zn_compress_delta_dev(const void* d_src, const void* d_delta, size_t n, int num_buf, int bits_mode, int bytes_mode, size_t chunk,
                          float threshold, void* d_body, size_t body_cap, size_t* body_len, void* stream_) {
  if (!body_len) return ZN_E_ARG;
  zn_cbatch_item it; it.d_delta = d_delta;
  it.d_src = d_src; it.n = n; it.num_buf = num_buf; it.bits_mode = bits_mode; it.bytes_mode = bytes_mode; it.chunk = chunk;
  it.threshold = threshold; it.d_body = d_body; it.body_cap = body_cap; it.body_len = 0;
  int rc;
  try { rc = compress_items(&it, 1, (hipStream_t)stream_); } catch (...) { return ZN_E_ALLOC; }
  *body_len = it.body_len;
  return rc;
}

int zn_compress_dev(const void* d_src, size_t n, int num_buf, int bits_mode, int bytes_mode, size_t chunk,
                    float threshold, void* d_body, size_t body_cap, size_t* body_len, void* stream_) {
  return zn_compress_delta_dev(d_src, nullptr, n, num_buf, bits_mode, bytes_mode, chunk, threshold, d_body, body_cap, body_len, stream_);
}

int zn_compress_batch_dev(zn_cbatch_item* items, size_t count, void* stream_) {
  try { return compress_items(items, count, (hipStream_t)stream_); } catch (...) { return ZN_E_ALLOC; }
}

// Decode `count` tensors in one set of launches per plane count.  A single tensor travels to the kernels as an
// argument; a batch as a segment table in device memory.
#define ZN_REST_MAX_CHUNKS 2048u          // (512 MiB of 256 KiB chunks)
#define ZN_REST_TAIL_MAX_CHUNKS 24576u    // (6 GiB: a launch WITH partial chunks stays with the rest instance up to here)
// A batch that mixes one-plane tensors (fp8: dense codes, the decode is LDS-bound at a fifth of the HBM roofline) with two- / four-plane ones (memory-bound) decodes
// the two kinds CONCURRENTLY: the one-plane launches go to a second stream, forked from and joined to the caller's with events, so that the dispatcher fills a CU with
// workgroups of both kernels — one kind waits on LDS look-ups while the other waits on HBM.  ZIPNN_AMD_DECODE_OVERLAP=0 keeps everything on the caller's stream.
static int zn_decode_overlap_on() {
  static std::atomic<int> v{-1};
  int x = v.load(std::memory_order_relaxed);
  if (x < 0) { const char* e = getenv("ZIPNN_AMD_DECODE_OVERLAP"); x = (e && e[0] >= '0' && e[0] <= '9') ? e[0] - '0' : 1; v.store(x, std::memory_order_relaxed); }
  return x;
}
// What a decode call launches: the segments of its tensors / chunk windows by plane count, and the form choice.  Built once (build_segments: every argument and
// geometry check, the knobs read), launched by launch_segments — once by the one-shot entry points, any number of times by a plan (zn_plan_run).
struct DecodeSet {
  std::vector<ZnSeg> segs[3];                    // by plane count: 1, 2, 4
  std::vector<ZnHintSeg> hsegs[3];               // a hinted call: entry i = the index of segs[q][i] (hints == null: none), else empty
  bool hinted[3] = {false, false, false};        // … and whether any segment of the plane count has one
  uint64_t pk_of[3] = {0, 0, 0}, k_of[3] = {0, 0, 0}, wg_of[3] = {0, 0, 0}, tail_of[3] = {0, 0, 0};
  bool delta_of[3] = {false, false, false}, rest_ok[3] = {true, true, true};
  bool inplace_rot_of[3] = {false, false, false};   // … and that segment has the sign rotate (zn_k_alias_rotate goes ahead of the generic kernels)
  bool inplace_of[3] = {false, false, false};    // some segment's delta base is its destination (xr == dst: the in-place contract of zipnn_hip.h)
  uint64_t total_chunks = 0;
  int wide = 0;
};
// bytes and chunks of an item's window (arguments not yet checked: clamped, so that nothing here can wrap)
static inline void zn_window_of(const zn_window_item& it, uint64_t* n, uint64_t* k) {
  *n = 0; *k = 0;
  if (!it.chunk) return;
  const uint64_t kb = zn_num_chunks(it.orig_size, it.chunk);
  const uint64_t hi = it.chunk_hi < kb ? it.chunk_hi : kb, lo = it.chunk_lo < hi ? it.chunk_lo : hi;
  const uint64_t end = hi == kb ? (uint64_t)it.orig_size : hi * it.chunk;
  *n = end - lo * it.chunk; *k = hi - lo;
}

// ---- decode hints: sizing ----
// The sizing pass over one whole body: *bytes = the length of its index (offset table + hint bytes); d_offs (may be null) receives the table.  One launch and
// one 8-byte read-back; takes the device's workspace lock.
static int hint_size_run(const zn_window_item& it, const ZnGeom& g, int kind, uint32_t* d_offs, size_t* bytes, hipStream_t stream) {
  WsLease L;
  if (L.rc) return L.rc;
  Workspace& w = *L.w;
  int rc;
  if ((rc = w.reserve(WS_TOTALS, 64))) return rc;
  if ((rc = w.host_words())) return rc;
  if ((rc = L.acquire(stream))) return rc;
  zn_launch_hint_size(g, (const uint8_t*)it.d_body, it.body_len, d_offs, (uint64_t*)w.buf[WS_TOTALS], stream, kind);
  if (launch_failed()) return ZN_E_HIP;
  ZN_HIP(hipMemcpyAsync(w.h_total, w.buf[WS_TOTALS], sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
  ZN_HIP(hipStreamSynchronize(stream));
  const uint64_t total = *w.h_total;
  if (total > 0xFFFFFFFFull) return ZN_E_ARG;      // (the table's offsets are 32 bits: a body of hundreds of GiB)
  *bytes = (size_t)total;
  return ZN_OK;
}
// What the hinted entry points hold a caller's hint_len against: the sizes zn_hint_size_dev / zn_hint_build_dev have worked out, remembered per body (address,
// length, geometry); a body they have not seen is sized on the spot (a read-back: once per body).  Only an argument check — the kernels hold every read of an
// index against the length they are given, whatever this says.
struct HintKey { const void* body; size_t body_len, n, chunk; int P, kind; bool operator==(const HintKey& o) const { return body == o.body && body_len == o.body_len && n == o.n && chunk == o.chunk && P == o.P && kind == o.kind; } };
struct HintKeyHash { size_t operator()(const HintKey& k) const { return std::hash<const void*>()(k.body) ^ (k.body_len * 0x9E3779B97F4A7C15ull) ^ (k.n << 1) ^ (size_t)k.P ^ ((size_t)k.kind << 8); } };
static std::mutex g_hint_mu;
static std::unordered_map<HintKey, size_t, HintKeyHash> g_hint_sizes;
static void hint_size_remember(const zn_window_item& it, const ZnGeom& g, int kind, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_hint_mu);
  if (g_hint_sizes.size() > (1u << 20)) g_hint_sizes.clear();
  g_hint_sizes[HintKey{it.d_body, it.body_len, it.orig_size, it.chunk, (int)g.P, kind}] = bytes;
}
static int hint_size_cached(const zn_window_item& it, const ZnGeom& g, int kind, size_t* bytes) {
  {
    std::lock_guard<std::mutex> lk(g_hint_mu);
    auto f = g_hint_sizes.find(HintKey{it.d_body, it.body_len, it.orig_size, it.chunk, (int)g.P, kind});
    if (f != g_hint_sizes.end()) { *bytes = f->second; return ZN_OK; }
  }
  const int rc = hint_size_run(it, g, kind, nullptr, bytes, nullptr);
  if (rc == ZN_OK) hint_size_remember(it, g, kind, *bytes);
  return rc;
}

// hints (may be null): one entry per item; kinds (may be null: every index is ZN_HINT_PLAIN): the kind of each
static int build_segments(const zn_window_item* items, size_t count, DecodeSet& D, const ZnHintSeg* hints = nullptr, const int* kinds = nullptr) {
  if (count && !items) return ZN_E_ARG;
  std::vector<ZnSeg>* segs = D.segs;
  uint64_t* pk_of = D.pk_of; uint64_t* k_of = D.k_of; uint64_t* wg_of = D.wg_of; uint64_t* tail_of = D.tail_of;
  bool* delta_of = D.delta_of; bool* rest_ok = D.rest_ok;
  uint64_t total_chunks = 0;
  bool any_delta = false;
  uint64_t full_chunks = 0; bool all_rotated = true; uint64_t tail_wgs = 0;
  uint64_t kq[3] = {0, 0, 0};                    // chunks per launch (one launch per plane count)
  struct Window { uint64_t n, k; };
  std::vector<Window> win(count);                // (a window is a tensor of its own to everything that follows)
  for (size_t i = 0; i < count; i++) {
    zn_window_of(items[i], &win[i].n, &win[i].k);
    const uint64_t wn = win[i].n;
    total_chunks += win[i].k; if (items[i].d_delta) any_delta = true;
    // (FULL chunks: a partial last chunk is the tail workgroups' — the workgroup its group index maps to only skips it, and counting it would push a tensor of exactly
    //  n rounds into n + 1: 6 144 chunks + a tail took single-chunk groups, 0.64 ms, where three-chunk groups take 0.59)
    if (items[i].chunk) kq[zn_class_of((uint32_t)items[i].num_buf)] += wn / items[i].chunk;
    if (items[i].chunk) full_chunks += wn / items[i].chunk;
    // (tensors without the sign rotate — fp16, fp8, integers: their Huffman planes are dense codes, which the wide kernel parses and declines)
    if (!(items[i].bits_mode == 1 && items[i].num_buf > 1)) all_rotated = false;
    // (… a partial last chunk: its tail workgroups ride at the front of the wide launch and its merge workgroups at the end of it, as in a fused launch; the tail
    //  workgroups take workgroup slots of their own — 64 MiB + 250 KB = 256 chunks + 8 took two rounds of the 16-wave form on 256 CUs, 113 µs against the 8-wave form's 73)
    if (items[i].chunk && wn % items[i].chunk) tail_wgs += 4u * (uint64_t)(items[i].num_buf > 0 ? items[i].num_buf : 1) + 32u;      // (… + the tensor's merge workgroups at the end of the grid)
  }
  const int wide = zn_decode_use_wide(full_chunks, any_delta, all_rotated, tail_wgs);       // small calls: a 16-wave workgroup per full chunk (zn_decode_wide.hpp)
  uint32_t ncg_of[3];
  for (int q = 0; q < 3; q++) ncg_of[q] = wide ? 1u : zn_decode_fused_group(kq[q]);
  for (size_t i = 0; i < count; i++) {
    const zn_window_item& it = items[i];
    ZnSeg sg;
    int rc = check_geom(it.orig_size, it.num_buf, it.bytes_mode, it.chunk, &sg.g, it.bits_mode);      // the BODY's geometry …
    if (rc) return rc;
    if (it.chunk_lo > it.chunk_hi || it.chunk_hi > sg.g.K) return ZN_E_ARG;
    ZnHintSeg hseg = {nullptr, 0};
    if (hints) {
      const int kind = kinds ? kinds[i] : ZN_HINT_PLAIN;
      if (kind != ZN_HINT_PLAIN && kind != ZN_HINT_DELTA) return ZN_E_ARG;
      // an index is a pointer AND a length, 16-byte aligned, at least as long as zn_hint_size_dev2 says for this body and kind
      if ((hints[i].hints == nullptr) != (hints[i].len == 0) || (((uintptr_t)hints[i].hints) & 15u) != 0) return ZN_E_ARG;
      if (hints[i].hints && it.d_body && it.body_len >= 9u * (size_t)sg.g.P * sg.g.K) {
        size_t need = 0;
        rc = hint_size_cached(it, sg.g, kind, &need);
        if (rc) return rc;
        if (hints[i].len < need) return ZN_E_ARG;
        // (an item reads the index of ITS instances: a tensor with a delta base a DELTA index, one without a PLAIN index; any other pairing decodes without)
        if ((kind == ZN_HINT_DELTA) == (it.d_delta != nullptr)) hseg = hints[i];
      }
    }
    sg.kb = (uint32_t)sg.g.K; sg.c_lo = (uint32_t)it.chunk_lo;                                        // (check_geom: P·K < 2^31)
    if (it.body_len < 9u * (size_t)sg.g.P * sg.g.K) return ZN_E_CORRUPT;
    if (it.chunk_lo == it.chunk_hi) continue;
    if (!it.d_body || !it.d_dst) return ZN_E_ARG;
    sg.g.n = win[i].n; sg.g.K = win[i].k;                                                             // … and the window's, which is what the kernels decode
    const int q = zn_class_of(sg.g.P);
    const uint32_t ncg = ncg_of[q];
    sg.body = (const uint8_t*)it.d_body; sg.body_len = it.body_len; sg.dst = (uint8_t*)it.d_dst;
    sg.xr = it.d_delta ? (const uint8_t*)it.d_delta + (uint64_t)it.chunk_lo * it.chunk : nullptr;
    if (sg.xr) delta_of[q] = true;
    if (sg.xr && sg.xr == sg.dst) { D.inplace_of[q] = true; if (sg.g.rot) D.inplace_rot_of[q] = true; }
    // (a LARGE call in a geometry the fused kernel takes no chunk of — its rule: whole rows per stream, a 16-byte aligned destination — goes to the generic
    //  KERNELS, which spread it over the whole chip with one wave per plane; the fused kernel's rest instance decodes the odd chunk, or the odd small tensor)
    { const uint64_t unit = 64ull * (sg.g.P == 1 ? 16u : 8u);
      if ((it.chunk % (4ull * sg.g.P * unit) != 0 || (((uintptr_t)it.d_dst) & 15u) != 0) && total_chunks > 1024u) rest_ok[q] = false; }
    sg.chunk0 = (uint32_t)k_of[q]; sg.desc0 = (uint32_t)pk_of[q]; sg.wg0 = (uint32_t)wg_of[q]; sg.ncg = ncg;
    sg.tail0 = (uint32_t)tail_of[q]; sg.has_tail = (sg.g.n % it.chunk) != 0 ? 1u : 0u;   // partial last chunk
    if (sg.has_tail) tail_of[q] += sg.g.P;
    k_of[q] += sg.g.K; pk_of[q] += (uint64_t)sg.g.P * sg.g.K; wg_of[q] += (sg.g.K + ncg - 1u) / ncg;
    if (pk_of[q] > 0x7FFFFFFFull || wg_of[q] > 0x7FFFFFFFull) return ZN_E_ARG;
    segs[q].push_back(sg);
    if (hints) { D.hsegs[q].push_back(hseg); if (hseg.hints) D.hinted[q] = true; }
  }
  // a launch that takes a delta instance reads DELTA indexes only: its segments without a base run through that instance too, and a PLAIN index was built for
  // the plain instance's sub-block sizes
  for (int q = 0; q < 3; q++) if (hints && delta_of[q]) {
    D.hinted[q] = false;
    for (size_t i = 0; i < segs[q].size(); i++) { if (!segs[q][i].xr) D.hsegs[q][i] = ZnHintSeg{nullptr, 0}; else if (D.hsegs[q][i].hints) D.hinted[q] = true; }
  }
  D.total_chunks = total_chunks; D.wide = wide;
  return ZN_OK;
}

// d_table: the segment table already in device memory (a plan's: 1-plane segments, then 2-, then 4-plane ones), or null — the call's own, staged through the
// workspace's pinned buffer, which is the one thing here that makes the host wait for earlier device work.
// d_htable: a hinted plan's table of ZnHintSeg, parallel to d_table (a one-shot hinted call stages its own behind the segment table)
// The steps of launch_segments, in its order.  What a launch reads of the call's tables and flags:
struct DecodeTables {
  const ZnSeg* d_segs = nullptr;                 // the launch-wide segment table (null: at most one segment, which travels as a kernel argument) …
  const ZnHintSeg* d_hsegs = nullptr;            // … and the table of indexes parallel to it
  uint32_t* d_status = nullptr;                  // the call's status slot
  uint32_t* d_tailsync = nullptr;                // two flag words per tensor with a partial chunk
  int wide = 0;
  bool status_zeroed = false;                    // by a memset or by the call's first kernel
};
struct ClassBase { size_t seg; uint64_t k, pk, tail; };      // where a plane count starts in the launch-wide arrays

static int decode_reserve(Workspace& w, uint64_t all_k, uint64_t all_pk, uint64_t all_tail, size_t sync_off, size_t stage_bytes) {
  int rc;
  if ((rc = w.reserve(WS_META_C, all_pk * sizeof(ZnPlaneDesc)))) return rc;
  if ((rc = w.reserve(WS_META_B, all_k))) return rc;                     // per-chunk "done by the fused kernel" flags
  if ((rc = w.reserve(WS_ENC, all_pk))) return rc;                       // … and the same per (plane, chunk)
  if ((rc = w.reserve(WS_PLANES, all_tail * ZN_TAIL_SLOT))) return rc;   // decoded Huffman planes of partial last chunks
  if ((rc = w.reserve(WS_META_A, sync_off + 2u * sizeof(uint32_t) * all_tail))) return rc;
  if ((rc = w.reserve(WS_WORDS, ZN_WORDS_BYTES))) return rc;
  if ((rc = w.host_words())) return rc;
  if (stage_bytes) {                             // (the table goes through the pinned staging buffer)
    if ((rc = w.reserve(WS_SEGS, stage_bytes))) return rc;
    if ((rc = w.h_segs.reserve(stage_bytes))) return rc;
  }
  return ZN_OK;
}
// this call's status slot (status word + the three "left to the generic kernels" counters); the rule zn_decode_status reads the slots by
// (chained, zn_decode_status_chain: the slot of this thread's previous unchecked call on the device, if it is still that call's — the verdicts add up)
static uint32_t* decode_status_slot(Workspace& w, int dev, int check, bool* chain) {
  *chain = !check && t_status_chain && t_status_dev == dev && t_status_gen != 0 && w.slot_gen[t_status_slot] == t_status_gen;
  const uint32_t slot = *chain ? t_status_slot : (uint32_t)(w.status_gen % ZN_STATUS_SLOTS);
  if (!*chain) w.slot_gen[slot] = ++w.status_gen;
  w.last_slot = slot;
  if (!check && !*chain) { t_status_dev = dev; t_status_slot = slot; t_status_gen = w.status_gen; }
  return (uint32_t*)w.buf[WS_WORDS] + 16 + 4u * slot;
}
// the call's own tables through the pinned buffer: the segments, and behind them (any_h) the ZnHintSeg table
static int decode_stage_tables(Workspace& w, const DecodeSet& D, const bool use_h[3], bool any_h, size_t nseg_all, size_t stage_bytes, hipStream_t stream) {
  // the previous batched call may still be reading the pinned staging: wait for it on the host
  ZN_HIP(hipEventSynchronize(w.busy));
  ZnSeg* hs = (ZnSeg*)w.h_segs.p; size_t o = 0;
  for (int q = 0; q < 3; q++) for (const ZnSeg& sg : D.segs[q]) hs[o++] = sg;
  if (any_h) {
    ZnHintSeg* hh = (ZnHintSeg*)(hs + nseg_all); size_t oh = 0;
    for (int q = 0; q < 3; q++) for (size_t i = 0; i < D.segs[q].size(); i++) hh[oh++] = use_h[q] ? D.hsegs[q][i] : ZnHintSeg{nullptr, 0};
  }
  ZN_HIP(hipMemcpyAsync(w.buf[WS_SEGS], hs, stage_bytes, hipMemcpyHostToDevice, stream));
  return ZN_OK;
}
// fork: the side streams wait for what the caller's stream holds so far (the memsets and the segment table)
static int decode_fork(Workspace& w, hipStream_t stream_main) {
  // (TWO streams of our own, created one behind the other — the runtime deals its hardware queues out in turn, so these two do not share one; the caller's stream
  //  may share a queue with either: under torch.distributed, with RCCL's streams in the process, the caller's stream + ONE new stream ran the two kinds one after the
  //  other.  Equal priorities: a higher or a lower one for the fp8 stream measured 4-5 % slower, profiles/r05_llama8b_overlap.txt)
  if (!w.dstream) ZN_HIP(hipStreamCreateWithFlags(&w.dstream, hipStreamNonBlocking));
  if (!w.dstream2) ZN_HIP(hipStreamCreateWithFlags(&w.dstream2, hipStreamNonBlocking));
  if (!w.djoin2) ZN_HIP(hipEventCreateWithFlags(&w.djoin2, hipEventDisableTiming));
  if (!w.dfork) ZN_HIP(hipEventCreateWithFlags(&w.dfork, hipEventDisableTiming));
  if (!w.djoin) ZN_HIP(hipEventCreateWithFlags(&w.djoin, hipEventDisableTiming));
  ZN_HIP(hipEventRecord(w.dfork, stream_main));          // behind the memsets and the segment table
  hipError_t e1 = hipStreamWaitEvent(w.dstream, w.dfork, 0), e2 = hipStreamWaitEvent(w.dstream2, w.dfork, 0);
  if (e1 != hipSuccess || e2 != hipSuccess) { t_hip_err = std::string("hipStreamWaitEvent(fork): ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2); (void)hipGetLastError(); return ZN_E_HIP; }     // (nothing queued on the side streams yet)
  zn_note_kernel("(two streams)");                        // (zn_last_kernels: the launches that follow are split over the two)
  return ZN_OK;
}
// join: the caller's stream waits for both side streams
static int decode_join(Workspace& w, hipStream_t stream_main) {
  hipError_t ej = hipEventRecord(w.djoin, w.dstream);
  if (ej == hipSuccess) ej = hipStreamWaitEvent(stream_main, w.djoin, 0);
  hipError_t ej2 = hipEventRecord(w.djoin2, w.dstream2);
  if (ej2 == hipSuccess) ej2 = hipStreamWaitEvent(stream_main, w.djoin2, 0);
  if (ej == hipSuccess && ej2 == hipSuccess) return ZN_OK;
  // the join itself failed: drain the side streams on the host, so that nothing of this call is still running when it returns
  (void)hipStreamSynchronize(w.dstream); (void)hipStreamSynchronize(w.dstream2);
  t_hip_err = std::string("two-stream join: ") + hipGetErrorString(ej != hipSuccess ? ej : ej2); (void)hipGetLastError();
  return ZN_E_HIP;
}
// The launches of one plane count (q) on `stream`; b: where it starts in the launch-wide arrays.  Returns nothing: a failed launch is found by the caller behind the join.
static void decode_launch_class(const DecodeSet& D, int q, const ClassBase& b, Workspace& w, DecodeTables& t, bool use_h, bool rest_ok, hipStream_t stream) {
  const int P = zn_planes_of(q);
  const ZnSeg& one = D.segs[q][0];
  const ZnSeg* d_segs = t.d_segs ? t.d_segs + b.seg : nullptr;
  const uint32_t nseg = (uint32_t)D.segs[q].size();
  const uint64_t pk = D.pk_of[q], k = D.k_of[q], tails = D.tail_of[q];
  uint8_t* d_done = (uint8_t*)w.buf[WS_META_B] + b.k;
  ZnPlaneDesc* d_descs = (ZnPlaneDesc*)w.buf[WS_META_C] + b.pk;
  uint8_t* d_tails = (uint8_t*)w.buf[WS_PLANES] + b.tail * ZN_TAIL_SLOT;
  uint8_t* d_tail_done = (uint8_t*)w.buf[WS_META_A] + 4u * b.tail;
  uint8_t* d_pdone = (uint8_t*)w.buf[WS_ENC] + b.pk;
  // (behind the wide kernel, in launches without partial chunks, the fused kernel's rest instance also does the generic kernels' job)
  // (round 5, three boxes, interleaved: at 4 GiB the plain instance + the two generic launches behind it decode 1.0-1.4 % FASTER than the rest instance alone —
  //  1.445 / 1.445 / 1.500 against 1.460 / 1.466 / 1.516 ms, profiles/r05_rest_instance_ab.txt —: the generic path's code in its cold paths costs the rest instance
  //  twelve spilled registers.  What it saves is two launches, ≈ 4-8 us: it is the instance of calls of up to ZN_REST_MAX_CHUNKS chunks.)
  // (… unless the launch has partial chunks: their merge workgroups ride in the rest instance — 1.0-1.4 % of a large call — where the plain instance needs the two
  //  generic launches behind it, and the generic merge of ONE partial chunk takes 33 µs: 1 GiB + 200 KB 445 µs that way, 417 this way; 4 GiB + 200 KB 1 573 / 1 555.
  //  From about 6 GiB on the percent outweighs the 33 µs: the Llama-3-8B batch — 16 GB of bf16, its 8 KB norm vectors the partial chunks — 12.12 ms against 11.94)
  if (D.total_chunks > ZN_REST_MAX_CHUNKS && (tails == 0 || k > ZN_REST_TAIL_MAX_CHUNKS)) rest_ok = false;
  if (use_h) {
    // (the plain instance's place — or, with delta bases, the delta instances': tail workgroups at the front, the generic launches behind it)
    zn_launch_decode_hinted(P, 1, one, d_segs, nseg, D.hsegs[q][0], t.d_hsegs ? t.d_hsegs + b.seg : nullptr, (uint32_t)D.wg_of[q], d_done, d_pdone, t.d_status, (uint32_t)tails, d_tails, d_tail_done, stream,
                            D.delta_of[q], D.inplace_of[q]);
    zn_launch_decode_generic(P, one, d_segs, nseg, pk, k, d_descs, t.d_status, d_done, d_pdone, d_tails, d_tail_done, stream, D.delta_of[q] && D.inplace_rot_of[q]);
    t.status_zeroed = true;
    return;
  }
  const bool rest = zn_launch_decode_fused(P, one, d_segs, nseg, (uint32_t)D.wg_of[q], d_done, d_pdone, t.d_status, (uint32_t)tails, d_tails,
                                           d_tail_done, D.delta_of[q], t.wide, t.status_zeroed, rest_ok ? d_descs : nullptr,
                                           tails ? t.d_tailsync + 2u * b.tail : nullptr, stream, D.inplace_of[q]);
  t.status_zeroed = true;
  if (!rest) zn_launch_decode_generic(P, one, d_segs, nseg, pk, k, d_descs, t.d_status, d_done, d_pdone, d_tails, d_tail_done, stream, D.inplace_rot_of[q]);
}

static int launch_segments(const DecodeSet& D, const ZnSeg* d_table, hipStream_t stream, int check, const ZnHintSeg* d_htable = nullptr) {
  const uint64_t all_k = D.k_of[0] + D.k_of[1] + D.k_of[2], all_pk = D.pk_of[0] + D.pk_of[1] + D.pk_of[2], all_tail = D.tail_of[0] + D.tail_of[1] + D.tail_of[2];
  if (all_k == 0) return ZN_OK;
  WsLease L;
  if (L.rc) return L.rc;
  Workspace& w = *L.w;
  t_kernels.clear();
  int rc;
  const size_t nseg_all = D.segs[0].size() + D.segs[1].size() + D.segs[2].size();
  const bool table = nseg_all > 1;
  const bool staged = table && !d_table;        // (the table goes through the pinned staging buffer)
  // hinted launches: per plane count, when some segment has an index its launch reads (build_segments: PLAIN indexes in a launch without delta
  // bases, DELTA indexes in one with) and the wide kernel does not go first
  bool use_h[3]; bool any_h = false;
  for (int q = 0; q < 3; q++) { use_h[q] = D.hinted[q] && !D.wide && D.hsegs[q].size() == D.segs[q].size() && !(table && d_table && !d_htable); any_h = any_h || use_h[q]; }
  const size_t stage_bytes = staged ? nseg_all * sizeof(ZnSeg) + (any_h ? nseg_all * sizeof(ZnHintSeg) : 0u) : 0u;      // staging: the ZnHintSeg table behind the segments
  const size_t sync_off = (4u * all_tail + 15u) & ~(size_t)15u;              // WS_META_A: whether the tail workgroups produced their planes (four flag bytes per plane: one per huff0 stream); behind that two flag words per tensor with a partial chunk
  // 1. reserve
  if ((rc = decode_reserve(w, all_k, all_pk, all_tail, sync_off, stage_bytes))) return rc;
  if ((rc = L.acquire(stream))) return rc;
  L.mark = staged;
  // 2. the status slot
  bool chain;
  DecodeTables t;
  t.d_status = decode_status_slot(w, L.dev, check, &chain);
  t.d_tailsync = (uint32_t*)((uint8_t*)w.buf[WS_META_A] + sync_off);
  t.wide = D.wide;
  if (table) { t.d_segs = d_table ? d_table : (const ZnSeg*)w.buf[WS_SEGS]; t.d_hsegs = d_table ? d_htable : (const ZnHintSeg*)((const ZnSeg*)w.buf[WS_SEGS] + nseg_all); }
  w.last_K = all_k; w.last_tails = all_tail;
  // status + the three "left to the generic kernels" counters (a wide call: its first kernel zeroes them)
  if (chain) { ZN_HIP(hipMemsetAsync(t.d_status + 1, 0, 3 * sizeof(uint32_t), stream)); t.status_zeroed = true; }      // (the counters are this call's; the status word is kept)
  else if (!D.wide || all_tail) { ZN_HIP(hipMemsetAsync(t.d_status, 0, 4 * sizeof(uint32_t), stream)); t.status_zeroed = true; }
  if (all_tail) ZN_HIP(hipMemsetAsync(w.buf[WS_META_A], 0, sync_off + 2u * sizeof(uint32_t) * all_tail, stream));
  // 3. stage the tables
  if (staged && (rc = decode_stage_tables(w, D, use_h, any_h, nseg_all, stage_bytes, stream))) return rc;
  // 4. fork
  const bool overlap = zn_decode_overlap_on() && D.k_of[0] >= 512u && D.k_of[1] + D.k_of[2] >= 512u;      // (both kinds fill the chip: below that the fork and join cost more than they hide)
  if (overlap && (rc = decode_fork(w, stream))) return rc;
  // (from here to the join nothing returns: a failure is remembered, the side streams are joined — or, if even that fails, drained — and THEN the call fails;
  //  kernels already queued on them must not outlive the call's claim on d_dst and the workspace)
  // 5. one set of launches per plane count
  const bool fp8_last = overlap && zn_decode_overlap_on() == 2;
  ClassBase base[3]; { ClassBase b = {0, 0, 0, 0}; for (int q = 0; q < 3; q++) { base[q] = b; b.seg += D.segs[q].size(); b.k += D.k_of[q]; b.pk += D.pk_of[q]; b.tail += D.tail_of[q]; } }
  for (int qi = 0; qi < 3; qi++) {
    const int q = fp8_last ? (qi + 1) % 3 : qi;
    if (!D.segs[q].empty()) decode_launch_class(D, q, base[q], w, t, use_h[q], D.rest_ok[q], !overlap ? stream : (q == 0 ? w.dstream : w.dstream2));
  }
  // 6. join
  if (overlap && (rc = decode_join(w, stream))) return rc;
  // 7. verdict
  if (launch_failed()) return ZN_E_HIP;          // a launch that failed: the workspace is still handed back in stream order (the side streams are joined above)
  if (check) {
    ZN_HIP(hipMemcpyAsync(w.h_status, t.d_status, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    ZN_HIP(hipStreamSynchronize(stream));
    return status_to_rc(*w.h_status);
  }
  return ZN_OK;
}

static int hint_item_geom(const zn_window_item* it, ZnGeom* g) {
  if (!it || !it->d_body) return ZN_E_ARG;
  const int rc = check_geom(it->orig_size, it->num_buf, it->bytes_mode, it->chunk, g, it->bits_mode);
  if (rc) return rc;
  if (it->body_len < 9u * (size_t)g->P * g->K) return ZN_E_CORRUPT;
  return ZN_OK;
}

int zn_hint_size_dev(const zn_window_item* item, size_t* hint_bytes, void* stream_) { return zn_hint_size_dev2(item, ZN_HINT_PLAIN, hint_bytes, stream_); }
int zn_hint_size_dev2(const zn_window_item* item, int kind, size_t* hint_bytes, void* stream_) {
  if (!hint_bytes) return ZN_E_ARG;
  *hint_bytes = 0;
  if (kind != ZN_HINT_PLAIN && kind != ZN_HINT_DELTA) return ZN_E_ARG;
  try {
    ZnGeom g;
    int rc = hint_item_geom(item, &g);
    if (rc) return rc;
    t_kernels.clear();
    rc = hint_size_run(*item, g, kind, nullptr, hint_bytes, (hipStream_t)stream_);
    if (rc == ZN_OK) hint_size_remember(*item, g, kind, *hint_bytes);
    return rc;
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_hint_build_dev(const zn_window_item* item, void* d_hints, size_t hint_cap, void* stream_) { return zn_hint_build_dev2(item, ZN_HINT_PLAIN, d_hints, hint_cap, stream_); }
int zn_hint_build_dev2(const zn_window_item* item, int kind, void* d_hints, size_t hint_cap, void* stream_) {
  if (kind != ZN_HINT_PLAIN && kind != ZN_HINT_DELTA) return ZN_E_ARG;
  try {
    ZnGeom g;
    int rc = hint_item_geom(item, &g);
    if (rc) return rc;
    if (!d_hints || (((uintptr_t)d_hints) & 15u) != 0 || hint_cap < zn_hint_header_bytes_host((uint64_t)g.P * g.K)) return ZN_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    t_kernels.clear();
    // the table first (it is the head of the buffer: what fits the smallest legal capacity), and with it the size the bytes need
    size_t need = 0;
    rc = hint_size_run(*item, g, kind, (uint32_t*)d_hints, &need, stream);
    if (rc) return rc;
    hint_size_remember(*item, g, kind, need);
    if (hint_cap < need) return ZN_E_ARG;
    if (g.K == 0) return ZN_OK;
    WsLease L;
    if (L.rc) return L.rc;
    Workspace& w = *L.w;
    const uint64_t pk = (uint64_t)g.P * g.K;
    if ((rc = w.reserve(WS_META_B, g.K))) return rc;
    if ((rc = w.reserve(WS_ENC, pk))) return rc;
    if ((rc = w.reserve(WS_WORDS, ZN_WORDS_BYTES))) return rc;
    if ((rc = L.acquire(stream))) return rc;
    // (hint bytes of tiles the build does not reach — chunks it declines, slack of the tile bound — are zero: deterministic, and as good a guess as any)
    ZN_HIP(hipMemsetAsync((uint8_t*)d_hints + zn_hint_header_bytes_host(pk), 0, need - zn_hint_header_bytes_host(pk), stream));
    ZnSeg sg;
    sg.g = g; sg.body = (const uint8_t*)item->d_body; sg.body_len = item->body_len; sg.dst = nullptr;
    sg.chunk0 = 0; sg.kb = (uint32_t)g.K; sg.desc0 = 0; sg.c_lo = 0; sg.wg0 = 0; sg.ncg = zn_decode_fused_group(g.K);
    sg.tail0 = 0; sg.has_tail = (g.n % g.chunk) != 0 ? 1u : 0u; sg.xr = nullptr;
    // (the status words of a build are the first 16 bytes of the words buffer — no decode slot: a damaged body builds hints of whatever it holds, and the decode says so)
    uint32_t* d_status = (uint32_t*)w.buf[WS_WORDS];
    ZN_HIP(hipMemsetAsync(d_status, 0, 4 * sizeof(uint32_t), stream));
    const ZnHintSeg hs = {(uint8_t*)d_hints, (uint64_t)need};
    zn_launch_decode_hinted((int)g.P, 2, sg, nullptr, 1, hs, nullptr, (uint32_t)((g.K + sg.ncg - 1u) / sg.ncg), (uint8_t*)w.buf[WS_META_B], (uint8_t*)w.buf[WS_ENC], d_status, 0, nullptr, nullptr, stream,
                            kind == ZN_HINT_DELTA, false);      // (DELTA: built by the delta instance — no base, no rows —, whose sub-block sizes the delta decodes choose)
    if (launch_failed()) return ZN_E_HIP;
    ZN_HIP(hipStreamSynchronize(stream));
    return ZN_OK;
  } catch (...) { return ZN_E_ALLOC; }
}

// hinted items -> their windows, indexes and kinds
struct HintedSplit { std::vector<zn_window_item> win; std::vector<ZnHintSeg> hs; std::vector<int> kinds; };
static int split_hinted(const zn_hinted_item2* items, size_t count, HintedSplit& s) {
  if (count && !items) return ZN_E_ARG;
  s.win.resize(count); s.hs.resize(count); s.kinds.resize(count);
  for (size_t i = 0; i < count; i++) { s.win[i] = items[i].item; s.hs[i].hints = (uint8_t*)items[i].d_hints; s.hs[i].len = items[i].hint_len; s.kinds[i] = items[i].kind; }
  return ZN_OK;
}
// the entry points without a kind: every index is ZN_HINT_PLAIN
static std::vector<zn_hinted_item2> hinted_as_plain(const zn_hinted_item* items, size_t count) {
  std::vector<zn_hinted_item2> v(items ? count : 0);
  for (size_t i = 0; i < v.size(); i++) { v[i].item = items[i].item; v[i].d_hints = items[i].d_hints; v[i].hint_len = items[i].hint_len; v[i].kind = ZN_HINT_PLAIN; }
  return v;
}
int zn_decompress_hinted_batch_dev2(const zn_hinted_item2* items, size_t count, void* stream_, int check) {
  try {
    HintedSplit s;
    int rc = split_hinted(items, count, s);
    if (rc) return rc;
    DecodeSet D;
    rc = build_segments(s.win.data(), count, D, s.hs.data(), s.kinds.data());
    return rc ? rc : launch_segments(D, nullptr, (hipStream_t)stream_, check);
  } catch (...) { return ZN_E_ALLOC; }
}
int zn_decompress_hinted_batch_dev(const zn_hinted_item* items, size_t count, void* stream_, int check) {
  if (count && !items) return ZN_E_ARG;
  try { return zn_decompress_hinted_batch_dev2(hinted_as_plain(items, count).data(), count, stream_, check); } catch (...) { return ZN_E_ALLOC; }
}

static inline zn_window_item zn_whole_window(const zn_batch_item& it) {      // the window [0, K): the whole tensor
  zn_window_item w;
  w.d_body = it.d_body; w.body_len = it.body_len; w.orig_size = it.orig_size; w.chunk_lo = 0; w.chunk_hi = zn_num_chunks(it.orig_size, it.chunk);
  w.d_dst = it.d_dst; w.num_buf = it.num_buf; w.bits_mode = it.bits_mode; w.bytes_mode = it.bytes_mode; w.chunk = it.chunk; w.d_delta = it.d_delta;
  return w;
}
static int decompress_windows(const zn_window_item* items, size_t count, hipStream_t stream, int check) {
  DecodeSet D;
  const int rc = build_segments(items, count, D);
  return rc ? rc : launch_segments(D, nullptr, stream, check);
}

int zn_decompress_delta_dev(const void* d_body, size_t body_len, const void* d_delta, int num_buf, int bits_mode, int bytes_mode,
                            size_t chunk, size_t orig_size, void* d_dst, void* stream_, int check) {
  zn_batch_item it; it.d_delta = d_delta;
  it.d_body = d_body; it.body_len = body_len; it.d_dst = d_dst; it.orig_size = orig_size;
  it.num_buf = num_buf; it.bits_mode = bits_mode; it.bytes_mode = bytes_mode; it.chunk = chunk;
  try {
    const zn_window_item w = zn_whole_window(it);
    return decompress_windows(&w, 1, (hipStream_t)stream_, check);
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_decompress_dev(const void* d_body, size_t body_len, int num_buf, int bits_mode, int bytes_mode, size_t chunk,
                      size_t orig_size, void* d_dst, void* stream_, int check) {
  return zn_decompress_delta_dev(d_body, body_len, nullptr, num_buf, bits_mode, bytes_mode, chunk, orig_size, d_dst, stream_, check);
}

int zn_decompress_batch_dev(const zn_batch_item* items, size_t count, void* stream_, int check) {
  try {                                          // (the segment lists are std::vectors: nothing may unwind through the C ABI)
    if (count && !items) return ZN_E_ARG;
    std::vector<zn_window_item> win(count);
    for (size_t i = 0; i < count; i++) win[i] = zn_whole_window(items[i]);
    return decompress_windows(win.data(), count, (hipStream_t)stream_, check);
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_decompress_window_batch_dev(const zn_window_item* items, size_t count, void* stream_, int check) {
  try {
    return decompress_windows(items, count, (hipStream_t)stream_, check);
  } catch (...) { return ZN_E_ALLOC; }
}

// ---- content digests (zn_digest.hip) ----
int zn_digest_host(const void* src, size_t n, unsigned long long* out) {
  if (!out || (n && !src)) return ZN_E_ARG;
  *out = (unsigned long long)zn_digest_scalar((const uint8_t*)src, n);
  return ZN_OK;
}

int zn_digest_batch_dev(const zn_digest_item* items, size_t count, unsigned long long* d_out, void* stream_) {
  try {
    if (count == 0) return ZN_OK;
    if (!items || !d_out || (((uintptr_t)d_out) & 7u) != 0 || count > 0x7FFFFFFFull) return ZN_E_ARG;
    std::vector<ZnDigSeg> segs(count);
    uint64_t wg = 0;
    for (size_t i = 0; i < count; i++) {
      if (items[i].n && !items[i].d_src) return ZN_E_ARG;
      if ((uint64_t)items[i].n > (0x7FFFFFFFull << 18)) return ZN_E_ARG;      // (more blocks than a grid has workgroups; also keeps the rounding below from wrapping)
      segs[i].src = (const uint8_t*)items[i].d_src; segs[i].n = items[i].n; segs[i].wg0 = (uint32_t)wg; segs[i].slot = (uint32_t)i;
      wg += ((uint64_t)items[i].n + 262143u) >> 18;              // one workgroup per 256 KiB block
      if (wg > 0x7FFFFFFFull) return ZN_E_ARG;
    }
    hipStream_t stream = (hipStream_t)stream_;
    t_kernels.clear();
    if (count == 1) {                              // (the item travels as a kernel argument: no table, no workspace, nothing to wait for)
      zn_launch_digest(segs[0], nullptr, 1, (uint32_t)wg, d_out, stream);
      return launch_failed() ? ZN_E_HIP : ZN_OK;
    }
    WsLease L;
    if (L.rc) return L.rc;
    Workspace& w = *L.w;
    int rc;
    const size_t table_bytes = count * sizeof(ZnDigSeg);      // (through the batched calls' staging)
    if ((rc = w.reserve(WS_SEGS, table_bytes))) return rc;
    if ((rc = L.acquire(stream))) return rc;
    L.mark = true;
    ZN_HIP(hipEventSynchronize(w.busy));           // the previous batched call may still be reading the pinned staging
    if ((rc = w.h_segs.reserve(table_bytes))) return rc;
    memcpy(w.h_segs.p, segs.data(), table_bytes);
    ZN_HIP(hipMemcpyAsync(w.buf[WS_SEGS], w.h_segs.p, table_bytes, hipMemcpyHostToDevice, stream));
    zn_launch_digest(segs[0], (const ZnDigSeg*)w.buf[WS_SEGS], (uint32_t)count, (uint32_t)wg, d_out, stream);
    return launch_failed() ? ZN_E_HIP : ZN_OK;
  } catch (...) { return ZN_E_ALLOC; }
}

// A prepared batched decode: everything build_segments works out, and the segment table in device memory of its own — zn_release_workspace frees none of it,
// and a run stages nothing: no host-to-device copy, no wait for the pinned staging buffer that one-shot batched calls share.
struct zn_plan {
  DecodeSet D;
  ZnSeg* d_table = nullptr;      // 1-plane segments, then 2-, then 4-plane ones (null: at most one segment, which travels as a kernel argument)
  ZnHintSeg* d_htable = nullptr; // a hinted plan: the segments' indexes, in the same order (behind the segments, in the same allocation)
  hipEvent_t last = nullptr;     // recorded behind every run: what zn_plan_destroy waits for (no stream handle is kept — see WsLease)
  bool ran = false;
  int dev = 0;
  ~zn_plan() {                   // (on the plan's device; nothing of it is in use any more)
    if (d_table) (void)hipFree(d_table);
    if (last) (void)hipEventDestroy(last);
  }
};

static int plan_create(const zn_window_item* items, size_t count, const ZnHintSeg* hints, const int* kinds, zn_plan** plan) {
  if (!plan) return ZN_E_ARG;
  *plan = nullptr;
  try {
    int dev = 0, rc0 = zn_current_dev(&dev);
    if (rc0) return rc0;
    std::unique_ptr<zn_plan> pl(new zn_plan());          // (whatever throws or fails below takes the plan, its table and its event with it)
    pl->dev = dev;
    const int rc = build_segments(items, count, pl->D, hints, kinds);
    if (rc) return rc;
    std::vector<ZnSeg> all;
    for (int q = 0; q < 3; q++) all.insert(all.end(), pl->D.segs[q].begin(), pl->D.segs[q].end());
    std::vector<ZnHintSeg> allh;
    if (pl->D.hinted[0] || pl->D.hinted[1] || pl->D.hinted[2])
      for (int q = 0; q < 3; q++) for (size_t i = 0; i < pl->D.segs[q].size(); i++) allh.push_back(i < pl->D.hsegs[q].size() ? pl->D.hsegs[q][i] : ZnHintSeg{nullptr, 0});
    if (all.size() > 1) {
      hipError_t e = hipMalloc((void**)&pl->d_table, all.size() * sizeof(ZnSeg) + allh.size() * sizeof(ZnHintSeg));
      if (e != hipSuccess) { pl->d_table = nullptr; t_hip_err = std::string("hipMalloc: ") + hipGetErrorString(e); (void)hipGetLastError(); return ZN_E_ALLOC; }
      ZN_HIP(hipMemcpy(pl->d_table, all.data(), all.size() * sizeof(ZnSeg), hipMemcpyHostToDevice));
      if (!allh.empty()) {
        pl->d_htable = (ZnHintSeg*)(pl->d_table + all.size());
        ZN_HIP(hipMemcpy(pl->d_htable, allh.data(), allh.size() * sizeof(ZnHintSeg), hipMemcpyHostToDevice));
      }
    }
    ZN_HIP(hipEventCreateWithFlags(&pl->last, hipEventDisableTiming));
    *plan = pl.release();
    return ZN_OK;
  } catch (...) { return ZN_E_ALLOC; }
}
int zn_plan_create(const zn_window_item* items, size_t count, zn_plan** plan) { return plan_create(items, count, nullptr, nullptr, plan); }
int zn_plan_create_hinted2(const zn_hinted_item2* items, size_t count, zn_plan** plan) {
  if (!plan) return ZN_E_ARG;
  *plan = nullptr;
  try {
    HintedSplit s;
    const int rc = split_hinted(items, count, s);
    return rc ? rc : plan_create(s.win.data(), count, s.hs.data(), s.kinds.data(), plan);
  } catch (...) { return ZN_E_ALLOC; }
}
int zn_plan_create_hinted(const zn_hinted_item* items, size_t count, zn_plan** plan) {
  if (!plan) return ZN_E_ARG;
  *plan = nullptr;
  if (count && !items) return ZN_E_ARG;
  try { return zn_plan_create_hinted2(hinted_as_plain(items, count).data(), count, plan); } catch (...) { return ZN_E_ALLOC; }
}

int zn_plan_run(zn_plan* plan, void* stream_, int check) {
  if (!plan) return ZN_E_ARG;
  try {
    int dev = 0;
    ZN_HIP(hipGetDevice(&dev));
    if (dev != plan->dev) return ZN_E_ARG;       // (the table and everything it points to live on the device the plan was made on)
    const int rc = launch_segments(plan->D, plan->d_table, (hipStream_t)stream_, check, plan->d_htable);
    // (also behind a run that failed part-way: some of its kernels may be queued and read the table)
    if (plan->d_table) { if (hipEventRecord(plan->last, (hipStream_t)stream_) == hipSuccess) plan->ran = true; else { (void)hipGetLastError(); (void)hipDeviceSynchronize(); } }
    return rc;
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_plan_destroy(zn_plan* plan) {
  if (!plan) return ZN_OK;
  int rc = ZN_OK;
  {
    DeviceScope scope(plan->dev);
    // the plan's last run — that stream's work up to it, no other stream's — is over before the table goes
    if (!scope.ok || (plan->ran && hipEventSynchronize(plan->last) != hipSuccess)) { t_hip_err = "zn_plan_destroy"; (void)hipGetLastError(); (void)hipDeviceSynchronize(); rc = ZN_E_HIP; }
    delete plan;
  }
  return rc;
}


// The device-side status of the last decode call on the current device that was made with check = 0: waits for `stream`, reads the
// status word that call left in the workspace.  A loader launches its batched decode without the read-back, builds its tensor views
// while the kernels run, and asks here once at the end.
int zn_decode_status_chain(int on) { t_status_chain = on ? 1 : 0; return ZN_OK; }

int zn_decode_status(void* stream_) {
  try {
    WsLease L;                                   // (the lock only: nothing of the workspace is written on the device)
    if (L.rc) return L.rc;
    Workspace& w = *L.w; const int dev = L.dev;
    if (!w.buf[WS_WORDS] || w.cap[WS_WORDS] < ZN_WORDS_BYTES || w.status_gen == 0) {
      // no decode has run on this device — or its status words are gone (zn_release_workspace).  A thread that still holds the token of an unverified
      // check = 0 decode here gets "cannot vouch for it", not "ok" (ADVICE r5): the verdict went with the buffer
      if (t_status_dev == dev && t_status_gen != 0) { t_status_gen = 0; t_status_dev = -1; return ZN_E_CORRUPT; }
      return ZN_OK;
    }
    int rc;
    if ((rc = w.host_words())) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    // the calling thread's last check = 0 decode on this device — or, for a thread that made none (a loader that launches on one thread and asks on another),
    // the device's last decode.  Sixteen decodes later the slot belongs to another call: its answer is gone, and saying "ok" would be a guess
    uint32_t slot = w.last_slot;
    if (t_status_dev == dev) {
      if (w.slot_gen[t_status_slot] != t_status_gen) return ZN_E_CORRUPT;
      slot = t_status_slot;
    }
    if (w.multi && w.busy) ZN_HIP(hipStreamWaitEvent(stream, w.busy, 0));      // (several streams on this device: behind the last call's kernels, whichever stream they ran on — ADVICE r4)
    ZN_HIP(hipMemcpyAsync(w.h_status, (uint32_t*)w.buf[WS_WORDS] + 16 + 4u * slot, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    ZN_HIP(hipStreamSynchronize(stream));
    return status_to_rc(*w.h_status);
  } catch (...) { return ZN_E_ALLOC; }
}

// The last decode call's flags of one workspace buffer, read back (a device-wide wait): `items` items of `per` flag bytes each; counts the items whose bytes are all set.
static long long last_flags_set(int slot, size_t Workspace::*items, size_t per) {
  try {
    WsLease L;
    if (L.rc) return L.rc;
    Workspace& w = *L.w;
    const size_t n_items = w.*items;
    if (!n_items || !w.buf[slot]) return 0;
    std::string flags(per * n_items, '\0');
    ZN_HIP(hipDeviceSynchronize());
    ZN_HIP(hipMemcpy(&flags[0], w.buf[slot], flags.size(), hipMemcpyDeviceToHost));
    long long n = 0;
    for (size_t i = 0; i < n_items; i++) { bool all = true; for (size_t j = 0; j < per; j++) all = all && flags[per * i + j]; n += all; }
    return n;
  } catch (...) { return ZN_E_ALLOC; }
}
long long zn_last_fused_chunks(void) { return last_flags_set(WS_META_B, &Workspace::last_K, 1); }
long long zn_last_tail_planes(void) { return last_flags_set(WS_META_A, &Workspace::last_tails, 4); }      // (four flag bytes per plane: one per huff0 stream)


#if defined(ZN_SIMT_EMULATOR)
// test hook of the emulated build (tests/test_kernels_simt.py): holds one device's workspace lock for `ms` milliseconds,
// so that a test can show that calls on ANOTHER device do not wait for it and calls on the same one do
int zn_debug_hold_device_lock(int dev, int ms) {
  if (dev < 0 || dev >= 64) return ZN_E_ARG;
  std::lock_guard<std::mutex> lk(g_dev_mu[dev]);
  std::this_thread::sleep_for(std::chrono::milliseconds(ms));
  return ZN_OK;
}
#endif

int zn_release_workspace(void) {
  zn_arena().trim();
  zn_host_release_stage();
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
  for (int d = 0; d < 64; d++) {
    // same order as the host-buffer entry points: the device's host lock (its bounce buffers may be in use), then the table
    std::lock_guard<std::mutex> hk(g_host_mu[d]);
    std::lock_guard<std::mutex> lk(g_dev_mu[d]);
    Workspace& w = g_ws[d]; HostPath& hp = g_host[d];
    bool any = w.h_total != nullptr || w.busy != nullptr || w.h_segs.p != nullptr || w.h_totals.p != nullptr || hp.pipe.pin[0] != nullptr || hp.pipe2.pin[0] != nullptr || hp.cstream != nullptr || w.dstream != nullptr;
    for (int i = 0; i < WS_COUNT; i++) any = any || w.buf[i];
    for (int i = 0; i < HP_COUNT; i++) any = any || hp.buf[i];
    if (!any) continue;
    if (hipSetDevice(d) != hipSuccess) { (void)hipGetLastError(); continue; }
    for (int i = 0; i < WS_COUNT; i++) if (w.buf[i]) { (void)hipFree(w.buf[i]); w.buf[i] = nullptr; w.cap[i] = 0; }
    for (int i = 0; i < HP_COUNT; i++) if (hp.buf[i]) { (void)hipFree(hp.buf[i]); hp.buf[i] = nullptr; hp.cap[i] = 0; }
    w.h_segs.release();
    w.h_totals.release();
    if (w.h_total) { (void)hipHostFree(w.h_total); w.h_total = nullptr; w.h_status = nullptr; }
    zn_host_pipe_release(hp.pipe);
    zn_host_pipe_release(hp.pipe2);
    if (hp.cstream) { (void)hipStreamSynchronize(hp.cstream); (void)hipStreamDestroy(hp.cstream); hp.cstream = nullptr; }
    if (w.dstream) { (void)hipStreamSynchronize(w.dstream); (void)hipStreamDestroy(w.dstream); w.dstream = nullptr; }
    if (w.dstream2) { (void)hipStreamSynchronize(w.dstream2); (void)hipStreamDestroy(w.dstream2); w.dstream2 = nullptr; }
    if (w.djoin2) { (void)hipEventDestroy(w.djoin2); w.djoin2 = nullptr; }
    if (w.dfork) { (void)hipEventDestroy(w.dfork); w.dfork = nullptr; }
    if (w.djoin) { (void)hipEventDestroy(w.djoin); w.djoin = nullptr; }
    if (w.busy) { (void)hipDeviceSynchronize(); (void)hipEventDestroy(w.busy); w.busy = nullptr; }
    w.have_stream = false; w.multi = false;
    for (uint32_t i = 0; i < ZN_STATUS_SLOTS; i++) w.slot_gen[i] = 0;      // (the status slots went with the buffers: a thread's old token matches nothing;
    w.last_slot = 0; w.last_K = 0; w.last_tails = 0;                       //  status_gen keeps counting, so that no later call can be handed an old token's generation)
    w.op_backoff = 0; w.op_penalty = 0;
  }
  if (prev >= 0) (void)hipSetDevice(prev);
  return ZN_OK;
}

}  // extern "C"

// (for zn_patch.hip's apply calls, which report through the decode calls' status slots)
uint32_t* zn_take_status_slot(Workspace& w, int dev, int check, bool* chain) { return decode_status_slot(w, dev, check, chain); }
