// zn_api_host.hip — the entry points of the C ABI (include/zipnn_hip.h) that take HOST buffers: zn_compress / zn_decompress and their delta forms,
// the slice pipeline over one device, the multi-device fan-out, the copy helpers and the host-path knobs.
//
// Everything here works on a device's HostPath (zn_workspace.hpp), under g_host_mu alone, and reaches the device layer only through the
// public *_dev functions of zn_api.hip, which take the device's workspace lock themselves.
#include "zn_workspace.hpp"

#include <atomic>
#include <condition_variable>
#include <thread>
#include <vector>

namespace {
// host staging of the multi-device COMPRESS calls (a range's body before it is placed in the frame): one grow-only buffer per
// range slot, kept between calls (a fresh 0.5 GiB vector per range cost more in zero-fill and first-touch page faults than the
// coding itself); g_multi_mu guards it.  Decompress stages nothing on the host: the ranges' payload slices go from the caller's
// body straight into HBM.
std::mutex g_multi_mu;
struct ZnStage { uint8_t* p = nullptr; size_t cap = 0; };
ZnStage g_multi_stage[64];
uint8_t* zn_stage(int slot, size_t need) {
  ZnStage& s = g_multi_stage[slot];
  if (s.cap < need) { free(s.p); s.p = (uint8_t*)malloc(need + (need >> 3) + 4096); s.cap = s.p ? need + (need >> 3) + 4096 : 0; }
  return s.p;
}
struct ZnRange { size_t lo, hi; };                 // chunk range of one device
ZnRange zn_range_of(size_t K, int g, int G) { return ZnRange{(size_t)g * K / (size_t)G, (size_t)(g + 1) * K / (size_t)G}; }
// the bytes [*off, *off + *len) of an n-byte tensor that the chunks of `r` cover (the last chunk may be partial; an empty range: none)
void zn_range_bytes(const ZnRange& r, size_t chunk, size_t n, size_t* off, size_t* len) {
  *off = r.lo * chunk; *len = r.hi > r.lo ? (r.hi * chunk < n ? r.hi * chunk : n) - *off : 0;
}
uint64_t zn_rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

// the worker threads of one call: joined on EVERY way out of the scope (a std::thread destroyed while joinable terminates the
// process), and a thread that cannot be started — EAGAIN under a thread limit — fails the call instead of throwing through it
struct ZnWorkers {
  std::vector<std::thread> th;
  bool failed = false;
  template <class F> void start(F&& f) { if (failed) return; try { th.emplace_back(std::forward<F>(f)); } catch (...) { failed = true; } }
  void join() { for (auto& t : th) if (t.joinable()) t.join(); }
  ~ZnWorkers() { join(); }
};

// The size tables of a frame body, checked once: plane bases, and cumSizes monotone and inside the payload (every per-range
// sub-body below is cut out of them).
struct ZnBodyView { const uint8_t* types; const uint8_t* cums; const uint8_t* pay; size_t P, K, pay_len; std::vector<uint64_t> base; };
int zn_body_view(const void* body, size_t body_len, int num_buf, size_t chunk, size_t orig_size, ZnBodyView* v) {
  const size_t P = (size_t)num_buf, K = (orig_size + chunk - 1) / chunk;
  if (K > body_len / (9 * P)) return ZN_E_CORRUPT;
  const uint8_t* b = (const uint8_t*)body;
  v->P = P; v->K = K; v->types = b; v->cums = b + P * K; v->pay = v->cums + 8 * P * K; v->pay_len = body_len - 9 * P * K;
  v->base.assign(P, 0);
  uint64_t acc = 0;
  for (size_t p = 0; p < P; p++) {
    v->base[p] = acc;
    uint64_t prev = 0;
    for (size_t i = 0; i < K; i++) { const uint64_t c = zn_rd64(v->cums + 8 * (p * K + i)); if (c < prev || c > v->pay_len - acc) return ZN_E_CORRUPT; prev = c; }
    acc += prev;
  }
  return ZN_OK;
}
uint64_t zn_cum_before(const ZnBodyView& v, size_t p, size_t c) { return c ? zn_rd64(v.cums + 8 * (p * v.K + c - 1)) : 0; }
size_t zn_sub_need(const ZnBodyView& v, const ZnRange& r) {
  size_t need = 9 * v.P * (r.hi - r.lo);
  for (size_t p = 0; p < v.P; p++) need += (size_t)(zn_cum_before(v, p, r.hi) - zn_cum_before(v, p, r.lo));
  return need;
}

// The sub-body of the chunk range `r`, put together IN HBM at d_in (zn_sub_need bytes): its size tables (9 P k bytes, re-based) are built on
// the host, its P payload slices go from the caller's body through the device's pinned pipe — or, where `map` has them pinned, by DMA — to
// their place behind them: no host copy of the payload.
int zn_upload_sub_body(const ZnBodyView& v, const ZnRange& r, ZnHostPipe& pipe, uint8_t* d_in, ZnHostMap* map) {
  const size_t P = v.P, K = v.K, k = r.hi - r.lo;
  std::vector<uint8_t> meta(9 * P * k);
  std::vector<uint64_t> s0(P);
  for (size_t p = 0; p < P; p++) {
    s0[p] = zn_cum_before(v, p, r.lo);
    memcpy(meta.data() + p * k, v.types + p * K + r.lo, k);
    for (size_t i = 0; i < k; i++) { const uint64_t c = zn_rd64(v.cums + 8 * (p * K + r.lo + i)) - s0[p]; memcpy(meta.data() + P * k + 8 * (p * k + i), &c, 8); }
  }
  int rc = pipe_copy(pipe, d_in, meta.data(), meta.size(), true);      // (small: never pinned)
  size_t at = meta.size();
  for (size_t p = 0; !rc && p < P; p++) {
    const size_t m = (size_t)(zn_cum_before(v, p, r.hi) - s0[p]);
    rc = pipe_copy(pipe, d_in + at, v.pay + v.base[p] + s0[p], m, true, false, map);
    at += m;
  }
  return rc;
}

// ---- the host-buffer entry points on ONE device, pipelined over slices of the chunks -------------------------------------------
// zn_compress / zn_decompress hand over pageable host buffers: one shot = upload everything, code, download everything, each PCIe
// direction idle while the other works (1 GiB bf16: ≈ 30 GB/s each way).  Here the chunks are cut into S contiguous slices and
// three host threads run upload(i + 1) ‖ code(i) ‖ download(i - 1): two pinned pipes, the kernels on a stream of their own.
// Decompress: slice i's sub-body is put together in HBM as in zn_decode_range.  Compress: a slice's plane-0 payload goes to its
// place in the frame as soon as the slice is coded (its offset needs only the slices before it); the later planes follow when
// the last slice is done (plane p starts behind ALL of plane p - 1).  Same bytes as the one-shot path, slice by slice.
std::atomic<int> g_host_slices{0};               // zn_set_host_slices: 0 automatic, 1 never, 2..64 that many
struct ZnGate {                                   // "stage X has finished n items" between two pipeline threads
  std::mutex m; std::condition_variable cv; size_t done = 0; std::atomic<bool> fail{false};     // (fail is also read without the mutex)
  void publish(size_t n) { { std::lock_guard<std::mutex> lk(m); done = n; } cv.notify_all(); }
  void abort() { { std::lock_guard<std::mutex> lk(m); fail = true; } cv.notify_all(); }
  bool wait_for(size_t n) { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return done >= n || fail; }); return !fail; }
};
// Declared BEHIND the ZnWorkers of a pipelined call: when the coordinating thread leaves the scope by an exception (std::bad_alloc from a
// vector), this aborts the gates before ~ZnWorkers joins the threads — which would otherwise wait on a gate for ever.
struct ZnGateGuard {
  ZnGate* a; ZnGate* b; bool armed = true;
  ZnGateGuard(ZnGate* a_, ZnGate* b_) : a(a_), b(b_) {}
  void disarm() { armed = false; }
  ~ZnGateGuard() { if (armed) { a->abort(); b->abort(); } }
};
int zn_pipeline_stream(HostPath& hp) {
  if (!hp.cstream) ZN_HIP(hipStreamCreateWithFlags(&hp.cstream, hipStreamNonBlocking));
  return ZN_OK;
}

// Measured (1 GiB bf16, MI355X box, profiles/r03_host_buffer_path.txt): the transfers are bound by the host-side staging copies
// (pageable <-> pinned: 48-54 GB/s per direction with 8 threads, more threads do not help), and the two directions disturb each
// other when they run at once: compress 36.9 -> 32.1 ms pipelined (4 slices), decompress 35.2 -> 35.5-38.7 ms.  So the automatic
// choice pipelines compress only; zn_set_host_slices forces either.
static int zn_host_slices(size_t n, size_t chunk, bool decompress, bool direct) {
  const size_t K = chunk ? (n + chunk - 1) / chunk : 0;
  const int forced = g_host_slices.load(std::memory_order_relaxed);
  size_t S;
  if (forced == 1) return 0;
  if (forced >= 2) S = (size_t)forced;
  // (round 6: with the caller's buffers pinned ahead of the transfers — ZnHostMap — the two directions no longer share the host's copy threads, and the
  //  decompress pipeline pays as well: 1 GiB 33 -> 23 ms, profiles/r06_host_path.txt; without the direct path it stays what rounds 3-5 measured: compress only)
  else if (decompress && !direct) return 0;
  else { if (n < ((size_t)192 << 20)) return 0; S = n / ((size_t)(direct ? 128 : 256) << 20); if (S < 4) S = 4; if (S > 8) S = 8; }   // four to eight slices
  if (S > K) S = K;
  return S >= 2 ? (int)S : 0;
}

static int zn_decompress_host_pipelined(const void* body, size_t body_len, int num_buf, int bits_mode, int bytes_mode, size_t chunk,
                                        size_t orig_size, HostPath& hp, int dev, int S, bool direct, void* dst) {
  ZnBodyView v;
  int rc = zn_body_view(body, body_len, num_buf, chunk, orig_size, &v);
  if (rc) return rc;
  const size_t K = v.K;
  std::vector<ZnRange> rg((size_t)S); std::vector<size_t> need((size_t)S), in_off((size_t)S);
  size_t in_total = 0;
  for (int i = 0; i < S; i++) { rg[(size_t)i] = zn_range_of(K, i, S); need[(size_t)i] = zn_sub_need(v, rg[(size_t)i]); in_off[(size_t)i] = in_total; in_total += (need[(size_t)i] + 16 + 255) & ~(size_t)255; }
  if ((rc = hp.reserve(HP_IN, in_total + 16))) return rc;
  if ((rc = hp.reserve(HP_OUT, orig_size))) return rc;
  if ((rc = zn_pipeline_stream(hp))) return rc;
  uint8_t* d_in = (uint8_t*)hp.buf[HP_IN]; uint8_t* d_out = (uint8_t*)hp.buf[HP_OUT]; const hipStream_t cs = hp.cstream;
  ZnGate up, dec;
  int rc_up = ZN_OK, rc_down = ZN_OK, rc_dec = ZN_OK;
  // the caller's two buffers made DMA-able ahead of the transfers (zn_host_pipe.hpp: ZnHostMap): the payload for reading, the result — hinted to
  // huge pages, touched, pinned, piece by piece on helper threads — for writing.  Declared ahead of the workers: unpinned after they are joined.
  ZnHostMap src_map, dst_map;
  // (user memory is only pinned when the caller asked for it — zn_set_host_direct — and never a block of the library's own arena: that is pinned already)
  const bool pin_user = direct;
  if (pin_user && !zn_arena().covers(v.pay, v.pay_len)) src_map.start(const_cast<uint8_t*>(v.pay), v.pay_len, false, ~(size_t)0, dev); else src_map.gave_up = true;
  if (pin_user && !zn_arena().covers(dst, orig_size)) dst_map.start(dst, orig_size, true, ~(size_t)0, dev); else dst_map.gave_up = true;
  try {
    ZnWorkers wk;
    ZnGateGuard guard(&up, &dec);
    wk.start([&]() {                                // upload: re-based size tables + the P payload slices of every slice
      try {
        if (hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); rc_up = ZN_E_HIP; up.abort(); return; }
        for (int i = 0; i < S; i++) {
          const int rcu = zn_upload_sub_body(v, rg[(size_t)i], hp.pipe, d_in + in_off[(size_t)i], &src_map);
          if (rcu || dec.fail) { if (rcu) rc_up = rcu; up.abort(); return; }
          up.publish((size_t)i + 1);
        }
      } catch (...) { rc_up = ZN_E_ALLOC; up.abort(); }
    });
    wk.start([&]() {                                // download: slice i's bytes as soon as they are decoded
      try {
        if (hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); rc_down = ZN_E_HIP; return; }
        for (int i = 0; i < S; i++) {
          if (!dec.wait_for((size_t)i + 1)) return;
          size_t off, len; zn_range_bytes(rg[(size_t)i], chunk, orig_size, &off, &len);
          if (pipe_copy(hp.pipe2, d_out + off, (uint8_t*)dst + off, len, false, false, &dst_map)) { rc_down = ZN_E_HIP; return; }
        }
      } catch (...) { rc_down = ZN_E_ALLOC; }
    });
    if (wk.failed) { up.abort(); dec.abort(); wk.join(); return ZN_E_ALLOC; }
    for (int i = 0; i < S; i++) {                   // decode, on this thread
      if (!up.wait_for((size_t)i + 1)) { rc_dec = rc_up ? rc_up : ZN_E_HIP; break; }
      size_t off, len; zn_range_bytes(rg[(size_t)i], chunk, orig_size, &off, &len);
      rc_dec = zn_decompress_dev(d_in + in_off[(size_t)i], need[(size_t)i], num_buf, bits_mode, bytes_mode, chunk, len, d_out + off, cs, 1);
      if (rc_dec) break;
      dec.publish((size_t)i + 1);
    }
    if (rc_dec) { dec.abort(); up.abort(); }
    guard.disarm();
    wk.join();
  } catch (...) { return ZN_E_ALLOC; }
  return rc_dec ? rc_dec : rc_up ? rc_up : rc_down;
}

static int zn_compress_host_pipelined(const void* hdr, size_t hdr_len, const void* src, size_t n, int num_buf, int bits_mode, int bytes_mode,
                                      size_t chunk, float threshold, HostPath& hp, int dev, int S, bool direct, void* dst, size_t dst_cap, size_t* dst_len) {
  const size_t P = (size_t)num_buf, K = (n + chunk - 1) / chunk;
  if (hdr_len + 9 * P * K > dst_cap) return ZN_E_CAP;
  std::vector<ZnRange> rg((size_t)S); std::vector<size_t> boff((size_t)S), bcap((size_t)S), blen((size_t)S, 0);
  size_t b_total = 0;
  for (int i = 0; i < S; i++) {
    rg[(size_t)i] = zn_range_of(K, i, S);
    size_t off, len; zn_range_bytes(rg[(size_t)i], chunk, n, &off, &len);
    bcap[(size_t)i] = zn_compress_bound(len, num_buf, chunk, 0) + 16; boff[(size_t)i] = b_total; b_total += (bcap[(size_t)i] + 255) & ~(size_t)255;
  }
  int rc;
  if ((rc = hp.reserve(HP_IN, n))) return rc;
  if ((rc = hp.reserve(HP_OUT, b_total + 16))) return rc;
  if ((rc = zn_pipeline_stream(hp))) return rc;
  uint8_t* d_src = (uint8_t*)hp.buf[HP_IN]; uint8_t* d_body = (uint8_t*)hp.buf[HP_OUT]; const hipStream_t cs = hp.cstream;
  uint8_t* o = (uint8_t*)dst;
  uint8_t* types = o + hdr_len; uint8_t* cums = types + P * K; uint8_t* pay = cums + 8 * P * K;
  const size_t pay_cap = dst_cap - hdr_len - 9 * P * K;
  struct Job { const uint8_t* d; uint8_t* h; size_t len; };
  std::vector<Job> jobs; jobs.reserve((size_t)S + P);                 // (appended by this thread only, read by the downloader up to `queued.done`)
  ZnGate up, queued; bool all_queued = false;
  int rc_up = ZN_OK, rc_down = ZN_OK, rc_enc = ZN_OK;
  std::vector<std::vector<uint8_t>> metas((size_t)S);
  ZnHostMap src_map, dst_map;                       // (as in the decompress pipeline; the result is prepared as far as a weights-like tensor will need it, further on demand)
  const bool pin_user = direct;
  if (pin_user && !zn_arena().covers(src, n)) src_map.start(const_cast<void*>(src), n, false, ~(size_t)0, dev); else src_map.gave_up = true;
  if (pin_user && !zn_arena().covers(dst, dst_cap)) dst_map.start(dst, dst_cap, true, hdr_len + 9 * P * K + n / 2 + n / 4, dev); else dst_map.gave_up = true;
  try {
    ZnWorkers wk;
    ZnGateGuard guard(&up, &queued);
    wk.start([&]() {                                // upload the tensor slice by slice
      try {
        if (hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); rc_up = ZN_E_HIP; up.abort(); return; }
        for (int i = 0; i < S; i++) {
          size_t off, len; zn_range_bytes(rg[(size_t)i], chunk, n, &off, &len);
          if (pipe_copy(hp.pipe, d_src + off, (const uint8_t*)src + off, len, true, false, &src_map)) { rc_up = ZN_E_HIP; up.abort(); return; }
          if (queued.fail) { up.abort(); return; }
          up.publish((size_t)i + 1);
        }
      } catch (...) { rc_up = ZN_E_ALLOC; up.abort(); }
    });
    wk.start([&]() {                                // download the payload pieces in the order they are queued
      try {
        if (hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); rc_down = ZN_E_HIP; return; }
        size_t next = 0;
        for (;;) {
          size_t have; bool fin;
          { std::unique_lock<std::mutex> lk(queued.m); queued.cv.wait(lk, [&] { return queued.done > next || queued.fail || all_queued; }); have = queued.done; fin = all_queued; if (queued.fail) return; }
          for (; next < have; next++) {
            const Job j = jobs[next];
            if (pipe_copy(hp.pipe2, const_cast<uint8_t*>(j.d), j.h, j.len, false, false, &dst_map)) { rc_down = ZN_E_HIP; return; }
          }
          if (fin && next >= have) { std::lock_guard<std::mutex> lk(queued.m); if (queued.done == next) return; }
        }
      } catch (...) { rc_down = ZN_E_ALLOC; }
    });
    if (wk.failed) { up.abort(); queued.abort(); wk.join(); return ZN_E_ALLOC; }
    std::vector<uint64_t> tot((size_t)S * P, 0);
    size_t pay0_at = 0;
    for (int i = 0; i < S && !rc_enc; i++) {        // code slice i; its plane 0 can leave at once
      if (!up.wait_for((size_t)i + 1)) { rc_enc = rc_up ? rc_up : ZN_E_HIP; break; }
      const ZnRange r = rg[(size_t)i]; const size_t k = r.hi - r.lo;
      size_t off, len; zn_range_bytes(r, chunk, n, &off, &len);
      uint8_t* b = d_body + boff[(size_t)i];
      rc_enc = zn_compress_dev(d_src + off, len, num_buf, bits_mode, bytes_mode, chunk, threshold, b, bcap[(size_t)i], &blen[(size_t)i], cs);
      if (rc_enc) break;
      metas[(size_t)i].resize(9 * P * k);
      if (hipMemcpyAsync(metas[(size_t)i].data(), b, 9 * P * k, hipMemcpyDeviceToHost, cs) != hipSuccess || hipStreamSynchronize(cs) != hipSuccess) { (void)hipGetLastError(); rc_enc = ZN_E_HIP; break; }
      for (size_t p = 0; p < P; p++) tot[(size_t)i * P + p] = zn_rd64(metas[(size_t)i].data() + P * k + 8 * (p * k + k - 1));
      const size_t t0 = (size_t)tot[(size_t)i * P];
      if (pay0_at + t0 > pay_cap) { rc_enc = ZN_E_CAP; break; }
      jobs.push_back(Job{b + 9 * P * k, pay + pay0_at, t0});
      pay0_at += t0;
      queued.publish(jobs.size());
    }
    size_t total = 0;
    if (!rc_enc) {                                  // every slice is coded: the later planes have their places now
      std::vector<size_t> base(P, 0); size_t acc = 0;
      for (size_t p = 0; p < P; p++) { base[p] = acc; for (int i = 0; i < S; i++) acc += (size_t)tot[(size_t)i * P + p]; }
      if (acc > pay_cap) rc_enc = ZN_E_CAP;
      else {
        // planes 1.. are contiguous in the frame across the slices: their pieces are gathered on the device (into the input staging,
        // which nothing reads any more) and leave as ONE transfer per plane instead of S small ones
        size_t g_at = 0;
        for (size_t p = 1; p < P && !rc_enc; p++) {
          const size_t g0 = g_at;
          for (int i = 0; i < S; i++) {
            const size_t k = rg[(size_t)i].hi - rg[(size_t)i].lo;
            size_t before = 0; for (size_t q = 0; q < p; q++) before += (size_t)tot[(size_t)i * P + q];
            const size_t m = (size_t)tot[(size_t)i * P + p];
            if (m && hipMemcpyAsync(d_src + g_at, d_body + boff[(size_t)i] + 9 * P * k + before, m, hipMemcpyDeviceToDevice, cs) != hipSuccess) { (void)hipGetLastError(); rc_enc = ZN_E_HIP; break; }
            g_at += m;
          }
          if (!rc_enc) jobs.push_back(Job{d_src + g0, pay + base[p], g_at - g0});
        }
        if (!rc_enc && hipStreamSynchronize(cs) != hipSuccess) { (void)hipGetLastError(); rc_enc = ZN_E_HIP; }
        total = hdr_len + 9 * P * K + acc;
      }
    }
    if (rc_enc) { queued.abort(); up.abort(); }
    else { { std::lock_guard<std::mutex> lk(queued.m); queued.done = jobs.size(); all_queued = true; } queued.cv.notify_all(); }
    if (!rc_enc) {                                  // the size tables, re-based, while the last pieces are on their way
      if (hdr_len) memcpy(o, hdr, hdr_len);
      std::vector<uint64_t> run(P, 0);
      for (int i = 0; i < S; i++) {
        const ZnRange r = rg[(size_t)i]; const size_t k = r.hi - r.lo;
        const uint8_t* m = metas[(size_t)i].data();
        for (size_t p = 0; p < P; p++) {
          memcpy(types + p * K + r.lo, m + p * k, k);
          for (size_t j = 0; j < k; j++) { const uint64_t c = zn_rd64(m + P * k + 8 * (p * k + j)) + run[p]; memcpy(cums + 8 * (p * K + r.lo + j), &c, 8); }
          run[p] += tot[(size_t)i * P + p];
        }
      }
      if (hdr_len >= 32) { const uint64_t t64 = total; memcpy(o + 24, &t64, 8); }   // zipnn_core.c:121
    }
    guard.disarm();
    wk.join();
    if (!rc_enc && !rc_down) *dst_len = total;
  } catch (...) { return ZN_E_ALLOC; }
  return rc_enc ? rc_enc : rc_up ? rc_up : rc_down;
}
}  // namespace

void zn_host_release_stage() {
  std::lock_guard<std::mutex> mk(g_multi_mu);
  for (int i = 0; i < 64; i++) { free(g_multi_stage[i].p); g_multi_stage[i].p = nullptr; g_multi_stage[i].cap = 0; }
}

extern "C" {

void* zn_host_alloc(size_t n) { try { return zn_arena().alloc(n); } catch (...) { return nullptr; } }
int zn_host_free(void* p) { if (!p) return ZN_OK; try { return zn_arena().release(p) ? ZN_OK : ZN_E_ARG; } catch (...) { return ZN_E_ALLOC; } }
int zn_set_host_direct(int mode) {
  if (mode < 0 || mode > 7) return ZN_E_ARG;
  zn_host_pipe_detail::direct_mode_ref().store(mode, std::memory_order_relaxed);
  return ZN_OK;
}
int zn_set_host_slices(int slices) {
  if (slices < 0 || slices > 64) return ZN_E_ARG;
  g_host_slices.store(slices, std::memory_order_relaxed);
  return ZN_OK;
}

int zn_compress_delta(const void* hdr, size_t hdr_len, const void* src, const void* delta, size_t n, int num_buf, int bits_mode,
                      int bytes_mode, size_t chunk, float threshold, int device, void* dst, size_t dst_cap, size_t* dst_len) {
  if (!dst_len || (hdr_len && !hdr) || (n && !src) || !dst) return ZN_E_ARG;
  if (zn_device_count() <= 0) return ZN_E_NODEV;
  DeviceScope scope(device);              // (restored on every return path)
  if (!scope.ok) { t_hip_err = "hipSetDevice"; return ZN_E_HIP; }
  const size_t bound = zn_compress_bound(n, num_buf, chunk, 0);
  zn_host_thp_hint(dst, dst_cap);         // (a fresh result buffer faults in 2 MiB at a time, and is freed as fast: zn_host_pipe.hpp)
  // The DIRECT transfers (the caller's buffers pinned, DMA straight between them and HBM: zn_host_pipe.hpp) are for calls whose RESULT buffer is already
  // backed by pages — a recycled buffer, or one its owner has written before.  A call that has to fault its result in goes the staged way of rounds 1-5 in
  // BOTH directions: page faults in a process with pinned user memory were measured slow and disruptive to every DMA in flight (profiles/r06_host_path.txt).
  // (a result buffer from zn_host_alloc needs none of this: its downloads are plain DMAs whichever way the call is cut — zn_host_pipe_copy sees to that)
  const bool direct = zn_host_pipe_detail::direct_enabled() && !zn_arena().covers(dst, dst_cap) && zn_host_resident(dst, hdr_len + 9u * (size_t)num_buf * zn_num_chunks(n, chunk) + n / 2);
  HostLease H;                            // one host-path call at a time per device
  if (H.rc) return H.rc;
  HostPath& hp = *H.hp;
  if (!delta && (num_buf == 1 || num_buf == 2 || num_buf == 4) && chunk) {
    const int S = zn_host_slices(n, chunk, false, direct);
    if (S >= 2) {
      try { return zn_compress_host_pipelined(hdr, hdr_len, src, n, num_buf, bits_mode, bytes_mode, chunk, threshold, hp, H.dev, S, direct, dst, dst_cap, dst_len); }
      catch (...) { return ZN_E_ALLOC; }
    }
  }
  // device staging for host buffers: cached like the workspace (grow-only)
  int rc; size_t body_len = 0;
  void* d_delta = nullptr;
  if (delta && n) { if ((rc = hp.reserve(HP_DELTA, n))) return rc; d_delta = hp.buf[HP_DELTA]; }
  if ((rc = hp.reserve(HP_IN, n))) return rc;
  if ((rc = hp.reserve(HP_OUT, bound))) return rc;
  void* d_src = hp.buf[HP_IN]; void* d_body = hp.buf[HP_OUT];
  // (pageable host memory through the pinned, multi-threaded pipe of zn_host_pipe.hpp; g_host_mu serialises its use)
  if ((rc = pipe_copy(hp.pipe, d_src, src, n, true, !direct))) return rc;
  if (d_delta && (rc = pipe_copy(hp.pipe, d_delta, delta, n, true, !direct))) return rc;
  if ((rc = zn_compress_delta_dev(d_src, d_delta, n, num_buf, bits_mode, bytes_mode, chunk, threshold, d_body, bound ? bound : 16, &body_len, nullptr))) return rc;
  if (hdr_len + body_len > dst_cap) return ZN_E_CAP;
  if (hdr_len) memcpy(dst, hdr, hdr_len);
  if ((rc = pipe_copy(hp.pipe, d_body, (uint8_t*)dst + hdr_len, body_len, false, !direct))) return rc;
  *dst_len = hdr_len + body_len;
  if (hdr_len >= 32) { const uint64_t total = *dst_len; memcpy((uint8_t*)dst + 24, &total, 8); }   // zipnn_core.c:121
  return ZN_OK;
}

int zn_compress(const void* hdr, size_t hdr_len, const void* src, size_t n, int num_buf, int bits_mode, int bytes_mode,
                size_t chunk, float threshold, int device, void* dst, size_t dst_cap, size_t* dst_len) {
  return zn_compress_delta(hdr, hdr_len, src, nullptr, n, num_buf, bits_mode, bytes_mode, chunk, threshold, device, dst, dst_cap, dst_len);
}

int zn_decompress_delta(const void* body, size_t body_len, const void* delta, int num_buf, int bits_mode, int bytes_mode, size_t chunk,
                        size_t orig_size, int device, void* dst) {
  if ((body_len && !body) || (orig_size && !dst)) return ZN_E_ARG;
  if (zn_device_count() <= 0) return ZN_E_NODEV;
  DeviceScope scope(device);              // (restored on every return path)
  if (!scope.ok) { t_hip_err = "hipSetDevice"; return ZN_E_HIP; }
  zn_host_thp_hint(dst, orig_size);
  // (an arena result stays one shot like a pageable one: measured, the slice pipeline with a STAGED upload beside the arena's download DMAs is slower than their sum —
  //  36-38 ms against 33 for 1 GiB; the copy threads and the two DMA directions meet in the host's memory: profiles/r06_host_path.txt)
  const bool direct = zn_host_pipe_detail::direct_enabled() && !zn_arena().covers(dst, orig_size) && zn_host_resident(dst, orig_size);      // (see zn_compress_delta)
  HostLease H;
  if (H.rc) return H.rc;
  HostPath& hp = *H.hp;
  if (!delta && (num_buf == 1 || num_buf == 2 || num_buf == 4) && chunk) {
    const int S = zn_host_slices(orig_size, chunk, true, direct);
    if (S >= 2) {
      try { return zn_decompress_host_pipelined(body, body_len, num_buf, bits_mode, bytes_mode, chunk, orig_size, hp, H.dev, S, direct, dst); }
      catch (...) { return ZN_E_ALLOC; }
    }
  }
  int rc;
  void* d_delta = nullptr;
  if (delta && orig_size) { if ((rc = hp.reserve(HP_DELTA, orig_size))) return rc; d_delta = hp.buf[HP_DELTA]; }
  if ((rc = hp.reserve(HP_IN, body_len))) return rc;
  if ((rc = hp.reserve(HP_OUT, orig_size))) return rc;
  void* d_body = hp.buf[HP_IN]; void* d_dst = hp.buf[HP_OUT];
  if ((rc = pipe_copy(hp.pipe, d_body, body, body_len, true, !direct))) return rc;
  if (d_delta && (rc = pipe_copy(hp.pipe, d_delta, delta, orig_size, true, !direct))) return rc;
  if ((rc = zn_decompress_delta_dev(d_body, body_len, d_delta, num_buf, bits_mode, bytes_mode, chunk, orig_size, d_dst, nullptr, 1))) return rc;
  return pipe_copy(hp.pipe, d_dst, dst, orig_size, false, !direct);
}

int zn_decompress(const void* body, size_t body_len, int num_buf, int bits_mode, int bytes_mode, size_t chunk,
                  size_t orig_size, int device, void* dst) {
  return zn_decompress_delta(body, body_len, nullptr, num_buf, bits_mode, bytes_mode, chunk, orig_size, device, dst);
}

}  // extern "C"

// ---- one call, several GPUs (`const int* devices, int ndev`; north_star: "chunks partition embarrassingly
// across the GPUs of one node on independent HIP streams, no collectives") ------------------------------------------------
// Chunks are independent, so device i codes the contiguous chunk range [i K / G, (i + 1) K / G) as a tensor of its own, on a
// host thread of its own (per-device locks, workspaces and streams: zn_workspace.hpp), and the host does the plane-major
// bookkeeping: types and payload of the ranges concatenated per plane, cumSizes re-based by what the earlier ranges put into
// the plane.  The frame is byte-identical to the one a single device writes (zipnn_amd/sharding.py states the same
// arithmetic in numpy for the one-process-per-GPU path).  The reference's counterpart is its pthread fan-out over chunks
// (csrc/zipnn_core.c:294-301, 509-523).
namespace {
// Decode the chunk range `r` of a host-resident frame body on `device`: its sub-body is put together in HBM (zn_upload_sub_body), the decoded
// bytes land in `d_dst` (device memory of `device`, when given) or are copied to `h_dst` (host).
int zn_decode_range(const ZnBodyView& v, const ZnRange& r, int num_buf, int bits_mode, int bytes_mode, size_t chunk, size_t orig_size,
                    int device, void* h_dst, void* d_dst) {
  if (r.hi == r.lo) return ZN_OK;
  size_t off, len; zn_range_bytes(r, chunk, orig_size, &off, &len);
  DeviceScope scope(device);              // (restored on every return path)
  if (!scope.ok) { t_hip_err = "hipSetDevice"; return ZN_E_HIP; }
  HostLease H;
  if (H.rc) return H.rc;
  HostPath& hp = *H.hp;
  const size_t need = zn_sub_need(v, r);
  int rc;
  if ((rc = hp.reserve(HP_IN, need + 16))) return rc;
  uint8_t* d_in = (uint8_t*)hp.buf[HP_IN]; void* d_out = d_dst;
  if (!d_out) { if ((rc = hp.reserve(HP_OUT, len))) return rc; d_out = hp.buf[HP_OUT]; }
  if ((rc = zn_upload_sub_body(v, r, hp.pipe, d_in, nullptr))) return rc;
  if ((rc = zn_decompress_dev(d_in, need, num_buf, bits_mode, bytes_mode, chunk, len, d_out, nullptr, 1))) return rc;
  return h_dst ? pipe_copy(hp.pipe, d_out, (uint8_t*)h_dst + off, len, false) : ZN_OK;
}

// Bodies of CONSECUTIVE chunk ranges (part i: ks[i] chunks, plen[i] bytes = types ‖ cumSizes ‖ payload of that range alone) ->
// hdr ‖ one body: types and payload concatenated per plane, cumSizes re-based by what the earlier ranges put into the plane;
// one thread per range does the copying.
int zn_assemble_ranges(const void* hdr, size_t hdr_len, const std::vector<const uint8_t*>& part, const std::vector<size_t>& plen,
                       const std::vector<size_t>& ks, size_t P, void* dst, size_t dst_cap, size_t* dst_len) {
  const size_t G = part.size();
  size_t K = 0, pay_total = 0;
  for (size_t g = 0; g < G; g++) {
    const size_t k = ks[g];
    if (!k) continue;
    if (!part[g] || plen[g] < 9 * P * k) return ZN_E_ARG;
    K += k; pay_total += plen[g] - 9 * P * k;
  }
  const size_t total = hdr_len + 9 * P * K + pay_total;
  if (total > dst_cap) return ZN_E_CAP;
  uint8_t* o = (uint8_t*)dst;
  if (hdr_len) memcpy(o, hdr, hdr_len);
  uint8_t* types = o + hdr_len; uint8_t* cums = types + P * K; uint8_t* pay = cums + 8 * P * K;
  // where every (plane, range) piece goes and what re-bases its cumSizes
  std::vector<size_t> dst_at(G * P, 0), c0(G, 0); std::vector<uint64_t> rebase(G * P, 0);
  { size_t c = 0; for (size_t g = 0; g < G; g++) { c0[g] = c; c += ks[g]; } }
  // every part by itself: its cumSizes non-decreasing inside each plane and its plane totals adding up to ITS OWN payload length — a
  // global sum alone lets a part that is short by what another one is long through, and the copies below then read past its end
  for (size_t g = 0; g < G; g++) {
    const size_t k = ks[g];
    if (!k) continue;
    const uint8_t* c = part[g] + P * k;
    const size_t own = plen[g] - 9 * P * k;
    size_t sum = 0;
    for (size_t p = 0; p < P; p++) {
      uint64_t prev = 0;
      for (size_t i = 0; i < k; i++) { const uint64_t v = zn_rd64(c + 8 * (p * k + i)); if (v < prev) return ZN_E_CORRUPT; prev = v; }
      if (prev > own - sum) return ZN_E_CORRUPT;
      sum += (size_t)prev;
    }
    if (sum != own) return ZN_E_CORRUPT;
  }
  size_t pay_at = 0;
  for (size_t p = 0; p < P; p++) {
    uint64_t run = 0;                              // bytes the earlier ranges put into plane p
    for (size_t g = 0; g < G; g++) {
      const size_t k = ks[g];
      if (!k) continue;
      const size_t tot = (size_t)zn_rd64(part[g] + P * k + 8 * (p * k + k - 1));
      dst_at[g * P + p] = pay_at; rebase[g * P + p] = run;
      pay_at += tot; run += tot;
    }
  }
  if (pay_at != pay_total) return ZN_E_CORRUPT;   // a part whose cumSizes disagree with its length
  {
    ZnWorkers cp;
    for (size_t g = 0; g < G; g++) {
      const size_t k = ks[g];
      if (!k) continue;
      cp.start([&, g, k]() {
        const uint8_t* b = part[g];
        size_t base = 0;                             // where plane p starts in this range's payload
        for (size_t p = 0; p < P; p++) {
          memcpy(types + p * K + c0[g], b + p * k, k);
          const uint8_t* c = b + P * k + 8 * p * k;
          const uint64_t run = rebase[g * P + p];
          for (size_t i = 0; i < k; i++) { const uint64_t v = zn_rd64(c + 8 * i) + run; memcpy(cums + 8 * (p * K + c0[g] + i), &v, 8); }
          const size_t tot = (size_t)zn_rd64(c + 8 * (k - 1));
          memcpy(pay + dst_at[g * P + p], b + 9 * P * k + base, tot);
          base += tot;
        }
      });
    }
    cp.join();
    if (cp.failed) return ZN_E_ALLOC;
  }
  *dst_len = total;
  if (hdr_len >= 32) { const uint64_t t64 = total; memcpy(o + 24, &t64, 8); }   // zipnn_core.c:121
  return ZN_OK;
}

// Compress with the chunk ranges on several devices; `part_src(g)` says where range g's bytes are: a host pointer (h != null:
// staged through HBM by zn_compress) or a device pointer on devices[g].  The ranges' bodies come back to host staging and are
// placed in the frame by one thread per range.
struct ZnPartSrc { const void* h; const void* d; };
template <class SRC>
int zn_compress_ranges(const void* hdr, size_t hdr_len, size_t n, int num_buf, int bits_mode, int bytes_mode, size_t chunk, float threshold,
                       const int* devices, int ndev, void* dst, size_t dst_cap, size_t* dst_len, SRC&& part_src) {
  const size_t P = (size_t)num_buf, K = (n + chunk - 1) / chunk;
  std::lock_guard<std::mutex> mk(g_multi_mu);
  std::vector<uint8_t*> part((size_t)ndev, nullptr);
  std::vector<size_t> plen((size_t)ndev, 0);
  for (int g = 0; g < ndev; g++) {                 // (staging reserved here: the worker threads only fill it)
    const ZnRange r = zn_range_of(K, g, ndev);
    if (r.hi <= r.lo) continue;
    size_t off, len; zn_range_bytes(r, chunk, n, &off, &len);
    if (!(part[(size_t)g] = zn_stage(g, zn_compress_bound(len, num_buf, chunk, 0) + 16))) return ZN_E_ALLOC;
  }
  std::vector<int> rcs((size_t)ndev, ZN_OK);
  {
    ZnWorkers wk;
    for (int g = 0; g < ndev; g++) {
      const ZnRange r = zn_range_of(K, g, ndev);
      if (r.hi <= r.lo) continue;
      wk.start([&, g, r]() {
        try {
          size_t off, len; zn_range_bytes(r, chunk, n, &off, &len);
          const size_t cap =zn_compress_bound(len, num_buf, chunk, 0) + 16;
          const ZnPartSrc ps = part_src(g, off);
          if (ps.h || !len) {
            rcs[(size_t)g] = zn_compress(nullptr, 0, ps.h, len, num_buf, bits_mode, bytes_mode, chunk, threshold, devices[g], part[(size_t)g], cap, &plen[(size_t)g]);
            return;
          }
          // the range is in HBM already: code it there, bring only the body back
          DeviceScope scope(devices[g]);
          if (!scope.ok) { rcs[(size_t)g] = ZN_E_HIP; return; }
          HostLease H;
          if (H.rc) { (void)hipGetLastError(); rcs[(size_t)g] = ZN_E_HIP; return; }
          HostPath& hp = *H.hp;
          if ((rcs[(size_t)g] = hp.reserve(HP_OUT, cap))) return;
          void* d_body = hp.buf[HP_OUT];
          size_t blen = 0;
          int rc = zn_compress_dev(ps.d, len, num_buf, bits_mode, bytes_mode, chunk, threshold, d_body, cap, &blen, nullptr);
          if (!rc) rc = pipe_copy(hp.pipe, d_body, part[(size_t)g], blen, false);
          plen[(size_t)g] = blen; rcs[(size_t)g] = rc;
        } catch (...) { rcs[(size_t)g] = ZN_E_ALLOC; }
      });
    }
    wk.join();
    if (wk.failed) return ZN_E_ALLOC;
  }
  for (int g = 0; g < ndev; g++) if (rcs[(size_t)g]) return rcs[(size_t)g];
  std::vector<const uint8_t*> cpart((size_t)ndev, nullptr); std::vector<size_t> ks((size_t)ndev, 0);
  for (int g = 0; g < ndev; g++) { const ZnRange r = zn_range_of(K, g, ndev); cpart[(size_t)g] = part[(size_t)g]; ks[(size_t)g] = r.hi - r.lo; }
  return zn_assemble_ranges(hdr, hdr_len, cpart, plen, ks, P, dst, dst_cap, dst_len);
}
}  // namespace

extern "C" {

int zn_compress_multi(const void* hdr, size_t hdr_len, const void* src, size_t n, int num_buf, int bits_mode, int bytes_mode,
                      size_t chunk, float threshold, const int* devices, int ndev, void* dst, size_t dst_cap, size_t* dst_len) {
  if (!dst_len || (hdr_len && !hdr) || (n && !src) || !dst || !devices || ndev <= 0 || ndev > 64 || !chunk) return ZN_E_ARG;
  if (num_buf != 1 && num_buf != 2 && num_buf != 4) return ZN_E_ARG;
  if (ndev == 1) return zn_compress(hdr, hdr_len, src, n, num_buf, bits_mode, bytes_mode, chunk, threshold, devices[0], dst, dst_cap, dst_len);
  try {
    return zn_compress_ranges(hdr, hdr_len, n, num_buf, bits_mode, bytes_mode, chunk, threshold, devices, ndev, dst, dst_cap, dst_len,
                              [&](int, size_t off) { return ZnPartSrc{(const uint8_t*)src + off, nullptr}; });
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_compress_multi_dev(const void* hdr, size_t hdr_len, const void* const* d_src, size_t n, int num_buf, int bits_mode, int bytes_mode,
                          size_t chunk, float threshold, const int* devices, int ndev, void* dst, size_t dst_cap, size_t* dst_len) {
  if (!dst_len || (hdr_len && !hdr) || (n && !d_src) || !dst || !devices || ndev <= 0 || ndev > 64 || !chunk) return ZN_E_ARG;
  if (num_buf != 1 && num_buf != 2 && num_buf != 4) return ZN_E_ARG;
  if (zn_device_count() <= 0) return ZN_E_NODEV;
  const size_t K = (n + chunk - 1) / chunk;
  for (int g = 0; g < ndev; g++) { const ZnRange r = zn_range_of(K, g, ndev); if (r.hi > r.lo && !d_src[g]) return ZN_E_ARG; }
  try {
    return zn_compress_ranges(hdr, hdr_len, n, num_buf, bits_mode, bytes_mode, chunk, threshold, devices, ndev, dst, dst_cap, dst_len,
                              [&](int g, size_t) { return ZnPartSrc{nullptr, d_src[g]}; });
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_multi_range(size_t n, size_t chunk, int ndev, int i, size_t* off, size_t* len) {
  if (!chunk || ndev <= 0 || i < 0 || i >= ndev || !off || !len) return ZN_E_ARG;
  const size_t K = (n + chunk - 1) / chunk;
  zn_range_bytes(zn_range_of(K, i, ndev), chunk, n, off, len);
  return ZN_OK;
}

int zn_merge_range_bodies(const void* const* bodies, const size_t* body_lens, const size_t* num_chunks, int nparts, int num_buf,
                          void* dst, size_t dst_cap, size_t* dst_len) {
  if (nparts < 0 || (nparts && (!bodies || !body_lens || !num_chunks)) || !dst || !dst_len) return ZN_E_ARG;
  if (num_buf != 1 && num_buf != 2 && num_buf != 4) return ZN_E_ARG;
  try {
    std::vector<const uint8_t*> part((size_t)nparts); std::vector<size_t> plen((size_t)nparts), ks((size_t)nparts);
    for (int i = 0; i < nparts; i++) { part[(size_t)i] = (const uint8_t*)bodies[i]; plen[(size_t)i] = body_lens[i]; ks[(size_t)i] = num_chunks[i]; }
    return zn_assemble_ranges(nullptr, 0, part, plen, ks, (size_t)num_buf, dst, dst_cap, dst_len);
  } catch (...) { return ZN_E_ALLOC; }
}

int zn_decompress_range_dev(const void* body, size_t body_len, int num_buf, int bits_mode, int bytes_mode, size_t chunk, size_t orig_size,
                            size_t chunk_lo, size_t chunk_hi, int device, void* d_dst) {
  if ((body_len && !body) || !chunk) return ZN_E_ARG;
  if (num_buf != 1 && num_buf != 2 && num_buf != 4) return ZN_E_ARG;
  const size_t K = (orig_size + chunk - 1) / chunk;
  if (chunk_lo > chunk_hi || chunk_hi > K) return ZN_E_ARG;
  if (chunk_lo == chunk_hi) return ZN_OK;
  if (!d_dst) return ZN_E_ARG;
  if (zn_device_count() <= 0) return ZN_E_NODEV;
  try {
    ZnBodyView v;
    const int rc = zn_body_view(body, body_len, num_buf, chunk, orig_size, &v);
    if (rc) return rc;
    return zn_decode_range(v, ZnRange{chunk_lo, chunk_hi}, num_buf, bits_mode, bytes_mode, chunk, orig_size, device, nullptr, d_dst);
  } catch (...) { return ZN_E_ALLOC; }
}

static int zn_decompress_ranges(const void* body, size_t body_len, int num_buf, int bits_mode, int bytes_mode, size_t chunk, size_t orig_size,
                                const int* devices, int ndev, void* h_dst, void* const* d_dst) {
  ZnBodyView v;
  int rc = zn_body_view(body, body_len, num_buf, chunk, orig_size, &v);
  if (rc) return rc;
  std::vector<int> rcs((size_t)ndev, ZN_OK);
  {
    ZnWorkers wk;
    for (int g = 0; g < ndev; g++) {
      const ZnRange r = zn_range_of(v.K, g, ndev);
      if (r.hi <= r.lo) continue;
      wk.start([&, g, r]() {
        try { rcs[(size_t)g] = zn_decode_range(v, r, num_buf, bits_mode, bytes_mode, chunk, orig_size, devices[g], h_dst, d_dst ? d_dst[g] : nullptr); }
        catch (...) { rcs[(size_t)g] = ZN_E_ALLOC; }
      });
    }
    wk.join();
    if (wk.failed) return ZN_E_ALLOC;
  }
  for (int g = 0; g < ndev; g++) if (rcs[(size_t)g]) return rcs[(size_t)g];
  return ZN_OK;
}

int zn_decompress_multi(const void* body, size_t body_len, int num_buf, int bits_mode, int bytes_mode, size_t chunk, size_t orig_size,
                        const int* devices, int ndev, void* dst) {
  if ((body_len && !body) || (orig_size && !dst) || !devices || ndev <= 0 || ndev > 64 || !chunk) return ZN_E_ARG;
  if (num_buf != 1 && num_buf != 2 && num_buf != 4) return ZN_E_ARG;
  if (ndev == 1 || orig_size == 0) return zn_decompress(body, body_len, num_buf, bits_mode, bytes_mode, chunk, orig_size, devices[0], dst);
  if (zn_device_count() <= 0) return ZN_E_NODEV;
  try { return zn_decompress_ranges(body, body_len, num_buf, bits_mode, bytes_mode, chunk, orig_size, devices, ndev, dst, nullptr); }
  catch (...) { return ZN_E_ALLOC; }
}

int zn_decompress_multi_dev(const void* body, size_t body_len, int num_buf, int bits_mode, int bytes_mode, size_t chunk, size_t orig_size,
                            const int* devices, int ndev, void* const* d_dst) {
  if ((body_len && !body) || !devices || ndev <= 0 || ndev > 64 || !chunk || (orig_size && !d_dst)) return ZN_E_ARG;
  if (num_buf != 1 && num_buf != 2 && num_buf != 4) return ZN_E_ARG;
  if (orig_size == 0) return ZN_OK;
  if (zn_device_count() <= 0) return ZN_E_NODEV;
  const size_t K = (orig_size + chunk - 1) / chunk;
  for (int g = 0; g < ndev; g++) { const ZnRange r = zn_range_of(K, g, ndev); if (r.hi > r.lo && !d_dst[g]) return ZN_E_ARG; }
  try { return zn_decompress_ranges(body, body_len, num_buf, bits_mode, bytes_mode, chunk, orig_size, devices, ndev, nullptr, d_dst); }
  catch (...) { return ZN_E_ALLOC; }
}

static int zn_copy_host(void* d, void* h, size_t n, bool to_device) {
  if (n == 0) return ZN_OK;
  if (!d || !h) return ZN_E_ARG;
  if (zn_device_count() <= 0) return ZN_E_NODEV;
  HostLease H;                                            // one user of the device's bounce buffers at a time
  if (H.rc) return H.rc;
  try { return pipe_copy(H.hp->pipe, d, h, n, to_device); } catch (...) { return ZN_E_ALLOC; }
}
int zn_copy_to_device(void* d_dst, const void* src, size_t n) { return zn_copy_host(d_dst, const_cast<void*>(src), n, true); }
int zn_copy_to_host(void* dst, const void* d_src, size_t n) { return zn_copy_host(const_cast<void*>(d_src), dst, n, false); }

}  // extern "C"
