// zn_workspace.hpp — the per-device state of the C-ABI host layer and the one way to hold it.
//
// Shared by zn_api.hip (the device-pointer API) and zn_api_host.hip (everything that takes host buffers); the globals
// declared here are defined once, in zn_api.hip.  Two structs per device, one lock each:
//   Workspace (g_dev_mu): the kernels' scratch, the status slots, the event that orders calls between streams — held through a WsLease;
//   HostPath  (g_host_mu): the device staging of host buffers, the two pinned pipes and the pipeline's stream.
// A host-buffer call takes g_host_mu first and reaches the device layer through the public *_dev functions, which take g_dev_mu.
#pragma once

#include "../../include/zipnn_hip.h"
#include "zn_internal.hpp"
#include "zn_host_pipe.hpp"

#include <mutex>
#include <string>
#include <string.h>
#include <stdlib.h>

extern thread_local std::string t_hip_err;       // zn_last_hip_error
extern thread_local std::string t_kernels;       // zn_last_kernels

#define ZN_HIP(call)                                                            \
  do {                                                                          \
    hipError_t e_ = (call);                                                     \
    if (e_ != hipSuccess) {                                                     \
      t_hip_err = std::string(#call) + ": " + hipGetErrorString(e_);            \
      return ZN_E_HIP;                                                          \
    }                                                                           \
  } while (0)

// ---- small pure helpers ----
// plane count (1, 2, 4) <-> class index (0, 1, 2): the per-plane-count arrays of a call
static inline int zn_class_of(uint32_t P) { return P == 1 ? 0 : P == 2 ? 1 : 2; }
static inline int zn_planes_of(int q) { return 1 << q; }

// a device status word as a return code
static inline int status_to_rc(uint32_t st) {
  if (st & ZN_DEV_BAD_TYPE) return ZN_E_TYPE;
  if (st & ZN_DEV_CORRUPT) return ZN_E_CORRUPT;
  if (st & ZN_DEV_SYNC_TIMEOUT) { t_hip_err = "a workgroup gave up waiting for another one of the same launch (device preempted or faulted?)"; return ZN_E_TIMEOUT; }
  return ZN_OK;
}

// did a kernel launch since the last look fail?  (sets zn_last_hip_error)
static inline bool launch_failed() {
  const hipError_t el = hipGetLastError();
  if (el == hipSuccess) return false;
  t_hip_err = std::string("kernel launch: ") + hipGetErrorString(el);
  return true;
}

// the current device, as an index into the per-device tables
static inline int zn_current_dev(int* dev) {
  ZN_HIP(hipGetDevice(dev));
  return (*dev < 0 || *dev >= 64) ? ZN_E_ARG : ZN_OK;
}

// the host entry points take a device ordinal: switch to it for the call and leave the caller's current device as it was
struct DeviceScope {
  int prev = -1; bool ok = true;
  explicit DeviceScope(int device) {
    if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); ok = false; }
  }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// a grow-only device buffer (a slot of Workspace or of HostPath)
static inline int zn_dev_reserve(void** buf, size_t* cap, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (*cap >= bytes) return ZN_OK;
  if (*buf) { ZN_HIP(hipFree(*buf)); *buf = nullptr; *cap = 0; }
  hipError_t e = hipMalloc(buf, bytes);
  if (e != hipSuccess) { t_hip_err = std::string("hipMalloc: ") + hipGetErrorString(e); (void)hipGetLastError(); return ZN_E_ALLOC; }
  *cap = bytes;
  return ZN_OK;
}

// A grow-only pinned staging buffer; the capacity is in BYTES and its users copy by bytes.
struct ZnPinned {
  void* p = nullptr; size_t cap = 0;
  int reserve(size_t bytes) {
    if (cap >= bytes) return ZN_OK;
    if (p) { ZN_HIP(hipHostFree(p)); p = nullptr; cap = 0; }
    ZN_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    cap = bytes;
    return ZN_OK;
  }
  void release() { if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; } }
};

// ---- the device workspace: everything g_dev_mu guards ----
#define ZN_STATUS_SLOTS 16u
#define ZN_WORDS_BYTES (64u + ZN_STATUS_SLOTS * 4u * sizeof(uint32_t))
enum { WS_PLANES = 0, WS_ENC, WS_META_A, WS_META_B, WS_META_C, WS_WORDS, WS_DESC, WS_SEGS, WS_TOTALS, WS_LB, WS_COUNT };

// Grow-only device buffers cached per device; guarded by one mutex (calls on the same
// device serialise on their workspace — independent GPUs run in independent processes).
struct Workspace {
  size_t last_K = 0;             // chunks of the last decompress call (for zn_last_fused_chunks)
  size_t last_tails = 0;         // tail planes of the last decompress call (for zn_last_tail_planes)
  void* buf[WS_COUNT] = {};
  size_t cap[WS_COUNT] = {};
  uint32_t op_backoff = 0, op_penalty = 0;   // automatic one-pass encoding sits out `op_backoff` calls after a misspeculated one (compress_items)
  uint32_t lb_gen = 0;           // generation tag of the one-pass encoder's look-back words (WS_LB): a launch only believes words of its own generation, so the array is never zeroed between calls
  ZnPinned h_segs;               // pinned staging for the table of a batched call (encode segments / decode segments + hint table / digest items)
  ZnPinned h_totals;             // pinned: body lengths of a batched compress
  uint64_t* h_total = nullptr;   // pinned host word for the length read-back
  uint32_t* h_status = nullptr;
  hipEvent_t busy = nullptr;     // orders the workspace between streams (WsLease)
  hipStream_t only_stream = nullptr; bool have_stream = false, multi = false;   // one stream so far (its handle is only ever COMPARED) / several: an event per call
  // (a stream created at a destroyed one's address compares equal: the header's contract — destroy a stream only after its asynchronous calls have
  //  finished — is what covers that; hipStreamGetId, which could tell the two apart, is a hip_7.1 symbol and the runtime PyTorch 2.10 loads is 7.0)
  // decode status words: ZN_STATUS_SLOTS slots of four words behind the buffer's first 64 bytes, handed out in turn — a decode on another thread or stream
  // does not zero the word a check = 0 caller has yet to read (zn_decode_status)
  uint64_t status_gen = 0, slot_gen[ZN_STATUS_SLOTS] = {};
  uint32_t last_slot = 0;
  hipStream_t dstream = nullptr, dstream2 = nullptr; hipEvent_t dfork = nullptr, djoin = nullptr, djoin2 = nullptr;   // a mixed batched decode: the one-plane tensors' launches on one of these streams, the others' on the other

  int reserve(int slot, size_t bytes) { return zn_dev_reserve(&buf[slot], &cap[slot], bytes); }
  int host_words() {
    if (!h_total) ZN_HIP(hipHostMalloc((void**)&h_total, 64, hipHostMallocDefault));
    h_status = (uint32_t*)(h_total + 4);
    return ZN_OK;
  }
};

// ---- the host path of a device: everything g_host_mu guards, and nothing else does ----
enum { HP_IN = 0, HP_OUT, HP_DELTA, HP_COUNT };
struct HostPath {
  void* buf[HP_COUNT] = {};      // device staging for host buffers: cached like the workspace (grow-only), one host-path call at a time per device
  size_t cap[HP_COUNT] = {};
  ZnHostPipe pipe;               // pinned bounce buffers + copy stream of the host-buffer entry points
  ZnHostPipe pipe2;              // a second one: the pipelined host path downloads slice i - 1 while it uploads slice i + 1
  hipStream_t cstream = nullptr; // … and codes slice i on a stream of its own
  int reserve(int slot, size_t bytes) { return zn_dev_reserve(&buf[slot], &cap[slot], bytes); }
};

// One lock PER DEVICE (the workspace tables of different devices share nothing): threads that drive different GPUs of a
// node from one process — north_star's "independent HIP streams" — do not serialise each other.
extern std::mutex g_dev_mu[64];
extern Workspace g_ws[64];
extern std::mutex g_host_mu[64];  // serialises the host-buffer entry points of a device (they share two staging buffers)
extern HostPath g_host[64];

// "This call holds the current device's workspace on this stream."  Construction: the current device, its lock, its Workspace (rc != 0: none of them).
//
// The workspace is shared by every call on the device.  Host-side the mutex serialises them; device-side a call on another stream must not
// start before the previous call's kernels are done with the buffers: an event recorded behind every call, waited for by the next.  That
// record costs 3.5-6 us of a 60-120 us decode call (measured), and calls that follow each other on ONE stream are ordered by the stream itself:
// as long as the device's workspace has only ever seen one stream, nothing is recorded (`mark` excepted: a batched call's pinned segment table
// is rewritten from the HOST by the next batched call, which waits for the event).  The first call on a second stream synchronises the device
// once and switches the workspace to event-per-call for good.  (No stream handle is ever used after the call it came with: the caller may
// have destroyed it — hipEventRecord on a destroyed stream crashes, tried.)
//
// Once acquire() has succeeded the destructor hands the workspace back in stream order on EVERY way out of the call — behind kernels that a
// failed call has already queued, too: the next call on another stream must not run over them.
struct WsLease {
  int dev = 0, rc;
  Workspace* w = nullptr;
  bool mark = false;             // set by a call that staged a table through the pinned buffer
  WsLease() : rc(zn_current_dev(&dev)) { if (!rc) { lk = std::unique_lock<std::mutex>(g_dev_mu[dev]); w = &g_ws[dev]; } }
  WsLease(const WsLease&) = delete;
  WsLease& operator=(const WsLease&) = delete;
  int acquire(hipStream_t s) {
    if (!w->busy) ZN_HIP(hipEventCreateWithFlags(&w->busy, hipEventDisableTiming));
    if (w->multi) ZN_HIP(hipStreamWaitEvent(s, w->busy, 0));
    else if (w->have_stream && s != w->only_stream) {
      ZN_HIP(hipDeviceSynchronize());            // a second stream: whatever the first one still holds of the workspace is over after this
      w->multi = true;
    }
    stream = s; held = true;
    return ZN_OK;
  }
  ~WsLease() {
    if (!held) return;
    if (!w->multi) { w->only_stream = stream; w->have_stream = true; if (!mark) return; }
    if (hipEventRecord(w->busy, stream) != hipSuccess) (void)hipGetLastError();
  }
 private:
  std::unique_lock<std::mutex> lk;
  hipStream_t stream = nullptr; bool held = false;
};

// "This call holds the current device's host path": the current device, its host lock, its HostPath (rc != 0: none of them).
struct HostLease {
  int dev = 0, rc;
  HostPath* hp = nullptr;
  HostLease() : rc(zn_current_dev(&dev)) { if (!rc) { lk = std::unique_lock<std::mutex>(g_host_mu[dev]); hp = &g_host[dev]; } }
 private:
  std::unique_lock<std::mutex> lk;
};

// one transfer between a host buffer and device memory through a device's pinned pipe (through `map` where the caller's range is pinned); sets zn_last_hip_error
static inline int pipe_copy(ZnHostPipe& p, void* d, const void* h, size_t n, bool to_device, bool staged_only = false, ZnHostMap* map = nullptr) {
  if (n == 0) return ZN_OK;
  const hipError_t e = map ? zn_host_copy_mapped(*map, p, d, const_cast<void*>(h), n, to_device) : zn_host_pipe_copy(p, d, const_cast<void*>(h), n, to_device, nullptr, staged_only);
  if (e == hipSuccess) return ZN_OK;
  t_hip_err = to_device ? "host pipe H2D" : "host pipe D2H"; (void)hipGetLastError();
  return ZN_E_HIP;
}

// The status slot of a call that reports the way decodes do (zn_api.hip: a new slot, or — zn_decode_status_chain — the slot of the thread's previous unchecked
// call, *chain then true: its status word is kept).  The caller holds the device's WsLease and has reserved WS_WORDS.
uint32_t* zn_take_status_slot(Workspace& w, int dev, int check, bool* chain);

// zn_release_workspace's part of zn_api_host.hip: the host staging of the multi-device compress calls
void zn_host_release_stage();
