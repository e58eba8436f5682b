/*
 * zipnn_hip.h — C ABI of libzipnn_hip.so, the MI355X (gfx950) implementation of
 * ZipNN's compress/decompress hot path.
 *
 * This is the drop-in boundary.  In the reference the boundary is the CPython
 * extension `zipnn_core` (csrc/zipnn_core_module.c:9-23) with two functions:
 *
 *   zipnn_core.zipnn_core(header, data, numBuf, bits_mode, bytes_mode, is_redata,
 *                         origChunkSize, compThreshold, checkThAfterPercent, threads)
 *                                                  csrc/zipnn_core.c:401-702, called at zipnn/zipnn.py:714-725
 *   zipnn_core.combine_dtype(data_after_header, numBuf, bits_mode, bytes_mode,
 *                            origChunkSize, origSize, threads)
 *                                                  csrc/zipnn_core.c:881-1164, called at zipnn/zipnn.py:1143-1151
 *
 * zn_compress() / zn_decompress() below take exactly those arguments (minus the dead
 * ones: is_redata, checkThAfterPercent, threads — SURVEY.md Appendix D) as plain
 * pointers and sizes, and produce / consume exactly the same bytes (wire format:
 * SURVEY.md Appendix A).  The *_dev variants are the same operations on buffers that
 * already live in HBM (what bench.py times, and what a device-aware safetensors
 * loader calls).  No torch types, no exceptions, no longjmp: every function returns
 * 0 or a negative zn_status and never touches the caller's input buffers (the
 * reference rotates its input in place, csrc/data_manipulation_dtype16.c:68 — we
 * deliberately do not).
 *
 * Parameters shared by all entry points
 *   num_buf     1 (fp8), 2 (bf16/fp16), 4 (fp32)            zipnn/zipnn.py:786-815
 *   bits_mode   1 = sign-bit rotate (bf16/fp32), 0 = none   csrc/data_manipulation_dtype16.c:10-29, dtype32.c:39-58
 *   bytes_mode  10 for num_buf 1/2, 220 for num_buf 4        csrc/data_manipulation_dtype16.c:77, dtype32.c:219-268
 *   chunk       origChunkSize in bytes (power of two; callers pass min(128 KiB, chunk)
 *               for num_buf == 1, zipnn/zipnn.py:721,1148)
 *   threshold   compThreshold: a plane is kept Huffman-coded iff
 *               0 < csize < plane_len * (double)threshold    csrc/zipnn_core.c:371-373
 */
#ifndef ZIPNN_HIP_H
#define ZIPNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum zn_status {
  ZN_OK = 0,
  ZN_E_ARG = -1,      /* bad argument (unsupported num_buf/bytes_mode, chunk == 0, ...) */
  ZN_E_HIP = -2,      /* a HIP runtime call failed; zn_last_hip_error() has the text */
  ZN_E_CAP = -3,      /* destination capacity too small */
  ZN_E_CORRUPT = -4,  /* compressed body is malformed (sizes, huff0 header, streams) */
  ZN_E_TYPE = -5,     /* a chunk-type byte is not 0/1 (reference: MemoryError "Compress Type is not correct", zipnn_core.c:993-996) */
  ZN_E_NODEV = -6,    /* no usable GPU */
  ZN_E_ALLOC = -7,    /* device/host allocation failed */
  ZN_E_TIMEOUT = -8   /* a bounded device-side wait between workgroups of one launch ran out (a preempted or faulted device): the data was not judged */
} zn_status;

/* ABI version of this header (bumped on incompatible change). */
int zn_abi_version(void);
const char* zn_strerror(int status);
/* Text of the last failing HIP call on this thread ("" if none). */
const char* zn_last_hip_error(void);
/* Number of visible HIP devices (0 when none; never fails). */
int zn_device_count(void);

/* numChunks = ceil(n / chunk)                                   csrc/zipnn_core.c:420,893 */
size_t zn_num_chunks(size_t n, size_t chunk);
/* Upper bound of a frame: hdr_len + 9*num_buf*numChunks + n     csrc/zipnn_core.c:105-118 */
size_t zn_compress_bound(size_t n, int num_buf, size_t chunk, size_t hdr_len);

/* ---- host-buffer entry points (replace the two zipnn_core functions) ---- */

/* dst <- hdr ‖ types[P][K] ‖ cumSizes[P][K] (u64) ‖ payload (plane-major); when
 * hdr_len >= 32 the total frame length is written to dst[24:32] (zipnn_core.c:121).
 * `hdr`/`src`/`dst` are host pointers; the call stages through HBM on `device`. */
int zn_compress(const void* hdr, size_t hdr_len, const void* src, size_t n, int num_buf,
                int bits_mode, int bytes_mode, size_t chunk, float threshold, int device,
                void* dst, size_t dst_cap, size_t* dst_len);

/* body = frame minus (32-byte header + shape ext-header); dst receives orig_size bytes. */
int zn_decompress(const void* body, size_t body_len, int num_buf, int bits_mode, int bytes_mode,
                  size_t chunk, size_t orig_size, int device, void* dst);

/* ---- device-resident entry points (inputs and outputs already in HBM) ---- */

/* d_src: n bytes on the current device.  d_body (capacity body_cap >=
 * zn_compress_bound(n, num_buf, chunk, 0)) receives types ‖ cumSizes ‖ payload; its
 * length is returned in *body_len (one 8-byte device→host read).  `stream` is a
 * hipStream_t (NULL = the null stream); work is enqueued on it and the call returns
 * after the length has been read back. */
int zn_compress_dev(const void* d_src, size_t n, int num_buf, int bits_mode, int bytes_mode,
                    size_t chunk, float threshold, void* d_body, size_t body_cap,
                    size_t* body_len, void* stream);

/* d_body: body_len bytes on the current device; d_dst receives orig_size bytes.
 * Asynchronous on `stream` unless `check` is non-zero, in which case the call
 * synchronises and returns ZN_E_CORRUPT / ZN_E_TYPE if a kernel flagged bad input.
 * Streams: calls on one stream are ordered by it; once a device has seen calls on more than one stream, every call records an event that the
 * next one waits for on the device (the library's per-device workspace is shared).  Destroy a stream only after the asynchronous calls issued
 * on it have finished (synchronise it, or ask zn_decode_status, first). */
int zn_decompress_dev(const void* d_body, size_t body_len, int num_buf, int bits_mode,
                      int bytes_mode, size_t chunk, size_t orig_size, void* d_dst, void* stream,
                      int check);

/* Batched compress: `count` tensors (any mix of dtypes) through one launch per stage, one read-back of all body
 * lengths — what a safetensors producer or the streaming writer does per file (reference
 * scripts/zipnn_compress_safetensors.py:75-120, zipnn/zipnn.py:612-635).  Per item the semantics of
 * zn_compress_dev; body_len is filled in for every item. */
typedef struct zn_cbatch_item {
  const void* d_src; size_t n;            /* tensor bytes on the current device */
  int num_buf, bits_mode, bytes_mode;
  size_t chunk; float threshold;
  void* d_body; size_t body_cap;          /* >= zn_compress_bound(n, num_buf, chunk, 0) */
  size_t body_len;                        /* out */
  const void* d_delta;                    /* NULL, or n bytes on the device: the tensor is compressed as src ^ delta */
} zn_cbatch_item;
int zn_compress_batch_dev(zn_cbatch_item* items, size_t count, void* stream);

/* Batched decompress: `count` tensors (any mix of dtypes) decoded by one set of kernel launches, so that
 * many small tensors fill the device as one large one does.  What a safetensors loader does per file:
 * replaces the per-tensor loop around decompress_safetensors_tensor (reference zipnn/zipnn.py:1584-1596,
 * scripts/zipnn_decompress_safetensors.py:75-120).  Same semantics per item as zn_decompress_dev; an error
 * in any item fails the call. */
typedef struct zn_batch_item {
  const void* d_body; size_t body_len;   /* frame body (after the header), on the current device */
  void* d_dst; size_t orig_size;         /* receives orig_size bytes */
  int num_buf, bits_mode, bytes_mode;
  size_t chunk;
  const void* d_delta;                   /* NULL, or orig_size bytes on the device: dst <- decoded ^ delta */
} zn_batch_item;
int zn_decompress_batch_dev(const zn_batch_item* items, size_t count, void* stream, int check);

/* Chunk windows of device-resident bodies: item i decodes chunks [chunk_lo, chunk_hi) of its tensor from the WHOLE frame
 * body where it lies — the kernels read the window's rows of the body's size tables themselves, so nothing is copied or
 * re-based and the host never looks at the body.  For a checkpoint kept compressed in HBM: a layer, a tensor or a row
 * range is decoded when it is needed.  A window [0, zn_num_chunks(orig_size, chunk)) is zn_decompress_batch_dev's item;
 * chunk_lo == chunk_hi is an empty item; chunk_lo > chunk_hi or chunk_hi past the last chunk is ZN_E_ARG.  Everything
 * else (stream, check, zn_decode_status) as for zn_decompress_batch_dev. */
typedef struct zn_window_item {
  const void* d_body; size_t body_len;      /* the WHOLE frame body, on the current device */
  size_t orig_size;                         /* of the whole tensor */
  size_t chunk_lo, chunk_hi;                /* decode chunks [chunk_lo, chunk_hi) */
  void* d_dst;                              /* receives min(chunk_hi*chunk, orig_size) - chunk_lo*chunk bytes */
  int num_buf, bits_mode, bytes_mode; size_t chunk;
  const void* d_delta;                      /* NULL, or the whole tensor's base (orig_size bytes); the library offsets it */
} zn_window_item;
int zn_decompress_window_batch_dev(const zn_window_item* items, size_t count, void* stream, int check);

/* A prepared batched decode.  zn_plan_create (on the current device) does everything a batched decode call does before
 * its first launch — argument and geometry checks, the choice of kernels (the tuning knobs are read here, once), the
 * segment table — and keeps the table in device memory the plan owns.  zn_plan_run reserves the shared workspace, takes
 * a status slot and launches: no host-to-device copy and no host-side wait for earlier device work, so a caller can
 * enqueue the decode of layer i + 1 while layer i still runs.  It orders itself against other calls on the device as
 * every decode call does; check = 0 with zn_decode_status works as usual.  The plan refers to the items' bodies,
 * destinations and delta bases by address and does not own them: they must stay valid for every run.
 * zn_plan_destroy waits for the plan's last run (an event recorded behind every run: that stream, not the whole device) before it frees the table.  zn_release_workspace leaves plans intact. */
typedef struct zn_plan zn_plan;
int zn_plan_create(const zn_window_item* items, size_t count, zn_plan** plan);
int zn_plan_run(zn_plan* plan, void* stream, int check);
int zn_plan_destroy(zn_plan* plan);

/* Decode hints: a sidecar index for bodies that STAY where they are (a resident checkpoint decodes the same streams on every forward).  huff0 has no gap
 * array, so the fused decoder finds the start of every 64th-of-a-tile sub-block of a stream by speculation: a run-in, a check, now and then a second pass.  Those
 * starts are the same every time.  zn_hint_build_dev decodes a body once and keeps them — one byte per sub-block of the first Huffman-coded plane of every full
 * chunk, behind a table of one 32-bit offset per (chunk, plane) — in a device buffer of the caller's, next to the body, never inside it: frames and files are
 * untouched.  A hinted decode starts every sub-block from its byte and checks the result exactly as it checks a guess: hints are ADVICE.  Wrong, stale or random
 * bytes (or tables) cost time, never correctness — output bytes and the verdict are those of the unhinted call — and nothing is ever read outside
 * [d_hints, d_hints + hint_len).
 * VALIDITY: the tile geometry depends on the body's address modulo 4 and on this library's choice of sub-block sizes, so an index serves the body AT THE ADDRESS
 * it had when the index was built, decoded by the library build that built it (a resident store guarantees both).  Anything else is only slower.
 * What reads hints: the fused kernel's full-chunk workgroups in calls WITHOUT a delta base that do not take the small-input (wide) form — zn_set_decode_wide's
 * automatic rule decides that as for any call, before hints are looked at.  Partial last chunks, further Huffman planes of a chunk, the generic path and items
 * with a delta base (which make their whole launch unhinted — for an index of THIS kind; ZN_HINT_DELTA below is the kind such items read) decode as they always do.
 * zn_hint_size_dev: the index's length for the WHOLE body of `item` (chunk_lo / chunk_hi / d_dst / d_delta are ignored) — one small launch, one 8-byte read-back.
 * zn_hint_build_dev: fills d_hints (16-byte aligned; hint_cap >= that length, else ZN_E_ARG); synchronous; device scratch: a byte per (plane, chunk).
 * A hinted item is a window item plus its body's index (NULL / 0: none; a hint_len below zn_hint_size_dev's answer, NULL with a length, or an unaligned
 * pointer: ZN_E_ARG — the first hinted call on a body the two functions above have not seen sizes it itself, with their read-back).  Windows index the table by
 * the body's chunk numbers: one index serves every window of its body.  A plan made by zn_plan_create_hinted is run and destroyed like any other.
 * (The emulated test build also exports a counter read-out with the signature (unsigned long long out[4], int reset), named like the tile counters' but with
 * "hint" for "tile": out[0] tiles that started from hints, [1] those of them that needed a fix-up iteration, [2] tiles of hinted launches that ran without
 * hints, [3] hint bytes written by builds.  The device build has no counters.) */
typedef struct zn_hinted_item {
  zn_window_item item;
  const void* d_hints; size_t hint_len;
} zn_hinted_item;
int zn_hint_size_dev(const zn_window_item* item, size_t* hint_bytes, void* stream);
int zn_hint_build_dev(const zn_window_item* item, void* d_hints, size_t hint_cap, void* stream);
int zn_decompress_hinted_batch_dev(const zn_hinted_item* items, size_t count, void* stream, int check);
int zn_plan_create_hinted(const zn_hinted_item* items, size_t count, zn_plan** plan);
/* Index KINDS.  The four functions above make and read indexes of kind ZN_HINT_PLAIN: for bodies decoded WITHOUT a delta base.  A body that holds tensor ^ base (a
 * fine-tune kept as a delta, decoded with d_delta set) is decoded by other instances of the fused kernel — they choose other sub-block sizes, and every plane of
 * such a body compresses, so that the planes behind the first Huffman-coded one are decoded by further passes.  ZN_HINT_DELTA is the index for them: the same
 * container (offset table, 64-byte padding, hint bytes; four streams one behind the other per region), in which EVERY Huffman-coded plane of a full chunk the
 * fused kernel takes has a region — a plane without one has an empty region, table entry == the next entry — and whose bytes are valid for the delta instances'
 * sub-block sizes: it is built by those instances (without a base: the build needs none and writes no rows) and read by them, separate destination, plain base
 * tensor or IN PLACE (below), the undo of a chunk handed down included.
 * WHICH INDEX IS READ: an item reads its index iff (kind == ZN_HINT_DELTA) == (item.d_delta != NULL).  A launch that has a delta base anywhere among its items
 * of one plane count runs the delta instances for all of them and reads DELTA indexes only; a PLAIN index beside a delta base, a DELTA index beside none, or any
 * index in a call that takes the small-input form decodes unhinted, exactly as before.  Either kind is ADVICE with the guarantees stated above; an index of one
 * kind handed over as the other costs time at most.  The argument checks are those of the functions above, against the length zn_hint_size_dev2 gives for the
 * KIND named; a kind other than these two is ZN_E_ARG.  zn_hint_size_dev / zn_hint_build_dev / zn_decompress_hinted_batch_dev / zn_plan_create_hinted are
 * kind ZN_HINT_PLAIN of the functions below, byte for byte.  Not hinted, in either kind: partial last chunks and the small-input (wide) form. */
#define ZN_HINT_PLAIN 0
#define ZN_HINT_DELTA 1
typedef struct zn_hinted_item2 {
  zn_window_item item;
  const void* d_hints; size_t hint_len;
  int kind;                                 /* ZN_HINT_PLAIN / ZN_HINT_DELTA: what d_hints was built as */
} zn_hinted_item2;
int zn_hint_size_dev2(const zn_window_item* item, int kind, size_t* hint_bytes, void* stream);
int zn_hint_build_dev2(const zn_window_item* item, int kind, void* d_hints, size_t hint_cap, void* stream);
int zn_decompress_hinted_batch_dev2(const zn_hinted_item2* items, size_t count, void* stream, int check);
int zn_plan_create_hinted2(const zn_hinted_item2* items, size_t count, zn_plan** plan);

/* Delta ("byte"/"file" delta_compressed_type of the reference, zipnn/zipnn.py:625-640 and :983-1004: the bytes
 * are XORed with a second buffer of the same length before compression and after decompression).  The XOR is
 * fused into the kernels that read the tensor / write the output — no extra pass over HBM.  d_delta = NULL gives
 * zn_compress_dev / zn_decompress_dev.  Batched: set d_delta in the items above.
 * IN PLACE: in zn_decompress_delta_dev, zn_decompress_batch_dev, zn_decompress_window_batch_dev, zn_decompress_hinted_batch_dev and plans an item's
 * destination may BE its base — a whole tensor: d_dst == d_delta; a window: d_dst == (char*)d_delta + chunk_lo * chunk.  The destination then ends as
 * decoded ^ (what it held), the bytes a decode into a separate buffer gives, in every form of the decoder: any address alignment, partial last chunks, every
 * chunk the fused kernel hands down.  XOR is its own inverse: the same call (a plan run a second time) over the result gives the base back — a tensor that
 * holds a base model's weights becomes the fine-tune's and the base's again without a second copy.  Exactly that aliasing and no other: a base that overlaps
 * its destination in any other way is undefined, as are two items of a call that write the same bytes.  A call that fails (ZN_E_CORRUPT, ZN_E_TYPE) leaves
 * an in-place destination undefined like any other — the base with it. */
int zn_compress_delta_dev(const void* d_src, const void* d_delta, size_t n, int num_buf, int bits_mode,
                          int bytes_mode, size_t chunk, float threshold, void* d_body, size_t body_cap,
                          size_t* body_len, void* stream);
int zn_decompress_delta_dev(const void* d_body, size_t body_len, const void* d_delta, int num_buf, int bits_mode,
                            int bytes_mode, size_t chunk, size_t orig_size, void* d_dst, void* stream, int check);
/* … and with host buffers (`delta`: n / orig_size host bytes, or NULL): zn_compress / zn_decompress plus one more upload. */
int zn_compress_delta(const void* hdr, size_t hdr_len, const void* src, const void* delta, size_t n, int num_buf,
                      int bits_mode, int bytes_mode, size_t chunk, float threshold, int device,
                      void* dst, size_t dst_cap, size_t* dst_len);
int zn_decompress_delta(const void* body, size_t body_len, const void* delta, int num_buf, int bits_mode,
                        int bytes_mode, size_t chunk, size_t orig_size, int device, void* dst);

/* One call, several GPUs of the node (SURVEY.md §8b proposes exactly this `devices, ndev` form of the two entry points; the
 * reference's counterpart is its `threads` argument — csrc/zipnn_core.c:401 "y*y*iiiinfii", :881 "y*iiinni" — which fans the
 * chunks out over pthreads, zipnn_core.c:294-390 / 768-861).  Device i codes the contiguous chunk range [i K / ndev,
 * (i + 1) K / ndev) on a host thread, stream and workspace of its own; no collective; the host concatenates types and payload
 * per plane and re-bases cumSizes.  The frame / the bytes are identical to the single-device call's.  ndev = 1 IS that call.
 * The same device may be listed more than once (its ranges then run one after the other). */
int zn_compress_multi(const void* hdr, size_t hdr_len, const void* src, size_t n, int num_buf, int bits_mode, int bytes_mode,
                      size_t chunk, float threshold, const int* devices, int ndev, void* dst, size_t dst_cap, size_t* dst_len);
int zn_decompress_multi(const void* body, size_t body_len, int num_buf, int bits_mode, int bytes_mode, size_t chunk,
                        size_t orig_size, const int* devices, int ndev, void* dst);

/* The same with the TENSOR resident in HBM, range by range — what a sharded loader / saver holds: device i owns the bytes of the
 * chunk range zn_multi_range(n, chunk, ndev, i) gives, at d_dst[i] / d_src[i] (device memory of devices[i]; NULL for an empty
 * range).  The frame (or its body) stays a host buffer — it comes from / goes to a file.  Decompress: each range's size tables are
 * re-based on the host (9 num_buf bytes per chunk), its payload slices go from `body` straight through that device's pinned pipe
 * into HBM, the decoded bytes never cross PCIe.  Compress: each device codes its range where it lies; only the compressed bodies
 * come back.  One host thread, stream and workspace per listed device; no collective.  Bytes identical to the single-device call. */
int zn_multi_range(size_t n, size_t chunk, int ndev, int i, size_t* off, size_t* len);
int zn_decompress_multi_dev(const void* body, size_t body_len, int num_buf, int bits_mode, int bytes_mode, size_t chunk,
                            size_t orig_size, const int* devices, int ndev, void* const* d_dst);
int zn_compress_multi_dev(const void* hdr, size_t hdr_len, const void* const* d_src, size_t n, int num_buf, int bits_mode,
                          int bytes_mode, size_t chunk, float threshold, const int* devices, int ndev, void* dst, size_t dst_cap,
                          size_t* dst_len);

/* The two halves of the same for ONE process per GPU (torch.distributed ranks, each with its own device): a rank decodes the chunk
 * range [chunk_lo, chunk_hi) of a host-resident frame body straight into its own HBM (the sub-body is put together on the device:
 * re-based size tables from the host, payload slices through the pinned pipe; nothing decoded crosses PCIe) … */
int zn_decompress_range_dev(const void* body, size_t body_len, int num_buf, int bits_mode, int bytes_mode, size_t chunk,
                            size_t orig_size, size_t chunk_lo, size_t chunk_hi, int device, void* d_dst);
/* … and the bodies the ranks wrote for CONSECUTIVE chunk ranges (rank i: zn_compress_dev of its num_chunks[i] chunks) become the one
 * body a single device would have written: types and payload concatenated per plane, cumSizes re-based (host pointers; one thread
 * per part does the copying).  dst_cap >= the sum of the body lengths. */
int zn_merge_range_bodies(const void* const* bodies, const size_t* body_lens, const size_t* num_chunks, int nparts, int num_buf,
                          void* dst, size_t dst_cap, size_t* dst_len);

/* CONTENT DIGESTS ("zn64-1").  The frame format carries no checksums, and a damaged raw plane decodes cleanly to wrong bytes: a digest of the DECODED bytes
 * is what tells.  It is an error-detecting code, NOT a cryptographic hash: it catches damage, not an adversary.  The definition (all arithmetic unsigned, wrapping):
 *
 *   fmix32(x): x ^= x>>16; x *= 0x85EBCA6B; x ^= x>>13; x *= 0xC2B2AE35; x ^= x>>16                             (mod 2^32)
 *   mix64(z):  z ^= z>>30; z *= 0xBF58476D1CE4E5B9; z ^= z>>27; z *= 0x94D049BB133111EB; z ^= z>>31             (mod 2^64)
 *   G = 0x9E3779B97F4A7C15
 *   bytes b[0..n), zero-padded to a multiple of 4; w_j = little-endian 32-bit word j, counted from the FIRST BYTE (not from an aligned address)
 *   block c = words [65536 c, 65536 (c+1))                 -- 256 KiB of data, whatever the frame's chunk size or dtype
 *   B_c = sum_i (u64)w_{65536 c + i} * (u64)fmix32(i + 1)                                                           (mod 2^64)
 *   D   = mix64(n + G) + sum_c mix64(B_c + (c + 1) G)                                                               (mod 2^64)
 *
 * D("") = 0xe220a8397b1dcdaf, D("\x01") = 0x947511c5412f4857.  Inside a block every change of one word and every swap of two words changes B_c (a nonzero
 * difference below 2^32 times a nonzero key difference below 2^32 cannot vanish mod 2^64; fmix32 is a bijection and never 0 on 1..65536); block order and
 * length enter through c and n.  Blocks combine by a commutative sum: every schedule gives the same value.
 *
 * zn_digest_batch_dev: `count` byte ranges in device memory (any byte address, any length, ragged) -> d_out[i] = D(item i), `count` 8-byte-aligned device
 * slots; one launch for the whole batch on `stream`, NO host wait for the result (read d_out behind the stream).  A call with count > 1 stages its item table in
 * the pinned buffer the batched decode calls use, and like them waits on the host until the previous batched call on the device has read it; a single item travels
 * as a kernel argument and waits for nothing.  count == 0 and n == 0 are valid; a null
 * d_src with n > 0 (or a null d_out) is ZN_E_ARG.  The kernel reads aligned 16-byte granules and only those that hold a byte of the item.
 * zn_digest_host: the same value by a scalar loop on the host, for host buffers and files. */
typedef struct zn_digest_item { const void* d_src; size_t n; } zn_digest_item;
int zn_digest_batch_dev(const zn_digest_item* items, size_t count, unsigned long long* d_out, void* stream);
int zn_digest_host(const void* src, size_t n, unsigned long long* out);

/* CHANGED-ELEMENT PATCHES ("znp1").  huff0 spends at least a bit on every symbol of every plane it codes, so a delta body (tensor ^ base) is never much below
 * 1/8 of a bf16 tensor however little changed.  A patch is the representation below that floor: the canonical list of the elements that differ from the base,
 * with their XOR values.  It covers a tensor of n bytes with element size E in {1, 2, 4} (E = the plane count num_buf), n % E == 0, m = n / E < 2^32; anything
 * else is not eligible (ZN_E_ARG).  Blocks hold 65 536 elements whatever a frame's chunk size; NB = ceil(m / 65536); T = the number of elements whose bytes
 * differ from the base's.  Everything little-endian, every section at a multiple of 16, padding bytes zero:
 *
 *   offset 0                               "ZNP1", u8 E, three zero bytes
 *   offset 8                               u64 n
 *   offset 16                              u64 T
 *   offset 24                              u64 L, the patch's total length
 *   offset 32                              u32 first[NB + 1]: entries in front of block b; first[NB] == T
 *   A1 = round16(32 + 4 (NB + 1))          u16 off[T]: the element's offset inside its block, strictly ascending within a block
 *   A2 = round16(A1 + 2 T)                 val[T], E bytes each: tensor ^ base at that element, never zero
 *   L  = A2 + E T
 *
 * The patch of a (tensor, base) pair is UNIQUE: exactly the differing elements, in ascending order — every schedule produces the same bytes.  Applying is
 * dst[e] ^= val; the same patch applied twice gives the base back.
 * zn_patch_len: L for (n, elem, T) — 0 when (n, elem) is not eligible or T > m.
 * zn_patch_size_batch_dev: the count pass alone — sizes_out[i] = L of item i, or 0 when its bytes are the base's (T == 0); one read-back of all lengths.
 * zn_patch_build_batch_dev: count, scan and emit; patch_len = L, or 0 (nothing written) for an identical item; d_patch 16-byte aligned; ZN_E_CAP when a capacity
 *   is short (patch_len then holds what every item needs and nothing was written).  Both are synchronous, like compress; d_src / d_base at any elem-aligned
 *   address (16-byte loads when both are 16-byte aligned).  The source must not change during the call; if it does the patch is wrong, never the memory around it.
 * zn_patch_apply_batch_dev: one launch for the batch.  Only the entries inside the byte window [byte_lo, byte_hi) (multiples of elem, byte_hi <= n) are applied;
 *   d_dst (elem-aligned) is where the window's first byte lies and receives that range.  d_base == NULL: in place, d_dst ^= patch.  Otherwise the window's bytes
 *   are first copied from d_base + byte_lo on the stream.  An empty window and a patch with T == 0 are valid.  d_patch 16-byte aligned, patch_len >= 32 (else
 *   ZN_E_ARG).  A patch may come from anywhere: the kernel writes nothing outside the window, reads nothing outside [d_patch, d_patch + patch_len), and reports
 *   ZN_E_CORRUPT through the call's status slot — check, zn_decode_status, zn_decode_status_chain, exactly as decodes do — for a header that disagrees with the
 *   item (E, n, L against patch_len), a first[] that decreases or exceeds T, an offset beyond the tensor's last element, offsets not strictly ascending inside a
 *   block, or a zero value.  (first[] is checked for the blocks the window touches.)  A wrong patch costs the verdict, never a byte outside the destination;
 *   the destination itself is then undefined.
 * zn_patch_plan_*: mirror zn_plan_*: the table lives in device memory the plan owns, a run launches only (and enqueues the base copies of items with d_base), its
 *   verdict joins a chain when the thread has one open; the plan refers to patches, destinations and bases by address.
 * zn_patch_check_batch_dev: is each patch WELL-FORMED — the whole of it, before anything is applied?  What a reader does with a patch it did not build itself (a
 *   file's): apply checks only what its window reads and has written by the time it knows.  One launch for the batch (zn_k_patch_check: one workgroup
 *   per block of every item), which reads [d_patch, d_patch + patch_len) and writes nothing but the verdict words; synchronous, one read-back for the batch, like
 *   zn_patch_size_batch_dev.  verdicts_out[i] (host) = 0 for a well-formed patch of a tensor of n bytes in elements of `elem`, else a mask of
 *     ZN_PATCH_BAD_HEADER   the magic, E or n is not the item's, T > m, or L is not patch_len and the formula's value for T (nothing else is read then)
 *     ZN_PATCH_BAD_FIRST    first[0] != 0, first[NB] != T, or a pair first[b] > first[b + 1] or first[b + 1] > T — every pair, not a window's
 *     ZN_PATCH_BAD_OFFSET   an offset at or beyond the tensor's last element, or offsets not strictly ascending inside a block
 *     ZN_PATCH_BAD_VALUE    a zero value
 *     ZN_PATCH_BAD_PADDING  the canonical form, which apply never reads: header bytes 5-7, the bytes between first[] and off[] or between off[] and val[] not zero
 *   entries_out[i] (host, may be NULL) = T of a well-formed item, 0 otherwise.  The call returns ZN_OK whenever it ran — the verdicts are per item —, ZN_E_ARG before
 *   any launch for patch_len < 32, a d_patch that is null or not 16-byte aligned, or an (n, elem) that is not eligible.
 *   What it cannot see: a first[] boundary moved so that both neighbouring blocks still ascend is a well-formed patch — of another tensor.  Only the content
 *   digests (verify) catch that.
 * zn_patch_apply_strided_batch_dev: the patch applied through a STRIDED VIEW of live memory whose logical row-major order is the tensor's: a
 *   weight kept transposed, a column slice of a fused buffer, a tile-shuffled or channels-last layout.  An index map per entry, not a pass over the tensor.
 *   d_dst (elem-aligned) is where LOGICAL element 0 lies; size[] / stride[] (strides in ELEMENTS, ndim in 0 .. ZN_PATCH_MAX_DIMS, ndim == 0: one element)
 *   describe the view, and the sizes' product must be n / elem.  The call is IN PLACE ONLY: no d_base, no byte window, no plan form — the whole patch is
 *   always applied, every block is visited, and a call that returns clean has validated everything but the canonical padding.  One launch for the batch
 *   (zn_k_patch_apply_strided: one workgroup per block of every item); the verdict goes through the call's status slot — check, zn_decode_status,
 *   zn_decode_status_chain — exactly as zn_patch_apply_batch_dev's, with the same tests; an entry that fails them is not applied.  Nothing outside
 *   [d_patch, d_patch + patch_len) is read, and nothing is written but the elem bytes of elements of the view.
 *   Before the launch the host makes the layout canonical — dimensions of size 1 dropped, neighbours merged where stride[i] == size[i + 1] stride[i + 1]; a
 *   batch whose layouts all collapse to contiguous tensors takes zn_patch_apply_batch_dev's launch — and tests what remains for INJECTIVITY: sorted by stride
 *   ascending, every stride must exceed the sum over the smaller ones of (size - 1) stride, and no stride is 0.  The test is SUFFICIENT, NOT NECESSARY: it
 *   refuses expand() and overlapping as_strided views, and also injective views whose dimensions interleave.  ZN_E_ARG before any launch: ndim outside
 *   0 .. ZN_PATCH_MAX_DIMS, a product of the sizes that is not n / elem, a negative stride, a layout that fails the test or whose last element lies 2^62
 *   elements or more from the first, an (n, elem) that is not eligible, d_dst null with n > 0 or not elem-aligned, d_patch null or not 16-byte aligned,
 *   patch_len < 32.  A patch with T == 0 and a tensor with n == 0 are valid and write nothing.
 * zn_patch_size_strided_batch_dev / zn_patch_build_strided_batch_dev: zn_patch_size_batch_dev / zn_patch_build_batch_dev for a source and a base that are STRIDED
 *   VIEWS: what a trainer left in an engine's own layout, against the base in its own — two stride lists over one logical shape, d_src / d_base
 *   where LOGICAL element 0 of each lies.  The same semantics: count, scan, one read-back, emit; ZN_E_CAP with the needed lengths and nothing written;
 *   patch_len == 0 for identical bytes; synchronous.  The result is BYTE FOR BYTE the patch zn_patch_build_batch_dev gives for contiguous copies of the two
 *   views; no copy is made (zn_k_patch_count_strided, zn_k_patch_scan, zn_k_patch_emit_strided: one workgroup per block of every item, both sides read through
 *   their layouts).  The host makes the two layouts canonical JOINTLY — dimensions of size 1 dropped, neighbours merged only where both stride lists merge —;
 *   a batch whose items all collapse to contiguous tensors on both sides takes zn_patch_build_batch_dev's launches.  Views are only READ: there is no
 *   injectivity test, expand() (a stride of 0) and overlapping views are accepted.  ZN_E_ARG before any launch: ndim outside 0 .. ZN_PATCH_MAX_DIMS, a product
 *   of the sizes that is not n / elem, a negative stride, a last element 2^62 elements or more from the first, an (n, elem) that is not eligible, d_src or
 *   d_base null with n > 0 or not elem-aligned, a d_patch (with patch_cap > 0) that is not 16-byte aligned, or whose [d_patch, d_patch + patch_cap) overlaps
 *   the address span — first to last element — of either view.  The views must not change during the call; if they do the patch is wrong, never the memory
 *   around it. */
#define ZN_PATCH_BAD_HEADER 1u
#define ZN_PATCH_BAD_FIRST 2u
#define ZN_PATCH_BAD_OFFSET 4u
#define ZN_PATCH_BAD_VALUE 8u
#define ZN_PATCH_BAD_PADDING 16u
typedef struct zn_patch_size_item { const void* d_src; const void* d_base; size_t n; int elem; } zn_patch_size_item;
typedef struct zn_patch_build_item {
  const void* d_src; const void* d_base; size_t n; int elem;
  void* d_patch; size_t patch_cap;
  size_t patch_len;                         /* out */
} zn_patch_build_item;
typedef struct zn_patch_apply_item {
  const void* d_patch; size_t patch_len;
  size_t n; int elem;                       /* of the whole tensor */
  size_t byte_lo, byte_hi;
  void* d_dst; const void* d_base;
} zn_patch_apply_item;
typedef struct zn_patch_plan zn_patch_plan;
size_t zn_patch_len(size_t n, int elem, size_t entries);
int zn_patch_size_batch_dev(const zn_patch_size_item* items, size_t count, size_t* sizes_out, void* stream);
int zn_patch_build_batch_dev(zn_patch_build_item* items, size_t count, void* stream);
int zn_patch_apply_batch_dev(const zn_patch_apply_item* items, size_t count, void* stream, int check);
int zn_patch_plan_create(const zn_patch_apply_item* items, size_t count, zn_patch_plan** plan);
int zn_patch_plan_run(zn_patch_plan* plan, void* stream, int check);
int zn_patch_plan_destroy(zn_patch_plan* plan);
#define ZN_PATCH_MAX_DIMS 8
typedef struct zn_patch_apply_strided_item {
  const void* d_patch; size_t patch_len;    /* 16-byte aligned, >= 32 */
  size_t n; int elem;                       /* the whole tensor: n bytes, elements of elem */
  void* d_dst;                              /* where LOGICAL element 0 lies; elem-aligned */
  int ndim; unsigned long long size[ZN_PATCH_MAX_DIMS]; long long stride[ZN_PATCH_MAX_DIMS];   /* strides in elements */
} zn_patch_apply_strided_item;
int zn_patch_apply_strided_batch_dev(const zn_patch_apply_strided_item* items, size_t count, void* stream, int check);
typedef struct zn_patch_build_strided_item {
  const void* d_src; const void* d_base;    /* where LOGICAL element 0 of each lies; elem-aligned */
  size_t n; int elem; int ndim;             /* the tensor: n bytes, elements of elem; ONE logical shape … */
  unsigned long long size[ZN_PATCH_MAX_DIMS];
  long long src_stride[ZN_PATCH_MAX_DIMS], base_stride[ZN_PATCH_MAX_DIMS];   /* … and a layout of its own for each side, strides in elements */
  void* d_patch; size_t patch_cap;          /* 16-byte aligned; unused by the size call */
  size_t patch_len;                         /* out (the build call) */
} zn_patch_build_strided_item;
int zn_patch_size_strided_batch_dev(const zn_patch_build_strided_item* items, size_t count, size_t* sizes_out, void* stream);
int zn_patch_build_strided_batch_dev(zn_patch_build_strided_item* items, size_t count, void* stream);
typedef struct zn_patch_check_item { const void* d_patch; size_t patch_len; size_t n; int elem; } zn_patch_check_item;
int zn_patch_check_batch_dev(const zn_patch_check_item* items, size_t count,
                             unsigned int* verdicts_out,        /* host, one per item: 0 = well-formed */
                             unsigned long long* entries_out,   /* host, may be NULL: T of each well-formed item */
                             void* stream);

/* MERGING PATCHES.  Patches are XOR lists, so two patches of one tensor combine without the tensor: the XOR-merge a (+) b holds the union of their elements, the
 * XOR of the two values where both have an entry, and no entry where that XOR is zero.  The format is canonical, so the result is unique, and it is byte for
 * byte what zn_patch_build_batch_dev builds from the tensors the merge never sees: merging the patch of A over a base with the patch of B over the same base
 * gives the patch of B over A (and of A over B — the merge is symmetric); merging the patches of consecutive steps s1 over s0, s2 over s1, … gives the patch of
 * the last step over s0.
 * zn_patch_merge_size_batch_dev: the count pass alone — sizes_out[i] = L of item i's merge, or 0 when everything cancels; one read-back; d_out / out_cap ignored.
 * zn_patch_merge_batch_dev: count, scan (zn_k_patch_scan), one read-back, emit; synchronous.  out_len = L, or 0 (nothing written) when everything cancels — the
 *   convention of an identical pair in build.  ZN_E_CAP when a capacity is short: every out_len then holds what is needed and nothing was written.
 * Both inputs describe a tensor of n bytes in elements of `elem` (eligible as above).  d_a, d_b and d_out 16-byte aligned, a_len and b_len >= 32, and
 * [d_out, d_out + out_cap) overlaps neither input; anything else — or an (n, elem) that is not eligible — is ZN_E_ARG before any launch.
 * Inputs may come from anywhere.  The kernels read nothing outside [d_x, d_x + x_len) — the header first: magic, E and n against the item, L against x_len and
 * the formula's value for T; then first[0] == 0, first[b] <= first[b + 1] <= T, first[NB] == T — and EVERY block of both inputs is visited, so a merge that
 * returns ZN_OK has validated both inputs whole: no offset beyond the tensor's last element, offsets strictly ascending inside a block, no zero value.  Only the
 * canonical padding is not looked at (zn_patch_check_batch_dev's ZN_PATCH_BAD_PADDING).  Anything wrong in any input of any item is ZN_E_CORRUPT for the call:
 * the outputs are then unspecified, and nothing outside [d_out, d_out + out_cap) was written. */
typedef struct zn_patch_merge_item {
  const void* d_a; size_t a_len;            /* 16-byte aligned, len >= 32 */
  const void* d_b; size_t b_len;
  size_t n; int elem;                       /* the tensor both patches cover */
  void* d_out; size_t out_cap;              /* 16-byte aligned; overlaps neither input */
  size_t out_len;                           /* out */
} zn_patch_merge_item;
int zn_patch_merge_size_batch_dev(const zn_patch_merge_item* items, size_t count, size_t* sizes_out, void* stream);
int zn_patch_merge_batch_dev(zn_patch_merge_item* items, size_t count, void* stream);

/* SHARDING PATCHES.  A patch is a sorted list of element indices, so the patch of a rectangle of a tensor follows from the tensor's patch without the tensor.
 * View the tensor as rows x cols elements and take rows [row_lo, row_hi) and cols [col_lo, col_hi), h x w elements.  The map from the rectangle's row-major index
 * j to the tensor's, phi(j) = (row_lo + j / w) cols + col_lo + j % w, is strictly increasing: SELECT keeps the entries inside the rectangle and re-indexes them
 * by the inverse of phi, PLACE re-indexes a rectangle's entries by phi; both re-block into blocks of 65 536 elements, neither sorts.  The format is canonical, so
 *   select(patch(T over B))           is byte for byte  patch(T[rect] over B[rect]),
 *   place(patch(S over B[rect]))      is byte for byte  patch(B with its rectangle set to S, over B),
 *   select(place(p)) == p, and the XOR-merge (above) of the placed selects of rectangles that tile the tensor is the tensor's patch again.
 * A narrow(dim, lo, hi - lo) of any shape is such a rectangle: rows = prod(shape[:dim]), cols = shape[dim] inner, cols [lo inner, hi inner), all rows.
 * zn_patch_select_size_batch_dev / zn_patch_place_size_batch_dev: the count pass alone — sizes_out[i] = L of item i's result, or 0 when no entry results; one
 *   read-back; d_out / out_cap ignored.
 * zn_patch_select_batch_dev / zn_patch_place_batch_dev: count, scan (zn_k_patch_scan), one read-back (totals and the verdict), emit; synchronous, like build and
 *   merge.  out_len = L, or 0 (nothing written) when no entry results.  ZN_E_CAP when a capacity is short: every out_len then holds what is needed and nothing
 *   was written.
 * The input's header must carry n = rows cols elem for select and n = h w elem for place.  ZN_E_ARG before any launch: an empty rectangle or one that is not
 * inside the tensor, an elem that is not 1, 2 or 4, rows cols >= 2^32, d_patch or d_out null or not 16-byte aligned, patch_len < 32, or [d_out, d_out + out_cap)
 * overlapping the input.
 * Inputs may come from anywhere.  The kernels read nothing outside [d_patch, d_patch + patch_len) — the header first: magic, E and n against the item, T <= m, L
 * against patch_len and the formula's value for T — and, for every input block a workgroup visits, first[b] <= first[b + 1] <= T, first[0] == 0, first[NB] == T,
 * no more entries than the block has elements, and for every entry of it: the index inside the tensor, offsets strictly ascending, no zero value.  What a returned
 * ZN_OK has validated: PLACE — the whole input (every input block is visited); SELECT — the header and the input blocks it visits (for each output block: those from
 * its first element's to its last element's, so at least every block that holds an element of the rectangle), and NOTHING of the others — blocks in front of the
 * rectangle's first row, behind its last, or in the gap between two output blocks: validating the rest is zn_patch_check_batch_dev's job.  (The canonical
 * padding is never looked at.)  Anything wrong in any visited part of any item is ZN_E_CORRUPT for the call: the outputs are then unspecified, and nothing outside
 * [d_out, d_out + out_cap) was written. */
typedef struct zn_patch_select_item {
  const void* d_patch; size_t patch_len;    /* 16-byte aligned, len >= 32 */
  int elem;
  size_t rows, cols;                        /* the WHOLE tensor as rows x cols elements; rows * cols < 2^32 */
  size_t row_lo, row_hi, col_lo, col_hi;    /* the rectangle, non-empty, inside the tensor */
  void* d_out; size_t out_cap;              /* 16-byte aligned; does not overlap the input */
  size_t out_len;                           /* out: L, or 0 (nothing written) when no entry results */
} zn_patch_select_item;
int zn_patch_select_size_batch_dev(const zn_patch_select_item* items, size_t count, size_t* sizes_out, void* stream);
int zn_patch_select_batch_dev(zn_patch_select_item* items, size_t count, void* stream);
int zn_patch_place_size_batch_dev(const zn_patch_select_item* items, size_t count, size_t* sizes_out, void* stream);
int zn_patch_place_batch_dev(zn_patch_select_item* items, size_t count, void* stream);

/* Plumbing for callers that keep the tensors in HBM but hold pageable host buffers (files, Python bytes): the same
 * pinned, multi-threaded transfer the host-buffer entry points above use internally (zipnn_amd/csrc/zn_host_pipe.hpp),
 * on the current device; returns when the n bytes have arrived.  No reference counterpart — the reference's buffers
 * never leave the host (zipnn/zipnn.py:714-725, 1143-1151 hand host pointers straight to the C core). */
int zn_copy_to_device(void* d_dst, const void* src, size_t n);
int zn_copy_to_host(void* dst, const void* d_src, size_t n);

/* ---------------------------------------------------------------------------------------------------------------------------
 * DEVELOPER / TEST KNOBS — not part of the drop-in boundary.  The setters below are process-wide mutable state: they exist so that
 * the test-suite and the A/B scripts can force every kernel form on every input (tests/, scripts/) and so that a frame can be made
 * byte-identical to a PyPI wheel's; a production caller never needs them — every default is "automatic", and the bytes a call produces
 * or accepts do not depend on them (zn_set_legacy_tree_descriptions excepted).  They are NOT synchronised with calls in flight: set them before the first call of a
 * process (or between calls, from the one thread that drives the library) — never while another host thread is inside an entry point.
 * One host thread per GPU, as the multi-device entry points use the library, is safe with the defaults.
 * ------------------------------------------------------------------------------------------------------------------------- */

/* chunks one workgroup of the fused decoder takes, 1..4; 0 (default) = automatic: the group size whose launch takes the fewest
 * rounds of workgroups x (one parse of the group's tree descriptions + its chunks), a round being as many workgroups as the device
 * holds at once (profiles/r05_decode_group_rule.txt).  Returns 0 or ZN_E_ARG. */
int zn_set_decode_group(int chunks_per_workgroup);
/* what that rule (or the knob) gives a launch of `chunks` chunks on the current device: 1..4 */
int zn_decode_group_for(unsigned long long chunks);

/* the small-input form of the decoder (one workgroup per chunk, four or two waves per huff0 stream) — 0 = never,
 * 1 (default) = automatic: calls whose tensors are all split with the sign rotate (bits_mode 1 with 2 or 4 byte planes: bf16, fp32), have no
 * delta base and few workgroups per compute unit of the device — one per full chunk, plus, for a tensor with a partial last chunk (round 6), its tail
 * and merge workgroups, which ride in the same launch; 2 / 3 = every call without a
 * delta base, 16- / 8-wave form.  The bytes produced are the same in every mode.  Returns 0 or ZN_E_ARG. */
int zn_set_decode_wide(int mode);

/* slices of the three-stage pipeline upload | code | download that large pageable buffers can go through in the host-buffer entry points
 * (zn_compress / zn_decompress).  0 (default) = automatic (compress: 4-8 slices from 192 MiB up; decompress: one shot — measured: no gain
 * there — unless the direct transfers of zn_set_host_direct are on), 1 = never, 2..64 = that many, both directions.  Returns 0 or ZN_E_ARG. */
int zn_set_host_slices(int slices);

/* how the host-buffer entry points (zn_compress / zn_decompress, the *_multi forms, zn_copy_to_host / _to_device) move a caller's pageable buffer:
 * bit 2 (default, = 4): result buffers get madvise(MADV_HUGEPAGE) before they are first written — a page-size hint, nothing else;
 * bit 0 / bit 1 (opt-in; 7 = everything): device-to-host / host-to-device transfers of 128 MiB and more may go DIRECT — the caller's pages pinned piece
 * by piece (hipHostRegister), DMA straight between them and HBM, the two directions of a call pipelined in 4-8 slices; only for calls whose result buffer
 * is already backed by pages (recycled buffers), anything else takes the staged copy through the library's own pinned buffers.  1 GiB bf16 each way:
 * 23 ms direct with recycled buffers against 31-36 ms staged; why it is not the default: profiles/r06_host_path.txt (calls that fault a fresh result
 * buffer in get slower in a long-lived process that has pinned user memory).  Also ZIPNN_AMD_HOST_DIRECT=0..7 in the environment.  Returns 0 or ZN_E_ARG. */
int zn_set_host_direct(int mode);

/* Pinned host memory from the library's arena, for buffers that cross PCIe — above all the RESULT of zn_compress / zn_decompress, which the reference's extension
 * also allocates itself and returns as a memoryview (csrc/zipnn_core.c:596, 1126).  A transfer between such a block and HBM is one DMA (57 GB/s, no staging copy, no
 * page faults, and releasing it costs nothing: a pageable 1 GiB result costs its owner 40-130 ms of munmap): with a FRESH block per call — allocate, call, release —
 * 1 GiB of bf16 takes 28-30 ms to compress and 33-36 ms to decompress, all in, against 59-61 and 75 ms with a fresh pageable result; freed blocks are recycled (up to ZIPNN_AMD_HOST_ARENA_MB = 8192 MiB of them are kept;
 * zn_release_workspace returns them to the driver).  zn_host_alloc: NULL when the driver has no more pinned memory; zn_host_free: 0, or ZN_E_ARG for a pointer that
 * is not a live block.  Thread-safe. */
void* zn_host_alloc(size_t n);
int zn_host_free(void* p);

/* the one-pass encoder (full chunks histogrammed, coded and placed by one workgroup each, the chunk's second read aimed at the Infinity Cache) —
 * 0 = never (the four-kernel encoder only), 1 (default; ZIPNN_AMD_ONEPASS=0/1/2 in the environment changes the default) = automatic: calls whose
 * bf16-like tensors (two planes, sign rotate) bring at least 6144 full chunks — where it has measured faster —, 2 = every call with full chunks.
 * The four-kernel encoder is the fall-back for tensors whose planes other than the last do not all stay raw.  The bytes produced are the same in
 * every mode.  Returns 0 or ZN_E_ARG. */
int zn_set_encode_onepass(int mode);

/* Which huff0 the compressed bytes imitate where the two in circulation differ — the FSE-coded tree description of a plane, when one
 * of its code-weight values is rare enough to round below one FSE cell: 0 (default) = zstd >= 1.4.7 (a full cell, "+1"; what the
 * reference writes when built against a current libzstd, oracle/_ref), 1 = the FiniteStateEntropy library the reference's PyPI wheels
 * bundle (/root/reference/setup.py:23-28; the "less than one" marker, "-1").  Every huff0 decoder — this library's included — reads both;
 * with 1 the frames are byte-identical to a wheel's.  (The one knob that changes bytes; read once per compress call, at its start.)
 * Returns 0 or ZN_E_ARG. */
int zn_set_legacy_tree_descriptions(int on);

/* Frees the per-device workspaces this library caches (scratch planes, size tables). */
int zn_release_workspace(void);

/* The device-side verdict of the CALLING THREAD's last zn_decompress*_dev call on the current device with check = 0 (no read-back,
 * asynchronous): waits for `stream` and returns ZN_OK / ZN_E_TYPE / ZN_E_CORRUPT exactly as that call would have with check = 1.  For
 * callers that overlap host work with the decode (a checkpoint loader builds its tensor views while the kernels run) — the reference's
 * combine_dtype (csrc/zipnn_core.c:881) is synchronous and reports through its return value at once.  Every decode call writes its
 * verdict to a slot of its own (sixteen per device, handed out in turn), so decodes by other threads or on other streams in between
 * do not disturb it; after sixteen further decode calls on the device the slot is reused and the answer is ZN_E_CORRUPT ("cannot
 * vouch for it") rather than a guess.  A thread whose most recent check = 0 call was not on this device (it made none, or its last one
 * went to another device) gets the device's most recent decode: ask on the device you launched on, before you launch on another. */
int zn_decode_status(void* stream);
/* on != 0: from now on the calling thread's check = 0 decode calls (batches, windows, plan runs) on a device ADD their verdict to the status of its previous
 * check = 0 call there instead of starting a new one, so that one zn_decode_status speaks for a sequence of calls — a base decoded into a buffer and a delta
 * decoded in place over it.  The calls of a sequence run on one stream.  on == 0: back to one status per call.  Returns 0. */
int zn_decode_status_chain(int on);

/* Names of the kernels the last *_dev call launched, ';'-separated (for profiles). */
const char* zn_last_kernels(void);

/* Diagnostic: how many chunks of the last zn_decompress_dev call on the current device were
 * decoded by the fused single-pass kernel (the rest went through the generic two-kernel path).
 * Synchronises the device.  Returns a count >= 0 or a negative zn_status. */
long long zn_last_fused_chunks(void);

/* Diagnostic: how many Huffman planes of partial last chunks the parallel tail kernel decoded in the last
 * zn_decompress(_batch)_dev call (the rest of a partial chunk goes through the serial generic kernel). */
long long zn_last_tail_planes(void);

#ifdef __cplusplus
}
#endif
#endif /* ZIPNN_HIP_H */
