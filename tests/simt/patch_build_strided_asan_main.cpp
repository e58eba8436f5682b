// Stand-alone driver (test infrastructure, CPU only): "znp1" patches built from strided views (zn_patch_size_strided_batch_dev / zn_patch_build_strided_batch_dev,
// DESIGN §3.16) on the EMULATED kernels under AddressSanitizer / UBSan.  (1) The joint canonicalisation zn_patch_layout_canon, for pairs of layouts with no memory
// behind them: every element's offset through the canonical layout against a 128-bit unravelling of the original, on both sides.  (2) Builds from N-dimensional views — every layout of tests/patch_strided_util.py, and a pair of two
// different layouts whose `fast` dimension is a middle one — whose memory is a heap block of exactly the span the view covers, into a patch block of exactly the length the size call gave: a read or write outside any of them
// is a report; the bytes are zn_patch_build_batch_dev's for contiguous copies.  (3) An emit pass launched over a source that was altered after the count pass:
// the patch may be wrong, but nothing outside the altered block's own entries is written — the patch block is exact, and the other block's entries, first[] and
// the header are what the unaltered emit gives.  Build and run, from the repository root:
//   F=""; for f in zipnn_amd/csrc/*.hip; do F="$F -x c++ $f"; done
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=alignment -w -Itests/simt -DZN_SIMT_EMUL=1 $F -x c++ tests/simt/patch_build_strided_asan_main.cpp -o /tmp/patch_build_strided_asan -lpthread
//   ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 /tmp/patch_build_strided_asan          (the lanes are ucontext fibers: their stacks are not ASan fake stacks)
#include "../../include/zipnn_hip.h"
#include "../../zipnn_amd/csrc/zn_patch_format.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
static void* exact(size_t n) { void* p = nullptr; if (posix_memalign(&p, 16, n ? n : 1)) abort(); return p; }

struct Pair { int ndim; unsigned long long size[8]; long long sa[8], sb[8]; };
static unsigned __int128 unravel(int ndim, const unsigned long long* size, const long long* stride, uint64_t e) {
  unsigned __int128 at = 0;
  for (int d = ndim - 1; d >= 0; d--) { at += (unsigned __int128)(e % size[d]) * (unsigned __int128)stride[d]; e /= size[d]; }
  return at;
}

static int check_canon() {
  const Pair pairs[] = {
      {2, {65537, 65535}, {1ll << 33, 3}, {65535, 1}},                                  // one side contiguous, the other not: nothing merges
      {3, {300, 1, 257}, {257, 9, 1}, {257, 0, 1}},                                     // both contiguous behind a size-1 dimension: one dimension
      {4, {16, 16, 10, 32}, {16, 1, 8192, 256}, {5120, 32, 512, 1}},                    // transposed against tile-shuffled
      {4, {16, 16, 10, 32}, {5120, 320, 32, 1}, {5120, 32, 512, 1}},                    // the source merges whole, the base does not
      {3, {1000, 50, 80}, {0, 80, 1}, {4000, 80, 1}},                                   // expand() in front: the last two merge on both sides
      {3, {1000, 50, 80}, {0, 0, 1}, {0, 0, 1}},                                        // two expanded dimensions merge into one of stride 0
      {8, {2, 3, 2, 3, 2, 3, 2, 5}, {1ll << 33, 1ll << 30, 1ll << 27, 1ll << 24, 1ll << 21, 1ll << 18, 1ll << 15, 1}, {1080, 360, 180, 60, 30, 10, 5, 1}},
      {8, {7, 5, 3, 2, 11, 13, 17, 19}, {1, 7, 35, 105, 210, 2310, 30030, 510510}, {1, 7, 35, 105, 210, 2310, 30030, 510510}},
      {1, {4294967295ull}, {1ll << 29}, {1}},
      {0, {}, {}, {}},
  };
  const uint32_t dims_left[] = {2, 1, 4, 4, 2, 2, 8, 8, 1, 0};
  std::mt19937_64 rng(13);
  long long checked = 0;
  int k = 0;
  for (const Pair& P : pairs) {
    uint32_t size[8] = {}; uint64_t sa[8] = {}, sb[8] = {};
    uint64_t m = 1;
    for (int d = 0; d < P.ndim; d++) m *= P.size[d];
    const uint32_t nd = zn_patch_layout_canon(P.ndim, P.size, P.sa, P.sb, size, sa, sb);
    if (nd != dims_left[k]) { printf("canon: pair %d keeps %u dimensions, expected %u\n", k, nd, dims_left[k]); return 1; }
    uint64_t prod = 1;
    for (uint32_t d = 0; d < nd; d++) { prod *= size[d]; if (size[d] == 1u) { printf("canon: pair %d keeps a size of 1\n", k); return 1; } }
    if (prod != m) { printf("canon: pair %d changes the number of elements\n", k); return 1; }
    std::vector<uint64_t> es = {0, m - 1, m / 2, m > 65536 ? 65535u : 0u, m > 65536 ? 65536u : 0u};
    for (int j = 0; j < 100000; j++) es.push_back(rng() % m);
    for (uint64_t e : es) {
      const unsigned __int128 wa = unravel(P.ndim, P.size, P.sa, e), wb = unravel(P.ndim, P.size, P.sb, e);
      if ((uint64_t)wa != zn_patch_layout_offset(nd, size, sa, (uint32_t)e) || (uint64_t)wb != zn_patch_layout_offset(nd, size, sb, (uint32_t)e)) {
        printf("canon: pair %d e=%llu differs\n", k, (unsigned long long)e); return 1;
      }
      checked++;
    }
    k++;
  }
  // with one stride list (the strided apply's use) the second is not looked at
  {
    const unsigned long long size[3] = {4, 5, 6}; const long long st[3] = {30, 6, 1};
    uint32_t os[8] = {}; uint64_t oa[8] = {}, ob[8] = {};
    if (zn_patch_layout_canon(3, size, st, nullptr, os, oa, ob) != 1u || os[0] != 120u || oa[0] != 1u) { printf("canon: a contiguous layout does not collapse\n"); return 1; }
  }
  printf("canonicalisation: %lld elements of 10 layout pairs agree with the 128-bit unravelling on both sides\n", checked);
  return 0;
}

// rows x cols logical elements; a side's memory: `span` elements, logical (r, c) at r * rs + c * cs
struct View { const char* name; size_t rows, cols; long long rs, cs; };
static size_t span_of(const View& v) { return (v.rows - 1) * v.rs + (v.cols - 1) * v.cs + 1; }
static uint8_t* place(const View& v, const uint8_t* logical, int E) {
  uint8_t* mem = (uint8_t*)exact(span_of(v) * E);
  memset(mem, 0x5C, span_of(v) * E);
  for (size_t r = 0; r < v.rows; r++) for (size_t c = 0; c < v.cols; c++) memcpy(mem + (r * v.rs + c * v.cs) * E, logical + (r * v.cols + c) * E, E);
  return mem;
}

// N dimensions: the logical shape and one side's strides over it (in elements; logical element 0 at offset 0).  The side's memory is a block of exactly the
// span first to last element; element e lies where the 128-bit unravelling of check_canon puts it.
struct NView { const char* name; int ndim; unsigned long long size[8]; long long stride[8]; };
static size_t count_of(const NView& v) { size_t m = 1; for (int d = 0; d < v.ndim; d++) m *= v.size[d]; return m; }
static size_t span_of(const NView& v) {
  if (count_of(v) == 0) return 0;
  size_t s = 1;
  for (int d = 0; d < v.ndim; d++) s += (v.size[d] - 1) * (size_t)v.stride[d];
  return s;
}
static NView flat_of(const NView& v) {
  NView f = v; f.name = "flat";
  long long st = 1;
  for (int d = v.ndim - 1; d >= 0; d--) { f.stride[d] = st; st *= (long long)v.size[d]; }
  return f;
}
static uint8_t* place(const NView& v, const uint8_t* logical, int E) {
  const size_t span = span_of(v), m = count_of(v);
  uint8_t* mem = (uint8_t*)exact(span * E);
  memset(mem, 0x5C, span * E);
  for (size_t e = 0; e < m; e++) memcpy(mem + (size_t)unravel(v.ndim, v.size, v.stride, e) * E, logical + e * E, E);
  return mem;
}

// one build: the source through vs, the base through vb (one logical shape), every buffer exact; `want` / L: the contiguous build's patch
static int one_build(int E, const char* what, const NView& vs, const NView& vb, const uint8_t* src, const uint8_t* base, const uint8_t* want, size_t L, int& builds) {
  const size_t m = count_of(vs), n = m * E;
  uint8_t* ms = place(vs, src, E); uint8_t* mb = place(vb, base, E);
  zn_patch_build_strided_item it{};
  it.d_src = m ? ms : nullptr; it.d_base = m ? mb : nullptr; it.n = n; it.elem = E; it.ndim = vs.ndim;
  for (int d = 0; d < vs.ndim; d++) { it.size[d] = vs.size[d]; it.src_stride[d] = vs.stride[d]; it.base_stride[d] = vb.stride[d]; }
  size_t got = ~(size_t)0;
  if (zn_patch_size_strided_batch_dev(&it, 1, &got, nullptr) != ZN_OK || got != L) { printf("strided size failed E=%d %s\n", E, what); return 1; }
  uint8_t* patch = (uint8_t*)exact(L);
  memset(patch, 0x5C, L);
  it.d_patch = patch;
  if (L) {
    it.patch_cap = L - 1;
    if (zn_patch_build_strided_batch_dev(&it, 1, nullptr) != ZN_E_CAP || it.patch_len != L) { printf("a short capacity was not refused E=%d %s\n", E, what); return 1; }
    for (size_t i = 0; i < L; i++) if (patch[i] != 0x5C) { printf("a short capacity wrote E=%d %s\n", E, what); return 1; }
  }
  it.patch_cap = L;
  if (zn_patch_build_strided_batch_dev(&it, 1, nullptr) != ZN_OK || it.patch_len != L || (L && memcmp(patch, want, L))) { printf("strided build differs E=%d %s\n", E, what); return 1; }
  builds++;
  if (m > 1) {                                                  // refused before any launch
    int big = 0;
    for (int d = 0; d < vs.ndim; d++) if (vs.size[d] > 1) big = d;
    zn_patch_build_strided_item neg = it; neg.src_stride[big] = -1;
    zn_patch_build_strided_item nine = it; nine.ndim = 9;
    zn_patch_build_strided_item prod = it; prod.size[big]++;
    zn_patch_build_strided_item far = it; far.base_stride[big] = 1ll << 62;
    zn_patch_build_strided_item over = it; over.d_patch = ms; over.patch_cap = 64;
    for (const zn_patch_build_strided_item* r : {&neg, &nine, &prod, &far, &over}) {
      zn_patch_build_strided_item c = *r;
      if (zn_patch_build_strided_batch_dev(&c, 1, nullptr) != ZN_E_ARG) { printf("a refusal failed E=%d %s\n", E, what); return 1; }
    }
  }
  free(patch); free(ms); free(mb);
  return 0;
}

static int check_builds(int& builds) {
  std::mt19937 rng(7);
  // the layouts of tests/patch_strided_util.py (LAYOUTS), as shape and strides, and a second two-block transposed one
  const NView views[] = {
      {"transposed", 2, {300, 257}, {1, 300}},
      {"narrow", 2, {130, 517}, {1031, 1}},                                             // rows of 517 elements: the 16-byte path is defeated
      {"permute3", 3, {1021, 6, 11}, {1, 11231, 1021}},                                // view(6, 11, 1021).permute(2, 0, 1): `fast` is dimension 0 of 3
      {"tile-shuffle", 4, {16, 16, 10, 32}, {5120, 32, 512, 1}},
      {"eight-dims", 8, {5, 2, 3, 2, 3, 2, 3, 2}, {1, 5, 10, 30, 60, 180, 360, 1080}},  // does not collapse
      {"zero-dim", 0, {}, {}},
      {"size-1-dims", 4, {1, 300, 1, 257}, {77100, 1, 300, 300}},
      {"empty", 2, {0, 5}, {5, 1}},
      {"contiguous", 1, {70001}, {1}},
      {"two-blocks-transposed", 2, {8197, 16}, {1, 8197}},
  };
  // … and a pair of DIFFERENT layouts over one shape: a transposed source seen as (16, 16, 10, 32) — its stride-1 dimension, `fast`, is a middle one —
  // against a tile-shuffled base
  const NView mid{"transposed-as-4d", 4, {16, 16, 10, 32}, {16, 1, 8192, 256}};
  for (int E : {1, 2, 4}) {
    for (size_t vi = 0; vi <= sizeof(views) / sizeof(views[0]); vi++) {
      const bool pair = vi == sizeof(views) / sizeof(views[0]);
      const NView& v = pair ? mid : views[vi];
      const size_t m = count_of(v), n = m * E;
      uint8_t* base = (uint8_t*)exact(n); uint8_t* src = (uint8_t*)exact(n);
      for (size_t i = 0; i < n; i++) base[i] = (uint8_t)rng();
      memcpy(src, base, n);
      for (int k = 0; m && k < 3000; k++) {
        const size_t e = (k == 0) ? 0 : (k == 1) ? m - 1 : (k == 2 && m > 65536) ? 65536 : (k == 3 && m > 65535) ? 65535 : rng() % m;
        src[e * E + (rng() % E)] ^= (uint8_t)(1 + rng() % 255);
      }
      if (m) src[0] = (uint8_t)(base[0] ^ 1);                   // (element 0 always differs: no patch of the loop cancels to nothing)
      zn_patch_size_item si{m ? src : nullptr, m ? base : nullptr, n, E}; size_t L = 0;
      if (zn_patch_size_batch_dev(&si, 1, &L, nullptr) != ZN_OK || (L == 0) != (m == 0)) { printf("size failed E=%d %s\n", E, v.name); return 1; }
      uint8_t* want = (uint8_t*)exact(L);
      if (L) {
        zn_patch_build_item bi{src, base, n, E, want, L, 0};
        if (zn_patch_build_batch_dev(&bi, 1, nullptr) != ZN_OK || bi.patch_len != L) { printf("build failed\n"); return 1; }
      }
      const NView flat = flat_of(v);
      if (pair) {
        const NView tile = views[3];
        if (one_build(E, "transposed source against tile-shuffled base", v, tile, src, base, want, L, builds)) return 1;
        if (one_build(E, "tile-shuffled source against transposed base", tile, v, src, base, want, L, builds)) return 1;
      }
      if (one_build(E, v.name, v, flat, src, base, want, L, builds)) return 1;            // the source in the layout
      if (one_build(E, v.name, flat, v, src, base, want, L, builds)) return 1;            // the base
      if (one_build(E, v.name, v, v, src, base, want, L, builds)) return 1;               // both
      free(want); free(src); free(base);
    }
  }
  return 0;
}

// the passes by hand: count and scan over the source as it was, the source altered inside block 0, emit
static int check_altered() {
  std::mt19937 rng(17);
  const int E = 2;
  const View v{"transposed", 300, 257, 1, 300};
  const size_t m = v.rows * v.cols, n = m * E, nb = (m + 65535) / 65536;
  uint8_t* base = (uint8_t*)exact(n); uint8_t* src = (uint8_t*)exact(n);
  for (size_t i = 0; i < n; i++) base[i] = (uint8_t)rng();
  memcpy(src, base, n);
  for (int k = 0; k < 4000; k++) { const size_t e = rng() % m; src[e * E] ^= (uint8_t)(1 + rng() % 255); }
  uint8_t* ms = place(v, src, E);
  ZnPatchGSeg sg{ms, base, nullptr, m, {1, 300}, {257, 1}, {300, 257}, 0u, 0u, (uint32_t)E, 2u, 0u, 0u};
  ZnPatchBSeg scan{nullptr, nullptr, nullptr, m, 0u, 0u, (uint32_t)E, 0u};
  uint32_t* words = (uint32_t*)exact((nb + 1) * 4); uint64_t* total = (uint64_t*)exact(8);
  zn_launch_patch_count_strided(sg, nullptr, 1, (uint32_t)nb, words, nullptr);
  zn_launch_patch_scan(scan, nullptr, 1, words, total, nullptr);
  const uint64_t T = *total;
  const size_t L = (size_t)zn_patch_total(m, E, T), a1 = (size_t)zn_patch_a1(nb), a2 = (size_t)zn_patch_a2(nb, T);
  if (T == 0 || words[0] != 0 || words[nb] != T || words[1] == 0 || words[1] == T) { printf("altered: the count pass\n"); return 1; }
  uint8_t* before = (uint8_t*)exact(L); uint8_t* after = (uint8_t*)exact(L);
  sg.patch = before;
  zn_launch_patch_emit_strided(sg, nullptr, 1, (uint32_t)nb, words, nullptr);
  // block 0 of the source: 3 000 more elements differ, and every fifth that differed does not any more
  for (int k = 0; k < 3000; k++) { const size_t e = rng() % 65536; const size_t r = e / v.cols, c = e % v.cols; ms[(r * v.rs + c * v.cs) * E + 1] ^= (uint8_t)(1 + rng() % 255); }
  for (size_t e = 0; e < 65536; e += 5) { const size_t r = e / v.cols, c = e % v.cols; memcpy(ms + (r * v.rs + c * v.cs) * E, base + e * E, E); }
  memset(after, 0x5C, L);
  sg.patch = after;
  zn_launch_patch_emit_strided(sg, nullptr, 1, (uint32_t)nb, words, nullptr);
  const uint32_t f1 = words[1];
  if (memcmp(before, after, a1)) { printf("altered: the header or first[] differs\n"); return 1; }
  if (memcmp(before + a1 + 2 * f1, after + a1 + 2 * f1, a2 - (a1 + 2 * f1)) || memcmp(before + a2 + (size_t)E * f1, after + a2 + (size_t)E * f1, (size_t)E * (T - f1))) {
    printf("altered: block 1's entries were touched\n"); return 1;
  }
  printf("an emit over a source altered after the count pass: %llu entries, block 0's %u may be wrong, everything else is what it was\n", (unsigned long long)T, f1);
  free(before); free(after); free(words); free(total); free(ms); free(src); free(base);
  return 0;
}

int main() {
  if (check_canon()) return 1;
  int builds = 0;
  if (check_builds(builds)) return 1;
  if (check_altered()) return 1;
  zn_release_workspace();
  printf("%d strided builds from exact-size views into exact-size patches equal the contiguous build\n", builds);
  return 0;
}
