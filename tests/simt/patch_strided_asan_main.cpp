// Stand-alone driver (test infrastructure, CPU only): the strided apply of "znp1" patches (zn_patch_apply_strided_batch_dev) on the EMULATED kernels under
// AddressSanitizer / UBSan.  (1) The index map zn_patch_layout_offset against a 128-bit unravelling, for layouts with no memory behind them: sizes such as 65 537 and
// 2^31 - 1, strides up to 2^33, e up to 2^32 - 1.  (2) Applies through views whose memory is a heap block of exactly the span the view covers, and hostile patches in
// blocks of exactly their length: a read or write outside either is a report.  Build and run, from the repository root:
//   F=""; for f in zipnn_amd/csrc/*.hip; do F="$F -x c++ $f"; done
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=alignment -w -Itests/simt -DZN_SIMT_EMUL=1 $F -x c++ tests/simt/patch_strided_asan_main.cpp -o /tmp/patch_strided_asan -lpthread
//   ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 /tmp/patch_strided_asan          (the lanes are ucontext fibers: their stacks are not ASan fake stacks)
#include "../../include/zipnn_hip.h"
#include "../../zipnn_amd/csrc/zn_patch_format.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
static void* exact(size_t n) { void* p = nullptr; if (posix_memalign(&p, 16, n ? n : 1)) abort(); return p; }

struct Layout { int ndim; unsigned long long size[8]; long long stride[8]; };
static unsigned __int128 unravel(const Layout& L, uint64_t e) {
  unsigned __int128 at = 0;
  for (int d = L.ndim - 1; d >= 0; d--) { at += (unsigned __int128)(e % L.size[d]) * (unsigned __int128)L.stride[d]; e /= L.size[d]; }
  return at;
}

static int check_map() {
  const Layout layouts[] = {
      {2, {65537, 65535}, {1ll << 33, 3}},                       // m = 2^32 - 1
      {2, {2, 2147483647}, {1, 4}},                              // m = 2^32 - 2
      {1, {4294967295ull}, {1ll << 29}},
      {3, {65537, 255, 257}, {7, 1ll << 33, 1ll << 20}},
      {8, {2, 3, 2, 3, 2, 3, 2, 5}, {1ll << 33, 1ll << 30, 1ll << 27, 1ll << 24, 1ll << 21, 1ll << 18, 1ll << 15, 1}},
      {8, {7, 5, 3, 2, 11, 13, 17, 19}, {1, 7, 35, 105, 210, 2310, 30030, 510510}},
      {0, {}, {}},
  };
  std::mt19937_64 rng(11);
  long long checked = 0;
  for (const Layout& L : layouts) {
    uint32_t size[8] = {}; uint64_t stride[8] = {};
    uint64_t m = 1;
    for (int d = 0; d < L.ndim; d++) { size[d] = (uint32_t)L.size[d]; stride[d] = (uint64_t)L.stride[d]; m *= L.size[d]; }
    if (m >= (1ull << 32)) { printf("layout with 2^32 elements or more\n"); return 1; }
    std::vector<uint64_t> es = {0, m - 1, m / 2, m > 65536 ? 65535u : 0u, m > 65536 ? 65536u : 0u};
    for (int k = 0; k < 200000; k++) es.push_back(rng() % m);
    for (uint64_t e : es) {
      const unsigned __int128 want = unravel(L, e);
      const uint64_t got = zn_patch_layout_offset((uint32_t)L.ndim, size, stride, (uint32_t)e);
      if ((want >> 64) != 0 || (uint64_t)want != got) { printf("index map: ndim=%d e=%llu got %llu\n", L.ndim, (unsigned long long)e, (unsigned long long)got); return 1; }
      checked++;
    }
  }
  printf("index map: %lld elements of 7 layouts agree with the 128-bit unravelling\n", checked);
  return 0;
}

int main() {
  if (check_map()) return 1;
  std::mt19937 rng(7);
  int fails = 0, cases = 0, applies = 0;
  // rows x cols logical elements; the view's memory: `span` elements, logical (r, c) at r * rs + c * cs
  struct View { const char* name; size_t rows, cols; long long rs, cs; };
  const View views[] = {{"transposed", 300, 257, 1, 300}, {"narrow", 130, 517, 1031, 1}, {"two-blocks-transposed", 8197, 16, 1, 8197}, {"contiguous", 1, 70001, 70001, 1}};
  for (int E : {1, 2, 4}) {
    for (const View& v : views) {
      const size_t m = v.rows * v.cols, n = m * E;
      const size_t span = (v.rows - 1) * v.rs + (v.cols - 1) * v.cs + 1;
      uint8_t* base = (uint8_t*)exact(n); uint8_t* src = (uint8_t*)exact(n);
      for (size_t i = 0; i < n; i++) base[i] = (uint8_t)rng();
      memcpy(src, base, n);
      for (int k = 0; k < 3000; k++) { size_t e = (k == 0) ? 0 : (k == 1) ? m - 1 : (k == 2) ? 65536 : (k == 3) ? 65535 : rng() % m; src[e * E + (rng() % E)] ^= (uint8_t)(1 + rng() % 255); }
      zn_patch_size_item si{src, base, n, E}; size_t L = 0;
      if (zn_patch_size_batch_dev(&si, 1, &L, nullptr) != ZN_OK || L == 0) { printf("size failed\n"); return 1; }
      uint8_t* patch = (uint8_t*)exact(L);
      zn_patch_build_item bi{src, base, n, E, patch, L, 0};
      if (zn_patch_build_batch_dev(&bi, 1, nullptr) != ZN_OK || bi.patch_len != L) { printf("build failed\n"); return 1; }
      // the view: exactly the span it covers, gaps (the narrow's other columns) filled with a sentinel
      auto fill = [&](uint8_t* mem, const uint8_t* logical) {
        memset(mem, 0x5C, span * E);
        for (size_t r = 0; r < v.rows; r++) for (size_t c = 0; c < v.cols; c++) memcpy(mem + (r * v.rs + c * v.cs) * E, logical + (r * v.cols + c) * E, E);
      };
      uint8_t* mem = (uint8_t*)exact(span * E); uint8_t* want = (uint8_t*)exact(span * E); uint8_t* was = (uint8_t*)exact(span * E);
      fill(mem, base); fill(want, src); fill(was, base);
      zn_patch_apply_strided_item it{patch, L, n, E, mem, 2, {v.rows, v.cols}, {v.rs, v.cs}};
      if (zn_patch_apply_strided_batch_dev(&it, 1, nullptr, 1) != ZN_OK || memcmp(mem, want, span * E)) { printf("apply failed E=%d %s\n", E, v.name); return 1; }
      if (zn_patch_apply_strided_batch_dev(&it, 1, nullptr, 1) != ZN_OK || memcmp(mem, was, span * E)) { printf("second apply failed E=%d %s\n", E, v.name); return 1; }
      applies += 2;
      // refused before any launch
      zn_patch_apply_strided_item bad = it; bad.stride[1] = 0;
      zn_patch_apply_strided_item neg = it; neg.stride[0] = -neg.stride[0];
      zn_patch_apply_strided_item nine = it; nine.ndim = 9;
      zn_patch_apply_strided_item prod = it; prod.size[0]++;
      for (const zn_patch_apply_strided_item* r : {&bad, &neg, &nine, &prod})
        if (zn_patch_apply_strided_batch_dev(r, 1, nullptr, 1) != ZN_E_ARG || memcmp(mem, was, span * E)) { printf("a refusal failed E=%d %s\n", E, v.name); return 1; }
      // hostile: single-field damage of the header and tables, truncations, random bytes — each in a block of exactly the length handed over
      const size_t nb = (m + 65535) / 65536, a1 = (32 + 4 * (nb + 1) + 15) / 16 * 16;
      uint64_t T; memcpy(&T, patch + 16, 8);
      const size_t a2 = (a1 + 2 * T + 15) / 16 * 16;
      struct Edit { size_t at; std::vector<uint8_t> bytes; size_t len; };
      std::vector<Edit> edits;
      auto put = [&](size_t at, uint64_t val, int w, size_t len = 0) { Edit e; e.at = at; e.len = len ? len : L; for (int i = 0; i < w; i++) e.bytes.push_back((uint8_t)(val >> (8 * i))); edits.push_back(e); };
      put(0, 0, 0, L - 16); put(0, 0, 0, 32); put(0, 0, 0, 16); put(0, 0, 0, L - 1);
      put(4, E == 4 ? 2 : 4, 1); put(8, n + E, 8); put(8, n - E, 8); put(24, L + 16, 8); put(24, L - 16, 8); put(16, T + 1, 8); put(16, T - 1, 8); put(16, ~0ull, 8); put(16, 1ull << 40, 8);
      put(32, 1, 4); put(32 + 4 * nb, T + 1, 4); put(32 + 4 * nb, T - 1, 4); put(32 + 4 * nb, 0xFFFFFFFFu, 4);
      put(32 + 4, 0xFFFFFFF0u, 4); put(32 + 4, T + 5, 4);
      put(a1 + 2 * (T - 1), 65535, 2); put(a1 + 2 * 4, 0, 2); put(a1 + 2 * 3, 65535, 2);
      put(a2 + E * (T / 2), 0, E);
      for (int r = 0; r < 8; r++) { Edit e; e.at = r < 4 ? 0 : 32; e.len = L; for (size_t i = e.at; i < L; i++) e.bytes.push_back((uint8_t)rng()); edits.push_back(e); }
      for (const Edit& e : edits) {
        uint8_t* p = (uint8_t*)exact(e.len);
        std::vector<uint8_t> full(patch, patch + L);
        for (size_t i = 0; i < e.bytes.size() && e.at + i < L; i++) full[e.at + i] = e.bytes[i];
        memcpy(p, full.data(), e.len);
        const bool same = e.len == L && !memcmp(p, patch, L);
        fill(mem, base);
        zn_patch_apply_strided_item h = it; h.d_patch = p; h.patch_len = e.len;
        const int rc = zn_patch_apply_strided_batch_dev(&h, 1, nullptr, 1);
        cases++;
        if (!same && rc != ZN_E_CORRUPT && rc != ZN_E_ARG) { printf("hostile patch accepted: E=%d %s at=%zu len=%zu rc=%d\n", E, v.name, e.at, e.len, rc); fails++; }
        // the gaps of the view are not elements of it: they keep the sentinel whatever the patch held
        if (v.cs == 1 && v.rows > 1)
          for (size_t r = 0; r + 1 < v.rows; r++)
            for (size_t g = (r * v.rs + v.cols) * E; g < (r + 1) * v.rs * E; g++)
              if (mem[g] != 0x5C) { printf("a hostile patch wrote outside the view: E=%d %s at=%zu\n", E, v.name, e.at); return 1; }
        free(p);
      }
      free(mem); free(want); free(was); free(patch); free(src); free(base);
    }
  }
  zn_release_workspace();
  printf("%d applies through exact-size views; %d hostile applies, %d accepted wrongly\n", applies, cases, fails);
  return fails ? 1 : 0;
}
