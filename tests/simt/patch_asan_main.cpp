// Stand-alone driver (test infrastructure, CPU only): "znp1" patches on the EMULATED kernels under AddressSanitizer / UBSan — well-formed builds, applies and windows, and
// hostile patches, every buffer a heap block of exactly the length handed over, so that a read or write outside it is a report.  Build and run, from the repository root:
//   F=""; for f in zipnn_amd/csrc/*.hip; do F="$F -x c++ $f"; done
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=alignment -w -Itests/simt -DZN_SIMT_EMUL=1 $F -x c++ tests/simt/patch_asan_main.cpp -o /tmp/patch_asan -lpthread
//   ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 /tmp/patch_asan          (the lanes are ucontext fibers: their stacks are not ASan fake stacks)
#include "../../include/zipnn_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
static void* exact(size_t n) { void* p = nullptr; if (posix_memalign(&p, 16, n ? n : 1)) abort(); return p; }
int main() {
  std::mt19937 rng(7);
  int fails = 0, cases = 0;
  for (int E : {1, 2, 4}) {
    for (size_t m : {(size_t)1, (size_t)65535, (size_t)65536 + 40, (size_t)2 * 65536 + 3}) {
      const size_t n = m * E;
      uint8_t* base = (uint8_t*)exact(n); uint8_t* src = (uint8_t*)exact(n);
      for (size_t i = 0; i < n; i++) base[i] = (uint8_t)rng();
      memcpy(src, base, n);
      for (int k = 0; k < 70 && m > 0; k++) { size_t e = (k == 0) ? 0 : (k == 1) ? m - 1 : (k == 2 && m > 65536) ? 65536 : (k == 3 && m > 65535) ? 65535 : rng() % m; src[e * E + (rng() % E)] ^= (uint8_t)(1 + rng() % 255); }
      zn_patch_size_item si{src, base, n, E}; size_t L = 0;
      if (zn_patch_size_batch_dev(&si, 1, &L, nullptr) != ZN_OK || L == 0) { printf("size failed E=%d m=%zu\n", E, m); return 1; }
      uint8_t* patch = (uint8_t*)exact(L);
      zn_patch_build_item bi{src, base, n, E, patch, L, 0};
      if (zn_patch_build_batch_dev(&bi, 1, nullptr) != ZN_OK || bi.patch_len != L) { printf("build failed\n"); return 1; }
      uint8_t* dst = (uint8_t*)exact(n); memcpy(dst, base, n);
      zn_patch_apply_item ai{patch, L, n, E, 0, n, dst, nullptr};
      if (zn_patch_apply_batch_dev(&ai, 1, nullptr, 1) != ZN_OK || memcmp(dst, src, n)) { printf("apply failed E=%d m=%zu\n", E, m); return 1; }
      // windows into exact-size destinations, over the base
      for (int w = 0; w < 12; w++) {
        size_t a = rng() % (m + 1), b = rng() % (m + 1); if (a > b) std::swap(a, b);
        uint8_t* wd = (uint8_t*)exact((b - a) * E);
        zn_patch_apply_item wi{patch, L, n, E, a * E, b * E, wd, base};
        if (zn_patch_apply_batch_dev(&wi, 1, nullptr, 1) != ZN_OK || memcmp(wd, src + a * E, (b - a) * E)) { printf("window failed\n"); return 1; }
        free(wd);
      }
      // hostile: every single-field damage of the header and tables, truncations, random bytes — each in a block of exactly the length handed over
      const size_t nb = (m + 65535) / 65536, a1 = (32 + 4 * (nb + 1) + 15) / 16 * 16;
      uint64_t T; memcpy(&T, patch + 16, 8);
      const size_t a2 = (a1 + 2 * T + 15) / 16 * 16;
      struct Edit { size_t at; std::vector<uint8_t> bytes; size_t len; };
      std::vector<Edit> edits;
      auto put = [&](size_t at, uint64_t v, int w, size_t len = 0) { Edit e; e.at = at; e.len = len ? len : L; for (int i = 0; i < w; i++) e.bytes.push_back((uint8_t)(v >> (8 * i))); edits.push_back(e); };
      put(0, 0, 0, L > 48 ? L - 16 : 32); put(0, 0, 0, 32); put(0, 0, 0, 16); put(0, 0, 0, L - 1);
      put(4, E == 4 ? 2 : 4, 1); put(8, n + E, 8); put(8, n - E, 8); put(24, L + 16, 8); put(24, L - 16, 8); put(16, T + 1, 8); put(16, T - 1, 8); put(16, ~0ull, 8); put(16, 1ull << 40, 8);
      put(32, 1, 4); put(32 + 4 * nb, T + 1, 4); put(32 + 4 * nb, T ? T - 1 : 7, 4); put(32 + 4 * nb, 0xFFFFFFFFu, 4);
      if (nb > 1) { put(32 + 4, 0xFFFFFFF0u, 4); put(32 + 4, T + 5, 4); }
      put(a1 + 2 * (T - 1), 65535, 2); if (T > 5) { put(a1 + 2 * 4, 0, 2); put(a1 + 2 * 3, 65535, 2); }
      put(a2 + E * (T / 2), 0, E);
      for (int r = 0; r < 8; r++) { Edit e; e.at = r < 4 ? 0 : 32; e.len = L; for (size_t i = e.at; i < L; i++) e.bytes.push_back((uint8_t)rng()); edits.push_back(e); }
      for (const Edit& e : edits) {
        uint8_t* p = (uint8_t*)exact(e.len);
        std::vector<uint8_t> full(patch, patch + L);
        for (size_t i = 0; i < e.bytes.size() && e.at + i < L; i++) full[e.at + i] = e.bytes[i];
        memcpy(p, full.data(), e.len);
        const bool same = e.len == L && !memcmp(p, patch, L);
        for (int form = 0; form < 3; form++) {
          size_t lo = form == 2 ? (m / 3) * E : 0, hi = form == 2 ? (m - m / 4) * E : n;
          uint8_t* d = (uint8_t*)exact(hi - lo); memcpy(d, base + lo, hi - lo);
          zn_patch_apply_item hi_{p, e.len, n, E, lo, hi, d, form == 1 ? base : nullptr};
          const int rc = zn_patch_apply_batch_dev(&hi_, 1, nullptr, 1);
          cases++;
          if (!same && rc != ZN_E_CORRUPT && rc != ZN_E_ARG) {
            // (a window may not see the damaged block or entry: then the bytes must still be right)
            if (rc != ZN_OK || form != 2 || memcmp(d, src + lo, hi - lo)) { printf("hostile patch accepted: E=%d m=%zu at=%zu len=%zu form=%d rc=%d\n", E, m, e.at, e.len, form, rc); fails++; }
          }
          free(d);
        }
        free(p);
      }
      free(dst); free(patch); free(src); free(base);
    }
  }
  zn_release_workspace();
  printf("%d hostile applies, %d accepted wrongly\n", cases, fails);
  return fails ? 1 : 0;
}
