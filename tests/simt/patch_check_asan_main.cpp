// Stand-alone driver (test infrastructure, CPU only): zn_patch_check_batch_dev on the EMULATED kernels under AddressSanitizer / UBSan — well-formed patches, the
// hostile corpus of patch_asan_main.cpp and a few thousand random damages, every patch a heap block of exactly the length handed over, so that a read outside
// [d_patch, d_patch + patch_len) is a report.  A damaged patch must cost a verdict (or pass: a damage may produce another well-formed patch — then apply must
// accept it too).  Build and run, from the repository root:
//   F=""; for f in zipnn_amd/csrc/*.hip; do F="$F -x c++ $f"; done
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=alignment -w -Itests/simt -DZN_SIMT_EMUL=1 $F -x c++ tests/simt/patch_check_asan_main.cpp -o /tmp/patch_check_asan -lpthread
//   ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 /tmp/patch_check_asan    (the lanes are ucontext fibers: their stacks are not ASan fake stacks)
#include "../../include/zipnn_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
static void* exact(size_t n) { void* p = nullptr; if (posix_memalign(&p, 16, n ? n : 1)) abort(); return p; }
int main() {
  std::mt19937 rng(11);
  int cases = 0, refused = 0, fails = 0;
  for (int E : {1, 2, 4}) {
    for (size_t m : {(size_t)1, (size_t)65535, (size_t)65536 + 40, (size_t)2 * 65536 + 3}) {
      const size_t n = m * E;
      uint8_t* base = (uint8_t*)exact(n); uint8_t* src = (uint8_t*)exact(n);
      for (size_t i = 0; i < n; i++) base[i] = (uint8_t)rng();
      memcpy(src, base, n);
      for (int k = 0; k < 75; k++) { size_t e = (k == 0) ? 0 : (k == 1) ? m - 1 : (k == 2 && m > 65536) ? 65536 : (k == 3 && m > 65535) ? 65535 : rng() % m; src[e * E + (rng() % E)] ^= (uint8_t)(1 + rng() % 255); }
      zn_patch_size_item si{src, base, n, E}; size_t L = 0;
      if (zn_patch_size_batch_dev(&si, 1, &L, nullptr) != ZN_OK || L == 0) { printf("size failed E=%d m=%zu\n", E, m); return 1; }
      uint8_t* patch = (uint8_t*)exact(L);
      zn_patch_build_item bi{src, base, n, E, patch, L, 0};
      if (zn_patch_build_batch_dev(&bi, 1, nullptr) != ZN_OK || bi.patch_len != L) { printf("build failed\n"); return 1; }
      uint64_t T; memcpy(&T, patch + 16, 8);
      unsigned int v = 99; unsigned long long t = 0;
      zn_patch_check_item good{patch, L, n, E};
      if (zn_patch_check_batch_dev(&good, 1, &v, &t, nullptr) != ZN_OK || v != 0 || t != T) { printf("a built patch was refused: E=%d m=%zu verdict=%u T=%llu\n", E, m, v, t); return 1; }
      const size_t nb = (m + 65535) / 65536, a1 = (32 + 4 * (nb + 1) + 15) / 16 * 16, a2 = (a1 + 2 * T + 15) / 16 * 16;
      struct Edit { size_t at; std::vector<uint8_t> bytes; size_t len; };
      std::vector<Edit> edits;
      auto put = [&](size_t at, uint64_t val, int w, size_t len = 0) { Edit e; e.at = at; e.len = len ? len : L; for (int i = 0; i < w; i++) e.bytes.push_back((uint8_t)(val >> (8 * i))); edits.push_back(e); };
      // the corpus of patch_asan_main.cpp …
      put(0, 0, 0, L > 48 ? L - 16 : 32); put(0, 0, 0, 32); put(0, 0, 0, L - 1);
      put(4, E == 4 ? 2 : 4, 1); put(8, n + E, 8); put(8, n - E, 8); put(24, L + 16, 8); put(24, L - 16, 8); put(16, T + 1, 8); put(16, T - 1, 8); put(16, ~0ull, 8); put(16, 1ull << 40, 8);
      put(32, 1, 4); put(32 + 4 * nb, T + 1, 4); put(32 + 4 * nb, T ? T - 1 : 7, 4); put(32 + 4 * nb, 0xFFFFFFFFu, 4);
      if (nb > 1) { put(32 + 4, 0xFFFFFFF0u, 4); put(32 + 4, T + 5, 4); }
      put(a1 + 2 * (T - 1), 65535, 2); if (T > 5) { put(a1 + 2 * 4, 0, 2); put(a1 + 2 * 3, 65535, 2); }
      put(a2 + E * (T / 2), 0, E);
      // … the canonical form …
      put(5, 1, 1); put(7, 0x80, 1);
      if (a1 > 32 + 4 * (nb + 1)) { put(32 + 4 * (nb + 1), 1, 1); put(a1 - 1, 1, 1); }
      if (a2 > a1 + 2 * T) { put(a1 + 2 * T, 1, 1); put(a2 - 1, 1, 1); }
      for (int r = 0; r < 8; r++) { Edit e; e.at = r < 4 ? 0 : 32; e.len = L; for (size_t i = e.at; i < L; i++) e.bytes.push_back((uint8_t)rng()); edits.push_back(e); }
      // … and random damages: one to four bytes anywhere, a random run, a random cut
      for (int r = 0; r < 300; r++) {
        Edit e; e.at = rng() % L; e.len = (r % 10 == 9 && L > 33) ? 32 + rng() % (L - 32) : L;
        const size_t run = (r % 7 == 6) ? 1 + rng() % 64 : 1 + rng() % 4;
        for (size_t i = 0; i < run; i++) e.bytes.push_back((uint8_t)rng());
        edits.push_back(e);
      }
      for (const Edit& e : edits) {
        uint8_t* p = (uint8_t*)exact(e.len);
        std::vector<uint8_t> full(patch, patch + L);
        for (size_t i = 0; i < e.bytes.size() && e.at + i < L; i++) full[e.at + i] = e.bytes[i];
        memcpy(p, full.data(), e.len);
        const bool same = e.len == L && !memcmp(p, patch, L);
        zn_patch_check_item it{p, e.len, n, E};
        v = 99; t = 99;
        const int rc = zn_patch_check_batch_dev(&it, 1, &v, &t, nullptr);
        cases++;
        if (rc != ZN_OK || v > 31u || (v != 0 && t != 0)) { printf("check failed: E=%d m=%zu at=%zu len=%zu rc=%d verdict=%u\n", E, m, e.at, e.len, rc, v); fails++; }
        else if (v) refused++;
        else if (!same) {
          // accepted although changed: it must be another well-formed patch (a value or an offset that stays legal) — apply must take it as well
          uint8_t* d = (uint8_t*)exact(n); memcpy(d, base, n);
          zn_patch_apply_item ai{p, e.len, n, E, 0, n, d, nullptr};
          if (zn_patch_apply_batch_dev(&ai, 1, nullptr, 1) != ZN_OK) { printf("accepted by the check, refused by apply: E=%d m=%zu at=%zu len=%zu\n", E, m, e.at, e.len); fails++; }
          free(d);
        }
        free(p);
      }
      // a batch: good, bad, good — only the bad item's word is set
      uint8_t* q = (uint8_t*)exact(L); memcpy(q, patch, L); q[a2] = 0; if (E > 1) memset(q + a2, 0, E);
      zn_patch_check_item three[3] = {{patch, L, n, E}, {q, L, n, E}, {patch, L, n, E}};
      unsigned int vs[3] = {9, 9, 9};
      if (zn_patch_check_batch_dev(three, 3, vs, nullptr, nullptr) != ZN_OK || vs[0] || vs[1] != ZN_PATCH_BAD_VALUE || vs[2]) { printf("batch verdicts wrong: %u %u %u\n", vs[0], vs[1], vs[2]); fails++; }
      free(q); free(patch); free(src); free(base);
    }
  }
  zn_release_workspace();
  printf("%d damaged patches checked: %d refused, %d failures\n", cases, refused, fails);
  return fails ? 1 : 0;
}
