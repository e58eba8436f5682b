// Stand-alone driver (test infrastructure, CPU only): the XOR-merge of "znp1" patches on the EMULATED kernels under AddressSanitizer / UBSan — well-formed merges against
// the patch built from the two tensors, and hostile inputs on either side, every buffer a heap block of exactly the length handed over, so that a read or write outside
// it is a report.  Build and run, from the repository root:
//   F=""; for f in zipnn_amd/csrc/*.hip; do F="$F -x c++ $f"; done
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=alignment -w -Itests/simt -DZN_SIMT_EMUL=1 $F -x c++ tests/simt/patch_merge_asan_main.cpp -o /tmp/patch_merge_asan -lpthread
//   ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 /tmp/patch_merge_asan    (the lanes are ucontext fibers: their stacks are not ASan fake stacks)
#include "../../include/zipnn_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
static void* exact(size_t n) { void* p = nullptr; if (posix_memalign(&p, 16, n ? n : 1)) abort(); return p; }

// the format's own rules (include/zipnn_hip.h), less the canonical padding: what a merge must accept, and nothing else
static bool well_formed(const uint8_t* p, size_t len, size_t n, int E) {
  if (len < 32) return false;
  uint32_t magic, e; uint64_t hn, T, L;
  memcpy(&magic, p, 4); memcpy(&e, p + 4, 4); memcpy(&hn, p + 8, 8); memcpy(&T, p + 16, 8); memcpy(&L, p + 24, 8);
  const uint64_t m = n / E, nb = (m + 65535) / 65536;
  if (magic != 0x31504E5Au || e != (uint32_t)E || hn != n || T > m || L != len) return false;
  const uint64_t a1 = (32 + 4 * (nb + 1) + 15) / 16 * 16, a2 = (a1 + 2 * T + 15) / 16 * 16;
  if (a2 + (uint64_t)E * T != L) return false;
  std::vector<uint32_t> first(nb + 1);
  memcpy(first.data(), p + 32, 4 * (nb + 1));
  if (first[0] != 0 || first[nb] != T) return false;
  for (uint64_t b = 0; b < nb; b++) {
    if (first[b] > first[b + 1] || first[b + 1] > T) return false;
    for (uint64_t i = first[b]; i < first[b + 1]; i++) {
      uint16_t o, prev = 0; memcpy(&o, p + a1 + 2 * i, 2);
      if (i > first[b]) memcpy(&prev, p + a1 + 2 * (i - 1), 2);
      if (b * 65536 + o >= m || (i > first[b] && prev >= o)) return false;
      uint32_t v = 0; memcpy(&v, p + a2 + E * i, E);
      if (v == 0) return false;
    }
  }
  return true;
}

static uint8_t* build(const uint8_t* src, const uint8_t* base, size_t n, int E, size_t* L) {
  zn_patch_size_item si{src, base, n, E};
  if (zn_patch_size_batch_dev(&si, 1, L, nullptr) != ZN_OK) { printf("size failed\n"); exit(1); }
  if (*L == 0) return nullptr;
  uint8_t* patch = (uint8_t*)exact(*L);
  zn_patch_build_item bi{src, base, n, E, patch, *L, 0};
  if (zn_patch_build_batch_dev(&bi, 1, nullptr) != ZN_OK || bi.patch_len != *L) { printf("build failed\n"); exit(1); }
  return patch;
}

int main() {
  std::mt19937 rng(11);
  int fails = 0, cases = 0, merges = 0;
  for (int E : {1, 2, 4}) {
    for (size_t m : {(size_t)1, (size_t)65535, (size_t)65536, (size_t)65537, (size_t)2 * 65536 + 3}) {
      const size_t n = m * E;
      uint8_t* base = (uint8_t*)exact(n); uint8_t* A = (uint8_t*)exact(n); uint8_t* B = (uint8_t*)exact(n);
      for (size_t i = 0; i < n; i++) base[i] = (uint8_t)rng();
      memcpy(A, base, n); memcpy(B, base, n);
      // A changes ~70 elements (the first, the last, both sides of a block edge among them); B takes half of them over — some with A's values, some with others — and changes more
      for (int k = 0; k < 70; k++) {
        const size_t e = (k == 0) ? 0 : (k == 1) ? m - 1 : (k == 2 && m > 65536) ? 65536 : (k == 3 && m > 65535) ? 65535 : rng() % m;
        A[e * E + (rng() % E)] ^= (uint8_t)(1 + rng() % 255);
        if (k % 2 == 0) { memcpy(B + e * E, A + e * E, E); if (k % 4 == 0 && m > 1) B[e * E] ^= 0x10; }
      }
      for (int k = 0; k < 40 && m > 1; k++) { const size_t e = rng() % m; B[e * E + (rng() % E)] ^= (uint8_t)(1 + rng() % 255); }
      if (!memcmp(A, base, n)) A[0] ^= 1;
      if (!memcmp(B, base, n)) B[n - 1] ^= 2;
      size_t La = 0, Lb = 0, Lw = 0;
      uint8_t* pa = build(A, base, n, E, &La); uint8_t* pb = build(B, base, n, E, &Lb); uint8_t* want = build(B, A, n, E, &Lw);
      if (!well_formed(pa, La, n, E) || !well_formed(pb, Lb, n, E)) { printf("the driver's own check refuses a built patch\n"); return 1; }
      // well-formed: (pa, pb), (pb, pa), (pa, pa) -> everything cancels; outputs of exactly the length the size call gave
      for (int form = 0; form < 3; form++) {
        const uint8_t* x = form == 1 ? pb : pa; const uint8_t* y = form == 0 ? pb : pa;
        const size_t lx = form == 1 ? Lb : La, ly = form == 0 ? Lb : La, lw = form == 2 ? 0 : Lw;
        zn_patch_merge_item it{x, lx, y, ly, n, E, nullptr, 0, 0}; size_t L = 1;
        if (zn_patch_merge_size_batch_dev(&it, 1, &L, nullptr) != ZN_OK || L != lw) { printf("merge size wrong E=%d m=%zu form=%d: %zu, want %zu\n", E, m, form, L, lw); return 1; }
        uint8_t* out = (uint8_t*)exact(L);
        it.d_out = out; it.out_cap = L;
        if (zn_patch_merge_batch_dev(&it, 1, nullptr) != ZN_OK || it.out_len != lw || (lw && memcmp(out, want, lw))) { printf("merge wrong E=%d m=%zu form=%d\n", E, m, form); return 1; }
        if (lw > 1) {                            // a capacity one byte short
          uint8_t* sh = (uint8_t*)exact(lw - 1);
          it.d_out = sh; it.out_cap = lw - 1;
          if (zn_patch_merge_batch_dev(&it, 1, nullptr) != ZN_E_CAP || it.out_len != lw) { printf("short capacity not refused\n"); return 1; }
          free(sh);
        }
        free(out); merges++;
      }
      // hostile: every single-field damage of the header and tables, truncations, random bytes — each in a block of exactly the length handed over, as the A side and as the B side
      const size_t L = La, nb = (m + 65535) / 65536, a1 = (32 + 4 * (nb + 1) + 15) / 16 * 16;
      uint64_t T; memcpy(&T, pa + 16, 8);
      const size_t a2 = (a1 + 2 * T + 15) / 16 * 16;
      struct Edit { size_t at; std::vector<uint8_t> bytes; size_t len; };
      std::vector<Edit> edits;
      auto put = [&](size_t at, uint64_t v, int w, size_t len = 0) { Edit e; e.at = at; e.len = len ? len : L; for (int i = 0; i < w; i++) e.bytes.push_back((uint8_t)(v >> (8 * i))); edits.push_back(e); };
      put(0, 0, 0, L > 48 ? L - 16 : 32); put(0, 0, 0, 32); put(0, 0, 0, 16); put(0, 0, 0, L - 1);
      put(0, 0x32504E5Au, 4); put(4, E == 4 ? 2 : 4, 1); put(8, n + E, 8); put(8, n - E, 8); put(24, L + 16, 8); put(24, L - 16, 8); put(16, T + 1, 8); put(16, T - 1, 8); put(16, ~0ull, 8); put(16, 1ull << 40, 8);
      put(32, 1, 4); put(32 + 4 * nb, T + 1, 4); put(32 + 4 * nb, T ? T - 1 : 7, 4); put(32 + 4 * nb, 0xFFFFFFFFu, 4);
      if (nb > 1) { put(32 + 4, 0xFFFFFFF0u, 4); put(32 + 4, T + 5, 4); }
      put(a1 + 2 * (T - 1), 65535, 2);                                           // an offset past the end (or, in a full block, a pair that no longer ascends)
      if (T > 5) { uint16_t o3; memcpy(&o3, pa + a1 + 2 * 3, 2); put(a1 + 2 * 4, 0, 2); put(a1 + 2 * 3, 65535, 2); put(a1 + 2 * 4, o3, 2); }      // descending pairs, a duplicate offset
      put(a2 + E * (T / 2), 0, E);                                                // a zero value
      for (int r = 0; r < 8; r++) { Edit e; e.at = r < 4 ? 0 : 32; e.len = L; for (size_t i = e.at; i < L; i++) e.bytes.push_back((uint8_t)rng()); edits.push_back(e); }
      for (const Edit& e : edits) {
        uint8_t* p = (uint8_t*)exact(e.len);
        std::vector<uint8_t> full(pa, pa + L);
        for (size_t i = 0; i < e.bytes.size() && e.at + i < L; i++) full[e.at + i] = e.bytes[i];
        memcpy(p, full.data(), e.len);
        const bool good = well_formed(p, e.len, n, E);
        for (int side = 0; side < 2; side++) {
          zn_patch_merge_item it{side ? pb : p, side ? Lb : e.len, side ? p : pb, side ? e.len : Lb, n, E, nullptr, 0, 0};
          size_t need = 0;
          const int rs = zn_patch_merge_size_batch_dev(&it, 1, &need, nullptr);
          const size_t cap = La + Lb + 64;      // (no merge of two patches of this tensor is longer)
          uint8_t* out = (uint8_t*)exact(cap);
          it.d_out = out; it.out_cap = cap;
          const int rm = zn_patch_merge_batch_dev(&it, 1, nullptr);
          cases += 2;
          const int want_rc = e.len < 32 ? ZN_E_ARG : good ? ZN_OK : ZN_E_CORRUPT;
          if (rs != want_rc || rm != want_rc) { printf("hostile input: E=%d m=%zu at=%zu len=%zu side=%d size rc=%d merge rc=%d (want %d)\n", E, m, e.at, e.len, side, rs, rm, want_rc); fails++; }
          free(out);
        }
        free(p);
      }
      free(pa); free(pb); free(want); free(A); free(B); free(base);
    }
  }
  zn_release_workspace();
  printf("%d well-formed merges, %d hostile merge calls, %d answered wrongly\n", merges, cases, fails);
  return fails ? 1 : 0;
}
