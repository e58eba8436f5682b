// Stand-alone driver (test infrastructure, CPU only): select and place of "znp1" patches on the EMULATED kernels under AddressSanitizer / UBSan — the shared geometries
// against the patches built from the sliced tensors, and hostile inputs, every buffer a heap block of exactly the length handed over, so that a read or write outside
// it is a report.  Build and run, from the repository root:
//   F=""; for f in zipnn_amd/csrc/*.hip; do F="$F -x c++ $f"; done
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=alignment -w -Itests/simt -DZN_SIMT_EMUL=1 $F -x c++ tests/simt/patch_select_asan_main.cpp -o /tmp/patch_select_asan -lpthread
//   ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 /tmp/patch_select_asan    (the lanes are ucontext fibers: their stacks are not ASan fake stacks)
#include "../../include/zipnn_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
static void* exact(size_t n) { void* p = nullptr; if (posix_memalign(&p, 16, n ? n : 1)) abort(); return p; }

struct Geo { size_t rows, cols, r0, r1, c0, c1; };

// the format's own rules (include/zipnn_hip.h), less the canonical padding, for the blocks [b_lo, b_hi] of a patch of m elements: what a call that visits exactly
// those blocks must accept, and nothing else
static bool well_formed(const uint8_t* p, size_t len, size_t m, int E, size_t b_lo, size_t b_hi) {
  if (len < 32) return false;
  uint32_t magic, e; uint64_t hn, T, L;
  memcpy(&magic, p, 4); memcpy(&e, p + 4, 4); memcpy(&hn, p + 8, 8); memcpy(&T, p + 16, 8); memcpy(&L, p + 24, 8);
  const uint64_t nb = (m + 65535) / 65536;
  if (magic != 0x31504E5Au || e != (uint32_t)E || hn != m * E || T > m || L != len) return false;
  const uint64_t a1 = (32 + 4 * (nb + 1) + 15) / 16 * 16, a2 = (a1 + 2 * T + 15) / 16 * 16;
  if (a2 + (uint64_t)E * T != L) return false;
  std::vector<uint32_t> first(nb + 1);
  memcpy(first.data(), p + 32, 4 * (nb + 1));
  for (uint64_t b = b_lo; b <= b_hi && b < nb; b++) {
    if (first[b] > first[b + 1] || first[b + 1] > T || (b == 0 && first[0] != 0) || (b + 1 == nb && first[nb] != T)) return false;
    const uint64_t left = m - b * 65536 >= 65536 ? 65536 : m - b * 65536;
    if (first[b + 1] - first[b] > left) return false;
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

static void cut(const Geo& g, int E, const uint8_t* whole, uint8_t* part) {
  const size_t w = g.c1 - g.c0;
  for (size_t r = g.r0; r < g.r1; r++) memcpy(part + (r - g.r0) * w * E, whole + (r * g.cols + g.c0) * E, w * E);
}

// one call into an output of exactly the length the size call gave -> the result (nullptr: no entry), its length in *L
static uint8_t* run(bool place, const uint8_t* p, size_t len, int E, const Geo& g, size_t* L) {
  zn_patch_select_item it{p, len, E, g.rows, g.cols, g.r0, g.r1, g.c0, g.c1, nullptr, 0, 0};
  const int rs = place ? zn_patch_place_size_batch_dev(&it, 1, L, nullptr) : zn_patch_select_size_batch_dev(&it, 1, L, nullptr);
  if (rs != ZN_OK) { printf("size call failed: %d\n", rs); exit(1); }
  uint8_t* out = (uint8_t*)exact(*L);
  it.d_out = out; it.out_cap = *L;
  const int rc = place ? zn_patch_place_batch_dev(&it, 1, nullptr) : zn_patch_select_batch_dev(&it, 1, nullptr);
  if (rc != ZN_OK || it.out_len != *L) { printf("call failed: %d\n", rc); exit(1); }
  if (*L > 1) {                                  // a capacity one byte short
    uint8_t* sh = (uint8_t*)exact(*L - 1);
    it.d_out = sh; it.out_cap = *L - 1;
    const int r2 = place ? zn_patch_place_batch_dev(&it, 1, nullptr) : zn_patch_select_batch_dev(&it, 1, nullptr);
    if (r2 != ZN_E_CAP || it.out_len != *L) { printf("short capacity not refused\n"); exit(1); }
    free(sh);
  }
  if (*L == 0) { free(out); return nullptr; }
  return out;
}

int main() {
  std::mt19937 rng(13);
  const Geo geos[] = {{1, 1, 0, 1, 0, 1}, {65537, 1, 1, 65537, 0, 1}, {3, 65536, 0, 3, 65535, 65536}, {2, 65537, 0, 2, 1, 65537}, {700, 300, 0, 700, 7, 45},
                      {700, 300, 0, 700, 10, 250}, {700, 300, 1, 699, 0, 300}, {700, 300, 3, 650, 10, 250}, {700, 300, 0, 700, 0, 300}};
  int fails = 0, cases = 0, good_calls = 0;
  for (int E : {1, 2, 4}) {
    for (const Geo& g : geos) {
      const size_t m = g.rows * g.cols, n = m * E, h = g.r1 - g.r0, w = g.c1 - g.c0, mr = h * w, nr = mr * E;
      uint8_t* base = (uint8_t*)exact(n); uint8_t* T = (uint8_t*)exact(n);
      for (size_t i = 0; i < n; i++) base[i] = (uint8_t)rng();
      memcpy(T, base, n);
      // 2 % of the elements, the tensor's and the rectangle's corners and both sides of every block edge among them
      std::vector<size_t> hit = {0, m - 1, g.r0 * g.cols + g.c0, (g.r1 - 1) * g.cols + g.c1 - 1};
      for (size_t b = 65536; b < m; b += 65536) { hit.push_back(b - 1); hit.push_back(b); }
      for (size_t k = 0; k < m / 50 + 1; k++) hit.push_back(rng() % m);
      for (size_t e : hit) T[e * E + (rng() % E)] ^= (uint8_t)(1 + rng() % 255);
      if (!memcmp(T, base, n)) T[0] ^= 1;
      uint8_t* sb = (uint8_t*)exact(nr); uint8_t* st = (uint8_t*)exact(nr); uint8_t* back = (uint8_t*)exact(n);
      cut(g, E, base, sb); cut(g, E, T, st);
      memcpy(back, base, n);
      for (size_t r = g.r0; r < g.r1; r++) memcpy(back + (r * g.cols + g.c0) * E, T + (r * g.cols + g.c0) * E, w * E);
      size_t Lw = 0, Ls = 0, Lp = 0, L = 0;
      uint8_t* whole = build(T, base, n, E, &Lw); uint8_t* want = build(st, sb, nr, E, &Ls); uint8_t* placed = build(back, base, n, E, &Lp);
      // well-formed: select == the patch of the sliced tensors; place == the patch of the embedded rectangle; select(place) == the input
      uint8_t* got = run(false, whole, Lw, E, g, &L);
      if (L != Ls || (Ls && memcmp(got, want, Ls))) { printf("select wrong E=%d %zux%zu\n", E, g.rows, g.cols); return 1; }
      good_calls++;
      if (want) {
        uint8_t* gp = run(true, want, Ls, E, g, &L);
        if (L != Lp || memcmp(gp, placed, Lp)) { printf("place wrong E=%d %zux%zu\n", E, g.rows, g.cols); return 1; }
        uint8_t* again = run(false, gp, Lp, E, g, &L);
        if (L != Ls || memcmp(again, want, Ls)) { printf("select(place) wrong E=%d %zux%zu\n", E, g.rows, g.cols); return 1; }
        free(gp); free(again); good_calls += 2;
      }
      free(got);
      // hostile: every single-field damage of the header and tables, truncations, random bytes — each in a block of exactly the length handed over; as the input of
      // a select (the whole tensor's patch) and of a place (the rectangle's patch).  The program's own restatement of the rules, over the blocks the call visits,
      // decides what it must answer.
      for (int pl = 0; pl < 2; pl++) {
        const uint8_t* src = pl ? want : whole; const size_t LL = pl ? Ls : Lw, mm = pl ? mr : m;
        if (!src) continue;
        const size_t nb = (mm + 65535) / 65536, a1 = (32 + 4 * (nb + 1) + 15) / 16 * 16;
        uint64_t TT; memcpy(&TT, src + 16, 8);
        const size_t a2 = (a1 + 2 * TT + 15) / 16 * 16;
        // the input blocks the call visits: place — all; select — from the block of the rectangle's first element to that of its last, when the rectangle has one
        // output block (more: the gaps between output blocks may be skipped, and the answer for a damage there is open)
        size_t b_lo = 0, b_hi = nb - 1; bool open = false;
        if (!pl) { b_lo = (g.r0 * g.cols + g.c0) / 65536; b_hi = ((g.r1 - 1) * g.cols + g.c1 - 1) / 65536; open = mr > 65536 && w != g.cols; }
        struct Edit { size_t at; std::vector<uint8_t> bytes; size_t len; };
        std::vector<Edit> edits;
        auto put = [&](size_t at, uint64_t v, int wd, size_t len = 0) { Edit e; e.at = at; e.len = len ? len : LL; for (int i = 0; i < wd; i++) e.bytes.push_back((uint8_t)(v >> (8 * i))); edits.push_back(e); };
        put(0, 0, 0, LL > 48 ? LL - 16 : 32); put(0, 0, 0, 32); put(0, 0, 0, 16); put(0, 0, 0, LL - 1);
        put(0, 0x32504E5Au, 4); put(4, E == 4 ? 2 : 4, 1); put(8, mm * E + E, 8); put(8, mm * E - E, 8); put(24, LL + 16, 8); put(24, LL - 16, 8); put(16, TT + 1, 8); put(16, TT - 1, 8); put(16, ~0ull, 8); put(16, 1ull << 40, 8);
        put(32, 1, 4); put(32 + 4 * nb, TT + 1, 4); put(32 + 4 * nb, TT ? TT - 1 : 7, 4); put(32 + 4 * nb, 0xFFFFFFFFu, 4);
        if (nb > 1) { put(32 + 4, 0xFFFFFFF0u, 4); put(32 + 4, TT + 5, 4); }
        put(a1 + 2 * (TT - 1), 65535, 2);
        if (TT > 5) { uint16_t o3; memcpy(&o3, src + a1 + 2 * 3, 2); put(a1 + 2 * 4, 0, 2); put(a1 + 2 * 3, 65535, 2); put(a1 + 2 * 4, o3, 2); }
        put(a2 + E * (TT / 2), 0, E);
        for (int r = 0; r < 6; r++) { Edit e; e.at = r < 3 ? 0 : 32; e.len = LL; for (size_t i = e.at; i < LL; i++) e.bytes.push_back((uint8_t)rng()); edits.push_back(e); }
        for (const Edit& e : edits) {
          uint8_t* p = (uint8_t*)exact(e.len);
          std::vector<uint8_t> full(src, src + LL);
          for (size_t i = 0; i < e.bytes.size() && e.at + i < LL; i++) full[e.at + i] = e.bytes[i];
          memcpy(p, full.data(), e.len);
          const bool good = well_formed(p, e.len, mm, E, b_lo, b_hi), good_all = well_formed(p, e.len, mm, E, 0, nb - 1);
          zn_patch_select_item it{p, e.len, E, g.rows, g.cols, g.r0, g.r1, g.c0, g.c1, nullptr, 0, 0};
          size_t need = 0;
          const int rs = pl ? zn_patch_place_size_batch_dev(&it, 1, &need, nullptr) : zn_patch_select_size_batch_dev(&it, 1, &need, nullptr);
          const size_t cap = 2 * LL + 4 * ((m + 65535) / 65536) + 256;      // (a result has no more entries than its input)
          uint8_t* out = (uint8_t*)exact(cap);
          it.d_out = out; it.out_cap = cap;
          const int rm = pl ? zn_patch_place_batch_dev(&it, 1, nullptr) : zn_patch_select_batch_dev(&it, 1, nullptr);
          cases += 2;
          bool ok;
          if (e.len < 32) ok = rs == ZN_E_ARG && rm == ZN_E_ARG;
          else if (good_all) ok = rs == ZN_OK && rm == ZN_OK;
          else if (!good && !open) ok = rs == ZN_E_CORRUPT && rm == ZN_E_CORRUPT;
          else ok = (rs == ZN_OK || rs == ZN_E_CORRUPT) && rm == rs;          // damage only in blocks the select may skip
          if (!ok) { printf("hostile input: E=%d %zux%zu place=%d at=%zu len=%zu size rc=%d call rc=%d (visited-good %d, all-good %d)\n", E, g.rows, g.cols, pl, e.at, e.len, rs, rm, (int)good, (int)good_all); fails++; }
          free(out); free(p);
        }
      }
      free(whole); free(want); free(placed); free(base); free(T); free(sb); free(st); free(back);
    }
  }
  zn_release_workspace();
  printf("%d well-formed calls, %d hostile calls, %d answered wrongly\n", good_calls, cases, fails);
  return fails ? 1 : 0;
}
