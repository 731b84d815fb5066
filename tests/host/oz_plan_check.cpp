// oz_plan_check.cpp -- host-only check of the int8 products' constants and plans
// (gpemu_ozaki.hpp: oz_consts, oz_list, OzShape, trtri_level_pairs, oz_tri_pair_plan).  No HIP runtime
// call: it runs without a GPU.  Built and run by tests/test_ozaki_host.py:
//   hipcc --offload-arch=gfx950 -std=c++17 -I gp_emu_uqsa_amd/csrc tests/host/oz_plan_check.cpp
// Prints one line per failed check and "beta12_4096=<beta>"; exit status 0 and a last line
// "oz_plan_check OK" when every check holds.
#include <cstdint>
#include <cstdio>
#include <map>
#include <numeric>
#include <set>

#include "gpemu_kernels.hpp"
#include "gpemu_ozaki.hpp"

using namespace gpe;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++g_fail <= 50) {                                \
        std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                          \
        std::printf("\n");                                 \
      }                                                    \
    }                                                      \
  } while (0)

typedef unsigned __int128 u128;

static void check_consts() {
  std::vector<int> sizes;
  for (int np2 = 2048; np2 <= 131072; np2 *= 2) sizes.push_back(np2);
  for (int np2 : {256, 512, 1280, 1792, 8448, 65536 + 256, OZ_MAX_K / OZ_T * OZ_T}) sizes.push_back(np2);
  for (int nmod = 8; nmod <= OZ_MAXMOD; ++nmod)
    for (int np2 : sizes) {
      const OzConst k = oz_consts(nmod, np2);
      CHECK(k.nmod == nmod, "nmod %d", nmod);
      u128 M = 1;
      for (int l = 0; l < nmod; ++l) M *= (u128)k.m[l];   // < 2^128: 16 moduli <= 256 with one < 2^7.6
      for (int l = 0; l < nmod; ++l) {
        const int m = k.m[l];
        CHECK(m >= 3 && m <= 256, "m %d", m);
        CHECK(m % 2 == 0 || m <= 253, "odd modulus %d > 253", m);
        for (int j = 0; j < l; ++j) CHECK(std::gcd(m, k.m[j]) == 1, "moduli %d, %d share a factor", m, k.m[j]);
        CHECK(k.c16[l] == 65536 % m, "c16 of %d", m);
        CHECK(k.inv[l] == 1.0f / (float)m, "inv of %d", m);
        // k_oz_gemm's epilogue: t = (acc >> 16) c16 + (acc & 0xffff), |acc| <= K 2^14
        CHECK((long long)(OZ_MAX_K / 4 + 1) * k.c16[l] + 65535 < (1LL << 23), "|t| bound for m = %d", m);
        // rhi on the 2^-41 grid, 0 <= rlo < 2^-41, rhi + rlo = y / m with y = (M / m)^-1 mod m
        const double g = std::ldexp(k.rhi[l], 41);
        CHECK(g == std::floor(g) && g >= 0.0 && g < std::ldexp(1.0, 41), "rhi of %d off the grid", m);
        CHECK(k.rlo[l] >= 0.0 && k.rlo[l] < std::ldexp(1.0, -41), "rlo of %d = %g", m, k.rlo[l]);
        const long long y = std::llround((k.rhi[l] + k.rlo[l]) * m);
        CHECK(y >= 1 && y < m, "y of %d = %lld", m, y);
        CHECK(std::fabs((k.rhi[l] + k.rlo[l]) * m - (double)y) < 1e-9, "rhi + rlo of %d is not y / m", m);
        const long long Mm = (long long)((M / (u128)m) % (u128)m);
        CHECK((Mm * y) % m == 1, "(M / m) y != 1 mod %d", m);
      }
      // the product is fixed by its residues: |C'| <= np2 2^(2 beta) < M / 2, in exact
      // integers (M < 2^128, np2 2^(2 beta) <= 2^17 2^106), and beta is the most that allows
      CHECK(k.beta >= 1 && k.beta <= 53, "beta %d", k.beta);
      const u128 bound = ((u128)np2 << (2 * k.beta)) * 2;
      CHECK(bound < M, "np2 %d, %d moduli: np2 2^(2 beta) >= M / 2 at beta = %d", np2, nmod, k.beta);
      if (k.beta < 53)
        CHECK((((u128)np2 << (2 * k.beta + 2)) * 2) >= M, "np2 %d, %d moduli: beta = %d is not the largest", np2, nmod,
              k.beta);
      CHECK(std::fabs(k.Md - (double)M) <= 2e-15 * (double)M, "Md of %d moduli", nmod);   // (<= 16 roundings)
      if (nmod == OZ_MAXMOD && np2 <= 131072) CHECK(k.beta == 53, "16 moduli at np2 %d: beta = %d", np2, k.beta);
    }
  static_assert((long long)OZ_MAX_K * (1 << 14) < (1LL << 31), "int32 accumulators");
  static_assert(OZ_MAX_K <= (1 << 17) - 128, "K bound");
  std::printf("beta12_4096=%d\n", oz_consts(12, 4096).beta);
  std::printf("beta12_16384=%d beta14_16384=%d\n", oz_consts(12, 16384).beta, oz_consts(14, 16384).beta);
  // the constants tests/oz_product_ref.py restates (tests/test_oz_product_ref_host.py)
  std::printf("mods=");
  for (int l = 0; l < OZ_MAXMOD; ++l) std::printf("%d%s", oz_consts(OZ_MAXMOD, 64).m[l], l + 1 < OZ_MAXMOD ? "," : "\n");
  for (int nmod = 6; nmod <= OZ_MAXMOD; ++nmod) {
    std::printf("Md %d %a\n", nmod, oz_consts(nmod, 64).Md);
    for (int K : {64, 128, 192, 256, 320, 448, 512, 576, 1024, 1536, 4096, 16384, 65536, 130560, OZ_MAX_K})
      std::printf("beta %d %d %d\n", nmod, K, oz_consts(nmod, K).beta);
  }
}

// every wanted tile once, the rest 0xffffffff, length a multiple of 8
static void check_list(const std::vector<unsigned>& l, size_t off, size_t len, int nti, int ntj, bool lower, int ti0,
                       const char* what) {
  CHECK(len % 8 == 0, "%s: length %zu", what, len);
  CHECK(off + len <= l.size(), "%s: past the array", what);
  std::map<unsigned, int> seen;
  size_t pads = 0;
  for (size_t i = off; i < off + len && i < l.size(); ++i) {
    if (l[i] == 0xffffffffu) ++pads;
    else ++seen[l[i]];
  }
  size_t want = 0;
  for (int ti = ti0; ti < ti0 + nti; ++ti)
    for (int tj = 0; tj < (lower ? ti + 1 : ntj); ++tj) {
      ++want;
      const auto it = seen.find(((unsigned)ti << 16) | (unsigned)tj);
      CHECK(it != seen.end() && it->second == 1, "%s nti %d ntj %d ti0 %d: tile (%d, %d) %s", what, nti, ntj, ti0, ti,
            tj, it == seen.end() ? "missing" : "repeated");
    }
  CHECK(seen.size() == want, "%s nti %d ntj %d ti0 %d: %zu distinct entries for %zu tiles", what, nti, ntj, ti0,
        seen.size(), want);
  CHECK(pads + want == len, "%s: %zu pads + %zu tiles != %zu", what, pads, want, len);
}

static void check_lists() {
  for (int nti = 1; nti <= 20; ++nti)
    for (int ti0 : {0, 1, 3, 8}) {
      for (int ntj = 1; ntj <= 20; ++ntj) {
        const std::vector<unsigned> l = oz_list(nti, ntj, false, [](int ti, int tj) { return 1.0 + ti + 2.0 * tj; }, ti0);
        check_list(l, 0, l.size(), nti, ntj, false, ti0, "rect");
      }
      // lower lists are built with ntj = the last tile row + 1 (the LAUUM, the row-block slabs)
      const std::vector<unsigned> l = oz_list(nti, ti0 + nti, true, [](int ti, int) { return 100.0 - ti; }, ti0);
      check_list(l, 0, l.size(), nti, ti0 + nti, true, ti0, "lower");
    }
}

static void check_pairs() {
  const int N = OZ_MAXMOD;
  for (int NB = 2; NB <= 140; ++NB) {
    // the levels' X21 blocks tile the strictly lower triangle of the NB x NB tile grid
    std::vector<int> cover((size_t)NB * NB, 0);
    const int np2 = (NB * TILE + OZ_T - 1) / OZ_T * OZ_T;
    int levels = 0;
    for (int s = 2; s / 2 < NB; s *= 2) {
      const auto prs = trtri_level_pairs(NB, s);
      CHECK(!prs.empty(), "NB %d s %d: empty level", NB, s);
      ++levels;
      std::vector<unsigned> lists(5, 0u);   // (something before: offsets are into the array)
      for (size_t i = 0; i < prs.size(); ++i) {
        const int t0 = prs[i][0], h = prs[i][1], t1 = prs[i][2];
        CHECK(t0 % s == 0 && h == t0 + s / 2 && h < t1 && t1 <= std::min(NB, t0 + s), "NB %d pair (%d, %d, %d)", NB, t0,
              h, t1);
        CHECK(i + 1 == prs.size() ? (t1 == std::min(NB, t0 + s)) : (t1 == t0 + s), "NB %d: ragged pair not last", NB);
        for (int r = h; r < t1; ++r)
          for (int c = t0; c < h; ++c) ++cover[(size_t)r * NB + c];
        const size_t before = lists.size();
        const OzTriPair q = oz_tri_pair_plan(t0, h, t1, N, lists);
        CHECK(q.t0 == t0 && q.h == h && q.t1 == t1, "NB %d: pair ids", NB);
        CHECK(q.Ra == (h - t0) * TILE && q.Rb == (t1 - h) * TILE, "NB %d: rows", NB);
        CHECK(q.Pa % OZ_T == 0 && q.Pa >= q.Ra && q.Pa < q.Ra + OZ_T, "NB %d: Pa %d Ra %d", NB, q.Pa, q.Ra);
        CHECK(q.Pb % OZ_T == 0 && q.Pb >= q.Rb && q.Pb < q.Rb + OZ_T, "NB %d: Pb %d Rb %d", NB, q.Pb, q.Rb);
        // planes_bytes = N Pa (Pa + Pb) is the first product's need; the second's
        // N Pb (Pa + Pb) fits only while Pb <= Pa
        CHECK(q.Pb <= q.Pa, "NB %d pair (%d, %d, %d): Pb %d > Pa %d", NB, t0, h, t1, q.Pb, q.Pa);
        CHECK((size_t)N * ((size_t)q.Pb * q.Pa + (size_t)q.Pa * q.Pa) <= q.planes_bytes(N), "NB %d: planes, T = L21 X11", NB);
        CHECK((size_t)N * ((size_t)q.Pb * q.Pb + (size_t)q.Pa * q.Pb) <= q.planes_bytes(N), "NB %d: planes, X21 = -X22 T", NB);
        CHECK((size_t)N * (q.Pb / OZ_T) * (q.Pa / OZ_T) * OZ_T * OZ_T == q.resid_bytes(N), "NB %d: residues", NB);
        // exponents: ex[0, Pb) for the rows of L21 / X22, ex[Pb, Pb + Pa) for X11's / T's:
        // Pa + Pb ints, which passes np2 (the LAUUM's need) only for the one-tile blocks
        CHECK(q.Pa + q.Pb <= std::max(np2, 2 * OZ_T), "NB %d pair (%d, %d, %d): Pa + Pb = %d, np2 = %d", NB, t0, h, t1,
              q.Pa + q.Pb, np2);
        CHECK(q.Pa <= OZ_MAX_K && q.Pb <= OZ_MAX_K, "NB %d: K", NB);
        // the two lists: contiguous, disjoint, appended at the array's end
        CHECK(q.la_off == (long long)before && q.lb_off == q.la_off + q.la_len &&
                  lists.size() == (size_t)(q.lb_off + q.lb_len),
              "NB %d: list offsets %lld + %d, %lld + %d of %zu", NB, q.la_off, q.la_len, q.lb_off, q.lb_len, lists.size());
        check_list(lists, (size_t)q.la_off, (size_t)q.la_len, q.Pb / OZ_T, q.Pa / OZ_T, false, 0, "pair list a");
        check_list(lists, (size_t)q.lb_off, (size_t)q.lb_len, q.Pb / OZ_T, q.Pa / OZ_T, false, 0, "pair list b");
        CHECK(q.ops_a > 0.0 && q.ops_b > 0.0, "NB %d: ops", NB);
      }
    }
    for (int r = 0; r < NB; ++r)
      for (int c = 0; c < NB; ++c)
        CHECK(cover[(size_t)r * NB + c] == (r > c ? 1 : 0), "NB %d: tile block (%d, %d) filled %d times", NB, r, c,
              cover[(size_t)r * NB + c]);
    int want_levels = 0;
    while ((1 << want_levels) < NB) ++want_levels;
    CHECK(levels == want_levels, "NB %d: %d levels", NB, levels);
  }
}

// One product description against the closed forms its call site used to write out by hand,
// restated here (never taken from OzShape): over every tile the k-range length, the list entry
// for entry against oz_list with the closed form (nti, ntj, lower, ti0 as the site passed
// them), the operation count against the site's loop, the residue-tile count.  All integers
// far below 2^53: equality is exact.
template <class W>
static void check_shape(const OzShape& s, int nti, int ntj, bool lower, int ti0, W klen, double ops, long long tiles,
                        const char* what, int id) {
  for (int ti = ti0; ti < ti0 + nti; ++ti)
    for (int tj = 0; tj < (lower ? ti + 1 : ntj); ++tj)
      CHECK(s.klen(ti, tj) == klen(ti, tj), "%s %d: tile (%d, %d) k range %d, closed form %d", what, id, ti, tj,
            s.klen(ti, tj), klen(ti, tj));
  const std::vector<unsigned> got = s.list();
  const std::vector<unsigned> want = oz_list(nti, ntj, lower, [&](int ti, int tj) { return (double)klen(ti, tj); }, ti0);
  CHECK(got == want, "%s %d: list of %zu entries differs from oz_list with the closed form (%zu)", what, id, got.size(),
        want.size());
  check_list(got, 0, got.size(), nti, ntj, lower, ti0, what);
  CHECK(s.ops(OZ_MAXMOD) == ops, "%s %d: ops %.17g, the site's loop %.17g", what, id, s.ops(OZ_MAXMOD), ops);
  CHECK(s.tiles() == tiles, "%s %d: %lld residue tiles, %lld expected", what, id, s.tiles(), tiles);
  CHECK(s.res_bytes() == tiles * OZ_T * OZ_T, "%s %d: residue bytes", what, id);
}

// a TRTRI pair's two products, and its lists in the plan's array
static void check_pair_shapes(int t0, int h, int t1) {
  const int N = OZ_MAXMOD;
  std::vector<unsigned> lists(3, 0u);
  const OzTriPair q = oz_tri_pair_plan(t0, h, t1, N, lists);
  const int nti = q.Pb / OZ_T, ntj = q.Pa / OZ_T, id = 10000 * t0 + 100 * h + t1;
  double ops_a = 0.0, ops_b = 0.0;
  for (int tj = 0; tj < ntj; ++tj) ops_a += 2.0 * OZ_T * OZ_T * nti * (double)(q.Pa - OZ_T * tj) * N;
  for (int ti = 0; ti < nti; ++ti) ops_b += 2.0 * OZ_T * OZ_T * ntj * (double)(OZ_T * (ti + 1)) * N;
  const auto ka = [&](int, int tj) { return q.Pa - OZ_T * tj; };
  const auto kb = [&](int ti, int) { return OZ_T * (ti + 1); };
  check_shape(q.shape_a(), nti, ntj, false, 0, ka, ops_a, (long long)nti * ntj, "pair T = L21 X11", id);
  check_shape(q.shape_b(), nti, ntj, false, 0, kb, ops_b, (long long)nti * ntj, "pair X21 = -X22 T", id);
  const std::vector<unsigned> la = oz_list(nti, ntj, false, [&](int ti, int tj) { return (double)ka(ti, tj); });
  const std::vector<unsigned> lb = oz_list(nti, ntj, false, [&](int ti, int tj) { return (double)kb(ti, tj); });
  CHECK(std::vector<unsigned>(lists.begin() + q.la_off, lists.begin() + q.la_off + q.la_len) == la, "pair %d: list a", id);
  CHECK(std::vector<unsigned>(lists.begin() + q.lb_off, lists.begin() + q.lb_off + q.lb_len) == lb, "pair %d: list b", id);
  CHECK(q.ops_a == ops_a && q.ops_b == ops_b, "pair %d: the plan's ops %.17g, %.17g", id, q.ops_a, q.ops_b);
  CHECK(q.resid_bytes(N) == (size_t)N * nti * ntj * OZ_T * OZ_T, "pair %d: residues", id);
  // the split Cholesky's Schur complement on the same pair: every sum Pa long
  const int nts = q.Pb / OZ_T;
  check_shape(q.shape_schur(), nts, nts, true, 0, [&](int, int) { return q.Pa; },
              2.0 * OZ_T * OZ_T * (double)q.Pa * N * (nts * (nts + 1) / 2), (long long)nts * (nts + 1) / 2, "Schur", id);
}

static void check_shapes() {
  const int N = OZ_MAXMOD;
  // n_pad 1152 and 1280 share np2 = 1280, 8320 and 8448 share 8448; 2944 is NB = 23
  for (int n_pad : {1152, 1280, 2944, 8320, 8448}) {
    const int NB = n_pad / TILE, np2 = (n_pad + OZ_T - 1) / OZ_T * OZ_T, NT2 = np2 / OZ_T;
    {   // the LAUUM
      double ops = 0.0;
      for (int ti = 0; ti < NT2; ++ti) ops += 2.0 * OZ_T * OZ_T * (ti + 1) * (double)(np2 - OZ_T * ti) * N;
      check_shape(oz_lauum_shape(np2), NT2, NT2, true, 0, [&](int ti, int) { return np2 - OZ_T * ti; }, ops,
                  (long long)NT2 * (NT2 + 1) / 2, "LAUUM", n_pad);
    }
    for (int s = 2; s / 2 < NB; s *= 2)
      for (const auto& pr : trtri_level_pairs(NB, s)) check_pair_shapes(pr[0], pr[1], pr[2]);
    // the posterior's V = L^-1 K* for chunks of one and of three tile columns: the rows of
    // L^-1, k up to the row's tile end
    for (int ntj : {1, 3}) {
      double ops = 0.0;
      for (int ti = 0; ti < NT2; ++ti) ops += 2.0 * OZ_T * OZ_T * ntj * (double)(OZ_T * (ti + 1)) * N;
      check_shape(OzShape::rect(NT2, ntj, np2, 0, 1), NT2, ntj, false, 0, [&](int ti, int) { return OZ_T * (ti + 1); }, ops,
                  (long long)NT2 * ntj, "posterior", n_pad);
    }
    // the row-block partial: slabs of 6 and of 10 tile rows (all but the first with ti0 > 0)
    for (int P : {1, 2, 3, 8})
      for (int rows : {6, 10}) {
        const int Kp = ((NB - 1) / P + 1) * TILE;
        for (int a0 = 0; a0 < NB; a0 += rows) {
          const int a1 = std::min(NB, a0 + rows), ti0 = a0 / 2, ti1 = (a1 + 1) / 2;
          const auto kl = [&](int ti, int) { return std::max(0, Kp - 128 * ((2 * ti) / P)); };
          double ops = 0.0;
          for (int ti = ti0; ti < ti1; ++ti) ops += 2.0 * OZ_T * OZ_T * (ti + 1) * (double)kl(ti, 0) * N;
          check_shape(oz_slab_shape(a0, a1, Kp, P), ti1 - ti0, ti1, true, ti0, kl, ops,
                      (long long)ti1 * (ti1 + 1) / 2 - (long long)ti0 * (ti0 + 1) / 2, "slab", 100 * n_pad + P);
        }
      }
  }
  check_pair_shapes(0, 3, 4);   // Ra = 384, Rb = 128: Rb < Ra and Pb = 256 > Rb
}

int main() {
  check_consts();
  check_lists();
  check_pairs();
  check_shapes();
  if (g_fail) {
    std::printf("oz_plan_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("oz_plan_check OK\n");
  return 0;
}
