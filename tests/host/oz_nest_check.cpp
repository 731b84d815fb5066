// oz_nest_check.cpp -- host-only check of the nested split Cholesky's int8 product
// (gpemu_ozaki.hpp: OzCholNest, OzShape::lower_capped, oz_res_tile with a cap, oz_list).  No HIP
// runtime call: it runs without a GPU.  Built and run by tests/test_ozaki_nest_host.py:
//   hipcc --offload-arch=gfx950 -std=c++17 -I gp_emu_uqsa_amd/csrc tests/host/oz_nest_check.cpp
// For every n_pad from 1024 to 65536 in steps of 128 at which the plan can nest (the rule of
// oz_chol_split / oz_chol_nest_split restated here at the floors gpe_create allows, 256 rows
// each: every size that nests at any setting), the trapezoid {rows [q, NB), columns [q, h),
// column <= row} in 128-tiles against the product's 256-tiles.  Prints one line per failed
// check and "nested=<sizes>"; exit status 0 and a last line "oz_nest_check OK" when every
// check holds.
#include <cstdio>
#include <map>
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

static void check_nest(int n_pad, int q, int h, int NB) {
  const int N = OZ_MAXMOD;
  const OzCholNest n = oz_chol_nest_plan(q, h, NB);
  const OzShape s = n.shape();
  const int nti = (NB - q + 1) / 2, cap = (h - q) / 2;
  CHECK(n.Rb == (NB - q) * TILE && n.Pb == nti * OZ_T && n.K == q * TILE && n.cols == cap * OZ_T, "n_pad %d: plan", n_pad);
  CHECK(n.K % OZ_T == 0 && n.K <= OZ_MAX_K && n.K >= OZ_SK, "n_pad %d: K %d", n_pad, n.K);
  CHECK(cap >= 1 && cap < nti, "n_pad %d: cap %d of %d tile rows", n_pad, cap, nti);
  CHECK(s.tri == 1 && s.ntj == cap && s.nti == nti && s.ti0 == 0 && s.K == n.K && s.kbeg == 0 && s.kend == 0,
        "n_pad %d: shape", n_pad);
  // the list: every 256-tile of the capped triangle once, nothing else but padding
  const std::vector<unsigned> l = s.list();
  CHECK(l.size() % 8 == 0, "n_pad %d: list length %zu", n_pad, l.size());
  std::map<unsigned, int> seen;
  for (unsigned e : l)
    if (e != 0xffffffffu) ++seen[e];
  long long want = 0;
  for (int ti = 0; ti < nti; ++ti)
    for (int tj = 0; tj <= std::min(ti, cap - 1); ++tj) {
      ++want;
      const auto it = seen.find(((unsigned)ti << 16) | (unsigned)tj);
      CHECK(it != seen.end() && it->second == 1, "n_pad %d: tile (%d, %d) %s", n_pad, ti, tj,
            it == seen.end() ? "missing" : "repeated");
    }
  CHECK((long long)seen.size() == want, "n_pad %d: %zu distinct entries for %lld tiles", n_pad, seen.size(), want);
  // ... which are the 256-tiles that hold a 128-tile (i, j) of the trapezoid, no more, no fewer
  std::set<unsigned> need;
  for (int j = q; j < h; ++j)
    for (int i = j; i < NB; ++i) need.insert(((unsigned)((i - q) / 2) << 16) | (unsigned)((j - q) / 2));
  CHECK(need.size() == seen.size(), "n_pad %d: %zu tiles hold the trapezoid, the list has %zu", n_pad, need.size(), seen.size());
  for (unsigned e : need) CHECK(seen.count(e) == 1, "n_pad %d: trapezoid tile %x not in the list", n_pad, e);
  // closed forms
  const long long tiles = (long long)cap * (cap + 1) / 2 + (long long)(nti - cap) * cap;
  CHECK(want == tiles && s.tiles() == tiles, "n_pad %d: %lld tiles, closed form %lld", n_pad, s.tiles(), tiles);
  CHECK(s.ops(N) == 2.0 * OZ_T * OZ_T * (double)n.K * (double)tiles * N, "n_pad %d: ops %.17g", n_pad, s.ops(N));
  // residue tiles: one slot each inside [0, tiles)
  std::set<long long> slots;
  for (const auto& kv : seen) {
    const long long r = s.res_tile((int)(kv.first >> 16), (int)(kv.first & 0xffffu));
    CHECK(r >= 0 && r < tiles, "n_pad %d: residue tile %lld of %lld", n_pad, r, tiles);
    slots.insert(r);
  }
  CHECK((long long)slots.size() == tiles, "n_pad %d: residue tiles shared", n_pad);
  // the buffers oz_prepare takes for it: planes for every tile row of both operands (b's are
  // a's first cap), residues for every tile, an exponent per padded row; C inside A
  CHECK(n.planes_bytes(N) >= (size_t)N * nti * OZ_T * n.K, "n_pad %d: planes", n_pad);
  CHECK(n.resid_bytes(N) == (size_t)N * tiles * OZ_T * OZ_T && s.res_bytes() == tiles * OZ_T * OZ_T, "n_pad %d: residues", n_pad);
  const int np2 = (n_pad + OZ_T - 1) / OZ_T * OZ_T;
  CHECK(n.Pb <= np2, "n_pad %d: %d exponents, np2 %d", n_pad, n.Pb, np2);
  CHECK(q * TILE + n.Rb == n_pad && q * TILE + n.cols == h * TILE, "n_pad %d: C's block leaves A", n_pad);
  const OzSrc o = n.src(nullptr, n_pad);
  CHECK(o.trans && o.R == n.Rb && o.Kv == n.K && o.mask == 0 && q * TILE + o.R <= n_pad, "n_pad %d: operand", n_pad);
}

int main() {
  int nested = 0;
  for (int n_pad = 1024; n_pad <= 65536; n_pad += TILE) {
    const int NB = n_pad / TILE;
    int h = 1;
    while (2 * h < NB) h *= 2;
    if ((NB - h) * TILE < 256) continue;                    // not split (oz_chol_split at its floor)
    const int q = h / 2;
    if (h < 4 || q % 2 || (NB - q) * TILE < 256) continue;  // not nested (oz_chol_nest_split at its floor)
    check_nest(n_pad, q, h, NB);
    ++nested;
  }
  // small capped shapes beside the plan's: every cap below the row count, and a cap that is none
  for (int nti = 1; nti <= 12; ++nti)
    for (int cap = 1; cap <= nti + 1; ++cap) {
      const OzShape s = OzShape::lower_capped(nti, cap, 256);
      long long tiles = 0;
      for (int ti = 0; ti < nti; ++ti) tiles += std::min(ti + 1, cap);
      CHECK(s.tiles() == tiles, "nti %d cap %d: %lld tiles, %lld expected", nti, cap, s.tiles(), tiles);
      std::set<long long> slots;
      size_t entries = 0;
      for (unsigned e : s.list())
        if (e != 0xffffffffu) {
          ++entries;
          const int ti = (int)(e >> 16), tj = (int)(e & 0xffffu);
          CHECK(ti < nti && tj <= std::min(ti, cap - 1), "nti %d cap %d: tile (%d, %d) outside", nti, cap, ti, tj);
          slots.insert(s.res_tile(ti, tj));
        }
      CHECK((long long)entries == tiles && (long long)slots.size() == tiles && (slots.empty() || *slots.rbegin() == tiles - 1),
            "nti %d cap %d: %zu entries, %zu slots for %lld tiles", nti, cap, entries, slots.size(), tiles);
    }
  std::printf("nested=%d\n", nested);
  if (g_fail) {
    std::printf("oz_nest_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("oz_nest_check OK\n");
  return 0;
}
