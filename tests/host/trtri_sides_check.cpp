// trtri_sides_check.cpp -- host-only check of the TRTRI's block pairs by side of the split
// Cholesky's column (gpemu_ozaki.hpp: trtri_level_pairs, trtri_side_pairs) and of split_k's
// whole-level decision (gpemu_gemm_sched.hpp).  No HIP runtime call: it runs without a GPU.
// Built and run by tests/test_trtri_sides_host.py:
//   hipcc --offload-arch=gfx950 -std=c++17 -I gp_emu_uqsa_amd/csrc tests/host/trtri_sides_check.cpp
// Prints one line per failed check; exit status 0 and a last line "trtri_sides_check OK" when
// every check holds.
#include <cstdio>
#include <map>

#include "gpemu_kernels.hpp"
#include "gpemu_gemm_sched.hpp"
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

// the split column of NB tile columns: the largest power of two below NB (oz_chol_split)
static int split_col(int NB) {
  int h = 1;
  while (2 * h < NB) h *= 2;
  return h;
}

// Every pair of every level is on exactly one side or is the one top pair (0, h, NB); no pair
// of a side straddles h; the sides keep the level's order.
static void check_sides() {
  for (int NB = 2; NB <= 130; ++NB) {
    const int h = split_col(NB);
    int tops = 0;
    for (int s = 2; s / 2 < NB; s *= 2) {
      const auto prs = trtri_level_pairs(NB, s);
      std::map<std::array<int, 3>, int> seen;
      for (int sd = 0; sd < 2; ++sd) {
        int last = -1;
        for (const auto& pr : trtri_side_pairs(prs, h, sd)) {
          ++seen[pr];
          CHECK(sd == 0 ? pr[2] <= h : pr[0] >= h, "NB %d s %d: pair (%d, %d, %d) is not inside side %d", NB, s, pr[0],
                pr[1], pr[2], sd);
          CHECK(pr[0] > last, "NB %d s %d: side %d out of order", NB, s, sd);
          last = pr[0];
        }
      }
      for (const auto& pr : prs) {
        const bool top = pr[0] < h && pr[2] > h;
        if (top) {
          ++tops;
          CHECK(pr[0] == 0 && pr[1] == h && pr[2] == NB && prs.size() == 1, "NB %d s %d: straddling pair (%d, %d, %d)", NB,
                s, pr[0], pr[1], pr[2]);
        }
        CHECK(seen[pr] == (top ? 0 : 1), "NB %d s %d: pair (%d, %d, %d) on %d sides", NB, s, pr[0], pr[1], pr[2], seen[pr]);
      }
      CHECK(seen.size() <= prs.size(), "NB %d s %d: a side holds a pair the level has not", NB, s);
    }
    CHECK(tops == 1, "NB %d: %d top pairs", NB, tops);
  }
}

// split_k with the whole level's tile count and longest K gives every problem of a side's
// launch the split it has in the level's one launch, and its partial slots stay inside the
// SPLIT_SLOTS the level's launch may use.
static void check_split_k() {
  static double part[1];
  static int tcnt[1];
  for (int NB = 2; NB <= 130; ++NB) {
    const int h = split_col(NB);
    for (int s = 2; s / 2 < NB; s *= 2) {
      const auto prs = trtri_level_pairs(NB, s);
      auto probs_of = [&](const std::vector<std::array<int, 3>>& ps, bool second) {
        std::vector<GemmProb> out;
        for (const auto& pr : ps) {
          const int a = pr[1] - pr[0], b = pr[2] - pr[1];
          out.push_back(second ? mkprob(nullptr, 1, nullptr, 1, nullptr, 1, b, a, b * TILE, G_KEND_TI, -1.0, 0.0)
                               : mkprob(nullptr, 1, nullptr, 1, nullptr, 1, a, b, a * TILE, G_KBEG_TI, 1.0, 0.0));
        }
        return out;
      };
      for (int second = 0; second < 2; ++second) {
        std::vector<GemmProb> whole = probs_of(prs, second != 0);
        int T = 0, kmax = 0;
        for (const GemmProb& p : whole) { T += prob_tiles(p); kmax = std::max(kmax, p.K); }
        split_k(whole, part, tcnt);
        std::map<std::array<int, 3>, int> ks;
        for (size_t i = 0; i < prs.size(); ++i) ks[prs[i]] = whole[i].ksplit;
        for (int sd = 0; sd < 2; ++sd) {
          const auto sp = trtri_side_pairs(prs, h, sd);
          std::vector<GemmProb> side = probs_of(sp, second != 0);
          int tiles = 0;   // (before the split: prob_tiles counts the shares afterwards)
          for (const GemmProb& p : side) tiles += prob_tiles(p);
          split_k(side, part, tcnt, T, kmax);
          for (size_t i = 0; i < sp.size(); ++i)
            CHECK(side[i].ksplit == ks[sp[i]], "NB %d s %d side %d: ksplit %d against the level's %d", NB, s, sd,
                  side[i].ksplit, ks[sp[i]]);
          if (!side.empty() && side[0].ksplit > 1)
            CHECK(tiles * side[0].ksplit <= SPLIT_SLOTS, "NB %d s %d side %d: %d partial slots", NB, s, sd,
                  tiles * side[0].ksplit);
        }
      }
    }
  }
}

int main() {
  check_sides();
  check_split_k();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("trtri_sides_check OK\n");
  return 0;
}
