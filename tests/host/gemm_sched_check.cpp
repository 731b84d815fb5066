// gemm_sched_check.cpp -- host-only check of the grouped GEMM's launch layer
// (gpemu_gemm_sched.hpp: the kind table, the descriptors of a launch, split_k, xcd_order,
// order_tiles, list_launch).  No HIP runtime call: it runs without a GPU.  Built and run by
// tests/test_gemm_sched_host.py:
//   hipcc --offload-arch=gfx950 -std=c++17 -I gp_emu_uqsa_amd/csrc tests/host/gemm_sched_check.cpp
// Prints one line per failed check; exit status 0 and a last line "gemm_sched_check OK" when
// every check holds.  With the argument --digests it prints the digests of the pinned groups
// (name and value a line) instead of comparing them: the way to pin them anew after a
// deliberate change of the tile order.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "gpemu_gemm_sched.hpp"

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

// ---- 1. the kind table
static_assert(GEMM_PLAIN == 0 && GEMM_AK == 1 && GEMM_AK_BK == 2 && GEMM_BK == 3 && GEMM_FUSED == 4, "ABI values");
constexpr bool inst_is(GemmKind k, bool ak, bool bk, bool fused) {
  return gemm_instance(k).ak == ak && gemm_instance(k).bk == bk && gemm_instance(k).fused == fused;
}
static_assert(inst_is(GEMM_PLAIN, false, false, false), "0: <0, 0>");
static_assert(inst_is(GEMM_AK, true, false, false), "1: <1, 0>");
static_assert(inst_is(GEMM_AK_BK, true, true, false), "2: <1, 1>");
static_assert(inst_is(GEMM_BK, false, true, false), "3: <0, 1>");
static_assert(inst_is(GEMM_FUSED, false, false, true), "4: <0, 0, FUSED>");
static_assert(gemm_kind(false, false) == GEMM_PLAIN && gemm_kind(true, false) == GEMM_AK &&
              gemm_kind(true, true) == GEMM_AK_BK && gemm_kind(false, true) == GEMM_BK, "gemm_kind inverts the table");

// operands nobody dereferences, counters likewise
static double g_buf[2];
static int g_cnt[8];

static GemmProb plain(int mt, int nt, int K, int flags = 0, double beta = 0.0, int kti_mul = 1, int kti_off = 0) {
  GemmProb p = mkprob(g_buf, 2, g_buf, 2, g_buf, 2, mt, nt, K, flags, 1.0, beta);
  p.kti_mul = kti_mul;
  p.kti_off = kti_off;
  return p;
}

// One fused Cholesky step shaped as chain_step and SweepProbs::bulk (gpemu_chol_sched.hpp) assemble it: the diagonal tile's pending update in
// quadrant blocks (K > 0), the diagonal tile, m panel tiles in two halves, then the trailing
// update of nb columns (a lower-triangular block and the rows under it).
static std::vector<GemmProb> fused_step(int K, int m, int nb, int rows_under) {
  std::vector<GemmProb> g;
  if (K) {
    g.push_back(mkprob(g_buf, 2, nullptr, 0, g_buf, 2, DQ_N, 1, K, G_DQUAD, -1.0, 1.0));
    g.back().post = g_cnt + 0;
  }
  g.push_back(mkprob(nullptr, 2, nullptr, 2, g_buf, 2, 1, 1, 0, G_DIAG, 1.0, 1.0));
  if (K) {
    g.back().pre0 = g_cnt + 0;
    g.back().pre0_n = DQ_N;
  }
  g.back().flag = g_cnt + 1;
  if (m) {
    GemmProb h0 = mkprob(g_buf, 2, g_buf, 2, g_buf, 2, m, 1, K, G_PANEL | G_PHALF0, K ? -1.0 : 1.0, 1.0);
    h0.flag = g_cnt + 1;
    h0.cpost = g_cnt + 2;
    GemmProb h1 = h0;
    h1.flags = G_PANEL | G_PHALF1;
    h1.K = 0;
    h1.beta = 0.0;
    h1.cpost = nullptr;
    h1.pre0 = g_cnt + 2;
    h1.pre0_n = m;
    g.push_back(h0);
    g.push_back(h1);
  }
  if (nb) {
    g.push_back(mkprob(g_buf, 2, g_buf, 2, g_buf, 2, nb, nb, 1024, G_CLOWER, -1.0, 1.0));
    if (rows_under) g.push_back(mkprob(g_buf, 2, g_buf, 2, g_buf, 2, rows_under, nb, 1024, 0, -1.0, 1.0));
  }
  return g;
}

static std::vector<unsigned> all_tiles(const std::vector<GemmProb>& probs, bool ti_major) {
  std::vector<unsigned> t;
  for (int p = 0; p < (int)probs.size(); ++p) {
    const GemmProb& P = probs[p];
    if (ti_major) {
      for (int ti = 0; ti < P.mt; ++ti)
        for (int tj = 0; tj < P.nt; ++tj)
          if (!(P.flags & G_CLOWER) || tj <= ti) t.push_back(tile_code(p, ti, tj));
    } else {
      for (int tj = 0; tj < P.nt; ++tj)
        for (int ti = 0; ti < P.mt; ++ti)
          if (!(P.flags & G_CLOWER) || tj <= ti) t.push_back(tile_code(p, ti, tj));
    }
  }
  return t;
}

// ---- 2. the descriptors of a launch
static GemmLaunch build(std::vector<GemmProb>& arr, const std::vector<GemmProb>& group, GemmKind kind, bool cdef_ok) {
  GemmLaunch L = begin_launch(kind, arr, 1.5);
  for (const GemmProb& p : group) push_prob(L, arr, p, cdef_ok);
  return L;
}

static void check_descriptors(const char* what, const std::vector<GemmProb>& arr, const GemmLaunch& L, int first,
                              size_t count) {
  CHECK(L.first == first && L.count == (int)count && L.list == -1 && L.ticket == nullptr && L.flops == 1.5, "%s", what);
  int at = 0;
  for (int i = 0; i < L.count; ++i) {
    const GemmProb& p = arr[L.first + i];
    CHECK(p.tile_begin == at, "%s: problem %d begins at %d, not %d", what, i, p.tile_begin, at);
    CHECK(i == 0 || p.tile_begin >= arr[L.first + i - 1].tile_begin, "%s: tile_begin decreases at %d", what, i);
    CHECK(p.ntiles == prob_tiles(p), "%s: ntiles of %d", what, i);
    at += p.ntiles;
  }
  CHECK(at == L.tiles, "%s: problems cover [0, %d), the launch has %d tiles", what, at, L.tiles);
}

static void check_builder() {
  std::vector<GemmProb> arr(3, plain(1, 1, 128));   // (a launch need not start the array)
  // mkprob zeroes the whole descriptor, padding included
  {
    GemmProb a, b;
    std::memset(&a, 0xff, sizeof(a));
    std::memset(&b, 0, sizeof(b));
    a = mkprob(nullptr, 0, nullptr, 0, nullptr, 0, 0, 0, 0, 0, 0.0, 0.0);
    b.ksplit = 1;
    b.kti_mul = 1;
    CHECK(a.ksplit == 1 && a.kti_mul == 1 && a.kti_off == 0 && !a.part && !a.tcnt && !a.pre0 && !a.pre1 && !a.post &&
              !a.cpost && !a.flag && !a.X && !a.Ld && !a.logdet && a.tile_begin == 0 && a.ntiles == 0,
          "mkprob defaults");
    GemmProb c = mkprob(nullptr, 0, nullptr, 0, nullptr, 0, 0, 0, 0, 0, 0.0, 0.0);
    CHECK(std::memcmp(&c, &b, sizeof(b)) == 0, "mkprob leaves bytes unset");
  }
  const std::vector<GemmProb> two = {plain(3, 5, 512), plain(4, 4, 512, G_CLOWER)};
  GemmLaunch L = build(arr, two, GEMM_AK, true);
  check_descriptors("plain pair", arr, L, 3, 2);
  CHECK(L.tiles == 15 + 10 && L.kind == GEMM_AK && !L.cdef, "plain pair: %d tiles", L.tiles);
  // split K: every share is a workgroup
  std::vector<double> part((size_t)SPLIT_SLOTS * TILE * TILE);
  std::vector<int> tcnt(SPLIT_SLOTS);
  std::vector<GemmProb> sp = {plain(2, 3, 1024, G_KBEG_TI), plain(3, 3, 2048, G_CLOWER | G_KBEG_TI)};
  split_k(sp, part.data(), tcnt.data());
  CHECK(sp[0].ksplit == 8 && sp[1].ksplit == 8, "split group: ksplit %d, %d", sp[0].ksplit, sp[1].ksplit);
  L = build(arr, sp, GEMM_AK_BK, true);
  check_descriptors("split group", arr, L, 5, 2);
  CHECK(L.tiles == (6 + 6) * 8, "split group: %d tiles", L.tiles);
  // a fused step's chain: quadrants, diagonal tile, both halves of the panels
  const std::vector<GemmProb> ch = fused_step(384, 7, 0, 0);
  CHECK(ch.size() == 4 && (ch[0].flags & G_DQUAD) && (ch[1].flags & G_DIAG) && (ch[2].flags & G_PHALF0) &&
            (ch[3].flags & G_PHALF1), "chain group");
  L = build(arr, ch, GEMM_FUSED, true);
  check_descriptors("chain", arr, L, 7, 4);
  CHECK(L.tiles == DQ_N + 1 + 7 + 7, "chain: %d tiles", L.tiles);
  // CDEF is the site's choice: a problem that asks for it counts only where the site lets it
  const GemmProb acc = plain(2, 2, 1024, 0, 1.0);
  CHECK(gemm_cdef(acc) == (std::getenv("GPEMU_NO_CDEF") == nullptr), "gemm_cdef of a beta = 1, K = 1024 problem");
  CHECK(build(arr, {acc}, GEMM_PLAIN, true).cdef == gemm_cdef(acc), "cdef_ok = true");
  CHECK(!build(arr, {acc}, GEMM_PLAIN, false).cdef, "cdef_ok = false");
  CHECK(!build(arr, {plain(2, 2, 1024)}, GEMM_PLAIN, true).cdef, "beta = 0 never takes CDEF");
  // a list gives the launch its tiles
  std::vector<unsigned> lists = {7u, 7u};
  L = build(arr, two, GEMM_PLAIN, true);
  set_list(L, lists, {tile_code(1, 3, 2), tile_code(0, 2, 4), tile_code(0, 0, 0)});
  CHECK(L.list == 2 && L.tiles == 3 && lists.size() == 5 && lists[2] == tile_code(1, 3, 2), "set_list");
  L = build(arr, two, GEMM_PLAIN, true);
  list_launch(L, arr, lists);
  CHECK(L.list == 5 && L.tiles == 25 && lists.size() == 30, "list_launch: list %lld, %d tiles", L.list, L.tiles);
  std::vector<unsigned> got(lists.begin() + 5, lists.end());
  CHECK(got == xcd_order(two.data(), all_tiles(two, false)), "list_launch is xcd_order of every tile");
  // a G_CLOWER problem is square in tiles: prob_tiles and order_tiles do not read its nt,
  // list_launch keeps tj < nt
  const std::vector<GemmProb> narrow = {plain(4, 2, 512, G_CLOWER)};
  CHECK(prob_tiles(narrow[0]) == 10 && order_tiles(narrow).size() == 10, "G_CLOWER ignores nt");
  L = build(arr, narrow, GEMM_PLAIN, true);
  list_launch(L, arr, lists);
  CHECK(L.tiles == 7, "list_launch keeps tj < nt: %d tiles", L.tiles);
}

// ---- 3. order_tiles
struct Rng {
  uint64_t s;
  unsigned next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(s >> 33);
  }
  int in(int lo, int hi) { return lo + (int)(next() % (unsigned)(hi - lo + 1)); }
};

static void check_fused_order(int K, int m, int nb, int rows_under) {
  const std::vector<GemmProb> g = fused_step(K, m, nb, rows_under);
  const std::vector<unsigned> ord = order_tiles(g);
  const std::vector<unsigned> all = all_tiles(g, true);
  const std::multiset<unsigned> a(ord.begin(), ord.end()), b(all.begin(), all.end());
  CHECK(a == b && std::set<unsigned>(ord.begin(), ord.end()).size() == ord.size(), "K %d m %d: not a permutation", K, m);
  const size_t nq = K ? DQ_N : 0;
  for (size_t i = 0; i < nq && i < ord.size(); ++i)
    CHECK(ord[i] == tile_code(0, (int)i, 0), "K %d m %d: position %zu is not quadrant block %zu", K, m, i, i);
  const size_t diag_at = nq;
  CHECK(ord.size() > diag_at && (g[ord[diag_at] >> 24].flags & G_DIAG), "K %d m %d: diagonal tile not at %zu", K, m, diag_at);
  size_t first_panel = ord.size(), npanel = 0;
  for (size_t i = 0; i < ord.size(); ++i)
    if (g[ord[i] >> 24].flags & G_PANEL) {
      CHECK(i > diag_at, "K %d m %d: panel tile at %zu before the diagonal tile", K, m, i);
      if (first_panel == ord.size()) first_panel = i;
      ++npanel;
    }
  CHECK(npanel == 2 * (size_t)m, "K %d m %d: %zu panel tiles", K, m, npanel);
  if (m) {
    const size_t bulk = ord.size() - npanel;   // quadrants, diagonal tile, trailing update
    if (bulk > diag_at + 256) {
      CHECK(first_panel == diag_at + 256, "K %d m %d: first panel tile at %zu", K, m, first_panel);
      CHECK(ord[first_panel] == tile_code(K ? 2 : 1, 0, 0), "K %d m %d: not the first panel tile", K, m);
      for (size_t i = first_panel + 1; i <= bulk; ++i)
        CHECK(!(g[ord[i] >> 24].flags & G_PANEL), "K %d m %d: panel tile at %zu inside the bulk", K, m, i);
    } else {
      CHECK(first_panel == bulk, "K %d m %d: the panel tiles are not the tail", K, m);
    }
  }
  CHECK(waits_point_back(g.data(), ord), "K %d m %d: a tile waits on a later one", K, m);
  if (m) {
    std::vector<unsigned> rev(ord.rbegin(), ord.rend());
    CHECK(!waits_point_back(g.data(), rev), "K %d m %d: the reversed order passes", K, m);
  }
}

static void check_order() {
  for (int K : {0, 128, 896})
    for (int m : {0, 1, 9, 40}) {
      check_fused_order(K, m, 0, 0);
      check_fused_order(K, m, 3, 5);      // short list: the panel tiles are the tail
      check_fused_order(K, m, 15, 9);     // 255 update tiles: one short of the + 256 slot ...
      check_fused_order(K, m, 1, 255);    // ... and 256: the shortest list that has it
      check_fused_order(K, m, 12, 30);
    }
  Rng r{20261020};
  for (int it = 0; it < 20000; ++it) {
    std::vector<GemmProb> g;
    const int np = r.in(1, 6);
    for (int p = 0; p < np; ++p) {
      int flags = 0;
      if (r.in(0, 3) == 0) flags |= G_CLOWER;
      if (r.in(0, 2) == 0) flags |= G_KBEG_TI;
      if (r.in(0, 2) == 0) flags |= G_KEND_TI;
      const int mt = r.in(1, 12), nt = (flags & G_CLOWER) ? mt : r.in(1, 12);
      g.push_back(plain(mt, nt, 128 * r.in(1, 16), flags, 0.0, r.in(1, 3), r.in(0, 3)));
    }
    const std::vector<unsigned> ord = order_tiles(g);
    if (ord != xcd_order(g.data(), all_tiles(g, true)) || ord != xcd_order(g.data(), all_tiles(g, false))) {
      CHECK(false, "random group %d: order_tiles is not xcd_order of every tile", it);
      break;
    }
  }
}

// ---- 4. pinned orders, 5. split_k: digests taken from the functions these replaced
static uint64_t fnv1a(const std::vector<unsigned>& v) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned x : v)
    for (int b = 0; b < 4; ++b) {
      h ^= (x >> (8 * b)) & 0xffu;
      h *= 1099511628211ull;
    }
  return h;
}

struct Pinned { const char* name; uint64_t digest; size_t len; };

static std::vector<Pinned> pinned_now() {
  std::vector<Pinned> out;
  auto pin = [&](const char* name, const std::vector<unsigned>& l) { out.push_back({name, fnv1a(l), l.size()}); };
  {   // one TRTRI level: M^T = X11^T L21^T over the block pairs of width 8 of 24 tile columns
    std::vector<GemmProb> g(3, plain(4, 4, 4 * TILE, G_KBEG_TI));
    pin("trtri_kbeg", order_tiles(g));
  }
  {   // X21 = -X22 M over three ranks' rows of a cyclic partition
    std::vector<GemmProb> g;
    for (int rk = 0; rk < 3; ++rk) g.push_back(plain(5 - rk, 4, 16 * TILE, G_KEND_TI, 0.0, 3, rk + 1));
    pin("cyclic_kend", order_tiles(g));
    pin("cyclic_kend_listed", xcd_order(g.data(), all_tiles(g, false)));
  }
  pin("lauum", order_tiles({plain(20, 20, 20 * TILE, G_CLOWER | G_KBEG_TI)}));
  pin("fused_step", order_tiles(fused_step(640, 30, 12, 20)));   // 329 tiles before the panels': the + 256 slot
  pin("fused_step_first", order_tiles(fused_step(0, 33, 16, 11)));
  {   // a row-block trailing update: three ranks' rows, the tiles of columns [9, 14) under the diagonal
    const int P = 3, NT = 26, k = 7;
    std::vector<GemmProb> g;
    std::vector<unsigned> mine;
    for (int rk = 0; rk < P; ++rk) {
      const int nloc = (NT - 1 - rk) / P + 1, a = k < rk ? 0 : (k - rk) / P + 1;
      for (int li = a; li < nloc; ++li)
        for (int j = 9; j < 14 && j <= li * P + rk; ++j) mine.push_back(tile_code((int)g.size(), li, j));
      g.push_back(plain(nloc, NT, 4 * TILE, 0, 1.0));
    }
    pin("dist_update_subset", xcd_order(g.data(), mine));
  }
  {   // split_k: the shares and scratch offsets of a group that splits
    std::vector<double> part((size_t)SPLIT_SLOTS * TILE * TILE);
    std::vector<int> tcnt(SPLIT_SLOTS);
    std::vector<GemmProb> g = {plain(2, 3, 1024, G_KBEG_TI), plain(3, 3, 2048, G_CLOWER | G_KBEG_TI), plain(1, 5, 384)};
    split_k(g, part.data(), tcnt.data());
    std::vector<unsigned> v;
    for (const GemmProb& p : g) {
      v.push_back((unsigned)p.ksplit);
      v.push_back((unsigned)(p.part - part.data()));
      v.push_back((unsigned)(p.tcnt - tcnt.data()));
      v.push_back((unsigned)prob_tiles(p));
    }
    pin("split_k", v);
    // ... and of the groups that must not: beta != 0, 256 tiles, K under 128
    std::vector<GemmProb> no[3] = {{plain(2, 3, 1024), plain(2, 2, 1024, 0, 1.0)}, {plain(16, 16, 1024)}, {plain(2, 3, 112)}};
    v.clear();
    for (auto& grp : no) {
      split_k(grp, part.data(), tcnt.data());
      for (const GemmProb& p : grp) {
        v.push_back((unsigned)p.ksplit);
        v.push_back(p.part ? 1u : 0u);
        v.push_back(p.tcnt ? 1u : 0u);
      }
    }
    pin("split_k_refused", v);
  }
  return out;
}

// from order_tiles (gpemu.hip) and xcd_order (gpemu_dist.hip) as they stood before this
// header, on the same groups
static const Pinned PINNED[] = {
    {"trtri_kbeg", 0xd6b62cff8ff390e3ull, 48},
    {"cyclic_kend", 0x5a6e1ec77a3e2cabull, 48},
    {"cyclic_kend_listed", 0x5a6e1ec77a3e2cabull, 48},
    {"lauum", 0xb904ba6c674eca01ull, 210},
    {"fused_step", 0xc6e1748fb81e9232ull, 389},
    {"fused_step_first", 0xcf2f662bd6410b22ull, 379},
    {"dist_update_subset", 0xff5a9ffad84ee625ull, 75},
    {"split_k", 0xa8414a622843779dull, 12},
    {"split_k_refused", 0x6cefd56366c52863ull, 12},
};

static void check_pinned() {
  const std::vector<Pinned> now = pinned_now();
  CHECK(now.size() == sizeof(PINNED) / sizeof(PINNED[0]), "%zu pinned groups", now.size());
  for (size_t i = 0; i < now.size() && i < sizeof(PINNED) / sizeof(PINNED[0]); ++i)
    CHECK(std::string(now[i].name) == PINNED[i].name && now[i].digest == PINNED[i].digest && now[i].len == PINNED[i].len,
          "%s: digest %016llx over %zu words", now[i].name, (unsigned long long)now[i].digest, now[i].len);
  // the groups that split keep ksplit > 1 only there (read back by the digest above), and
  // 257 problems cannot be named by a list: the launch keeps the implicit order
  std::vector<GemmProb> arr;
  GemmLaunch L = begin_launch(GEMM_PLAIN, arr);
  for (int p = 0; p < 257; ++p) push_prob(L, arr, plain(1, 2, 256), false);
  std::vector<unsigned> lists;
  list_launch(L, arr, lists);
  CHECK(L.list == -1 && lists.empty() && L.tiles == 514 && arr[256].tile_begin == 512, "257 problems stay unlisted");
  L.count = 256;
  list_launch(L, arr, lists);
  CHECK(L.list == 0 && lists.size() == 512, "256 problems are listed");
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "--digests") {
    for (const Pinned& p : pinned_now())
      std::printf("    {\"%s\", 0x%016llxull, %zu},\n", p.name, (unsigned long long)p.digest, p.len);
    return 0;
  }
  check_builder();
  check_order();
  check_pinned();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("gemm_sched_check OK\n");
  return 0;
}
