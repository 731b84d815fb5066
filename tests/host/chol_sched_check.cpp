// chol_sched_check.cpp -- host-only check of the factorisation plan (gpemu_chol_sched.hpp:
// build_chol_plan, the function gpemu.hip's build_plan uploads the result of).  No HIP runtime
// call: it runs without a GPU.  Built and run by tests/test_chol_sched_host.py:
//   hipcc --offload-arch=gfx950 -std=c++17 -I gp_emu_uqsa_amd/csrc tests/host/chol_sched_check.cpp
// The descriptors are never dereferenced on the host, so the workspace's buffers are address
// space only (an inaccessible, unreserved mapping of their size: the pointer arithmetic stays
// inside an object).
//   a. coverage, read off the descriptors: every launch's problems decoded back to tile columns,
//      for the per-step and the group launches of every sweep;
//   b. wait safety of every launch that has a ticket, on the tile list it stores;
//   c. the rollback of the three optional parts under a small descriptor limit;
//   d. the digest of the whole plan per pinned configuration.
// Prints one line per failed check; exit status 0 and a last line "chol_sched_check OK" when
// every check holds.  --digests prints the pinned table instead of comparing it; --emit CONFIG
// prints the decoded launch lists of a. for one configuration, a line per sweep ("SWEEP config NB
// NC NR group", then per launch "|" and its entries "F t p0" / "B a b g0 k"), for
// tests/test_chol_split_schedule.py, which applies its own check to them.
#include <sys/mman.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <atomic>
#include <string>
#include <thread>

#include "gpemu_kernels.hpp"
#include "gpemu_chol_sched.hpp"

using namespace gpe;

static std::atomic<int> g_fail{0};
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

// ---- the workspace: address space for the largest size checked
constexpr int NB_MAX = 130;
constexpr int NO_LIMIT = 1 << 30;
static void* reserve(size_t bytes) {
  void* p = mmap(nullptr, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (p == MAP_FAILED) {
    std::printf("cannot reserve %zu bytes of address space\n", bytes);
    std::exit(2);
  }
  return p;
}
static FactBufs g_space;
static void reserve_workspace() {
  const size_t n = (size_t)NB_MAX * TILE;
  g_space.A = (double*)reserve(n * n * sizeof(double));
  g_space.B = (double*)reserve(n * n * sizeof(double));
  g_space.Faug = (double*)reserve(n * TILE * sizeof(double));
  g_space.flags = (int*)reserve(FACT_FLAG_INTS * (size_t)NB_MAX * sizeof(int));
  g_space.logdet = (double*)reserve((size_t)NB_MAX * sizeof(double));
  g_space.part = (double*)reserve((size_t)SPLIT_SLOTS * TILE * TILE * sizeof(double));
  g_space.tcnt = (int*)reserve((size_t)SPLIT_SLOTS * sizeof(int));
}
static FactBufs workspace(int NB, bool aug) {
  FactBufs F = g_space;
  F.NB = NB;
  F.ld = (long long)NB * TILE;
  if (!aug) F.Faug = nullptr;
  return F;
}

// the split columns as gpemu.hip's callers choose them (oz_chol_split, oz_chol_nest_split) with
// the floors chol_min / nest_min in rows
static int split_col(int NB, int chol_min) {
  if (NB < 2) return 0;
  int h = 1;
  while (2 * h < NB) h *= 2;
  return (NB - h) * TILE >= chol_min ? h : 0;
}
static int nest_col(int NB, int h, int nest_min) {
  if (h < 4 || (h / 2) % 2) return 0;
  return (NB - h / 2) * TILE >= nest_min ? h / 2 : 0;
}

static CholSchedParams params(std::vector<std::pair<int, int>> groups, int sb, int sb_min, bool group = true) {
  CholSchedParams P;
  P.groups = std::move(groups);
  P.sb = sb;
  P.sb_min = sb_min;
  P.group = group;
  return P;
}

// tests/test_chol_split_schedule.py's CONFIGS as they stood: the default, widths 1-8, and widths
// 2 and 4 without super-blocks and with three groups each from the start
static std::vector<CholSchedParams> coverage_configs() {
  std::vector<CholSchedParams> c = {CholSchedParams()};
  for (int w = 1; w <= 8; ++w) c.push_back(params({{w, 0}}, 2, 80));
  for (int w : {2, 4}) c.push_back(params({{w, 0}}, 1, 80));
  for (int w : {2, 4}) c.push_back(params({{w, 0}}, 3, 0));
  return c;
}

// ---- a. coverage
struct Entry { bool factor; int a, b, g0, k; };   // factor: column a with pending columns [b, a); else bulk
static bool tile_of(const FactBufs& F, const double* p, int* i, int* j) {   // tile (i, j) of A
  const long long off = p - F.A;
  if (p < F.A || off >= F.ld * F.ld || off % TILE) return false;
  *j = (int)(off / (TILE * F.ld));
  *i = (int)((off % (TILE * F.ld)) / TILE);
  return off % (TILE * F.ld) < F.ld;
}
static bool atile_of(const FactBufs& F, const double* p, int* j) {   // tile (aug, j)
  if (!F.Faug || p < F.Faug || (p - F.Faug) >= F.ld * TILE || (p - F.Faug) % (TILE * TILE)) return false;
  *j = (int)((p - F.Faug) / (TILE * TILE));
  return true;
}

// The problems of one launch as the entries of the sweep with origin o, in the problems' order
// (per-step: the chain, then the bulk; group: the early updates, the chains, the bulk).  Every
// problem is read back in full: a problem that is none of the chain's or the bulk's, or whose
// operands disagree with its target, fails.
static std::vector<Entry> decode(const FactBufs& F, const GemmProb* p, int count, int o, bool aug, const char* what) {
  std::vector<Entry> out;
  const int NB = F.NB;
  for (int k = 0; k < count; ++k) {
    const GemmProb& q = p[k];
    int i = -1, j = -1, ia = -1, ja = -1, ib = -1, jb = -1;
    if (q.flags & G_DQUAD) {   // the pending update of the diagonal tile that follows
      const GemmProb& d = p[k + 1];
      CHECK(k + 1 < count && (d.flags & G_DIAG) && d.C == q.C && tile_of(F, q.C, &i, &j) && i == j &&
                tile_of(F, q.A, &ia, &ja) && ia == i && ja + q.K / TILE == j && q.K > 0 && q.mt == DQ_N && q.nt == 1,
            "%s: quadrant problem %d", what, k);
      continue;
    }
    if (q.flags & G_DIAG) {
      CHECK(tile_of(F, q.C, &i, &j) && i == j && q.Ld == q.C && q.X == F.B + (q.C - F.A) && q.logdet == F.logdet + j &&
                q.flag == F.flags + j && q.diag_col0 == j * TILE,
            "%s: diagonal problem %d", what, k);
      int p0 = j;   // the pending columns: the quadrant problem's before it
      if (k > 0 && (p[k - 1].flags & G_DQUAD) && tile_of(F, p[k - 1].A, &ia, &ja)) p0 = ja;
      CHECK((p0 < j) == (q.pre0 != nullptr), "%s: diagonal problem %d waits for %s quadrants", what, k, q.pre0 ? "no" : "its");
      out.push_back({true, j - o, p0 - o, 0, 0});
      continue;
    }
    if (q.flags & G_PANEL) {   // the step's panel (or the augmented row's), agreeing with the last factor entry
      CHECK(!out.empty() && out.back().factor, "%s: panel problem %d before its diagonal tile", what, k);
      if (out.empty()) continue;
      const int t = out.back().a + o, p0 = out.back().b + o;
      bool ok = q.flag == F.flags + t && q.X == F.B + ((long long)t * TILE * (F.ld + 1)) && q.Ld == F.A + (q.X - F.B);
      if (tile_of(F, q.C, &i, &j)) {
        ok = ok && j == t && i == t + 1 && q.mt == NB - t - 1 && q.nt == 1;
        if (q.flags & G_PHALF0)
          ok = ok && q.K == (t - p0) * TILE &&
               (q.K == 0 ? !q.A && !q.B
                         : tile_of(F, q.A, &ia, &ja) && ia == t + 1 && ja == p0 && tile_of(F, q.B, &ib, &jb) && ib == t && jb == p0);
      } else {
        ok = ok && aug && atile_of(F, q.C, &j) && j == t && q.mt == 1 && q.nt == 1;
        if (q.flags & G_PHALF0)
          ok = ok && q.K == (t - p0) * TILE &&
               (q.K == 0 ? !q.A && !q.B : atile_of(F, q.A, &ja) && ja == p0 && tile_of(F, q.B, &ib, &jb) && ib == t && jb == p0);
      }
      if (q.flags & G_PHALF1) ok = ok && q.K == 0 && !q.A && !q.B;
      CHECK(ok, "%s: panel problem %d of step %d", what, k, t);
      continue;
    }
    // the bulk: a lower-triangular block of columns [a, b), then the rows under it, then the augmented row's tiles
    if (q.flags & G_CLOWER) {
      CHECK(tile_of(F, q.C, &i, &j) && i == j && q.nt == q.mt && tile_of(F, q.A, &ia, &ja) && ia == i && q.B == q.A &&
                q.K > 0 && q.K % TILE == 0 && q.alpha == -1.0 && q.beta == 1.0,
            "%s: bulk problem %d", what, k);
      out.push_back({false, j - o, j + q.mt - o, ja - o, q.K / TILE});
      continue;
    }
    CHECK(!out.empty() && !out.back().factor && q.flags == 0, "%s: problem %d is neither chain nor bulk", what, k);
    if (out.empty() || out.back().factor) continue;
    const Entry& e = out.back();
    const int a = e.a + o, b = e.b + o, g0 = e.g0 + o;
    if (tile_of(F, q.C, &i, &j))
      CHECK(i == b && j == a && q.mt == NB - b && q.nt == b - a && q.K == e.k * TILE && tile_of(F, q.A, &ia, &ja) && ia == b &&
                ja == g0 && tile_of(F, q.B, &ib, &jb) && ib == a && jb == g0 && b < NB,
            "%s: rows under bulk problem %d", what, k);
    else
      CHECK(aug && atile_of(F, q.C, &j) && j == a && q.mt == 1 && q.nt == b - a && q.K == e.k * TILE &&
                atile_of(F, q.A, &ja) && ja == g0 && tile_of(F, q.B, &ib, &jb) && ib == a && jb == g0,
            "%s: augmented row of bulk problem %d", what, k);
  }
  return out;
}

// tests/test_chol_split_schedule.py's check as it stood: every column < NC factored once, in
// order, having received each earlier column exactly once, each from a column factored before;
// nothing written at or past column NC.
static void check_coverage(const std::vector<std::vector<Entry>>& launches, int NC, const char* what) {
  std::vector<int> got((size_t)NC * NC, 0);   // got[j NC + i]: updates of column j by column i
  int done = 0;                               // columns [0, done) are factored
  bool ok = true;
  for (const auto& launch : launches)
    for (const Entry& e : launch) {
      if (e.factor) {
        const int t = e.a, p0 = e.b;
        ok = ok && t == done && t < NC && 0 <= p0 && p0 <= t;
        if (!ok) break;
        for (int i = p0; i < t; ++i) ++got[(size_t)t * NC + i];
        for (int i = 0; i < t; ++i) ok = ok && got[(size_t)t * NC + i] == 1;
        ++done;
      } else {
        ok = ok && done <= e.a && e.a < e.b && e.b <= NC;              // columns not yet factored, below NC
        ok = ok && 0 <= e.g0 && e.k > 0 && e.g0 + e.k <= done;         // sources already factored
        if (!ok) break;
        for (int j = e.a; j < e.b; ++j)
          for (int i = e.g0; i < e.g0 + e.k; ++i) ++got[(size_t)j * NC + i];
      }
    }
  ok = ok && done == NC;
  for (int j = 0; j < NC && ok; ++j)
    for (int i = 0; i < NC; ++i) ok = ok && got[(size_t)j * NC + i] == (i < j ? 1 : 0);
  CHECK(ok, "%s: coverage of %d columns (%d factored)", what, NC, done);
}

// the launches of columns [o, o + NC) of one index vector, decoded
static std::vector<std::vector<Entry>> sweep_launches(const Plan& pl, const FactBufs& F, const std::vector<int>& idx, int o,
                                                      int NC, bool aug, const char* what) {
  std::vector<std::vector<Entry>> out;
  for (int t = o; t < o + NC; ++t) {
    if (idx[t] < 0) continue;
    const GemmLaunch& L = pl.launches[idx[t]];
    CHECK(L.kind == GEMM_FUSED && L.ticket == F.flags + 3 * F.NB + t, "%s: launch of column %d", what, t);
    out.push_back(decode(F, pl.probs.data() + L.first, L.count, o, aug, what));
  }
  return out;
}

// ---- b. wait safety: the stored list of a launch with a ticket names every tile once, no tile
// waits on a later one, and every counter is awaited for as many tiles as post it
static void check_waits(const Plan& pl, const GemmLaunch& L, const char* what, int li) {
  const GemmProb* p = pl.probs.data() + L.first;
  CHECK(L.list >= 0 && L.list + L.tiles <= (long long)pl.tiles.size(), "%s: launch %d has a ticket and no list", what, li);
  if (L.list < 0) return;
  const std::vector<unsigned> order(pl.tiles.begin() + L.list, pl.tiles.begin() + L.list + L.tiles);
  int total = 0;
  std::map<const int*, int> posts;
  for (int k = 0; k < L.count; ++k) {
    total += prob_tiles(p[k]);
    if (p[k].post) posts[p[k].post] += prob_tiles(p[k]);
    if (p[k].cpost) posts[p[k].cpost] += prob_tiles(p[k]);
  }
  std::vector<char> seen((size_t)total, 0);   // by tile_begin + ti nt + tj (ti mt + tj covers a lower triangle too)
  bool named = (int)order.size() == total;
  for (unsigned code : order) {
    const int k = (int)(code >> 24), ti = (int)((code >> 12) & 0xfff), tj = (int)(code & 0xfff);
    named = named && k < L.count && ti < p[k].mt && tj < p[k].nt && (!(p[k].flags & G_CLOWER) || tj <= ti);
    if (!named) break;
    const int at = p[k].tile_begin + ((p[k].flags & G_CLOWER) ? ti * (ti + 1) / 2 + tj : ti * p[k].nt + tj);
    named = at < total && !seen[at];
    if (named) seen[at] = 1;
  }
  CHECK(named, "%s: the list of launch %d is not its %d tiles once each", what, li, total);
  if (!named) return;
  CHECK(waits_point_back(p, order), "%s: a tile of launch %d waits on a later one", what, li);
  for (int k = 0; k < L.count; ++k) {
    CHECK(!p[k].pre0 || posts[p[k].pre0] == p[k].pre0_n, "%s: launch %d problem %d awaits %d of %d posts (pre0)", what, li, k,
          p[k].pre0_n, posts[p[k].pre0]);
    CHECK(!p[k].pre1 || posts[p[k].pre1] == p[k].pre1_n, "%s: launch %d problem %d awaits %d of %d posts (pre1)", what, li, k,
          p[k].pre1_n, posts[p[k].pre1]);
    CHECK(p[k].pre0 || p[k].pre0_n == 0, "%s: launch %d problem %d counts without a counter", what, li, k);
    CHECK(p[k].pre1 || p[k].pre1_n == 0, "%s: launch %d problem %d counts without a counter", what, li, k);
  }
}

static void print_entries(const char* tag, int cfg, int NB, int NC, int NR, bool grp, const std::vector<std::vector<Entry>>& ls) {
  std::printf("%s %d %d %d %d %d", tag, cfg, NB, NC, NR, (int)grp);
  for (const auto& l : ls) {
    std::printf(" |");
    for (const Entry& e : l) {
      if (e.factor) std::printf(" F %d %d", e.a, e.b);
      else std::printf(" B %d %d %d %d", e.a, e.b, e.g0, e.k);
    }
  }
  std::printf("\n");
}

// NB = 8 ... 130 and every configuration: the three sweeps (h, NB), (NB - h, NB - h), (NB, NB)
// and the nested split's (q, NB), (h - q, NB - q), per step and by groups, with and without the
// augmented row (a.), and every launch with a ticket (b.)
static void check_config(const CholSchedParams& P, int ci, bool emit) {
  for (int NB = 8; NB <= NB_MAX; ++NB)
    // a workspace with the row builds the launches without it as well; one without, the same
    // launches again: checked for the default configuration (and the one emitted)
    for (int aug = (ci == 0 || emit) ? 0 : 1; aug < (emit ? 1 : 2); ++aug) {
      const FactBufs F = workspace(NB, aug != 0);
      const int h = split_col(NB, 0), q = nest_col(NB, h, 0);
      Plan pl;
      char what[96];
      std::snprintf(what, sizeof what, "config %d NB %d aug %d", ci, NB, aug);
      CHECK(build_chol_plan(pl, F, P, h, q, NO_LIMIT), "%s: internal error", what);
      CHECK(pl.split_h == h && pl.split_q == q && h > 0 && (q > 0) == (h % 4 == 0) && pl.sides, "%s: h %d q %d", what,
            pl.split_h, pl.split_q);
      if (pl.split_h != h || pl.split_q != q) continue;
      struct Sw { SweepKind kind; int o, NC; };
      std::vector<Sw> sweeps = {{SWEEP_SPLIT, 0, h}, {SWEEP_SPLIT, h, NB - h}, {SWEEP_WHOLE, 0, NB}};
      if (q) {
        sweeps.push_back({SWEEP_NESTED, 0, q});
        sweeps.push_back({SWEEP_NESTED, q, h - q});
      }
      for (int va = 0; va <= aug; ++va)
        for (int g = 0; g < 2; ++g) {
          for (int t = h; t < NB && q; ++t)   // the nested table's columns [h, NB) are the split table's
            CHECK(pl.steps(SWEEP_NESTED, g, va)[t] == pl.steps(SWEEP_SPLIT, g, va)[t], "%s: nested column %d", what, t);
          for (const Sw& s : sweeps) {
            const auto ls = sweep_launches(pl, F, pl.steps(s.kind, g, va), s.o, s.NC, va != 0, what);
            check_coverage(ls, s.NC, what);
            if (emit && va == 0) print_entries("SWEEP", ci, NB, s.NC, NB - s.o, g != 0, ls);
          }
        }
      if (emit) continue;
      for (size_t li = 0; li < pl.launches.size(); ++li)
        if (pl.launches[li].ticket) check_waits(pl, pl.launches[li], what, (int)li);
        else CHECK(pl.launches[li].kind != GEMM_FUSED, "%s: fused launch %zu without a ticket", what, li);
    }
}

static void check_range() {
  const std::vector<CholSchedParams> cfgs = coverage_configs();
  std::atomic<size_t> next{0};   // the configurations are independent: dealt over a few threads
  std::vector<std::thread> pool;
  for (unsigned w = 0; w < std::max(1u, std::min((unsigned)cfgs.size(), std::thread::hardware_concurrency())); ++w)
    pool.emplace_back([&] {
      for (size_t ci = next++; ci < cfgs.size(); ci = next++) check_config(cfgs[ci], (int)ci, false);
    });
  for (std::thread& t : pool) t.join();
}

// ---- d. (and c.) the digest of a plan: FNV-1a over the normalised descriptors, the tile array, every launch
// record, the index table and the scalar fields.  "Normalised": every pointer field of GemmProb
// and the launch's ticket enters as (buffer id, byte offset), so the value does not depend on
// where the buffers live.  GemmProb's pointer fields, from the struct definition (the size is
// asserted so that a new field cannot be missed): A B C X Ld logdet flag pre0 pre1 post cpost
// part tcnt.
struct DigBuf { const void* base; size_t bytes; };   // ids 1..: A, B, Faug, flags, logdet, part, tcnt
struct Fnv {
  uint64_t h = 1469598103934665603ull;
  int stray = 0;   // pointers into none of the buffers
  void bytes(const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  }
  template <class T> void pod(const T& v) { bytes(&v, sizeof(T)); }
  void ptr(const void* p, const std::vector<DigBuf>& bufs) {
    uint64_t id = 0, off = 0;
    if (p) {
      id = 255;
      for (size_t i = 0; i < bufs.size(); ++i) {
        const char* b = (const char*)bufs[i].base;
        if (b && (const char*)p >= b && (const char*)p < b + bufs[i].bytes) {
          id = i + 1;
          off = (uint64_t)((const char*)p - b);
          break;
        }
      }
      if (id == 255) ++stray;
    }
    pod(id);
    pod(off);
  }
  void ints(const std::vector<int>& v) {
    pod((uint64_t)v.size());
    for (int x : v) pod(x);
  }
};
static_assert(sizeof(GemmProb) == 216, "GemmProb changed: revisit the pointer fields below");
static uint64_t plan_digest(const Plan& pl, const FactBufs& F, int* stray = nullptr) {
  const size_t nn = (size_t)F.ld;
  const std::vector<DigBuf> bufs = {{F.A, nn * nn * 8}, {F.B, nn * nn * 8}, {F.Faug, F.Faug ? nn * TILE * 8 : 0},
                                    {F.flags, FACT_FLAG_INTS * (size_t)F.NB * 4}, {F.logdet, (size_t)F.NB * 8},
                                    {F.part, (size_t)SPLIT_SLOTS * TILE * TILE * 8}, {F.tcnt, (size_t)SPLIT_SLOTS * 4}};
  Fnv f;
  f.pod((uint64_t)pl.probs.size());
  for (const GemmProb& p : pl.probs) {
    GemmProb z = p;
    f.ptr(p.A, bufs); f.ptr(p.B, bufs); f.ptr(p.C, bufs); f.ptr(p.X, bufs); f.ptr(p.Ld, bufs);
    f.ptr(p.logdet, bufs); f.ptr(p.flag, bufs); f.ptr(p.pre0, bufs); f.ptr(p.pre1, bufs);
    f.ptr(p.post, bufs); f.ptr(p.cpost, bufs); f.ptr(p.part, bufs); f.ptr(p.tcnt, bufs);
    z.A = z.B = nullptr; z.C = z.X = nullptr; z.Ld = nullptr; z.logdet = nullptr;
    z.flag = z.pre0 = z.pre1 = z.post = z.cpost = nullptr; z.part = nullptr; z.tcnt = nullptr;
    f.bytes(&z, sizeof(z));   // every other byte, padding included
  }
  f.pod((uint64_t)pl.tiles.size());
  f.bytes(pl.tiles.data(), pl.tiles.size() * sizeof(unsigned));
  f.pod((uint64_t)pl.launches.size());
  for (const GemmLaunch& L : pl.launches) {
    f.pod((int)L.kind); f.pod(L.first); f.pod(L.count); f.pod(L.tiles); f.pod(L.list); f.pod((int)L.cdef);
    f.ptr(L.ticket, bufs);
    f.pod(L.flops);
  }
  for (int s = 0; s < 3; ++s)   // [whole, split, nested] x [per step, group] x [plain, augmented]
    for (int g = 0; g < 2; ++g)
      for (int a = 0; a < 2; ++a) f.ints(pl.idx[s][g][a]);
  f.pod(pl.n_pad); f.pod(pl.lauum); f.pod((int)pl.aug); f.pod(pl.split_h); f.pod(pl.aug_mid); f.pod(pl.split_q);
  f.pod(pl.aug_q); f.pod((int)pl.sides);
  f.ints(pl.trtri);
  f.pod((uint64_t)pl.tri_pairs.size());
  for (const auto& lv : pl.tri_pairs) {
    f.pod((uint64_t)lv.size());
    for (const auto& pr : lv) f.bytes(pr.data(), sizeof(int) * 3);
  }
  f.pod((uint64_t)pl.trtri_side.size());
  for (const auto& sd : pl.trtri_side) f.bytes(sd.data(), sizeof(int) * 4);
  if (stray) *stray = f.stray;
  return f.h;
}

// ---- c. the rollback
static bool same_plan(const Plan& a, const Plan& b, const FactBufs& F) {
  bool same = a.n_pad == b.n_pad && a.a_ptr == b.a_ptr && a.b_ptr == b.b_ptr && a.trtri == b.trtri &&
              a.tri_pairs == b.tri_pairs && a.lauum == b.lauum && a.aug == b.aug && a.split_h == b.split_h &&
              a.aug_mid == b.aug_mid && a.split_q == b.split_q && a.aug_q == b.aug_q && a.sides == b.sides &&
              a.trtri_side == b.trtri_side && a.tiles == b.tiles && a.probs.size() == b.probs.size() &&
              a.launches.size() == b.launches.size();
  for (int s = 0; s < 3; ++s)
    for (int g = 0; g < 2; ++g)
      for (int v = 0; v < 2; ++v) same = same && a.idx[s][g][v] == b.idx[s][g][v];
  if (!same) return false;
  if (!a.probs.empty() && std::memcmp(a.probs.data(), b.probs.data(), a.probs.size() * sizeof(GemmProb))) return false;
  for (size_t i = 0; i < a.launches.size(); ++i) {
    const GemmLaunch &x = a.launches[i], &y = b.launches[i];
    same = same && x.kind == y.kind && x.first == y.first && x.count == y.count && x.tiles == y.tiles &&
           std::memcmp(&x.flops, &y.flops, sizeof(double)) == 0 && x.list == y.list && x.cdef == y.cdef && x.ticket == y.ticket;
  }
  return same && plan_digest(a, F) == plan_digest(b, F);
}

static void check_rollback() {
  const CholSchedParams P;
  for (int NB : {8, 13, 23, 40})
    for (int aug = 0; aug < 2; ++aug) {
      const FactBufs F = workspace(NB, aug != 0);
      const int h = split_col(NB, 0), q = nest_col(NB, h, 0);
      Plan whole, split, full, got;
      CHECK(build_chol_plan(whole, F, P, 0, 0, NO_LIMIT) && build_chol_plan(split, F, P, h, 0, NO_LIMIT) &&
                build_chol_plan(full, F, P, h, q, NO_LIMIT),
            "NB %d: internal error", NB);
      CHECK(h && q && split.split_h == h && split.sides && !split.split_q && full.split_q == q && !whole.split_h, "NB %d", NB);
      // the split sweep does not fit: the whole plan, whatever q asks for
      CHECK(build_chol_plan(got, F, P, h, q, (int)whole.probs.size()) && same_plan(got, whole, F), "NB %d aug %d: split left out",
            NB, aug);
      // the nested split does not fit: the plan built without it
      CHECK(build_chol_plan(got, F, P, h, q, (int)split.probs.size()) && same_plan(got, split, F), "NB %d aug %d: nesting left out",
            NB, aug);
      CHECK(build_chol_plan(got, F, P, h, q, (int)full.probs.size()) && same_plan(got, full, F), "NB %d aug %d: all fits", NB, aug);
      // the TRTRI by sides does not fit (nor then the nested split, built after it): the plan
      // without it is the split plan cut off before the first side's launch
      int first = -1;
      for (const auto& sd : split.trtri_side)
        for (int l : sd)
          if (l >= 0 && (first < 0 || l < first)) first = l;
      CHECK(first > 0, "NB %d: no launch by side", NB);
      if (first <= 0) continue;
      Plan want = split;
      size_t nt = split.tiles.size();
      for (size_t l = split.launches.size(); l-- > (size_t)first;)
        if (split.launches[l].list >= 0) nt = (size_t)split.launches[l].list;
      want.tiles.resize(nt);
      want.probs.resize(split.launches[first].first);
      want.launches.resize(first);
      want.sides = false;
      want.trtri_side.clear();
      CHECK(build_chol_plan(got, F, P, h, q, (int)want.probs.size()) && same_plan(got, want, F) && got.split_h == h,
            "NB %d aug %d: sides left out", NB, aug);
    }
}

// ---- d. pinned configurations
struct Config { const char* name; int NB; bool aug; int chol_min, nest_min; bool tr; CholSchedParams P; };
// descriptor slots of the training workspace's plan and of the gpe_cholesky workspace's (gpemu.hip)
constexpr int LIMIT_TR = 1 << 15, LIMIT_AUX = (1 << 16) - 64 - (1 << 15);
static std::vector<Config> pinned_configs() {
  const CholSchedParams def;
  return {
      // tests/test_gpu_ozaki_chol_nest.py's shapes with its floors (256 rows each): split and nested, NB 9 whole
      {"nb8", 8, true, 256, 256, true, def},
      {"nb11", 11, true, 256, 256, true, def},
      {"nb23", 23, true, 256, 256, true, def},
      {"nb9", 9, true, 256, 256, true, def},
      {"nb13", 13, true, 256, 256, true, def},
      // the benchmark's size with the defaults (h 64, q 32), and with the per-step schedule only
      {"nb128", 128, true, 8192, 12288, true, def},
      {"nb128_fused", 128, true, 8192, 12288, true, params(def.groups, def.sb, def.sb_min, false)},
      // GPEMU_POTRF_W=8:0 GPEMU_POTRF_SB=3:0 at those floors
      {"nb23_w8_sb3", 23, true, 256, 256, true, params({{8, 0}}, 3, 0)},
      // the gpe_cholesky workspace: no augmented row, never split
      {"nb5_aux", 5, false, 0, 0, false, def},
  };
}
struct Pinned { std::string name; uint64_t digest; size_t probs, tiles, launches; };
static std::vector<Pinned> pinned_now() {
  std::vector<Pinned> out;
  for (const Config& c : pinned_configs()) {
    const FactBufs F = workspace(c.NB, c.aug);
    const int h = c.tr ? split_col(c.NB, c.chol_min) : 0, q = h ? nest_col(c.NB, h, c.nest_min) : 0;
    Plan pl;
    int stray = 0;
    CHECK(build_chol_plan(pl, F, c.P, h, q, c.tr ? LIMIT_TR : LIMIT_AUX), "%s: internal error", c.name);
    const uint64_t d = plan_digest(pl, F, &stray);
    CHECK(stray == 0, "%s: %d pointers outside the workspace", c.name, stray);
    CHECK(pl.split_h == h && pl.split_q == q && (int)pl.probs.size() <= (c.tr ? LIMIT_TR : LIMIT_AUX), "%s: h %d q %d", c.name,
          pl.split_h, pl.split_q);
    out.push_back({c.name, d, pl.probs.size(), pl.tiles.size(), pl.launches.size()});
  }
  return out;
}

// The digests of the plans build_plan built at 3f64e65, the commit before the builder moved here:
// printed there (the same digest function over its Plan, before the upload) by one small
// objective, or one gpe_cholesky for nb5_aux, per configuration on an MI355X.
static const Pinned PINNED[] = {
    {"nb8", 0xda154017da9923e2ull, 245, 877, 57},
    {"nb11", 0xc3529c9d8954225cull, 403, 1994, 81},
    {"nb23", 0x9c4445f61563c14cull, 899, 12374, 151},
    {"nb9", 0x40030178f4092766ull, 122, 536, 27},
    {"nb13", 0xa8fc063b2d95de52ull, 463, 2734, 91},
    {"nb128", 0x64dab57134d71cdcull, 9755, 681114, 841},
    {"nb128_fused", 0xb7b8977263dc5276ull, 5817, 363065, 681},
    {"nb23_w8_sb3", 0xee9565ad2b0cc419ull, 1505, 9837, 167},
    {"nb5_aux", 0x76663d3f1e7282e2ull, 29, 75, 12},
};

static void check_pinned() {
  const std::vector<Pinned> now = pinned_now();
  const size_t n = sizeof(PINNED) / sizeof(PINNED[0]);
  CHECK(now.size() == n, "%zu pinned configurations", now.size());
  for (size_t i = 0; i < now.size() && i < n; ++i)
    CHECK(now[i].name == PINNED[i].name && now[i].digest == PINNED[i].digest && now[i].probs == PINNED[i].probs &&
              now[i].tiles == PINNED[i].tiles && now[i].launches == PINNED[i].launches,
          "%s: digest %016llx over %zu descriptors, %zu tiles, %zu launches", now[i].name.c_str(),
          (unsigned long long)now[i].digest, now[i].probs, now[i].tiles, now[i].launches);
}

int main(int argc, char** argv) {
  reserve_workspace();
  const std::string opt = argc > 1 ? argv[1] : "";
  if (opt == "--digests") {
    for (const Pinned& p : pinned_now())
      std::printf("    {\"%s\", 0x%016llxull, %zu, %zu, %zu},\n", p.name.c_str(), (unsigned long long)p.digest, p.probs, p.tiles,
                  p.launches);
    return g_fail ? 1 : 0;
  }
  if (opt == "--emit") {   // --emit CONFIG: one configuration of coverage_configs()
    const std::vector<CholSchedParams> cfgs = coverage_configs();
    const int ci = argc > 2 ? std::atoi(argv[2]) : -1;
    if (ci < 0 || ci >= (int)cfgs.size()) return 2;
    check_config(cfgs[ci], ci, true);
    return g_fail ? 1 : 0;
  }
  check_range();
  check_rollback();
  check_pinned();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail.load());
    return 1;
  }
  std::printf("chol_sched_check OK\n");
  return 0;
}
