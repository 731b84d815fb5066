// gpemu_gemm_sched.hpp -- host side of the grouped GEMM (k_gemm, gpemu_kernels.hpp): which
// instance a launch takes, the launch record, the descriptors of one launch, split K, the
// XCD-aware tile order and the one place that issues k_gemm.  The single-GPU schedules
// (gpemu_chol_sched.hpp, gpemu.hip) and the row-block ones (gpemu_dist.hip) are both assembled from these;
// tests/host/gemm_sched_check.cpp checks them without a GPU.
#pragma once

#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "gpemu_kernels.hpp"

namespace gpe {

// The k_gemm instance of a launch.  The values 0..3 are ABI: gpe_test_gemm_group takes them.
enum GemmKind : int {
  GEMM_PLAIN = 0,   // <AK=0, BK=0>
  GEMM_AK = 1,      // <1, 0>
  GEMM_AK_BK = 2,   // <1, 1>
  GEMM_BK = 3,      // <0, 1>
  GEMM_FUSED = 4,   // <0, 0, FUSED>: the only instance whose problems may be G_DIAG / G_DQUAD / G_PANEL
};
struct GemmInstance { bool ak, bk, fused; };
constexpr GemmInstance gemm_instance(GemmKind k) {
  return {k == GEMM_AK || k == GEMM_AK_BK, k == GEMM_BK || k == GEMM_AK_BK, k == GEMM_FUSED};
}
constexpr GemmKind gemm_kind(bool ak, bool bk) { return ak ? (bk ? GEMM_AK_BK : GEMM_AK) : (bk ? GEMM_BK : GEMM_PLAIN); }

struct GemmLaunch {       // one grouped GEMM launch
  GemmKind kind = GEMM_PLAIN;
  int first = 0, count = 0;   // descriptor range
  int tiles = 0;              // workgroups
  double flops = 0.0;         // algorithmic flops (profiling)
  long long list = -1;        // offset of its tile list in the device list array (-1: implicit order)
  bool cdef = false;          // k_gemm's CDEF instance
  int* ticket = nullptr;      // fused launches with in-launch waits: list positions claimed by ticket (k_gemm)
};

inline GemmProb mkprob(const double* A, long long lda, const double* B, long long ldb, double* C, long long ldc,
                       int mt, int nt, int K, int flags, double alpha, double beta) {
  GemmProb p;
  std::memset(&p, 0, sizeof(p));   // (padding too: descriptors are compared and hashed as bytes)
  p.A = A; p.B = B; p.C = C;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.mt = mt; p.nt = nt; p.K = K; p.flags = flags;
  p.alpha = alpha; p.beta = beta;
  p.ksplit = 1;
  p.kti_mul = 1;
  return p;
}

// Tiles (workgroups) of a problem.  A G_CLOWER problem is square in tiles, mt x mt: here and
// in order_tiles its nt is not read, while list_launch keeps tj < nt as well.
inline int prob_tiles(const GemmProb& p) {
  return ((p.flags & G_CLOWER) ? p.mt * (p.mt + 1) / 2 : p.mt * p.nt) * std::max(1, p.ksplit);
}

inline unsigned tile_code(int p, int ti, int tj) { return ((unsigned)p << 24) | ((unsigned)ti << 12) | (unsigned)tj; }

// ---- the descriptors of one launch.  begin_launch, then push_prob for each problem (they
// follow each other in probs), then set_list where the launch has a tile list.  That keeps
// what k_gemm needs without a list: tile_begin non-decreasing over the problems and
// covering [0, tiles).
inline GemmLaunch begin_launch(GemmKind kind, const std::vector<GemmProb>& probs, double flops = 0.0) {
  GemmLaunch L;
  L.kind = kind;
  L.first = (int)probs.size();
  L.flops = flops;
  return L;
}

// cdef_ok: the launch takes the CDEF instance when this problem asks for it (gemm_cdef).
// The instance changes speed, not results, and stays each site's choice.
inline void push_prob(GemmLaunch& L, std::vector<GemmProb>& probs, GemmProb p, bool cdef_ok) {
  p.tile_begin = L.tiles;
  p.ntiles = prob_tiles(p);
  L.tiles += p.ntiles;
  ++L.count;
  L.cdef = L.cdef || (cdef_ok && gemm_cdef(p));
  probs.push_back(p);
}

// the launch runs the tiles of order (codes p << 24 | ti << 12 | tj, p counted from L.first)
inline void set_list(GemmLaunch& L, std::vector<unsigned>& tiles, const std::vector<unsigned>& order) {
  L.list = (long long)tiles.size();
  L.tiles = (int)order.size();
  tiles.insert(tiles.end(), order.begin(), order.end());
}

// Split K over workgroups for a launch with few tiles (small n, the TRTRI's first levels):
// there each tile's K loop on one CU is the launch's latency, and the chip has 512
// workgroup slots.  ks shares of at least 64 K each, at most SPLIT_SLOTS partials; beta = 0
// problems only.  The launch then takes the implicit tile order (no list).  t_all, k_all: decide
// as for a launch of that many tiles and that longest K (a TRTRI level's launch dealt over two:
// every tile then sums in the shares it has in the whole level's launch, bit for bit).
constexpr int SPLIT_SLOTS = 512;
inline void split_k(std::vector<GemmProb>& probs, double* part, int* tcnt, int t_all = 0, int k_all = 0) {
#ifdef GPE_NO_SPLITK   // dev A/B build (tools/ab_libs.sh)
  return;
#endif
  int T = 0, kmax = 0;
  for (const GemmProb& p : probs) {
    if (p.beta != 0.0 || p.ksplit > 1) return;
    T += prob_tiles(p);
    kmax = std::max(kmax, p.K);
  }
  if (t_all > 0) { T = t_all; kmax = k_all; }
  if (T <= 0 || T >= 256) return;
  // shares of at least 64 of K (4 stages): one 128 x 128 x 128 tile is ~16 us of fp64
  // MFMA on one CU, the first TRTRI level's whole launch
  const int ks = std::min({8, SPLIT_SLOTS / T, kmax / 64});
  if (ks < 2) return;
  int off = 0;
  for (GemmProb& p : probs) {
    const int tl = prob_tiles(p);
    p.ksplit = ks;
    p.part = part + (size_t)off * ks * TILE * TILE;
    p.tcnt = tcnt + off;
    off += tl;
  }
}

// XCD-aware order of the given tiles of a launch: rows (problem, ti) -- one A panel each --
// longest tiles first, greedily packed into 8 bins of equal work, the bins interleaved tile
// by tile.  Under round-robin dispatch each row's tiles then run on one XCD and its A panel
// stays in that XCD's L2: in implicit order (ti fastest) every XCD streams every panel, and
// a K = 8192 TRTRI level ran 2.7x over its MFMA time.
// Every code names a tile of its problem (ti < mt).  placed: tiles the caller puts elsewhere
// in the list; they weigh in the packing and are left out of the result.
inline std::vector<unsigned> xcd_order(const GemmProb* probs, const std::vector<unsigned>& tiles,
                                       const std::vector<unsigned>& placed = {}) {
  struct Row { double tw = 0.0; int at = 0, n = 0; };   // its tiles: by[at .. at + n)
  int np = 0;
  for (unsigned code : tiles) np = std::max(np, (int)(code >> 24) + 1);
  std::vector<int> row0(np + 1, 0);   // rows in (p, ti) order: problem p's start at row0[p]
  for (int p = 0; p < np; ++p) row0[p + 1] = row0[p] + std::max(probs[p].mt, 0);
  std::vector<Row> rows(row0[np]);
  const auto row_of = [&](unsigned code) -> Row& { return rows[row0[code >> 24] + ((code >> 12) & 0xfff)]; };
  for (unsigned code : tiles) ++row_of(code).n;
  std::vector<const Row*> order;
  int at = 0;
  for (int p = 0; p < np; ++p)
    for (int ti = 0; ti < probs[p].mt; ++ti) {
      Row& r = rows[row0[p] + ti];
      if (r.n == 0) continue;
      const GemmProb& P = probs[p];
      int kb = 0, ke = P.K;
      if (P.flags & G_KBEG_TI) kb = ti * TILE;
      if (P.flags & G_KEND_TI) ke = std::min(ke, (ti * P.kti_mul + P.kti_off + 1) * TILE);
      r.tw = (double)std::max(ke - kb, 0) + 2.0 * GK;   // + fixed per-tile cost
      r.at = at;
      at += r.n;
      r.n = 0;
      order.push_back(&r);
    }
  std::vector<unsigned> by(tiles.size());   // the tiles row by row, each row's in the order given
  for (unsigned code : tiles) {
    Row& r = row_of(code);
    by[r.at + r.n++] = code;
  }
  std::stable_sort(order.begin(), order.end(), [](const Row* a, const Row* b) { return a->tw > b->tw; });
  constexpr int NX = 8;
  std::vector<std::vector<unsigned>> bins(NX);
  std::vector<double> load(NX, 0.0);
  for (const Row* r : order) {
    const int x = (int)(std::min_element(load.begin(), load.end()) - load.begin());
    load[x] += r->tw * r->n;
    bins[x].insert(bins[x].end(), by.begin() + r->at, by.begin() + r->at + r->n);
  }
  for (unsigned code : placed)
    for (auto& b : bins) b.erase(std::remove(b.begin(), b.end(), code), b.end());
  std::vector<unsigned> out;
  out.reserve(tiles.size());
  size_t longest = 0;
  for (auto& b : bins) longest = std::max(longest, b.size());
  for (size_t j = 0; j < longest; ++j)
    for (int x = 0; x < NX; ++x)
      if (j < bins[x].size()) out.push_back(bins[x][j]);
  return out;
}

// The tile order of a whole group: xcd_order, with the chain of a fused Cholesky step placed
// by hand.  A factored diagonal tile (G_DIAG, one tile) starts first, after the quadrants
// of its pending update (G_DQUAD, nt = 1); the G_PANEL tiles wait on the G_DIAG tile and are
// dispatched last.
inline std::vector<unsigned> order_tiles(const std::vector<GemmProb>& probs) {
  std::vector<unsigned> out, diag, bulk, tail;
  size_t total = 0;
  for (const GemmProb& P : probs) total += (size_t)prob_tiles(P);
  bulk.reserve(total);
  for (int p = 0; p < (int)probs.size(); ++p) {
    const GemmProb& P = probs[p];
    for (int ti = 0; ti < P.mt; ++ti)
      for (int tj = 0; tj <= ((P.flags & G_CLOWER) ? ti : P.nt - 1); ++tj) {
        const unsigned code = tile_code(p, ti, tj);
        if (P.flags & G_PANEL) {
          tail.push_back(code);
          continue;
        }
        bulk.push_back(code);
        if (P.flags & G_DQUAD) out.push_back(code);
        else if (P.flags & G_DIAG) diag.push_back(code);
      }
  }
  const size_t diag_at = out.size() + diag.size() - 1;   // the last G_DIAG tile (when there is one)
  out.insert(out.end(), diag.begin(), diag.end());
  const std::vector<unsigned> rest = xcd_order(probs.data(), bulk, out);
  out.insert(out.end(), rest.begin(), rest.end());
  // The launch starts on an idle GPU and its first 512 workgroups fill two slots per CU
  // in order: workgroup 256 + k lands on the CU of workgroup k, here the G_DIAG tile's
  // (tools/hip/placement_probe.hip: 256 of 256 pairs i, i - 256 share a CU).  Give
  // that slot the first panel tile: after its own update it waits on the flag and
  // leaves the SIMDs to the diagonal factorisation, which beside a bulk tile's MFMAs
  // runs ~1.7x slower.
  if (!diag.empty() && !tail.empty() && out.size() > diag_at + 256) {
    out.insert(out.begin() + diag_at + 256, tail.front());
    tail.erase(tail.begin());
  }
  out.insert(out.end(), tail.begin(), tail.end());
  return out;
}

// every tile of a plain launch's problems, XCD-ordered, as L's list (launches of more than
// 256 problems, which the list code cannot name, keep the implicit order)
inline void list_launch(GemmLaunch& L, const std::vector<GemmProb>& probs, std::vector<unsigned>& tiles) {
  if (L.count == 0 || L.count > 256) return;
  std::vector<unsigned> all;
  for (int p = 0; p < L.count; ++p) {
    const GemmProb& P = probs[L.first + p];
    for (int tj = 0; tj < P.nt; ++tj)
      for (int ti = 0; ti < P.mt; ++ti)
        if (!(P.flags & G_CLOWER) || tj <= ti) all.push_back(tile_code(p, ti, tj));
  }
  set_list(L, tiles, xcd_order(probs.data() + L.first, all));
}

// A fused launch's tiles take their list positions by ticket, so a tile may wait only on
// tiles before it in the list (then the earliest unfinished tile can always run): every
// counter a tile waits on (pre0, pre1) is last posted before it, and a G_PANEL tile follows
// the G_DIAG tile that releases its flag.  probs: the launch's own problems.
inline bool waits_point_back(const GemmProb* probs, const std::vector<unsigned>& order) {
  std::map<const int*, size_t> last_post, diag_at;
  for (size_t i = 0; i < order.size(); ++i) {
    const GemmProb& q = probs[order[i] >> 24];
    if (q.post) last_post[q.post] = i;
    if (q.cpost) last_post[q.cpost] = i;
    if (q.flags & G_DIAG) diag_at[q.flag] = i;
  }
  for (size_t i = 0; i < order.size(); ++i) {
    const GemmProb& q = probs[order[i] >> 24];
    const bool ok = (!q.pre0 || (last_post.count(q.pre0) && last_post[q.pre0] < i)) &&
                    (!q.pre1 || (last_post.count(q.pre1) && last_post[q.pre1] < i)) &&
                    (!(q.flags & G_PANEL) || (diag_at.count(q.flag) && diag_at[q.flag] < i));
    if (!ok) return false;
  }
  return true;
}

// Issue one launch: the only switch over kind x cdef.  probs_base / tiles_base: the device
// arrays L.first and L.list index.  (A template so that a host-only program that includes
// this header does not instantiate the kernels.)
template <GemmKind KIND, bool CDEF, class L>
inline void launch_k_gemm_as(const L& l, const GemmProb* probs_base, const unsigned* tiles_base, int* info,
                             hipStream_t st) {
  constexpr GemmInstance I = gemm_instance(KIND);
  hipLaunchKernelGGL((k_gemm<I.ak, I.bk, I.fused, CDEF>), dim3(l.tiles), dim3(256),
                     G_LDS_LAUNCH_DOUBLES * sizeof(double), st, probs_base + l.first, l.count,
                     l.list >= 0 ? tiles_base + l.list : nullptr, info, l.ticket);
}

template <class L>
inline hipError_t launch_k_gemm(const L& l, const GemmProb* probs_base, const unsigned* tiles_base, int* info,
                                hipStream_t st) {
  if (l.count == 0 || l.tiles == 0) return hipSuccess;
#define GPE_GEMM_CASE(KIND)                                                                    \
  case KIND:                                                                                   \
    if (l.cdef) launch_k_gemm_as<KIND, true>(l, probs_base, tiles_base, info, st);             \
    else launch_k_gemm_as<KIND, false>(l, probs_base, tiles_base, info, st);                   \
    break;
  switch (l.kind) {
    GPE_GEMM_CASE(GEMM_PLAIN)
    GPE_GEMM_CASE(GEMM_AK)
    GPE_GEMM_CASE(GEMM_AK_BK)
    GPE_GEMM_CASE(GEMM_BK)
    GPE_GEMM_CASE(GEMM_FUSED)
  }
#undef GPE_GEMM_CASE
  return hipGetLastError();
}

}  // namespace gpe
