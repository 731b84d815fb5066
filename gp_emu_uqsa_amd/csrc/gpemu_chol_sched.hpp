// gpemu_chol_sched.hpp -- the cached GEMM schedule of one factorisation workspace (Plan): the
// fused Cholesky's launches per step and per column group, whole, split and nested, the TRTRI
// by levels and by sides of the split column, and the LAUUM.  Host only and data-independent:
// plain arithmetic on tile indices and on pointers into the workspace's buffers, no HIP runtime
// call.  gpemu.hip's build_plan calls build_chol_plan and uploads the result;
// tests/host/chol_sched_check.cpp checks the same function without a GPU.
#pragma once

#include <algorithm>
#include <array>
#include <utility>
#include <vector>

#include "gpemu_gemm_sched.hpp"
#include "gpemu_ozaki.hpp"

namespace gpe {

// The sweeps a plan may hold.  SWEEP_SPLIT (Plan::split_h): columns [0, h) over all rows, the
// Schur complement S = A22 - L21 L21^T on the int8 cores, then chol(S).  SWEEP_NESTED
// (Plan::split_q): phase A split once more at q = h / 2.
enum SweepKind : int { SWEEP_WHOLE = 0, SWEEP_SPLIT = 1, SWEEP_NESTED = 2 };

// What an optional part of the plan may change besides the three arrays below: copied before
// the part is built and put back when its descriptors do not fit (optional_part).
struct PlanIndex {
  long long n_pad = 0;
  const double* a_ptr = nullptr;   // buffers the descriptors point into
  const double* b_ptr = nullptr;
  // The Cholesky's launches per column step: idx[sweep][group][aug][t], -1 for none.
  //   group 0, the per-step (fused) schedule: one launch per column block;
  //   group 1, the group schedule (the default for a lone evaluation; CholSchedParams::group:
  //     it is built): ONE launch per column group of width >= 2 holding its whole chain (diagonal
  //     and panel tiles of every step, handed on by counters in the flags) beside the previous
  //     group's trailing update, -1 for the later steps of a group; a width-1 group's entry is
  //     its per-step launch;
  //   aug 1 (aug: these are built): the same launches also carrying the augmented row.
  // SWEEP_SPLIT holds phase A in columns [0, h) and the Schur complement's own sweep in [h, NB);
  // SWEEP_NESTED the sweeps [0, q) over all rows and [q, h) over the rows from q, its columns
  // [h, NB) being SWEEP_SPLIT's.
  std::vector<int> idx[3][2][2];
  std::vector<int> trtri;   // launches in order
  // per TRTRI level (launches trtri[2 l], trtri[2 l + 1]): its block pairs {t0, h, t1}
  std::vector<std::vector<std::array<int, 3>>> tri_pairs;
  int lauum = -1;
  bool aug = false;
  // the split sweep: tile column h > 0 where the factorisation of the training matrix is split,
  // and the launch that updates the augmented row's tiles [h, NB) by the first h columns
  int split_h = 0, aug_mid = -1;
  // the nested split: tile column q = h / 2 > 0, and the launch that updates the augmented row's
  // tiles [q, h) by the first q columns
  int split_q = 0, aug_q = -1;
  // the TRTRI by sides of the split column (tri_ahead; sides: these are built): per level below
  // the top one its launch pairs {T^T, X21} of the block pairs inside [0, h), then of those
  // inside [h, NB) (-1: none)
  bool sides = false;
  std::vector<std::array<int, 4>> trtri_side;
};

struct Plan : PlanIndex {
  std::vector<GemmLaunch> launches;
  std::vector<GemmProb> probs;
  std::vector<unsigned> tiles;   // concatenated tile lists
  const std::vector<int>& steps(SweepKind sweep, bool group, bool with_aug) const { return idx[sweep][group][with_aug]; }
};

// How the fused Cholesky is cut into launches (gpe_create fills it from the environment).
struct CholSchedParams {
  // GPEMU_POTRF=group / auto: the group launches are built (fused: per-step launches only)
  bool group = true;
  // list positions of the chain steps in a group launch (GPEMU_GROUP_P0, GPEMU_GROUP_STRIDE)
  int grp_p0 = 512, grp_stride = 896;
  // column-group widths of the fused Cholesky: {width, min remaining columns}, first
  // match wins, else 1 (GPEMU_POTRF_W="4:64,2:32" style).  Round 4 (a shorter chain per
  // step): 4 while more than 48 columns remain, then 2 while more than 24 -- at n = 16384
  // the two-try bench 14.70 / 14.72 -> 14.78 / 14.81 evals/s and the Cholesky 28.4 -> 28.1 ms
  // against round 3's {4, 80}, {2, 40} (profiles/group_width_ab_r04.log)
  std::vector<std::pair<int, int>> groups = {{4, 48}, {2, 24}};
  // super-blocks of the fused Cholesky (lazy far updates): up to sb consecutive column
  // groups of one width >= 2 form a super-block; the columns beyond it receive its update
  // as ONE trailing update of K = 128 x its width, spread over the next super-block's
  // launches (1: every group updates the whole trailing matrix, K = 128 x its width), while
  // more than sb_min tile columns remain (GPEMU_POTRF_SB="groups:min_remaining")
  int sb = 2, sb_min = 80;
};

// The buffers the descriptors point into: the matrix A (K-build -> L -> A^-1) and B (Dinv tiles
// -> L^-1), both NB x NB tiles with leading dimension ld; the augmented tile row Faug (TILE x ld,
// ld TILE; null: the workspace has none); flags (FACT_FLAG_INTS x NB ints: the diagonal-inverse
// flags, the group schedule's column and panel counters, the list tickets of the Cholesky
// launches (one per column step), the diagonal tiles' quadrant counters (G_DQUAD) and the panel
// tiles' stored-update counters (G_PHALF0)); logdet (NB); the split-K scratch part / tcnt.
// Nothing here is dereferenced on the host.
constexpr int FACT_FLAG_INTS = 6;
struct FactBufs {
  double* A = nullptr;
  double* B = nullptr;
  double* Faug = nullptr;
  long long ld = 0;
  int NB = 0;
  int* flags = nullptr;
  double* logdet = nullptr;
  double* part = nullptr;
  int* tcnt = nullptr;
};

// One launch of the cached schedule from its problems: in order_tiles' order, or in the
// given one (codes into probs), or -- split K, 256 problems or more -- the implicit one.
inline void add_launch(Plan& pl, GemmKind kind, const std::vector<GemmProb>& probs, double flops,
                       const std::vector<unsigned>* order = nullptr) {
  GemmLaunch L = begin_launch(kind, pl.probs, flops);
  bool listable = probs.size() < 256;
  for (const GemmProb& p : probs) {
    push_prob(L, pl.probs, p, true);
    listable = listable && p.mt <= 4096 && p.nt <= 4096 && p.ksplit <= 1;
  }
  if (order) {
    set_list(L, pl.tiles, *order);
  } else if (listable) {
    const std::vector<unsigned> tl = order_tiles(probs);
    if ((int)tl.size() == L.tiles) set_list(L, pl.tiles, tl);
  }
  pl.launches.push_back(L);
}

// An optional part of the plan (the split sweep, the TRTRI by sides, the nested split) is left
// out when its descriptors would not fit: the plan is then, field for field, what it was before.
// part() returns false on an internal error, which is handed on.
template <class Part>
inline bool optional_part(Plan& pl, int limit, Part part) {
  const size_t nl = pl.launches.size(), np = pl.probs.size(), nt = pl.tiles.size();
  const PlanIndex before = pl;
  if (!part()) return false;
  if ((int)pl.probs.size() > limit) {
    pl.launches.resize(nl);
    pl.probs.resize(np);
    pl.tiles.resize(nt);
    static_cast<PlanIndex&>(pl) = before;
  }
  return true;
}

// ---- column bookkeeping of one sweep: NC tile columns of a sub-matrix with NR tile rows, in
// its own (local) tile columns.  Index data only: it knows nothing about pointers.
//
// Columns are grouped (widths from CholSchedParams::groups by the rows left, NR - column: wide
// groups while the trailing matrix is large, width 1 at the end).
// Super-blocks (lazy far updates).  Group 0 is a super-block of its own; after it, up to
// sb consecutive groups of one width >= 2 form one while more than sb_min
// columns remain (later groups, and width-1 groups, stay single: there the longer pending
// update of a super-block's first column lengthens a chain the bulk no longer hides).
// For group gi with columns [gb, ge) in super-block [sb, se):
//   src0[gi]: start of the columns whose update its own columns still lack when it starts
//     -- the previous super-block when gi opens its super-block, else the previous group;
//   its launches carry (bulk segments, balanced over its W launches):
//     the update by [src0, gb) of its later columns [gb+1, ge) (the column factored next),
//     the update by [src0, gb) of the rest of its super-block [ge, se),
//     a share of the previous super-block's update of the columns beyond [se, NC)
//     (K = 128 x the previous super-block's width: the long-K far update, each far tile
//     read and written once per super-block instead of once per group).
// Every column j still receives every earlier column's update before it is factored: a
// far column gets super-block s's update during super-block s + 1, before s + 2 opens.
struct Seg { int a, b, g0, K; };   // columns [a, b) updated by columns [g0, g0 + K / 128)
struct SweepCols {
  std::vector<int> gs;     // group starts, then NC
  std::vector<int> src0;   // per group
  std::vector<std::vector<Seg>> segs;                // the bulk segments of group gi
  std::vector<std::vector<std::vector<Seg>>> part;   // ... dealt over its steps: part[gi][h]
  int groups() const { return (int)gs.size() - 1; }
};

inline SweepCols sweep_columns(int NC, int NR, const CholSchedParams& P) {
  SweepCols sc;
  std::vector<int>& gs = sc.gs;
  for (int g = 0; g < NC;) {
    gs.push_back(g);
    int w = 1;
    for (const auto& r : P.groups)
      if (NR - g > r.second) { w = r.first; break; }
    g += std::max(1, std::min(w, NC - g));
  }
  gs.push_back(NC);
  const int ng = sc.groups();
  std::vector<int> sbs(ng), sbe(ng);
  std::vector<int>& src0 = sc.src0;
  src0.assign(ng, 0);
  {
    int cur = 0, cnt = 0;
    for (int gi = 0; gi < ng; ++gi) {
      const int w = gs[gi + 1] - gs[gi];
      const bool open = gi <= 1 || w < 2 || w != gs[gi] - gs[gi - 1] || cnt >= P.sb || NR - gs[gi] <= P.sb_min;
      if (open) { cur = gs[gi]; cnt = 0; }
      sbs[gi] = cur;
      ++cnt;
    }
    for (int gi = ng - 1; gi >= 0; --gi) sbe[gi] = (gi + 1 < ng && sbs[gi + 1] == sbs[gi]) ? sbe[gi + 1] : gs[gi + 1];
    for (int gi = 1; gi < ng; ++gi) src0[gi] = (sbs[gi] == gs[gi]) ? sbs[gi - 1] : gs[gi - 1];
  }
  std::vector<std::vector<Seg>>& segs = sc.segs;
  segs.resize(ng);
  {
    auto cost = [&](int j, int K) { return (double)(NR - j) * K; };
    for (int gi = 1; gi < ng; ++gi) {   // a super-block's rest: by src0, within the super-block
      const int ge = gs[gi + 1], Kb = (gs[gi] - src0[gi]) * TILE;
      if (ge < sbe[gi]) segs[gi].push_back({ge, sbe[gi], src0[gi], Kb});
    }
    // the far update of each super-block [s0, s1) (the previous one of its successor's
    // groups), split over the successor's groups so their launches carry equal work
    for (int gi = 1; gi < ng; ++gi) {
      if (sbs[gi] != gs[gi]) continue;   // once per super-block, at its opening group
      const int s0 = sbs[gi - 1], s1 = gs[gi], se = sbe[gi], Kf = (s1 - s0) * TILE;
      std::vector<int> mem;
      for (int gj = gi; gj < ng && sbs[gj] == sbs[gi]; ++gj) mem.push_back(gj);
      std::vector<double> fixed(mem.size(), 0.0);
      double far = 0.0, tot = 0.0;
      for (int j = se; j < NC; ++j) far += cost(j, Kf);
      for (size_t m = 0; m < mem.size(); ++m) {
        const int gj = mem[m], Kb = (gs[gj] - src0[gj]) * TILE;
        for (int j = gs[gj] + 1; j < gs[gj + 1]; ++j) fixed[m] += cost(j, Kb);
        for (const Seg& sg : segs[gj])
          for (int j = sg.a; j < sg.b; ++j) fixed[m] += cost(j, sg.K);
        tot += fixed[m];
      }
      tot += far;
      int j = se;
      for (size_t m = 0; m < mem.size(); ++m) {
        const double want = std::max(0.0, tot / mem.size() - fixed[m]);
        const int a = j;
        double got = 0.0;
        while (j < NC && (m + 1 == mem.size() || got + 0.5 * cost(j, Kf) <= want)) got += cost(j++, Kf);
        if (j > a) segs[mem[m]].push_back({a, j, s0, Kf});
      }
    }
  }
  // each group's bulk segments, column by column, split into W1 parts of equal work
  // (part h also carries column gb + h + 1 by src0: the column factored next)
  sc.part.resize(ng);
  for (int gi = 0; gi < ng; ++gi) {
    const int gb = gs[gi], W1 = gs[gi + 1] - gb;
    std::vector<std::vector<Seg>>& part = sc.part[gi];
    part.resize(W1);
    if (gi == 0) continue;
    const int Kb = (gb - src0[gi]) * TILE;
    std::vector<double> load(W1, 0.0);
    for (int h = 0; h + 1 < W1; ++h) load[h] = (double)(NR - (gb + h + 1)) * Kb;
    double tot = 0.0;
    for (int h = 0; h < W1; ++h) tot += load[h];
    std::vector<std::pair<int, int>> cols;   // (column, segment)
    for (int si = 0; si < (int)segs[gi].size(); ++si)
      for (int j = segs[gi][si].a; j < segs[gi][si].b; ++j) {
        cols.push_back({j, si});
        tot += (double)(NR - j) * segs[gi][si].K;
      }
    size_t u = 0;
    double cum = 0.0;
    for (int h = 0; h < W1; ++h) {
      cum += load[h];
      const double target = tot * (h + 1) / W1;
      while (u < cols.size()) {
        const Seg& sg = segs[gi][cols[u].second];
        const double cj = (double)(NR - cols[u].first) * sg.K;
        if (h < W1 - 1 && cum + 0.5 * cj > target) break;
        cum += cj;
        std::vector<Seg>& ps = part[h];
        if (!ps.empty() && ps.back().b == cols[u].first && ps.back().g0 == sg.g0 && ps.back().K == sg.K) ++ps.back().b;
        else ps.push_back({cols[u].first, cols[u].first + 1, sg.g0, sg.K});
        ++u;
      }
    }
  }
  return sc;
}

// ---- the problems of one sweep: the sub-matrix whose origin is tile (o, o) and which has NR
// tile rows, on its own slices of the flags, logdet and the diagonal tiles of B.  t, p0, a, b,
// g0 are local to the sweep; diag_col0 and logdet report global columns.
struct SweepProbs {
  FactBufs F;
  int o, NR;
  double* tile(double* M, int i, int j) const { return M + (long long)(o + i) * TILE + (long long)(o + j) * TILE * F.ld; }
  // tile (0, j) of the augmented row (ld TILE)
  double* atile(int j) const { return F.Faug + (long long)(o + j) * TILE * TILE; }
  int* flags0() const { return F.flags + o; }
  int* cnt_col() const { return flags0() + F.NB; }       // the group schedule: updates of a column
  int* cnt_pan() const { return flags0() + 2 * F.NB; }   // ... and panel tiles of a step
  int* ticket(int t) const { return flags0() + 3 * F.NB + t; }
  int* cnt_dq() const { return flags0() + 4 * F.NB; }
  int* cnt_pc() const { return flags0() + 5 * F.NB; }
  // the diagonal tile of step t with K pending columns from p0: the pending update runs as
  // DQ_N G_DQUAD workgroups (dquad, pushed before the tile; none for K = 0) and the
  // G_DIAG workgroup waits for them, loads the updated tile and factors it
  GemmProb dquad(int t, int p0, int K, double alpha) const {
    GemmProb p = mkprob(tile(F.A, t, p0), F.ld, nullptr, 0, tile(F.A, t, t), F.ld, DQ_N, 1, K, G_DQUAD, alpha, 1.0);
    p.post = cnt_dq() + t;
    p.diag_col0 = (o + t) * TILE;
    return p;
  }
  GemmProb diagprob(int t, int K) const {
    GemmProb p = mkprob(nullptr, F.ld, nullptr, F.ld, tile(F.A, t, t), F.ld, 1, 1, 0, G_DIAG, 1.0, 1.0);
    if (K > 0) {
      p.pre0 = cnt_dq() + t;
      p.pre0_n = DQ_N;
    }
    p.X = tile(F.B, t, t);
    p.ldx = F.ld;
    p.logdet = F.logdet + o + t;
    p.diag_col0 = (o + t) * TILE;
    p.flag = flags0() + t;
    p.Ld = tile(F.A, t, t);
    p.ldd = F.ld;
    return p;
  }
  // panel tiles: the G_PHALF0 problem (pending update + rows 0-63 of the substitution) and,
  // from it, the G_PHALF1 problem (rows 64-127, after every G_PHALF0 tile of the step
  // stored its update: pc_n of them)
  GemmProb panelprob(int t, int p0, int K, double alpha) const {
    GemmProb p = mkprob(K ? tile(F.A, t + 1, p0) : nullptr, F.ld, K ? tile(F.A, t, p0) : nullptr, F.ld, tile(F.A, t + 1, t),
                        F.ld, NR - t - 1, 1, K, G_PANEL | G_PHALF0, alpha, 1.0);
    p.cpost = cnt_pc() + t;
    p.X = tile(F.B, t, t);
    p.ldx = F.ld;
    p.flag = flags0() + t;
    p.diag_col0 = (o + t) * TILE;   // step index for the GEMM_TRACE dev build
    p.Ld = tile(F.A, t, t);
    p.ldd = F.ld;
    return p;
  }
  // the augmented row's panel tile (aug, t): pending columns [p0, t), then x L_tt^-T
  GemmProb augpanel(int t, int p0, int K, double alpha) const {
    GemmProb p = mkprob(K ? atile(p0) : nullptr, TILE, K ? tile(F.A, t, p0) : nullptr, F.ld, atile(t), TILE, 1, 1, K,
                        G_PANEL | G_PHALF0, alpha, 1.0);
    p.cpost = cnt_pc() + t;
    p.X = tile(F.B, t, t);
    p.ldx = F.ld;
    p.flag = flags0() + t;
    p.Ld = tile(F.A, t, t);
    p.ldd = F.ld;
    p.diag_col0 = -TILE;   // (no GEMM_TRACE slot)
    return p;
  }
  static GemmProb half1(const GemmProb& h0, int pc_n) {
    GemmProb p = h0;
    p.flags = G_PANEL | G_PHALF1;
    p.A = p.B = nullptr;
    p.K = 0;
    p.alpha = 1.0;
    p.beta = 0.0;
    p.pre0 = h0.cpost;
    p.pre0_n = pc_n;
    p.pre1 = nullptr;
    p.pre1_n = 0;
    p.cpost = nullptr;
    return p;
  }
  // bulk problems: tiles (i, j), i >= j, j in [a, b), updated by columns [g0, g0 + K/128);
  // with the augmented row also its tiles (aug, j) (not counted as algorithmic flops)
  void bulk(std::vector<GemmProb>& fp, double& fl, bool aug, int a, int b, int g0, int K) const {
    if (a >= b) return;
    const double T = TILE;
    fp.push_back(mkprob(tile(F.A, a, g0), F.ld, tile(F.A, a, g0), F.ld, tile(F.A, a, a), F.ld, b - a, b - a, K, G_CLOWER,
                        -1.0, 1.0));
    fl += (double)(b - a) * T * ((double)(b - a) * T + 1.0) * K;
    if (b < NR) {
      fp.push_back(mkprob(tile(F.A, b, g0), F.ld, tile(F.A, a, g0), F.ld, tile(F.A, b, a), F.ld, NR - b, b - a, K, 0, -1.0,
                          1.0));
      fl += 2.0 * (NR - b) * T * (double)(b - a) * T * K;
    }
    if (aug) fp.push_back(mkprob(atile(g0), TILE, tile(F.A, a, g0), F.ld, atile(a), TILE, 1, b - a, K, 0, -1.0, 1.0));
  }
};

// The chain of step t with pending columns [p0, t), appended to fp in this order: the diagonal
// tile's quadrant blocks (K > 0), the diagonal tile, the panel (rows under t), the augmented
// row's panel (aug), then the rows 64-127 halves of the panels; its flops are added to fl.
// hook(q, role) sees every problem just before it is pushed (fp.size() is its index): the group
// launch wires its hand-offs there and collects the tile codes; the halves are made from the
// panels as the hook left them.
enum ChainRole { CHAIN_DQUAD, CHAIN_DIAG, CHAIN_PANEL, CHAIN_HALF1 };
template <class Hook>
inline void chain_step(const SweepProbs& S, int t, int p0, bool aug, std::vector<GemmProb>& fp, double& fl, Hook hook) {
  const double T = TILE;
  const int K = (t - p0) * TILE;
  const double al = K ? -1.0 : 1.0;
  const int m = S.NR - t - 1;
  const auto push = [&](GemmProb q, ChainRole role) {
    hook(q, role);
    fp.push_back(q);
  };
  if (K) push(S.dquad(t, p0, K, al), CHAIN_DQUAD);
  push(S.diagprob(t, K), CHAIN_DIAG);
  fl += T * (T + 1.0) * K;
  const int pc_n = (m >= 1 ? m : 0) + (aug ? 1 : 0);
  const size_t h0at = fp.size();
  if (m >= 1) {
    push(S.panelprob(t, p0, K, al), CHAIN_PANEL);
    fl += 2.0 * m * T * T * K + (double)m * T * T * T;
  }
  if (aug) push(S.augpanel(t, p0, K, al), CHAIN_PANEL);
  for (size_t k = h0at, e = fp.size(); k < e; ++k) push(SweepProbs::half1(fp[k], pc_n), CHAIN_HALF1);
}

// The tile list (= dispatch order) of a group launch from its pieces: head, the first step's
// quadrant blocks and diagonal tile at the front of seg[0]; early, the previous group's updates
// of the group's later columns; bulkc, the group's bulk segments in order_tiles' order; spliced
// into these, step h's chain tiles seg[h] at list position grp_p0 + h grp_stride (step 0's first
// panel at 256: workgroup 0's CU partner).  Step h >= 1 waits for step h-1's panels and its
// column's update, so every wait points to earlier tiles; one drain per group instead of one
// per step.
inline std::vector<unsigned> group_list(size_t head, const std::vector<unsigned>& early, const std::vector<unsigned>& bulkc,
                                        const std::vector<std::vector<unsigned>>& seg, const CholSchedParams& P) {
  const int W1 = (int)seg.size();
  // assemble: diag(gb) (after its quadrants), early, bulk; step 0's panels at grp_p0
  // (its first beside the diagonal tile), step h's chain at grp_p0 + h grp_stride
  std::vector<unsigned> base(seg[0].begin(), seg[0].begin() + head);
  base.insert(base.end(), early.begin(), early.end());
  base.insert(base.end(), bulkc.begin(), bulkc.end());
  const std::vector<unsigned> rest0(seg[0].begin() + head, seg[0].end());
  // step h's tiles go before base position min(|base|, p0 + h stride), for h >= 1 not
  // before the column updates they wait on: the positions do not decrease with h, so
  // the steps stay in order even where they clamp
  std::vector<unsigned> order;
  auto pos = [&](int h) {
    size_t at = (size_t)P.grp_p0 + (size_t)h * P.grp_stride;
    at = std::max(at, h >= 1 ? head + early.size() : head);   // after the step's diagonal tile
    return std::min(base.size(), at);
  };
  int h = 0;
  for (size_t i = 0; i <= base.size(); ++i) {
    while (h < W1 && pos(h) == i) {
      const std::vector<unsigned>& sg = h == 0 ? rest0 : seg[h];
      order.insert(order.end(), sg.begin(), sg.end());
      ++h;
    }
    if (i < base.size()) order.push_back(base[i]);
  }
  // The first 512 workgroups of a launch on an idle GPU fill two slots per CU in
  // order, workgroup 256 + k beside workgroup k (tools/hip/placement_probe.hip): step
  // 0's first panel tile goes to 256 + (head - 1), beside the diagonal tile, so the
  // factorisation has its CU's SIMDs to itself.  (Pinning the later steps' diagonal
  // tiles the same way measured no faster: DESIGN.md section 10.)
  if (!rest0.empty() && order.size() > 256 + head) {   // the first panel tile beside the diagonal
    const auto it = std::find(order.begin(), order.end(), rest0.front());
    if ((size_t)(it - order.begin()) > 255 + head) {
      order.erase(it);
      order.insert(order.begin() + std::min(255 + head, order.size()), rest0.front());
    }
  }
  return order;
}

// One sweep of the schedule: NC tile columns of the sub-matrix whose origin is tile (o, o)
// and which has NR tile rows, its launches indexed by global column in pl.idx[sweep].
// (0, NB, NB) is the whole factorisation.  The split sweep
// (Plan::split_h) is (0, h, NB): the first h columns over all rows, every trailing update
// clipped to columns < h, so L11 and L21 end final and A22 untouched -- then (h, NB - h,
// NB - h), the unsplit schedule of the Schur complement, on its own slices of the flags,
// logdet and the diagonal tiles of B, reporting global columns.
//
// Per-step schedule, one launch per column block t, t at position h of group gi:
//   critical: tile (t,t) updated by its pending columns [p0, t) -- the previous
//             group when h = 0, else the earlier columns of g -- then factored and
//             inverted in-kernel (G_DIAG); panel tiles (i,t), i > t, updated the
//             same way and multiplied by X_t^T once flags[t] is released (G_PANEL);
//   bulk:     part h of the trailing update by the previous group (K = its width
//             x 128) over columns j > start(g): part h holds column start(g)+h+1
//             (factored next) plus a balanced share of the columns after g.
// Group schedule: one launch per group of width >= 2 (group_list has its tile list): its chain
// tiles hand on by counters, per column (cnt_col: the previous group's updates of the group's
// later columns) and per step (cnt_pan: its panel tiles).
// Returns false when a group list has a tile waiting on a later one (an internal error).
inline bool add_sweep(Plan& pl, const FactBufs& F, const CholSchedParams& P, SweepKind sweep, int o, int NC, int NR) {
  const SweepProbs S{F, o, NR};
  const SweepCols sc = sweep_columns(NC, NR, P);
  const std::vector<int>& gs = sc.gs;
  for (int va = 0; va < (pl.aug ? 2 : 1); ++va) {
    const bool aug = va == 1;
    std::vector<int>& fidx = pl.idx[sweep][0][aug];
    for (int gi = 0; gi < sc.groups(); ++gi) {
      const int gb = gs[gi], W1 = gs[gi + 1] - gb;
      for (int h = 0; h < W1; ++h) {
        const int t = gb + h;
        std::vector<GemmProb> fp;
        double fl = 0.0;
        chain_step(S, t, h == 0 ? sc.src0[gi] : gb, aug, fp, fl, [](GemmProb&, ChainRole) {});
        if (gi > 0) {
          const int g0 = sc.src0[gi], Kb = (gb - g0) * TILE;
          if (h + 1 < W1) S.bulk(fp, fl, aug, t + 1, t + 2, g0, Kb);   // the column factored next
          for (const Seg& sg : sc.part[gi][h]) S.bulk(fp, fl, aug, sg.a, sg.b, sg.g0, sg.K);
        }
        fidx[o + t] = (int)pl.launches.size();
        add_launch(pl, GEMM_FUSED, fp, fl);
        pl.launches.back().ticket = S.ticket(t);
      }
    }
    if (!P.group) continue;
    std::vector<int>& gidx = pl.idx[sweep][1][aug];
    for (int gi = 0; gi < sc.groups(); ++gi) {
      const int gb = gs[gi], W1 = gs[gi + 1] - gb;
      if (W1 < 2) {
        gidx[o + gb] = fidx[o + gb];
        continue;
      }
      const int g0 = sc.src0[gi], Kb = (gb - g0) * TILE;
      std::vector<GemmProb> fp;
      double fl = 0.0;
      auto codes = [&](int pi, const GemmProb& q, std::vector<unsigned>& out) {
        for (int ti = 0; ti < q.mt; ++ti)
          for (int tj = 0; tj < q.nt && ((q.flags & G_CLOWER) == 0 || tj <= ti); ++tj) out.push_back(tile_code(pi, ti, tj));
      };
      std::vector<unsigned> early, bulkc;
      std::vector<std::vector<unsigned>> seg(W1);
      std::vector<int> ncol(W1, 0), npan(W1, 0);
      if (gi > 0)
        for (int h = 1; h < W1; ++h) {   // column gb+h by the previous group
          const size_t b0 = fp.size();
          S.bulk(fp, fl, aug, gb + h, gb + h + 1, g0, Kb);
          for (size_t k = b0; k < fp.size(); ++k) {
            fp[k].post = S.cnt_col() + gb + h;
            const size_t e0 = early.size();
            codes((int)k, fp[k], early);
            ncol[h] += (int)(early.size() - e0);
          }
        }
      for (int h = 0; h < W1; ++h) {
        const int t = gb + h;
        // step h >= 1 starts after step h-1's panels and its own column's update: the hand-offs
        // gate its diagonal tile's quadrants (the tile itself when nothing is pending) and its panels
        chain_step(S, t, h == 0 ? g0 : gb, aug, fp, fl, [&](GemmProb& q, ChainRole role) {
          const bool wired = role == CHAIN_DQUAD || role == CHAIN_PANEL || (role == CHAIN_DIAG && !q.pre0);
          if (wired && h > 0) {
            q.pre0 = S.cnt_pan() + t - 1;
            q.pre0_n = npan[h - 1];
            if (gi > 0) {
              q.pre1 = S.cnt_col() + t;
              q.pre1_n = ncol[h];
            }
          }
          if (role == CHAIN_PANEL) q.post = S.cnt_pan() + t;
          if (role == CHAIN_PANEL || role == CHAIN_HALF1) npan[h] += q.mt * q.nt;   // both halves of every panel tile post cnt_pan
          codes((int)fp.size(), q, seg[h]);
        });
      }
      if (gi > 0 && !sc.segs[gi].empty()) {   // the group's bulk segments (the rest of its super-block, a far share)
        const size_t b0 = fp.size();
        for (const Seg& sg : sc.segs[gi]) S.bulk(fp, fl, aug, sg.a, sg.b, sg.g0, sg.K);
        const std::vector<GemmProb> sub(fp.begin() + b0, fp.end());
        for (unsigned code : order_tiles(sub)) bulkc.push_back(code + ((unsigned)b0 << 24));
      }
      const size_t head = gi > 0 ? DQ_N + 1 : 1;   // step 0: quadrant blocks (when K > 0) and diagonal tile
      const std::vector<unsigned> order = group_list(head, early, bulkc, seg, P);
      // every tile may wait only on tiles before it in the list (the dispatch order):
      // then the earliest unfinished tile can always run.  Checked, not assumed.
      if (!waits_point_back(fp.data(), order)) return false;
      gidx[o + gb] = (int)pl.launches.size();
      add_launch(pl, GEMM_FUSED, fp, fl, &order);
      pl.launches.back().ticket = S.ticket(gb);
    }
  }
  return true;
}

// the index table of one sweep kind, nothing launched yet
inline void init_steps(Plan& pl, SweepKind sweep, int NB, const CholSchedParams& P) {
  pl.idx[sweep][0][0].assign(NB, -1);
  pl.idx[sweep][0][1].assign(NB, -1);
  if (P.group) {
    pl.idx[sweep][1][0].assign(NB, -1);
    if (pl.aug) pl.idx[sweep][1][1].assign(NB, -1);
  }
}

// the two problems of TRTRI block pair pr = {t0, h, t1}, appended to a level's two launches
inline void tri_pair(const FactBufs& F, const std::array<int, 3>& pr, std::vector<GemmProb>& pa, std::vector<GemmProb>& pb,
                     double& fa, double& fb) {
  const SweepProbs S{F, 0, F.NB};
  const double T = TILE;
  const int t0 = pr[0], h = pr[1], t1 = pr[2];
  const int a = h - t0, b = t1 - h;
  // T^T (a x b tiles, stored in the upper block rows t0:h, cols h:t1 of B)
  //   = X11^T L21^T ;  opA(m,k) = X11(k,m): K-contiguous, upper -> kbeg = ti*128
  pa.push_back(mkprob(S.tile(F.B, t0, t0), F.ld, S.tile(F.A, h, t0), F.ld, S.tile(F.B, t0, h), F.ld, a, b, a * TILE,
                      G_KBEG_TI, 1.0, 0.0));
  fa += (double)a * T * a * T * b * T;   // triangular a x a times a x b
  // X21 = -X22 T ;  opA = X22 lower -> kend = (ti+1)*128 ; opB(k,n) = T^T(n,k)
  pb.push_back(mkprob(S.tile(F.B, h, h), F.ld, S.tile(F.B, t0, h), F.ld, S.tile(F.B, h, t0), F.ld, b, a, b * TILE,
                      G_KEND_TI, -1.0, 0.0));
  fb += (double)b * T * b * T * a * T;
}

// the launch that updates the augmented row's tiles [from, to) by the first `from` columns
inline int add_aug_update(Plan& pl, const FactBufs& F, int from, int to) {
  const SweepProbs S{F, 0, F.NB};
  add_launch(pl, GEMM_PLAIN, {mkprob(F.Faug, TILE, S.tile(F.A, from, 0), F.ld, S.atile(from), TILE, 1, to - from,
                                     from * TILE, 0, -1.0, 1.0)}, 0.0);
  return (int)pl.launches.size() - 1;
}

// The (size-dependent, data-independent) GEMM schedule of a workspace: pl is filled from
// nothing.  F.Faug non-null: the launches carrying the augmented row are built too.  h > 0: the
// split sweep at tile column h, and with it the TRTRI by sides; q > 0 as well: the nested split
// at q.  Each of those three is left out when the descriptors would then pass limit; whether
// the rest fits is the caller's to check (pl.probs.size() > limit).  Descriptor and list
// offsets count from 0: the caller rebases them to where it uploads.  Returns false on the one
// internal error, a group list with a tile waiting on a later one.
inline bool build_chol_plan(Plan& pl, const FactBufs& F, const CholSchedParams& P, int h, int q, int limit) {
  pl = Plan();
  pl.n_pad = F.ld;
  pl.a_ptr = F.A;
  pl.b_ptr = F.B;
  const int NB = F.NB;
  pl.aug = F.Faug != nullptr;
  // --- Cholesky (right-looking, 128-column steps)
  init_steps(pl, SWEEP_WHOLE, NB, P);
  if (!add_sweep(pl, F, P, SWEEP_WHOLE, 0, NB, NB)) return false;
  // --- triangular inverse X = L^-1 in B (diagonal tiles already hold Dinv)
  for (int s = 2; s / 2 < NB; s *= 2) {
    std::vector<GemmProb> pa, pb;
    const std::vector<std::array<int, 3>> prs = trtri_level_pairs(NB, s);
    double fa = 0.0, fb = 0.0;
    for (const auto& pr : prs) tri_pair(F, pr, pa, pb, fa, fb);
    if (pa.empty()) continue;
    pl.tri_pairs.push_back(prs);
    split_k(pa, F.part, F.tcnt);
    split_k(pb, F.part, F.tcnt);
    pl.trtri.push_back((int)pl.launches.size());
    add_launch(pl, GEMM_AK, pa, fa);
    pl.trtri.push_back((int)pl.launches.size());
    add_launch(pl, GEMM_PLAIN, pb, fb);
  }
  // --- A^-1 = X^T X (lower tiles), written over L in A
  pl.lauum = (int)pl.launches.size();
  {
    const double N = (double)F.ld;
    std::vector<GemmProb> lp = {mkprob(F.B, F.ld, F.B, F.ld, F.A, F.ld, NB, NB, (int)F.ld, G_CLOWER | G_KBEG_TI, 1.0, 0.0)};
    split_k(lp, F.part, F.tcnt);
    add_launch(pl, GEMM_AK_BK, lp, N * N * N / 3.0);
  }
  if (!h) return true;
  // --- the split sweep (potrf with split): columns [0, h), the Schur
  // complement S = A22 - L21 L21^T on the int8 cores (chol_schur), then chol(S); between the
  // phases the augmented row's trailing part takes the first h columns' update in one launch.
  // Left out (the sweep stays whole) when its descriptors would not fit
  const bool ok = optional_part(pl, limit, [&] {
    init_steps(pl, SWEEP_SPLIT, NB, P);
    if (!add_sweep(pl, F, P, SWEEP_SPLIT, 0, h, NB) || !add_sweep(pl, F, P, SWEEP_SPLIT, h, NB - h, NB - h)) return false;
    if (pl.aug) pl.aug_mid = add_aug_update(pl, F, h, NB);
    pl.split_h = h;
    return true;
  });
  if (!ok || !pl.split_h) return ok;
  // --- the TRTRI levels below the top one by side of h (a power of two: no pair of theirs
  // straddles it), so X11 can be formed while the sweep's second phase runs (tri_ahead).  Each
  // side's launch splits K as the level's one launch does: the same sums, bit for bit.  Left
  // out the same way
  optional_part(pl, limit, [&] {
    for (size_t lv = 0; lv < pl.tri_pairs.size(); ++lv) {
      std::array<int, 4> side = {-1, -1, -1, -1};
      std::vector<GemmProb> wa, wb;
      double f0 = 0.0, f1 = 0.0;
      for (const auto& pr : pl.tri_pairs[lv]) tri_pair(F, pr, wa, wb, f0, f1);
      int ta = 0, tb = 0, ka = 0, kb = 0;
      for (const GemmProb& p : wa) { ta += prob_tiles(p); ka = std::max(ka, p.K); }
      for (const GemmProb& p : wb) { tb += prob_tiles(p); kb = std::max(kb, p.K); }
      for (int sd = 0; sd < 2; ++sd) {
        std::vector<GemmProb> pa, pb;
        double fa = 0.0, fb = 0.0;
        for (const auto& pr : trtri_side_pairs(pl.tri_pairs[lv], h, sd)) tri_pair(F, pr, pa, pb, fa, fb);
        if (pa.empty()) continue;
        split_k(pa, F.part, F.tcnt, ta, ka);
        split_k(pb, F.part, F.tcnt, tb, kb);
        side[2 * sd] = (int)pl.launches.size();
        add_launch(pl, GEMM_AK, pa, fa);
        side[2 * sd + 1] = (int)pl.launches.size();
        add_launch(pl, GEMM_PLAIN, pb, fb);
      }
      pl.trtri_side.push_back(side);
    }
    pl.sides = true;
    return true;
  });
  if (!q) return true;
  // --- the nested split: phase A once more at q = h / 2, the trapezoid's update by the columns
  // [0, q) a second int8 product (chol_schur at q): columns [0, q) over all rows, then [q, h)
  // over the rows from q on, then the Schur complement's sweep as above; before the middle sweep
  // the augmented row's tiles [q, h) take the first q columns' update in one launch (its tiles
  // [h, NB) still take all h columns' at h: aug_mid).  Left out the same way
  return optional_part(pl, limit, [&] {
    init_steps(pl, SWEEP_NESTED, NB, P);
    if (!add_sweep(pl, F, P, SWEEP_NESTED, 0, q, NB) || !add_sweep(pl, F, P, SWEEP_NESTED, q, h - q, NB - q)) return false;
    for (int g = 0; g < 2; ++g)   // (h, NB - h, NB - h): the split sweep's own launches
      for (int a = 0; a < 2; ++a)
        for (int t = h; t < NB && !pl.idx[SWEEP_NESTED][g][a].empty(); ++t)
          pl.idx[SWEEP_NESTED][g][a][t] = pl.idx[SWEEP_SPLIT][g][a][t];
    if (pl.aug) pl.aug_q = add_aug_update(pl, F, q, h);
    pl.split_q = q;
    return true;
  });
}

}  // namespace gpe
