// gpemu_postgroup.hpp -- the posterior covariance inside groups of G consecutive points
// (gpe_posterior_groups): the block diagonal of the m x m covariance, from the chunk's
// V = L^-1 K* (np x mp column-major, ld np) that the diagonal pipeline already holds.
//
//   k_post_groupgram<NT>  the G x G Gram of each group's columns of V on v_mfma_f64_16x16x4_f64,
//                         one partial per segment of PGC_SEG training rows
//   k_post_groupcov<FAM>  adds the segments in index order, takes rho from the chunk's scaled
//                         points (k_pairs' arithmetic) and writes coff rho(s_ab) - v_a . v_b off
//                         the diagonal, cdiag - |v_a|^2 on it, the lower triangle mirrored
//
// k_colnorm2 is the G = 1 case of the pair.  The host adds t_a . t_b and scales by sigma^2.
//
// Order of every sum (fixed by n alone; no atomics, no waits between workgroups): the rows are
// cut into segments of PGC_SEG whatever m and G are; inside a segment wave w of the workgroup
// takes rows 16 w .. 16 w + 15 of every panel of PGC_R rows, four at a time through the MFMA,
// the four waves' sums are added as ((w0 + w1) + w2) + w3, and k_post_groupcov adds the
// segments from 0 upwards.  An entry of a Gram is one dot product of the MFMA: it does not see
// the other columns of its tile, so a group's block is the same wherever the group stands.
#pragma once

#include "gpemu_kernels.hpp"

namespace gpe {

// PGC_R rows of a panel; PGC_LD its leading dimension in LDS (= 2 mod 32: the 16 columns x 2
// rows that one half-wave reads with ds_read_b64 fall on 32 different 8-byte banks);
// PGC_SEG rows per segment (a multiple of PGC_R; n_pad is a multiple of TILE = 2 PGC_R).
constexpr int PGC_R = 64, PGC_LD = PGC_R + 2, PGC_SEG = 1024, PGC_MAXG = 64;

// One work item = gpi whole groups side by side (gpi = 16 / G for G <= 8, else 1): cw = gpi G
// columns of V from column item * cw on, padded to NT tiles of 16.  Padding columns are
// selected to zero and never loaded.
struct GroupGramArgs {
  const double* V;   // np x mp, ld np
  long long ldv;
  double* part;      // [nseg][ngroups][G][G], the lower triangles written
  int np, G, gpi, ngroups;
};

inline int pgc_gpi(int G) { return G <= 8 ? 16 / G : 1; }
inline int pgc_nseg(long long np) { return (int)((np + PGC_SEG - 1) / PGC_SEG); }

template <int NT>
static __global__ void __launch_bounds__(256) k_post_groupgram(GroupGramArgs a) {
  constexpr int NTT = NT * (NT + 1) / 2, CPT = NT * 4;   // lower tiles; panel columns per thread
  static_assert(NT * 16 * PGC_LD >= NTT * 256, "the panel holds one wave's accumulators");
  __shared__ double pan[NT * 16 * PGC_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int item = (int)blockIdx.x, seg = (int)blockIdx.y;
  const int g0 = item * a.gpi;                         // the item's first group
  const int cw = min(a.gpi, a.ngroups - g0) * a.G;     // its columns
  const long long c0 = (long long)g0 * a.G;
  const int r_beg = seg * PGC_SEG, r_end = min(a.np, r_beg + PGC_SEG);
  // the lane's share of a panel: row lane of columns w, w + 4, ... (coalesced along the column)
  const double* src = a.V + c0 * a.ldv + lane;
  double nx[CPT];
  auto fetch = [&](int r0) {
#pragma unroll
    for (int u = 0; u < CPT; ++u) {
      const int c = w + 4 * u;
      nx[u] = c < cw ? src[(long long)c * a.ldv + r0] : 0.0;
    }
  };
  d4 acc[NTT];
#pragma unroll
  for (int t = 0; t < NTT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  const int fo = (lane & 15) * PGC_LD + 16 * w + (lane >> 4);   // the lane's operand element
  fetch(r_beg);
  for (int r0 = r_beg; r0 < r_end; r0 += PGC_R) {
    __syncthreads();   // the previous panel has been read
#pragma unroll
    for (int u = 0; u < CPT; ++u) pan[(w + 4 * u) * PGC_LD + lane] = nx[u];
    __syncthreads();
    if (r0 + PGC_R < r_end) fetch(r0 + PGC_R);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      // A(i, k) = V(row k, column i of tile t), B(k, j) likewise: on a diagonal tile the two
      // operands are the same register
      double f[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) f[t] = pan[t * 16 * PGC_LD + fo + 4 * ks];
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj) {
          const int t = ti * (ti + 1) / 2 + tj;
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[ti], f[tj], acc[t], 0, 0, 0);
        }
    }
  }
  // ((w0 + w1) + w2) + w3 through the panel's LDS
  for (int o = 1; o < 4; ++o) {
    __syncthreads();
    if (w == o) {
#pragma unroll
      for (int t = 0; t < NTT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) pan[(t * 4 + r) * 64 + lane] = acc[t][r];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int t = 0; t < NTT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] += pan[(t * 4 + r) * 64 + lane];
    }
  }
  if (w != 0) return;
  // D(i, j): column j = lane & 15, row i = (lane >> 4) + 4 r.  Entries of one group, j <= i.
  double* out = a.part + (long long)seg * a.ngroups * a.G * a.G;
#pragma unroll
  for (int ti = 0; ti < NT; ++ti)
#pragma unroll
    for (int tj = 0; tj <= ti; ++tj) {
      const int t = ti * (ti + 1) / 2 + tj;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * 16 + (lane >> 4) + 4 * r, j = tj * 16 + (lane & 15);
        const int gi = i / a.G, gj = j / a.G;
        if (i < cw && j <= i && gi == gj) {
          const int ia = i - gi * a.G, jb = j - gj * a.G;
          out[((long long)(g0 + gi) * a.G + ia) * a.G + jb] = acc[t][r];
        }
      }
    }
}

struct GroupCovArgs {
  const double* part;   // k_post_groupgram's segment sums
  const double* xsw;    // scaled points of the chunk (row-major, d each)
  double* cov;          // [ngroups][G][G]
  double coff, cdiag;
  int nseg, ngroups, G, d;
};

// One thread per entry (a, b <= a) of a group.  s = sum_k fma(df, df, s) over k = 0 .. d - 1
// in k_pairs' order (its zero padding adds fma(0, 0, s) = s, so a loop over d gives its bits
// for every d, the wide case included); "diagonal" is a == b, never equal coordinates.
template <int FAM>
static __global__ void __launch_bounds__(256) k_post_groupcov(GroupCovArgs a) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long gg = (long long)a.G * a.G, tot = (long long)a.ngroups * gg;
  if (e >= tot) return;
  const long long g = e / gg;
  const int ab = (int)(e - g * gg), ia = ab / a.G, jb = ab - ia * a.G;
  if (jb > ia) return;
  double gram = a.part[e];
  for (int s = 1; s < a.nseg; ++s) gram += a.part[(long long)s * tot + e];
  const double* xa = a.xsw + (g * a.G + ia) * a.d;
  const double* xb = a.xsw + (g * a.G + jb) * a.d;
  double s = 0.0;
  for (int k = 0; k < a.d; ++k) {
    const double df = xa[k] - xb[k];
    s = fma(df, df, s);
  }
  double rho;
  if constexpr (FAM == FAM_GAUSS) {
    rho = exp(-s);
  } else {
    double gfac;
    matern_rho_g<FAM>(s, rho, gfac);
  }
  const double v = ia == jb ? a.cdiag - gram : a.coff * rho - gram;
  a.cov[e] = v;
  a.cov[g * gg + (long long)jb * a.G + ia] = v;
}

}  // namespace gpe
