// gpemu_postmean.hpp -- the posterior mean alone (gpe_posterior_mean): the sum over the
// training rows y_s = sum_i gamma_i coff rho(s_si) fused with the covariance it reads, so that
// nothing of size n x m is written, and the kernel that adds its partial sums.
//
// Every term is k_pairs' entry of K* (gpemu_kernels.hpp): the scaled coordinates of
// k_scale_points, df = xw_ik - xsw_sk and s = fma(df, df, s) over k = 0 .. d - 1 in that order,
// exp(-s) or matern_rho_g<FAM>, then coff.  Only the order of the sum over i is this file's.
#pragma once

#include "gpemu_kernels.hpp"

namespace gpe {

// k_post_mean: PM_LANES lanes per workgroup, each with PM_PPL points (one when WIDE) whose
// coordinates stay in registers.  The training rows go by in tiles of PM_RI: their coordinates
// and gamma sit in LDS and are read at one address by the whole wave (a broadcast), and a
// value read once serves the lane's PM_PPL points.
// The rows are cut into segments of PM_SEG tiles (192 rows) whatever m is, one workgroup per
// segment and column of points (blockIdx.y: the segment), so a few points already fill the
// chip when n is large.  A lane sums its segment from zero and stores it, part[segment][point];
// k_post_mean_fin adds the segments in index order.  The order of the sum depends on n alone:
// the result is the same for every chunk length and on every call (fixed order, no atomics).
// Measured at n = 16384, d = 10, 65536 points (Gaussian): one segment per
// workgroup 1.49 ms against 1.99 ms with 11 (fewer, longer workgroups leave a tail and fewer
// waves to cover the barriers); 2 points per lane 1.55 ms against 1.62 ms with 1 and 1.51 ms
// with 4 (at 128 lanes); 256 lanes 1.49 ms against 1.55 ms with 128; tiles of 16, 32 or 64
// rows within 1 %.
// d <= 32: the distance from the registers.  d > 32 (WIDE): the squared distances of a tile's
// PM_RI rows are kept in registers while the coordinates pass through LDS 32 dimensions at a
// time, in k_pairs_wide's order.
// Padded rows enter with gamma = 0 (their coordinates are 0, rho is finite); padded points are
// computed and never copied out.
constexpr int PM_LANES = 256, PM_PPL = 2, PM_PTS = PM_LANES * PM_PPL, PM_RI = 32, PM_SEG = 6, PM_WIDE = 32;

struct PostMeanArgs {
  const double* xw;    // scaled training points (np x d, row-major)
  const double* xsw;   // scaled points of the chunk (mp x d, row-major)
  const double* gam;   // gamma = A^-1 (f - H beta) (np)
  double* part;        // the segments' sums [nseg][mp]
  double coff;
  int n, np, mp, d;
};

template <int FAM>
__device__ inline double post_mean_rho(double s) {
  if constexpr (FAM == FAM_GAUSS) {
    return exp(-s);
  } else {
    double rho, g;
    matern_rho_g<FAM>(s, rho, g);
    return rho;
  }
}

template <int DMAX, int FAM, bool WIDE>
static __global__ void __launch_bounds__(PM_LANES) k_post_mean(PostMeanArgs a) {
  constexpr int PPL = WIDE ? 1 : PM_PPL;
  __shared__ double xw_t[PM_RI * DMAX];
  __shared__ double gam_t[PM_RI];
  const int tid = threadIdx.x, d = a.d;
  const int p0 = (int)blockIdx.x * (PM_LANES * PPL) + tid;   // the lane's points: p0 + j PM_LANES
  const int nrt = a.np / PM_RI;
  const int seg = (int)blockIdx.y;
  double xs[WIDE ? 1 : PPL][DMAX];
  if constexpr (!WIDE) {
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const double* xp = a.xsw + (long long)(p0 + j * PM_LANES) * d;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) xs[j][k] = k < d ? xp[k] : 0.0;
    }
  }
  // the tile's rows: dimensions c0 .. c0 + DMAX (zero beyond d) and, with them, gamma
  auto stage = [&](int r0, int c0, bool with_gam) {
    for (int e = tid; e < PM_RI * DMAX; e += PM_LANES) {
      const int i = e / DMAX, k = e - i * DMAX;
      xw_t[e] = c0 + k < d ? a.xw[(long long)(r0 + i) * d + c0 + k] : 0.0;
    }
    if (with_gam && tid < PM_RI) gam_t[tid] = r0 + tid < a.n ? a.gam[r0 + tid] : 0.0;
  };
  double acc[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) acc[j] = 0.0;
  const int rt1 = min(nrt, (seg + 1) * PM_SEG);
  for (int rt = seg * PM_SEG; rt < rt1; ++rt) {
    const int r0 = rt * PM_RI;
    if constexpr (WIDE) {
      const double* xp = a.xsw + (long long)p0 * d;
      double s[PM_RI];
#pragma unroll
      for (int i = 0; i < PM_RI; ++i) s[i] = 0.0;
      for (int c0 = 0; c0 < d; c0 += DMAX) {
        __syncthreads();   // the previous coordinates (and, at c0 = 0, gamma) have been read
        stage(r0, c0, c0 == 0);
        double xq[DMAX];
#pragma unroll
        for (int k = 0; k < DMAX; ++k) xq[k] = c0 + k < d ? xp[c0 + k] : 0.0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PM_RI; ++i) {
#pragma unroll
          for (int k = 0; k < DMAX; ++k) {
            const double df = xw_t[i * DMAX + k] - xq[k];
            s[i] = fma(df, df, s[i]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < PM_RI; ++i) acc[0] = fma(gam_t[i], a.coff * post_mean_rho<FAM>(s[i]), acc[0]);
    } else {
      __syncthreads();   // the previous tile has been read
      stage(r0, 0, true);
      __syncthreads();
#pragma unroll 2
      for (int i = 0; i < PM_RI; ++i) {
        double s[PPL];
#pragma unroll
        for (int j = 0; j < PPL; ++j) s[j] = 0.0;
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
          const double xk = xw_t[i * DMAX + k];
#pragma unroll
          for (int j = 0; j < PPL; ++j) {
            const double df = xk - xs[j][k];
            s[j] = fma(df, df, s[j]);
          }
        }
        const double g = gam_t[i];
#pragma unroll
        for (int j = 0; j < PPL; ++j) acc[j] = fma(g, a.coff * post_mean_rho<FAM>(s[j]), acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < PPL; ++j) a.part[(long long)seg * a.mp + p0 + j * PM_LANES] = acc[j];
}

// y_s = the segments' sums added in index order (mp points)
static __global__ void k_post_mean_fin(const double* part, int nseg, int mp, double* y) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= mp) return;
  double acc = part[s];
  for (int j = 1; j < nseg; ++j) acc += part[(long long)j * mp + s];
  y[s] = acc;
}

}  // namespace gpe
