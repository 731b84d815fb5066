// gpemu_postmean_multi.hpp -- the posterior mean of p outputs that share one correlation
// matrix (gpe_posterior_mean_multi): y[s][c] = sum_i Gamma[i][c] coff rho(s_si), c < p, fused
// with the covariance it reads.  Nothing of size n x m is written, and every rho is formed once
// per (point, training row) whatever p is.
//
// Every rho is k_post_mean's (gpemu_postmean.hpp): the scaled coordinates of k_scale_points,
// s = fma(df, df, s) over k = 0 .. d - 1 in that order, post_mean_rho<FAM>, then coff.  The
// summation contract is k_post_mean's too: the training rows in segments of PM_SEG tiles (192
// rows) whatever m is, one partial per segment, point and output, the partials added in index
// order by k_post_mean_multi_fin.  The result does not depend on the chunk length and is the
// same on every call; there are no floating-point atomics and no waits between workgroups.
#pragma once

#include "gpemu_postmean.hpp"

namespace gpe {

struct PostMeanMultiArgs {
  const double* xw;    // scaled training points (np x d, row-major)
  const double* xsw;   // scaled points of the chunk (mp x d, row-major)
  const double* gam;   // Gamma = A^-1 (F - H B) (np x p, column-major, ld = np)
  double* part;        // the segments' sums [nseg][p][mp]
  double coff;
  int n, np, mp, d, p;
};

typedef double pmm_d4 __attribute__((ext_vector_type(4)));

// k_post_mean_multi: the sum over a segment's rows as a matrix product on the fp64 matrix
// cores.  A wave owns PMM_PG groups of 16 points; per step of 4 training rows its 64 lanes
// form the 64 values coff rho(point lane & 15, row lane >> 4) of a group -- one per lane, exactly
// the A operand of v_mfma_f64_16x16x4_f64 -- and multiply them by the 4 x 16 block of Gamma
// (B operand: lane l holds Gamma[row l >> 4][column l & 15], from the tile in LDS), once per
// block of 16 outputs (NCB of them: p <= 16 NCB).  D (lane l, register r) is point
// (l >> 4) + 4 r of the group and output l & 15 of the block.  A lane computes one rho per
// group and step whatever p is; the products ride on the matrix pipe beside the next step's
// distances.
// The training rows go by in tiles of PM_RI, coordinates (row pitch DMAX + 1: the four rows a
// wave reads lie in different banks) and Gamma in LDS.  d > 32 (WIDE): the squared distances of
// a lane's 8 rows of the tile stay in registers while the coordinates pass through LDS 32
// dimensions at a time, as in k_post_mean.
// Padded rows enter with Gamma = 0 (their coordinates are 0, rho is finite); padded points are
// computed and never copied out; outputs c >= p of the last block are multiplied by zeros and
// never stored.
// Measured at n = 16384, d = 10, 1e6 points (Gaussian): 2 groups per wave 31.1 /
// 34.2 / 37.7 ms at p = 1 / 8 / 16 against 30.5 / 33.4 / 36.3 ms with 4, whose d <= 32 instances
// no longer fit the registers (1 KB of scratch per lane): 2 kept.
constexpr int PMM_PG = 2, PMM_PTS = (PM_LANES / 64) * 16 * PMM_PG, PMM_MAXP = 64;

template <int DMAX, int FAM, bool WIDE, int NCB>
static __global__ void __launch_bounds__(PM_LANES) k_post_mean_multi(PostMeanMultiArgs a) {
  constexpr int XP = DMAX + 1, PBW = NCB * 16, STEPS = PM_RI / 4;
  __shared__ double xw_t[PM_RI * XP];
  __shared__ double gam_t[PM_RI * PBW];
  const int tid = threadIdx.x, d = a.d;
  const int lane = tid & 63, wave = tid >> 6, lr = lane >> 4, lc = lane & 15;
  const int pbase = (int)blockIdx.x * PMM_PTS + wave * (16 * PMM_PG);   // the wave's first point
  const int nrt = a.np / PM_RI;
  const int seg = (int)blockIdx.y;
  double xs[WIDE ? 1 : PMM_PG][DMAX];
  if constexpr (!WIDE) {
#pragma unroll
    for (int g = 0; g < PMM_PG; ++g) {
      const double* xp = a.xsw + (long long)(pbase + g * 16 + lc) * d;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) xs[g][k] = k < d ? xp[k] : 0.0;
    }
  }
  // the tile's rows: dimensions c0 .. c0 + DMAX (zero beyond d) and, with them, Gamma
  auto stage = [&](int r0, int c0, bool with_gam) {
    for (int e = tid; e < PM_RI * DMAX; e += PM_LANES) {
      const int i = e / DMAX, k = e - i * DMAX;
      xw_t[i * XP + k] = c0 + k < d ? a.xw[(long long)(r0 + i) * d + c0 + k] : 0.0;
    }
    if (with_gam)
      for (int e = tid; e < PM_RI * PBW; e += PM_LANES) {
        const int c = e / PM_RI, i = e - c * PM_RI;
        gam_t[i * PBW + c] = (c < a.p && r0 + i < a.n) ? a.gam[(long long)c * a.np + r0 + i] : 0.0;
      }
  };
  pmm_d4 acc[PMM_PG][NCB];
#pragma unroll
  for (int g = 0; g < PMM_PG; ++g)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[g][cb] = pmm_d4{0.0, 0.0, 0.0, 0.0};
  // one step: the lane's rho of each group times the step's block of Gamma
  auto step = [&](int t, const double (&s)[PMM_PG]) {
    double bv[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) bv[cb] = gam_t[(4 * t + lr) * PBW + cb * 16 + lc];
#pragma unroll
    for (int g = 0; g < PMM_PG; ++g) {
      const double av = a.coff * post_mean_rho<FAM>(s[g]);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[g][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[cb], acc[g][cb], 0, 0, 0);
    }
  };
  const int rt1 = min(nrt, (seg + 1) * PM_SEG);
  for (int rt = seg * PM_SEG; rt < rt1; ++rt) {
    const int r0 = rt * PM_RI;
    if constexpr (WIDE) {
      double s[STEPS][PMM_PG];
#pragma unroll
      for (int t = 0; t < STEPS; ++t)
#pragma unroll
        for (int g = 0; g < PMM_PG; ++g) s[t][g] = 0.0;
      for (int c0 = 0; c0 < d; c0 += DMAX) {
        __syncthreads();   // the previous coordinates (and, at c0 = 0, Gamma) have been read
        stage(r0, c0, c0 == 0);
        double xq[PMM_PG][DMAX];
#pragma unroll
        for (int g = 0; g < PMM_PG; ++g) {
          const double* xp = a.xsw + (long long)(pbase + g * 16 + lc) * d;
#pragma unroll
          for (int k = 0; k < DMAX; ++k) xq[g][k] = c0 + k < d ? xp[c0 + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < STEPS; ++t) {
#pragma unroll
          for (int k = 0; k < DMAX; ++k) {
            const double xk = xw_t[(4 * t + lr) * XP + k];
#pragma unroll
            for (int g = 0; g < PMM_PG; ++g) {
              const double df = xk - xq[g][k];
              s[t][g] = fma(df, df, s[t][g]);
            }
          }
        }
      }
#pragma unroll
      for (int t = 0; t < STEPS; ++t) step(t, s[t]);
    } else {
      __syncthreads();   // the previous tile has been read
      stage(r0, 0, true);
      __syncthreads();
#pragma unroll 2
      for (int t = 0; t < STEPS; ++t) {
        double s[PMM_PG];
#pragma unroll
        for (int g = 0; g < PMM_PG; ++g) s[g] = 0.0;
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
          const double xk = xw_t[(4 * t + lr) * XP + k];
#pragma unroll
          for (int g = 0; g < PMM_PG; ++g) {
            const double df = xk - xs[g][k];
            s[g] = fma(df, df, s[g]);
          }
        }
        step(t, s);
      }
    }
  }
#pragma unroll
  for (int g = 0; g < PMM_PG; ++g)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int c = cb * 16 + lc;
      if (c < a.p) {
        double* out = a.part + ((long long)seg * a.p + c) * a.mp + pbase + g * 16 + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[4 * r] = acc[g][cb][r];
      }
    }
}

// y[s][c] (mp x p row-major) = the segments' sums added in index order
static __global__ void k_post_mean_multi_fin(const double* part, int nseg, int p, int mp, double* y) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)p * mp) return;
  const int c = (int)(e / mp), s = (int)(e - (long long)c * mp);
  double acc = part[e];
  for (int j = 1; j < nseg; ++j) acc += part[(long long)j * p * mp + e];
  y[(long long)s * p + c] = acc;
}

}  // namespace gpe
