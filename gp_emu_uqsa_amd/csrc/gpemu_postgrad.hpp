// gpemu_postgrad.hpp -- the gradient of the posterior mean and variance with respect to the
// point (gpe_posterior_grad): the fused sums over the training rows, the per-point tau = Q^-1 T
// and the epilogue that turns the sums into d mean / dx and d var / dx.
//
// With s_i = |xs - x_i|^2 in scaled coordinates and g the family's derivative factor
// (gpemu_kernels.hpp, FAM_*), d K*_i / dx_k = -2 coff g(s_i) (xsw_k - xw_ik) / delta_k, so
//   d mean / dx_k = d_k h . beta - (2 coff / delta_k) a_k,   a_k = sum_i gamma_i g_i (xsw_k - xw_ik)
//   d var / dx_k  = s2 (4 coff / delta_k b_k + 2 tau . d_k h), b_k = sum_i U_i g_i (xsw_k - xw_ik)
// for U = L^-T V + G tau (one column per point).  Nothing divides by r: a point on a training
// point adds 0 for that row.
#pragma once

#include "gpemu_kernels.hpp"

namespace gpe {

// k_post_grad: a lane per point, 128 points per workgroup, the training rows split over
// blockIdx.y.  A lane keeps its point's coordinates and its 2 x DMAX running sums in
// registers.  The rows go by in tiles of PG_RI: their coordinates and gamma sit in LDS and are
// read at one address by the whole wave (a broadcast, no bank conflict); U is column-major
// over the rows, so a lane reading its own column in place would touch one 64-B line per row
// and lane -- instead the tile's 128 x PG_RI block of U is loaded along the rows (coalesced)
// and stored as [point][row] with pitch PG_RI + 1 doubles: odd, so the 32 lanes of a half-wave
// read 32 different bank pairs.  A lane per row would keep U coalesced for free but pay 2 d
// cross-lane reductions per point.
// Each workgroup stores its partial sums; k_post_grad_fin adds them in index order (fixed
// order, no atomics: repeated calls return the same bits).
// d <= 32: one pass, the distance from the registers.  d > 32 (WIDE): blockIdx.z picks the 32
// dimensions whose sums the workgroup keeps; per row tile it first takes the squared distances
// over all dimensions, staged through LDS 32 at a time in k_pairs_wide's order, then the sums.
// Padded rows enter with gamma = U = 0; padded points are dropped by the epilogue.
constexpr int PG_PTS = 128, PG_RI = 32, PG_UP = PG_RI + 1, PG_WIDE = 32;

struct PostGradArgs {
  const double* xw;    // scaled training points (np x d, row-major)
  const double* xsw;   // scaled points of the chunk (mp x d, row-major)
  const double* gam;   // gamma = A^-1 (f - H beta) (np)
  const double* U;     // np x mp column-major (ldu), read only by the WB instances
  long long ldu;
  double* part;        // a sums [nsplit][mp][d], then the b sums the same
  int n, np, mp, d, nsplit;
};

template <int FAM>
__device__ inline double post_grad_g(double s) {
  if constexpr (FAM == FAM_GAUSS) {
    return exp(-s);
  } else {
    double rho, g;
    matern_rho_g<FAM>(s, rho, g);
    return g;
  }
}

template <int DMAX, int FAM, bool WIDE, bool WB>
static __global__ void __launch_bounds__(PG_PTS) k_post_grad(PostGradArgs a) {
  __shared__ double xw_t[PG_RI * DMAX];
  __shared__ double gam_t[PG_RI];
  __shared__ double u_t[WB ? PG_PTS * PG_UP : 1];
  const int tid = threadIdx.x, d = a.d;
  const int p0 = (int)blockIdx.x * PG_PTS, sp = p0 + tid;
  const int k0 = (int)blockIdx.z * DMAX;
  const int nrt = a.np / PG_RI, per = (nrt + a.nsplit - 1) / a.nsplit;
  const int rt0 = (int)blockIdx.y * per, rt1 = min(nrt, rt0 + per);
  const double* xp = a.xsw + (long long)sp * d;
  double xs[DMAX], aa[DMAX], bb[DMAX];
#pragma unroll
  for (int k = 0; k < DMAX; ++k) {
    xs[k] = k0 + k < d ? xp[k0 + k] : 0.0;
    aa[k] = 0.0;
    bb[k] = 0.0;
  }
  // the rows' coordinates of dimensions c0 .. c0 + DMAX, zero beyond d
  auto stage_x = [&](int r0, int c0) {
    for (int e = tid; e < PG_RI * DMAX; e += PG_PTS) {
      const int i = e / DMAX, k = e - i * DMAX;
      xw_t[e] = c0 + k < d ? a.xw[(long long)(r0 + i) * d + c0 + k] : 0.0;
    }
  };
  for (int rt = rt0; rt < rt1; ++rt) {
    const int r0 = rt * PG_RI;
    double s[WIDE ? PG_RI : 1];
    if constexpr (WIDE) {
#pragma unroll
      for (int i = 0; i < PG_RI; ++i) s[i] = 0.0;
      for (int c0 = 0; c0 < d; c0 += DMAX) {
        __syncthreads();
        stage_x(r0, c0);
        double xq[DMAX];
#pragma unroll
        for (int k = 0; k < DMAX; ++k) xq[k] = c0 + k < d ? xp[c0 + k] : 0.0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PG_RI; ++i) {
#pragma unroll
          for (int k = 0; k < DMAX; ++k) {
            const double df = xq[k] - xw_t[i * DMAX + k];
            s[i] = fma(df, df, s[i]);
          }
        }
      }
    }
    __syncthreads();   // the previous tile has been read
    stage_x(r0, k0);
    if (tid < PG_RI) gam_t[tid] = r0 + tid < a.n ? a.gam[r0 + tid] : 0.0;
    if constexpr (WB) {
      const int i = tid % PG_RI;
      const bool live = r0 + i < a.n;
      const double* up = a.U + (r0 + i) + (long long)p0 * a.ldu;
      for (int p = tid / PG_RI; p < PG_PTS; p += PG_PTS / PG_RI)
        u_t[p * PG_UP + i] = live ? up[(long long)p * a.ldu] : 0.0;
    }
    __syncthreads();
    auto row = [&](int i, double si, const double* df) {
      const double g = post_grad_g<FAM>(si);
      const double wa = gam_t[i] * g;
#pragma unroll
      for (int k = 0; k < DMAX; ++k) aa[k] = fma(wa, df[k], aa[k]);
      if constexpr (WB) {
        const double wb = u_t[tid * PG_UP + i] * g;
#pragma unroll
        for (int k = 0; k < DMAX; ++k) bb[k] = fma(wb, df[k], bb[k]);
      }
    };
    if constexpr (WIDE) {
#pragma unroll
      for (int i = 0; i < PG_RI; ++i) {
        double df[DMAX];
#pragma unroll
        for (int k = 0; k < DMAX; ++k) df[k] = xs[k] - xw_t[i * DMAX + k];
        row(i, s[i], df);
      }
    } else {
#pragma unroll 2
      for (int i = 0; i < PG_RI; ++i) {
        double df[DMAX], si = 0.0;
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
          df[k] = xs[k] - xw_t[i * DMAX + k];
          si = fma(df[k], df[k], si);
        }
        row(i, si, df);
      }
    }
  }
  const long long slab = (long long)a.mp * d;
  double* pa = a.part + (long long)blockIdx.y * slab + (long long)sp * d + k0;
#pragma unroll
  for (int k = 0; k < DMAX; ++k)
    if (k0 + k < d) pa[k] = aa[k];
  if constexpr (WB) {
    double* pb = pa + (long long)a.nsplit * slab;
#pragma unroll
    for (int k = 0; k < DMAX; ++k)
      if (k0 + k < d) pb[k] = bb[k];
  }
}

// tau = Q^-1 (hs - G^T K*) per point, from the chunk's Y = K*^T [gamma, G] (mp x (q + 1)
// column-major): tau (mp x kq column-major, zero beyond q columns and mc points), the second
// operand of the rank-q update U += G tau^T.
static __global__ void k_post_tau(const double* Y, int mp, int mc, int q, int kq, const double* Hs,
                                  const double* Qinv, double* tau) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)mp * kq) return;
  const int s = (int)(e % mp), o = (int)(e / mp);
  double acc = 0.0;
  if (s < mc && o < q)
    for (int i = 0; i < q; ++i)
      acc = fma(Qinv[o * q + i], Hs[(long long)s * q + i] - Y[s + (long long)(i + 1) * mp], acc);
  tau[e] = acc;
}

struct PostGradFin {
  const double* part;      // k_post_grad's partial sums
  const double* invdelta;  // 1 / delta (d)
  const double* dHs;       // each basis column's derivative in its own input (mc x q, row-major)
  const int* hdim;         // the input of each basis column, -1: constant (q)
  const double* beta;      // (q)
  const double* tau;       // mp x kq column-major (dvar only)
  double* dmean;           // mp x d row-major
  double* dvar;            // mp x d row-major, or NULL
  double coff, s2;
  int nsplit, mp, mc, d, q;
};

// The partial sums added in index order, then the factors and the basis terms.
static __global__ void k_post_grad_fin(PostGradFin f) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long slab = (long long)f.mp * f.d;
  if (e >= slab) return;
  const int s = (int)(e / f.d), k = (int)(e - (long long)s * f.d);
  if (s >= f.mc) {
    f.dmean[e] = 0.0;
    if (f.dvar) f.dvar[e] = 0.0;
    return;
  }
  double a = 0.0, b = 0.0;
  for (int j = 0; j < f.nsplit; ++j) a += f.part[j * slab + e];
  if (f.dvar)
    for (int j = 0; j < f.nsplit; ++j) b += f.part[(f.nsplit + j) * slab + e];
  double hm = 0.0, hv = 0.0;
  for (int j = 0; j < f.q; ++j)
    if (f.hdim[j] == k) {
      const double dh = f.dHs[(long long)s * f.q + j];
      hm = fma(dh, f.beta[j], hm);
      if (f.dvar) hv = fma(dh, f.tau[s + (long long)j * f.mp], hv);
    }
  const double w = -2.0 * f.coff * f.invdelta[k];
  f.dmean[e] = fma(w, a, hm);
  if (f.dvar) f.dvar[e] = f.s2 * (2.0 * hv - 2.0 * w * b);
}

}  // namespace gpe
