// gpemu_hm.hpp -- history matching over a resident set of emulators (gpe_hm_*): from the
// candidate points to the implausibility without K* or V = L^-1 K* in memory.
//
//   k_hm_pack    an emulator's L^-1 and [gamma, G] into MFMA operand order (gpe_hm_add, once)
//   k_hm_post    one workgroup per tile of points: K* in LDS, V on the fp64 matrix cores row
//                block by row block, |V|^2, [gamma, G]^T K* from the same loop, the q x q tail,
//                the variance and I^2 (one launch per emulator and chunk)
//   k_hm_select  per point the maxno largest sqrt(I^2) over the emulators, ascending, NaN last
//
// Every K* entry is k_pairs' (gpemu_kernels.hpp): the scaled coordinates of k_scale_points
// (x / delta as x * (1 / delta)), df = xw_ik - xsw_sk and s = fma(df, df, s) over k = 0 .. d - 1
// in that order, exp(-s) or matern_rho_g<FAM>, then coff.  The mean and the variance are
// Posterior::point()'s formulas (gpemu.hip) in its order of operations; only the order of the
// sums over the training rows is this file's, and it depends on n alone: the results do not
// depend on m, the chunk length or the tile a point falls in, and there are no floating-point
// atomics.  Layouts and sizes: gpemu_hm_plan.hpp.
#pragma once

#include <type_traits>

#include "gpemu_hm_plan.hpp"
#include "gpemu_postmean.hpp"

namespace gpe {

typedef double hm_d4 __attribute__((ext_vector_type(4)));

// One workgroup per block of the packed matrix.  Linv: the context's L^-1 (column-major, ld;
// only entries on and below the diagonal are read).  The blocks behind L^-1's hold p + q rows:
// rows [0, p) the columns of Gam, rows [p, p + q) those of G (both column-major, ld).  A single
// emulator has p = 1, Gam = gamma and G behind it in [gamma, G] = A^-1 [f - H beta, H]; a
// multi-output member Gam = Gamma = A^-1 (F - H B).  Rows from n on, columns from n on, rows
// from p + q on and everything above the diagonal are written as zeros.
static __global__ void __launch_bounds__(256) k_hm_pack(const double* Linv, const double* Gam, const double* G,
                                                       long long ld, int n, int p, int q, double* W) {
  const int nrb = hm_nrb(n), b = (int)blockIdx.x;
  const int cnt = hm_block_steps(nrb, b) * HM_STEP;
  double* dst = W + hm_block_first(nrb, b) * HM_STEP;
  for (int e = (int)threadIdx.x; e < cnt; e += (int)blockDim.x) {
    const int lane = e & (HM_STEP - 1), r = lane & (HM_RB - 1), k = (e / HM_STEP) * HM_KS + lane / HM_RB;
    double v = 0.0;
    if (b < nrb) {
      const int i = b * HM_RB + r;
      if (i < n && k <= i) v = Linv[i + (long long)k * ld];
    } else {
      const int j = (b - nrb) * HM_RB + r;
      if (k < n) {
        if (j < p) v = Gam[k + (long long)j * ld];
        else if (j < p + q) v = G[k + (long long)(j - p) * ld];
      }
    }
    dst[e] = v;
  }
}

struct HmPostArgs {
  const double* xw;        // scaled training rows (n x d, row-major)
  const double* invdelta;  // d
  const int* active;       // d columns of the candidate rows
  const double* W;         // the packed matrix
  const int* hdim;         // q: -1 a constant column, else the active input
  const double* hval;      // q: the constants
  const double* beta;      // q
  const double* kinv;      // Kq^-1 (q x q row-major), Kq Kq^T = H^T A^-1 H
  const double* Xs;        // the chunk's candidate rows (mc x D)
  double* i2;              // mc
  double* mean;            // mc, or NULL
  double* var;             // mc, or NULL
  double z, ve, s2, coff, cdiag;
  int n, d, q, D, mc;
};

// The tail of k_hm_post for one point (column pt of the tile's yb and ssb, point s of the chunk):
// Posterior::point()'s mean and T Kq^-T row by row, the variance and I^2.  t_i = h_i - (G^T K*)_i
// replaces row 1 + i of yb in place (this thread's column).  No contraction here: the variance that
// is stored is the one that is divided by, so I^2 is NumPy's expression of the returned mean and
// variance bit for bit, and the sums run as the host's in Posterior::point() do.
__device__ inline void hm_point(const HmPostArgs& a, double* yb, const double* ssb, int PT, int pt, long long s) {
#pragma clang fp contract(off)
  const int q = a.q;
  double nrm = ssb[pt];
  for (int j = 1; j < 16; ++j) nrm += ssb[j * PT + pt];
  const double* xrow = a.Xs + s * a.D;
  double mu = yb[pt];
  for (int i = 0; i < q; ++i) {
    const double h = a.hdim[i] < 0 ? a.hval[i] : xrow[a.active[a.hdim[i]]];
    mu += h * a.beta[i];
    yb[(1 + i) * PT + pt] = h - yb[(1 + i) * PT + pt];
  }
  double tq = 0.0;
  for (int o = 0; o < q; ++o) {
    double acc = 0.0;
    for (int i = 0; i < q; ++i) acc += yb[(1 + i) * PT + pt] * a.kinv[o * q + i];
    tq += acc * acc;
  }
  const double var = a.s2 * (a.cdiag - nrm + tq);
  const double dz = mu - a.z;
  a.i2[s] = dz * dz / (var + a.ve);
  if (a.mean) a.mean[s] = mu;
  if (a.var) a.var[s] = var;
}

// A member of p outputs (gpe_hm_add_multi): the packed matrix holds [Gamma, G] behind L^-1, so yb
// has rows [0, p) Gamma^T K* and rows [p, p + q) G^T K*.  beta, z, ve, s2 of HmPostArgs are not
// read.  Univariate mode (gpe_hm_implausibility): output a goes to row a of i2, mean and var
// (leading dimension ldo).  Joint mode (gpe_hm_implausibility_mv): i2 one value per point, mean
// p rows, var one row (c).
struct HmPostMultiArgs : HmPostArgs {
  const double* B;       // q x p row-major
  const double* sdiag;   // p: Sigma_aa
  const double* Wj;      // joint: p x p row-major, W^T V W = I, W^T Sigma W = Lambda (gpemu_hm_mv.hpp)
  const double* lam;     // joint: p
  long long ldo;
  int p, joint;
  double zs[HM_MAX_ROWS], ves[HM_MAX_ROWS];   // p: the observations; univariate: var_extra
};

// The tail of a multi-output member for one point: c is hm_point's variance at sigma = 1 in its
// order of operations; the means and the residuals live in rows [0, p) of yb, in this thread's
// column, so nothing of length p is held in registers.
//   t_i = h_i - yb[p + i] (in place), tq = |t Kq^-T|^2, c = cdiag - nrm + tq
//   mu_a = yb[a] + sum_i h_i B[i, a], i = 0 .. q - 1 in order
//   univariate: I^2_a = (mu_a - z_a)^2 / (Sigma_aa c + ve_a)
//   joint: r_a = mu_a - z_a, y_j = sum_a W[a, j] r_a (a in order), I^2 = sum_j y_j^2 / (c lam_j + 1)
// No contraction, as hm_point: NumPy restates every line on the returned parts.
__device__ inline void hm_point_multi(const HmPostMultiArgs& a, double* yb, const double* ssb, int PT, int pt,
                                      long long s) {
#pragma clang fp contract(off)
  const int q = a.q, p = a.p;
  double nrm = ssb[pt];
  for (int j = 1; j < 16; ++j) nrm += ssb[j * PT + pt];
  const double* xrow = a.Xs + s * a.D;
  for (int i = 0; i < q; ++i) {
    const double h = a.hdim[i] < 0 ? a.hval[i] : xrow[a.active[a.hdim[i]]];
    yb[(p + i) * PT + pt] = h - yb[(p + i) * PT + pt];
    for (int o = 0; o < p; ++o) yb[o * PT + pt] += h * a.B[i * p + o];
  }
  double tq = 0.0;
  for (int o = 0; o < q; ++o) {
    double acc = 0.0;
    for (int i = 0; i < q; ++i) acc += yb[(p + i) * PT + pt] * a.kinv[o * q + i];
    tq += acc * acc;
  }
  const double c = a.cdiag - nrm + tq;
  if (!a.joint) {
    for (int o = 0; o < p; ++o) {
      const double mu = yb[o * PT + pt], var = a.sdiag[o] * c;
      const double dz = mu - a.zs[o];
      a.i2[o * a.ldo + s] = dz * dz / (var + a.ves[o]);
      if (a.mean) a.mean[o * a.ldo + s] = mu;
      if (a.var) a.var[o * a.ldo + s] = var;
    }
    return;
  }
  for (int o = 0; o < p; ++o) {
    const double mu = yb[o * PT + pt];
    if (a.mean) a.mean[o * a.ldo + s] = mu;
    yb[o * PT + pt] = mu - a.zs[o];
  }
  double i2 = 0.0;
  for (int j = 0; j < p; ++j) {
    double y = 0.0;
    for (int o = 0; o < p; ++o) y += a.Wj[o * p + j] * yb[o * PT + pt];
    i2 += y * y / (c * a.lam[j] + 1.0);
  }
  a.i2[s] = i2;
  if (a.var) a.var[s] = c;
}

// PT points per workgroup of HM_WAVES waves.  LDS: kst, the tile's K* (n16 x PT, rows from n on
// zero); behind it 48 PT doubles: first the tile's scaled points (PT x (d | 1): the odd pitch
// keeps the points of a wave in different banks), then yb (32 x PT: [gamma, G]^T K*) and ssb
// (16 x PT: the waves' and lane groups' sums of squares).
// The blocks of the packed matrix are dealt to the waves from the longest down, back and forth,
// so that the waves' MFMA counts differ by less than one block.  Per block and step of 4 columns
// it loads one A operand (512 contiguous bytes, from L2) and multiplies it by the PT / 16 B
// operands of the step from LDS (lane l: K*(4 step + (l >> 4), point 16 g + (l & 15))); the
// next 16 columns' operands are loaded before the current ones are multiplied.  D (lane l,
// register r) is row (l >> 4) + 4 r of the block at point 16 g + (l & 15).  A row block of
// L^-1 ends in the squares of its 4 registers added, r = 0 .. 3, to the lane's sum; a block of
// [gamma, G] is stored to yb.  The tail, one thread per point, adds the 16 sums of a point in
// the order wave 0 .. 3, lane group 0 .. 3.
// Points from mc on enter with zero coordinates, are computed and never stored.
// Args = HmPostMultiArgs: the instances of a multi-output member, which differ in the number of
// blocks behind L^-1's (p + q rows in place of 1 + q) and in the tail alone.
template <int FAM, int PT, class Args = HmPostArgs>
static __global__ void __launch_bounds__(HM_LANES) k_hm_post(Args a) {
  constexpr int NG = PT / 16;
  constexpr bool MULTI = std::is_same<Args, HmPostMultiArgs>::value;
  extern __shared__ __attribute__((aligned(16))) double hm_lds[];
  const int n = a.n, d = a.d, q = a.q, n16 = hm_n16(n), nrb = hm_nrb(n);
  double* kst = hm_lds;
  double* xs_t = hm_lds + (long long)n16 * PT;
  double* yb = xs_t;
  double* ssb = xs_t + 32 * PT;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane >> 4, lc = lane & 15;
  const long long s0 = (long long)blockIdx.x * PT;
  const int XP = d | 1;
  // the tile's scaled points
  for (int e = tid; e < PT * d; e += HM_LANES) {
    const int pt = e / d, k = e - pt * d;
    xs_t[pt * XP + k] = s0 + pt < a.mc ? a.Xs[(s0 + pt) * a.D + a.active[k]] * a.invdelta[k] : 0.0;
  }
  __syncthreads();
  // K*
  for (int e = tid; e < n16 * PT; e += HM_LANES) {
    const int i = e / PT, pt = e - i * PT;
    double v = 0.0;
    if (i < n) {
      const double* xi = a.xw + (long long)i * d;
      double s = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = xi[k] - xs_t[pt * XP + k];
        s = fma(df, df, s);
      }
      v = a.coff * post_mean_rho<FAM>(s);
    }
    kst[e] = v;
  }
  __syncthreads();   // (xs_t has been read: yb and ssb may be written)
  double ss[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) ss[g] = 0.0;
  int nb;
  if constexpr (MULTI) nb = nrb + hm_nxb_rows(a.p + q);
  else nb = nrb + hm_nxb(q);
  for (int i = 0; i < nb; ++i) {
    // the blocks from the longest down, dealt to the waves back and forth (0 1 2 3 3 2 1 0 ...)
    const int pos = i & (2 * HM_WAVES - 1);
    if ((pos < HM_WAVES ? pos : 2 * HM_WAVES - 1 - pos) != wave) continue;
    const int b = nb - 1 - i;
    const int steps = hm_block_steps(nrb, b);   // (a multiple of 4)
    const double* wp = a.W + hm_block_first(nrb, b) * HM_STEP + lane;
    hm_d4 acc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = hm_d4{0.0, 0.0, 0.0, 0.0};
    double av[HM_KS], an[HM_KS];
#pragma unroll
    for (int u = 0; u < HM_KS; ++u) av[u] = wp[u * HM_STEP];
    for (int t = 0; t < steps; t += HM_KS) {
      const bool more = t + HM_KS < steps;
#pragma unroll
      for (int u = 0; u < HM_KS; ++u) an[u] = more ? wp[(t + HM_KS + u) * HM_STEP] : 0.0;
#pragma unroll
      for (int u = 0; u < HM_KS; ++u) {
        const double* kp = kst + ((t + u) * HM_KS + lr) * PT + lc;
#pragma unroll
        for (int g = 0; g < NG; ++g)
          acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], kp[16 * g], acc[g], 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < HM_KS; ++u) av[u] = an[u];
    }
    if (b < nrb) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) ss[g] = fma(acc[g][r], acc[g][r], ss[g]);
    } else {
      const int j0 = (b - nrb) * HM_RB + lr;
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) yb[(j0 + 4 * r) * PT + 16 * g + lc] = acc[g][r];
    }
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) ssb[(wave * 4 + lr) * PT + 16 * g + lc] = ss[g];
  __syncthreads();
  if (tid < PT && s0 + tid < a.mc) {
    if constexpr (MULTI) hm_point_multi(a, yb, ssb, PT, tid, s0 + tid);
    else hm_point(a, yb, ssb, PT, tid, s0 + tid);
  }
}

// a < b with a NaN above every number (np.sort's order)
__device__ inline bool hm_less(double a, double b) { return a == a && (b != b || a < b); }

// One thread per point: I = sqrt(I^2[o][s]) for the p emulators (I^2: p x ld), the maxno largest
// kept ascending in registers (an insertion per value; every loop is unrolled to the set's limit
// so that the array stays in registers), then stored to out (mc x maxno).
static __global__ void __launch_bounds__(256) k_hm_select(const double* i2, long long ld, int p, int maxno, int mc,
                                                         double* out) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= mc) return;
  double top[HM_MAX_EMUL];
#pragma unroll
  for (int j = 0; j < HM_MAX_EMUL; ++j) top[j] = -INFINITY;
  for (int o = 0; o < p; ++o) {
    const double v = sqrt(i2[(long long)o * ld + s]);
    if (hm_less(v, top[0])) continue;
    top[0] = v;
#pragma unroll
    for (int j = 0; j + 1 < HM_MAX_EMUL; ++j)
      if (j + 1 < maxno && hm_less(top[j + 1], top[j])) {
        const double t = top[j];
        top[j] = top[j + 1];
        top[j + 1] = t;
      }
  }
#pragma unroll
  for (int j = 0; j < HM_MAX_EMUL; ++j)
    if (j < maxno) out[(long long)s * maxno + j] = top[j];
}

}  // namespace gpe
