// gpemu_pivchol.hpp -- the pivot loop of gpe_posterior_pivchol: greedy (maximum remaining
// conditional variance) pivoted Cholesky S = P L L^T P^T of the posterior covariance that
// posterior_impl(keep_dev) leaves on the device (symmetric, column-major, ld = m_pad).
//
// One launch per pivot step, no physical swaps.  The remaining variances d, the chosen flags
// and the per-workgroup (max, index) partials live in global fp64 / int32 arrays.  Workgroup g
// owns rows [64 g, 64 g + 64).  A step
//   1. reduces the partials the previous launch wrote to the pivot p (every workgroup the
//      same p: value descending, then index ascending; a NaN never wins),
//   2. forms its rows of c = S[:, p] - W[:, :j] W[p, :j]^T from the panel's earlier columns
//      (W: m_pad x 128, the current panel of L; the panels before it were applied to S by the
//      trailing update S -= W W^T, a grouped MFMA GEMM issued by the host side) and writes
//      column j of W: sqrt(d_p) at row p, c_i / sqrt(d_p) at unchosen rows, exactly 0 at rows
//      chosen earlier and at the padding,
//   3. downdates d, marks p chosen and writes its slab's partial for the next step (the
//      partials are double-buffered by step parity: other workgroups may still read this
//      step's).
// Workgroup 0 records p, d_p and the number of steps taken.  The stop rule (k steps, or
// d_p <= tol max d^0) is decided on the device: a stopped factorisation's later launches
// return at once.  Sums run in a fixed order (wave w of a workgroup takes columns w, w + 4,
// ..., the four partial sums are added in wave order), so a call's bits do not depend on
// scheduling.  k_pc_panel_out stores a finished panel into the row-major device copy of L.
#pragma once
#include <hip/hip_runtime.h>

namespace gpe {

constexpr int PC_PANEL = 128;   // pivots per panel (K of the trailing update)
constexpr int PC_ROWS = 64;     // rows per workgroup of the step kernel (one per lane)

struct PcState {
  double thr;   // tol * max d^0, set by step 0
  int stop;     // the stop rule fired: later steps are no-ops
  int rank;     // steps taken
};

struct PcArgs {
  const double* S;   // covariance, column-major m_pad x m_pad (symmetric)
  long long ld;      // m_pad (a multiple of 128)
  int m;             // points taking part (rows / columns >= m are padding)
  int G;             // workgroups = m_pad / PC_ROWS
  double* d;         // m_pad remaining variances
  int* chosen;       // m_pad flags (padding: 1)
  double* pmax;      // 2 x G partial maxima (by step parity)
  int* pidx;         // 2 x G their indices (-1: no candidate)
  PcState* st;
  int* piv;          // k
  double* pivvar;    // k
  double tol;
};

// (v, i) replaces (bv, bi) when it is a candidate and larger, or equal with a lower index
__device__ __forceinline__ void pc_better(double& bv, int& bi, double v, int i) {
  if (i >= 0 && (v > bv || (v == bv && (bi < 0 || i < bi)))) {
    bv = v;
    bi = i;
  }
}

// the best (value, index) of the wave's 64 lanes, in every lane
__device__ __forceinline__ void pc_wave_argmax(double& bv, int& bi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    pc_better(bv, bi, ov, oi);
  }
}

// d^0 = diag S, the flags, the first partials, piv / pivvar = -1 / 0, the state
__global__ __launch_bounds__(PC_ROWS) void k_pc_init(PcArgs a, int k) {
  const int lane = threadIdx.x, g = blockIdx.x;
  const int i = g * PC_ROWS + lane;   // < m_pad
  const bool live = i < a.m;
  const double v = live ? a.S[i + (long long)i * a.ld] : 0.0;
  a.d[i] = v;
  a.chosen[i] = live ? 0 : 1;
  double bv = -INFINITY;
  int bi = -1;
  pc_better(bv, bi, v, live ? i : -1);
  pc_wave_argmax(bv, bi);
  if (lane == 0) {
    a.pmax[g] = bv;
    a.pidx[g] = bi;
  }
  for (int t = i; t < k; t += a.G * PC_ROWS) {
    a.piv[t] = -1;
    a.pivvar[t] = 0.0;
  }
  if (i == 0) {
    a.st->thr = 0.0;
    a.st->stop = 0;
    a.st->rank = 0;
  }
}

// pivot step t, column j = t % 128 of the panel W
__global__ __launch_bounds__(256) void k_pc_step(PcArgs a, double* __restrict__ W, int t, int j) {
  __shared__ double s_v[4];
  __shared__ int s_i[4];
  __shared__ int s_stop;
  __shared__ double s_wp[PC_PANEL];
  __shared__ double s_acc[3][PC_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int par = t & 1;
  // 1. the pivot, from the previous launch's partials
  const double* pm = a.pmax + (long long)par * a.G;
  const int* pi = a.pidx + (long long)par * a.G;
  double bv = -INFINITY;
  int bi = -1;
  for (int g = tid; g < a.G; g += 256) pc_better(bv, bi, pm[g], pi[g]);
  pc_wave_argmax(bv, bi);
  if (lane == 0) {
    s_v[wave] = bv;
    s_i[wave] = bi;
  }
  if (tid == 0) s_stop = a.st->stop;
  __syncthreads();
  if (s_stop) return;
  bv = s_v[0];
  bi = s_i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) pc_better(bv, bi, s_v[w], s_i[w]);
  const int p = bi;
  const double dp = bv;
  const double thr = t == 0 ? a.tol * dp : a.st->thr;
  if (p < 0 || !(dp > thr)) {   // every workgroup decides the same; workgroup 0 records it
    if (blockIdx.x == 0 && tid == 0) a.st->stop = 1;
    return;
  }
  // 2. row p of the panel's earlier columns, then this slab of c
  for (int s = tid; s < j; s += 256) s_wp[s] = W[p + (long long)s * a.ld];
  const int i = blockIdx.x * PC_ROWS + lane;   // < m_pad
  const double sp = wave == 0 ? a.S[i + (long long)p * a.ld] : 0.0;
  __syncthreads();
  const double* wr = W + i;
  double acc = 0.0;
#pragma unroll 8
  for (int s = wave; s < j; s += 4) acc = fma(wr[(long long)s * a.ld], s_wp[s], acc);
  if (wave) s_acc[wave - 1][lane] = acc;
  __syncthreads();
  if (wave) return;
  acc = ((acc + s_acc[0][lane]) + s_acc[1][lane]) + s_acc[2][lane];
  const double c = sp - acc;
  const double r = __dsqrt_rn(dp);
  // 3. the new column, the downdate and the slab's partial
  double l = 0.0, cv = -INFINITY;
  int ci = -1;
  if (i < a.m) {
    if (i == p) {
      l = r;
      a.chosen[i] = 1;
    } else if (!a.chosen[i]) {
      l = c / r;
      cv = fma(-l, l, a.d[i]);
      a.d[i] = cv;
      ci = i;
    }
  }
  W[i + (long long)j * a.ld] = l;
  bv = -INFINITY;
  bi = -1;
  pc_better(bv, bi, cv, ci);
  pc_wave_argmax(bv, bi);
  if (lane == 0) {
    a.pmax[(long long)(par ^ 1) * a.G + blockIdx.x] = bv;
    a.pidx[(long long)(par ^ 1) * a.G + blockIdx.x] = bi;
    if (blockIdx.x == 0) {
      a.piv[t] = p;
      a.pivvar[t] = dp;
      a.st->rank = t + 1;
      if (t == 0) a.st->thr = thr;
    }
  }
}

// A finished panel into the device copy of L, row-major m x k as L_out wants it:
// Lr[i, t0 + j] = W[i, j] for the steps taken (t0 + j < rank), 0 for the columns of a stopped
// factorisation (W holds stale values there).  64 x 64 tiles through LDS; grid
// (m_pad / 64, ceil(cols / 64)).
__global__ __launch_bounds__(256) void k_pc_panel_out(const double* __restrict__ W, long long ld, int m, int cols,
                                                       const PcState* st, double* __restrict__ Lr, long long k,
                                                       long long t0) {
  __shared__ double tile[64][65];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
  for (int c = w; c < 64; c += 4) {
    const int j = j0 + c;
    tile[c][lane] = j < cols ? W[(i0 + lane) + (long long)j * ld] : 0.0;   // i0 + lane < m_pad
  }
  __syncthreads();
  const long long rank = st->rank;
  const int j = j0 + lane;
  for (int r = w; r < 64; r += 4) {
    const int i = i0 + r;
    if (i < m && j < cols) Lr[(long long)i * k + t0 + j] = (t0 + j < rank) ? tile[lane][r] : 0.0;
  }
}

}  // namespace gpe
