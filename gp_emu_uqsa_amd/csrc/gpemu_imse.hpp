// gpemu_imse.hpp -- the pick loop of gpe_posterior_imse: the greedy integrated-variance (IMSE,
// Cohn's ALC) batch among the first m_c of the m points whose posterior covariance S
// posterior_impl(keep_dev) leaves on the device (symmetric, column-major, ld = m_pad); the last
// m_r = m - m_c points are the reference sample the variance is averaged over.
//
// State besides gpemu_pivchol.hpp's (d, the chosen flags, the panel W of L over the candidate
// rows): C (m_r x m_c, column-major, ld = m_r rounded up to 2 so that every column starts on
// 16 bytes, columns rounded up to IM_NC; the padding holds zeros), the cross-covariance of the
// reference points with the candidates given the picks so far, copied out of S once
// (k_im_copy) so that the lazy trailing update S -= W W^T never touches it.
//
// Two launches per pick, no waits between workgroups:
//   k_im_col, step t (as k_pc_step, over the candidate rows only):
//     1. reduces the (score, index) partials the previous sweep wrote to the pick p (score
//        descending, then index ascending; an ineligible candidate carries index -1); nobody
//        eligible: the stop flag, and every later launch returns at once,
//     2. forms its 64 rows of l = (S[:, p] - W[:, :j] W[p, :j]^T) / sqrt(d_p) into column j of
//        W (sqrt(d_p) at p, exactly 0 at candidates chosen earlier and at rows >= m_c) and
//        downdates d,
//     3. writes its share of lambda = C[:, p] / sqrt(d_p) into a vector of its own: the sweep
//        skips column p from now on and reads only that vector,
//     4. (workgroup 0) records piv, gain = score_p, pivvar = d_p and the rank.
//   k_im_sweep<DOWN> (the hot path: one read and one write of C per pick): a workgroup owns
//     IM_NC columns; per chunk of 1024 rows a lane loads its two row pairs of lambda and w once
//     (16-byte loads) and runs down the IM_NC columns with them: C[:, c] -= lambda l_c, stored
//     back for unchosen c, and q_c += w C^2.  Then score_c = q_c / d_c, and the workgroup's best
//     eligible (unchosen, d_c > thr, score not NaN) candidate goes to the partials of the other
//     parity.  DOWN = false is step 0's scores: the same pass without the downdate.
// Sums run in an order fixed by the code: a lane adds its rows in ascending order (x then y of a
// pair), the wave's lanes by an xor tree, the four waves in wave order.  Nothing depends on the
// grid or on scheduling; no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "gpemu_pivchol.hpp"

namespace gpe {

constexpr int IM_NC = 8;                    // columns of C per workgroup of the sweep
constexpr int IM_U = 2;                     // row pairs per lane and chunk
constexpr int IM_CHUNK = 256 * 2 * IM_U;    // rows per chunk

struct ImState {
  double thr;     // tol * max d^0 over the candidates
  int stop;       // nobody eligible: later launches are no-ops
  int rank;       // picks taken
  double imse0;   // sum_r w_r S[m_c + r, m_c + r]
};

struct ImArgs {
  const double* S;   // covariance, column-major m_pad x m_pad (symmetric)
  long long ld;      // m_pad (a multiple of 128)
  int mc;            // candidates: rows / columns [0, mc) of S
  int mr;            // reference points: rows [mc, mc + mr) of S
  int Gc;            // workgroups of k_im_col: 64 rows each, Gc * 64 = mc rounded up to 128
  int Gs;            // workgroups of k_im_sweep = ceil(mc / IM_NC)
  double* C;         // ldc x (Gs * IM_NC)
  long long ldc;     // mr rounded up to 2
  double* lam;       // ldc
  const double* w;   // ldc weights (padding 0)
  double* d;         // Gc * 64 remaining variances of the candidates
  int* chosen;       // Gc * 64 flags (padding: 1)
  double* psc;       // 2 x Gs partial best scores (by step parity)
  int* pidx;         // 2 x Gs their candidates (-1: none eligible)
  ImState* st;
  int* piv;          // k
  double* gain;      // k
  double* pivvar;    // k
  double tol;
};

// d^0, the flags, thr, imse0, piv / gain / pivvar = -1 / 0 / 0 and the state: one workgroup.
// imse0 is summed in index order (products staged through LDS, then added by one lane).
__global__ __launch_bounds__(256) void k_im_init(ImArgs a, int k) {
  __shared__ double s_p[2048];
  __shared__ double s_v[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double mx = -INFINITY;
  for (int i = tid; i < a.Gc * PC_ROWS; i += 256) {
    const bool live = i < a.mc;
    const double v = live ? a.S[i + (long long)i * a.ld] : 0.0;
    a.d[i] = v;
    a.chosen[i] = live ? 0 : 1;
    if (live && v > mx) mx = v;   // a NaN is never greater
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) s_v[wave] = mx;
  for (int t = tid; t < k; t += 256) {
    a.piv[t] = -1;
    a.gain[t] = 0.0;
    a.pivvar[t] = 0.0;
  }
  double sum = 0.0;
  for (int r0 = 0; r0 < a.mr; r0 += 2048) {
    __syncthreads();
    for (int r = r0 + tid; r < min(r0 + 2048, a.mr); r += 256) {
      const long long i = a.mc + r;
      s_p[r - r0] = a.w[r] * a.S[i + i * a.ld];
    }
    __syncthreads();
    if (tid == 0)
      for (int r = 0; r < min(2048, a.mr - r0); ++r) sum += s_p[r];
  }
  __syncthreads();
  if (tid == 0) {
    mx = fmax(fmax(s_v[0], s_v[1]), fmax(s_v[2], s_v[3]));
    a.st->thr = a.tol * mx;
    a.st->stop = 0;
    a.st->rank = 0;
    a.st->imse0 = sum;
  }
}

// C = S[mc.., 0..mc) with zeros in the padding rows and columns; grid (ceil(ldc / 256), Gs * IM_NC)
__global__ __launch_bounds__(256) void k_im_copy(ImArgs a) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (r >= a.ldc) return;
  a.C[r + (long long)c * a.ldc] = (r < a.mr && c < a.mc) ? a.S[(a.mc + r) + (long long)c * a.ld] : 0.0;
}

// pick t, column j = t % 128 of the panel W
__global__ __launch_bounds__(256) void k_im_col(ImArgs a, double* __restrict__ W, int t, int j) {
  __shared__ double s_v[4];
  __shared__ int s_i[4];
  __shared__ int s_stop;
  __shared__ double s_wp[PC_PANEL];
  __shared__ double s_acc[3][PC_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int par = t & 1;
  // 1. the pick, from the previous sweep's partials
  const double* ps = a.psc + (long long)par * a.Gs;
  const int* pi = a.pidx + (long long)par * a.Gs;
  double bv = -INFINITY;
  int bi = -1;
  for (int g = tid; g < a.Gs; g += 256) pc_better(bv, bi, ps[g], pi[g]);
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
  if (p < 0) {   // every workgroup decides the same; workgroup 0 records it
    if (blockIdx.x == 0 && tid == 0) a.st->stop = 1;
    return;
  }
  const double dp = a.d[p];   // (entry p is not written in this launch)
  const double rt = __dsqrt_rn(dp);
  // 2. row p of the panel's earlier columns, then this slab of l
  for (int s = tid; s < j; s += 256) s_wp[s] = W[p + (long long)s * a.ld];
  const int i = blockIdx.x * PC_ROWS + lane;   // < Gc * 64 <= m_pad
  const double sp = wave == 0 ? a.S[i + (long long)p * a.ld] : 0.0;
  __syncthreads();
  const double* wr = W + i;
  double acc = 0.0;
#pragma unroll 8
  for (int s = wave; s < j; s += 4) acc = fma(wr[(long long)s * a.ld], s_wp[s], acc);
  if (wave) s_acc[wave - 1][lane] = acc;
  // 3. lambda (column p of C is current: the sweeps downdated it while p was unchosen, and
  // no launch writes it from here on)
  const double* cp = a.C + (long long)p * a.ldc;
  for (long long r = (long long)blockIdx.x * 256 + tid; r < a.ldc; r += (long long)a.Gc * 256) a.lam[r] = cp[r] / rt;
  __syncthreads();
  if (wave) return;
  acc = ((acc + s_acc[0][lane]) + s_acc[1][lane]) + s_acc[2][lane];
  const double c = sp - acc;
  double l = 0.0;
  if (i < a.mc) {
    if (i == p) {
      l = rt;
      a.chosen[i] = 1;
    } else if (!a.chosen[i]) {
      l = c / rt;
      a.d[i] = fma(-l, l, a.d[i]);
    }
  }
  W[i + (long long)j * a.ld] = l;
  // 4. the outputs
  if (blockIdx.x == 0 && lane == 0) {
    a.piv[t] = p;
    a.gain[t] = bv;
    a.pivvar[t] = dp;
    a.st->rank = t + 1;
  }
}

// The sweep after pick t (DOWN; ell = column j of W) or before pick 0 (!DOWN): its partials go
// to parity (t + 1) & 1, which the next k_im_col reads.
template <bool DOWN>
__global__ __launch_bounds__(256) void k_im_sweep(ImArgs a, const double* __restrict__ ell, int t) {
  __shared__ double s_q[4][IM_NC];
  if (a.st->stop) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * IM_NC;   // c0 + IM_NC <= the padded columns of C
  bool live[IM_NC];
  double lc[IM_NC], q[IM_NC];
#pragma unroll
  for (int cc = 0; cc < IM_NC; ++cc) {
    const int c = c0 + cc;
    live[cc] = c < a.mc && !a.chosen[c];
    lc[cc] = (DOWN && live[cc]) ? ell[c] : 0.0;
    q[cc] = 0.0;
  }
  double* cb = a.C + (long long)c0 * a.ldc;
  for (long long r0 = 0; r0 < a.ldc; r0 += IM_CHUNK) {
    double2 lam[IM_U], w[IM_U];
    long long r[IM_U];
#pragma unroll
    for (int u = 0; u < IM_U; ++u) {
      r[u] = r0 + 2 * (u * 256 + tid);
      const bool in = r[u] < a.ldc;   // ldc is even: a pair is inside or outside as a whole
      lam[u] = in && DOWN ? *reinterpret_cast<const double2*>(a.lam + r[u]) : make_double2(0.0, 0.0);
      w[u] = in ? *reinterpret_cast<const double2*>(a.w + r[u]) : make_double2(0.0, 0.0);
    }
    double2 v[IM_NC][IM_U];
#pragma unroll
    for (int cc = 0; cc < IM_NC; ++cc)
#pragma unroll
      for (int u = 0; u < IM_U; ++u)
        v[cc][u] = r[u] < a.ldc ? *reinterpret_cast<const double2*>(cb + (long long)cc * a.ldc + r[u])
                                : make_double2(0.0, 0.0);
#pragma unroll
    for (int cc = 0; cc < IM_NC; ++cc)
#pragma unroll
      for (int u = 0; u < IM_U; ++u) {
        double2 x = v[cc][u];
        if (DOWN) {
          x.x = fma(-lam[u].x, lc[cc], x.x);
          x.y = fma(-lam[u].y, lc[cc], x.y);
          if (live[cc] && r[u] < a.ldc) *reinterpret_cast<double2*>(cb + (long long)cc * a.ldc + r[u]) = x;
        }
        q[cc] = fma(w[u].x * x.x, x.x, q[cc]);
        q[cc] = fma(w[u].y * x.y, x.y, q[cc]);
      }
  }
#pragma unroll
  for (int cc = 0; cc < IM_NC; ++cc) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) q[cc] += __shfl_xor(q[cc], off, 64);
    if (lane == 0) s_q[wave][cc] = q[cc];
  }
  __syncthreads();
  if (tid) return;
  const double thr = a.st->thr;
  double bv = -INFINITY;
  int bi = -1;
#pragma unroll
  for (int cc = 0; cc < IM_NC; ++cc) {
    const int c = c0 + cc;
    if (!live[cc]) continue;
    const double dc = a.d[c];
    const double sc = (((s_q[0][cc] + s_q[1][cc]) + s_q[2][cc]) + s_q[3][cc]) / dc;
    pc_better(bv, bi, sc, (dc > thr && sc == sc) ? c : -1);
  }
  const int par = (t + 1) & 1;
  a.psc[(long long)par * a.Gs + blockIdx.x] = bv;
  a.pidx[(long long)par * a.Gs + blockIdx.x] = bi;
}

}  // namespace gpe
