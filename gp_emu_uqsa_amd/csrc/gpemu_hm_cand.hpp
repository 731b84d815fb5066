// gpemu_hm_cand.hpp -- candidates made and reduced on the device, around the unchanged k_hm_post
// (gpemu_hm.hpp): the generators write the chunk's candidate rows into the buffer k_hm_post
// reads, the reducers turn the chunk's I^2 into what the caller asked for, so that only the
// answer crosses to the host.
//
//   k_hm_mesh      the rows of a mesh of two inputs (gpe_hm_cells): copies of x1, x2 and `others`
//   k_hm_cells     selection and cell reduction in one: per piece (cell n chunk) and level the
//                  NaN-propagating minimum and the count below the cut-off
//   k_hm_draw      the rows of NumPy's PCG64 stream in a box (gpe_hm_sample)
//   k_hm_count     accepted candidates per workgroup of 256
//   k_hm_ranks     the workgroups' counts to ranks in the output, behind the earlier chunks'
//   k_hm_scatter   the accepted rows and their candidate numbers, in stream order
//
// The selection is k_hm_select's (the maxno largest sqrt(I^2), ascending, a NaN above every
// number).  Minima and integer counts do not depend on the order they are combined in, the
// launches of a stream are ordered, and the ranks come from a scan: no atomics, and neither the
// chunk length nor the tile shows in a result.  Layouts, sizes and PCG64: gpemu_hm_cand_plan.hpp.
#pragma once

#include "gpemu_hm.hpp"
#include "gpemu_hm_cand_plan.hpp"

namespace gpe {

// One thread per entry of the chunk's rows [s0, s0 + mc) of the mesh: candidate s = (i g2 + j) ns
// + t has x1[i] in column ca, x2[j] in column cb and others[t, :] in the other columns in
// ascending order.
static __global__ void __launch_bounds__(256) k_hm_mesh(const double* x1, const double* x2, const double* others,
                                                       int D, int ca, int cb, long long g2, long long ns,
                                                       long long s0, long long mc, double* Xs) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= mc * D) return;
  const long long r = e / D, s = s0 + r, cell = s / ns, t = s - cell * ns;
  const int k = (int)(e - r * D);
  double v;
  if (k == ca) v = x1[cell / g2];
  else if (k == cb) v = x2[cell % g2];
  else v = others[t * (D - 2) + (k - (k > ca) - (k > cb))];
  Xs[e] = v;
}

// k_hm_select's insertion for candidate s: top[0 .. maxno) the maxno largest sqrt(I^2) over the p
// outputs, ascending.  An output whose bit of `use` is clear enters with I^2 = 0 exactly and its
// row of i2 is not read.  MX: the register slots, maxno <= MX (HM_TOP_FEW for the usual one to
// four levels, HM_MAX_EMUL otherwise: hm_top_slots).
constexpr int HM_TOP_FEW = 4;
inline int hm_top_slots(int maxno) { return maxno <= HM_TOP_FEW ? HM_TOP_FEW : HM_MAX_EMUL; }
template <int MX>
__device__ inline void hm_top(const double* i2, long long ld, int p, int maxno, unsigned use, long long s,
                              double (&top)[MX]) {
#pragma unroll
  for (int j = 0; j < MX; ++j) top[j] = -INFINITY;
  for (int o = 0; o < p; ++o) {
    const double v = (use >> o) & 1u ? sqrt(i2[(long long)o * ld + s]) : 0.0;
    if (hm_less(v, top[0])) continue;
    top[0] = v;
#pragma unroll
    for (int j = 0; j + 1 < MX; ++j)
      if (j + 1 < maxno && hm_less(top[j + 1], top[j])) {
        const double t = top[j];
        top[j] = top[j + 1];
        top[j + 1] = t;
      }
  }
}

// NumPy's min of two: a NaN wins
__device__ inline double hm_nanmin(double a, double b) { return (a != a || b < a) ? a != a ? a : b : (b != b ? b : a); }

// One workgroup per piece of the chunk [s0, s0 + mc) (hm_piece).  Level l is the (l + 1)-th
// largest sqrt(I^2): top[maxno - 1 - l].  Each thread runs over the piece's samples with stride
// 256, keeping per level a minimum and a count; the lanes of a wave combine them by shuffles, the
// four waves through LDS, and thread l stores level l: over the cell's accumulators where the
// piece starts the cell, combined with them otherwise.  imp, below: maxno x cells.
template <int MX>
static __global__ void __launch_bounds__(HM_LANES) k_hm_cells(const double* i2, long long ld, int p, int maxno,
                                                             unsigned use, double cm, long long s0, long long mc,
                                                             long long ns, long long cells, double* imp,
                                                             long long* below) {
  __shared__ double smin[HM_WAVES][MX];
  __shared__ long long scnt[HM_WAVES][MX];
  const HmPiece pc = hm_piece(s0, mc, ns, (long long)blockIdx.x);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long base = pc.cell * ns - s0;   // the cell's sample 0 in the chunk (may be negative)
  double mn[MX], top[MX];
  long long cnt[MX];
#pragma unroll
  for (int l = 0; l < MX; ++l) mn[l] = INFINITY, cnt[l] = 0;
  for (long long t = pc.t0 + tid; t <= pc.t1; t += HM_LANES) {
    hm_top<MX>(i2, ld, p, maxno, use, base + t, top);
#pragma unroll
    for (int j = 0; j < MX; ++j)
      if (j < maxno) {
        mn[j] = hm_nanmin(mn[j], top[j]);
        cnt[j] += top[j] < cm ? 1 : 0;
      }
  }
#pragma unroll
  for (int j = 0; j < MX; ++j)
    if (j < maxno) {
      double m = mn[j];
      long long c = cnt[j];
      for (int off = 32; off > 0; off >>= 1) {
        m = hm_nanmin(m, __shfl_down(m, off, 64));
        c += __shfl_down(c, off, 64);
      }
      if (lane == 0) smin[wave][j] = m, scnt[wave][j] = c;
    }
  __syncthreads();
  if (tid < maxno) {
    const int j = maxno - 1 - tid;   // level tid
    double m = smin[0][j];
    long long c = scnt[0][j];
    for (int w = 1; w < HM_WAVES; ++w) m = hm_nanmin(m, smin[w][j]), c += scnt[w][j];
    const long long at = (long long)tid * cells + pc.cell;
    if (pc.t0 != 0) m = hm_nanmin(imp[at], m), c += below[at];
    imp[at] = m;
    below[at] = c;
  }
}

// One thread per row of the chunk: row r starts r D steps behind `start`, the state before the
// chunk's first element; coordinate k is the output after k + 1 more steps, mapped into the box.
static __global__ void __launch_bounds__(256) k_hm_draw(const uint64_t* table, int digits, uint64_t start_hi,
                                                       uint64_t start_lo, uint64_t inc_hi, uint64_t inc_lo,
                                                       const double* box, int D, long long mc, double* Xs) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= mc) return;
  const hm_u128 inc = hm_u128_of(inc_hi, inc_lo);
  hm_u128 s = hm_row_state(table, digits, hm_u128_of(start_hi, start_lo), r);
  double* row = Xs + r * D;
  for (int k = 0; k < D; ++k) {
    s = hm_pcg_step(s, inc);
    row[k] = hm_affine(box[k], box[D + k], hm_pcg_double(hm_pcg_output(s)));
  }
}

// accepted: the maxno-th largest sqrt(I^2) is below cm (a NaN is not)
template <int MX>
__device__ inline bool hm_accepted(const double* i2, long long ld, int p, int maxno, double cm, long long s) {
  double top[MX];
  hm_top<MX>(i2, ld, p, maxno, ~0u, s, top);
  return top[0] < cm;
}

// counts[b]: the accepted among candidates [256 b, 256 b + 256) of the chunk
template <int MX>
static __global__ void __launch_bounds__(HM_ACC_BLOCK) k_hm_count(const double* i2, long long ld, int p, int maxno,
                                                                 double cm, long long mc, long long* counts) {
  __shared__ int wc[HM_ACC_BLOCK / 64];
  const long long s = (long long)blockIdx.x * HM_ACC_BLOCK + threadIdx.x;
  const bool ok = s < mc && hm_accepted<MX>(i2, ld, p, maxno, cm, s);
  const unsigned long long b = __ballot(ok);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int w = 0; w < HM_ACC_BLOCK / 64; ++w) c += wc[w];
    counts[blockIdx.x] = c;
  }
}

// One workgroup: counts[0 .. nb) to ranks in place (the accepted before workgroup b, earlier
// chunks included: *total on entry), and *total grows by their sum.  Tiles of 256 counts: a scan
// by shuffles inside each wave, the waves' sums and the carry through LDS.
static __global__ void __launch_bounds__(256) k_hm_ranks(long long* counts, long long nb, long long* total) {
  __shared__ long long ws[4];
  __shared__ long long carry;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry = *total;
  __syncthreads();
  for (long long b0 = 0; b0 < nb; b0 += 256) {
    const long long b = b0 + tid;
    const long long c = b < nb ? counts[b] : 0;
    long long inc = c;   // inclusive scan over the wave
    for (int off = 1; off < 64; off <<= 1) {
      const long long o = __shfl_up(inc, off, 64);
      if (lane >= off) inc += o;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    long long before = carry;
    for (int w = 0; w < wave; ++w) before += ws[w];
    if (b < nb) counts[b] = before + inc - c;
    __syncthreads();
    if (tid == 255) carry = before + inc;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// The accepted candidates of workgroup b go to rows ranks[b] ... of the output in thread order;
// rows from cap on are not stored.  c0: the candidate number of the chunk's first row.
template <int MX>
static __global__ void __launch_bounds__(HM_ACC_BLOCK) k_hm_scatter(const double* i2, long long ld, int p, int maxno,
                                                                   double cm, long long mc, const double* Xs, int D,
                                                                   long long c0, const long long* ranks,
                                                                   long long cap, double* pts, long long* idx) {
  __shared__ int wc[HM_ACC_BLOCK / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long s = (long long)blockIdx.x * HM_ACC_BLOCK + tid;
  const bool ok = s < mc && hm_accepted<MX>(i2, ld, p, maxno, cm, s);
  const unsigned long long b = __ballot(ok);
  if (lane == 0) wc[wave] = __popcll(b);
  __syncthreads();
  if (!ok) return;
  long long at = ranks[blockIdx.x] + __popcll(b & ((1ULL << lane) - 1ULL));
  for (int w = 0; w < wave; ++w) at += wc[w];
  if (at >= cap) return;
  for (int k = 0; k < D; ++k) pts[at * D + k] = Xs[s * D + k];
  idx[at] = c0 + s;
}

}  // namespace gpe
