// gpemu_hm_cand_plan.hpp -- what the candidate generators and reducers of the resident emulator
// set (gpe_hm_cells, gpe_hm_cells_mv, gpe_hm_sample; kernels in gpemu_hm_cand.hpp) share with the
// host: the pieces a chunk cuts the cells of a mesh into, the workspace sizes of the three
// entries, and NumPy's PCG64 (step, output, double, skip-ahead) as plain C++.  Host-checkable
// as gpemu_hm_plan.hpp: no HIP header, so tests/host/hm_cells_check.cpp and hm_draw_check.cpp
// compile it with any C++17 compiler; the kernels call the same functions on the device.
#pragma once

#include <cstdint>

#include "gpemu_hm_plan.hpp"

namespace gpe {

// ---------------------------------------------------------------- the mesh of two inputs
// Candidate s = cell * ns + t is sample t of cell = i * g2 + j.  A chunk [s0, s0 + mc) of the
// linear candidate index cuts the cells into pieces: piece k of the chunk is the part of cell
// hm_first_cell + k that lies inside the chunk, samples [t0, t1] of the cell.  The piece that
// has t0 == 0 is the first of its cell (over all chunks): it overwrites the cell's accumulators,
// every other piece combines into them.
struct HmPiece {
  long long cell;
  long long t0, t1;   // first and last sample of the cell in this piece (inclusive)
};
GPE_HM_HD inline long long hm_pieces(long long s0, long long mc, long long ns) {
  return (s0 + mc - 1) / ns - s0 / ns + 1;
}
GPE_HM_HD inline HmPiece hm_piece(long long s0, long long mc, long long ns, long long k) {
  const long long cell = s0 / ns + k, c0 = cell * ns, c1 = c0 + ns, e = s0 + mc;
  return HmPiece{cell, (s0 > c0 ? s0 : c0) - c0, (e < c1 ? e : c1) - 1 - c0};
}
// the most candidates a mesh may have (g1 g2 ns below it)
constexpr long long HM_CELLS_MAX = 1LL << 40;

// Candidates per workgroup of the sampler's count and scatter kernels (one thread each)
constexpr int HM_ACC_BLOCK = 256;
GPE_HM_HD inline long long hm_acc_blocks(long long mc) { return (mc + HM_ACC_BLOCK - 1) / HM_ACC_BLOCK; }

// ---------------------------------------------------------------- workspace, in 8-byte words
// gpe_hm_cells (p outputs, maxno levels) and gpe_hm_cells_mv (p = 0 here: one I^2 row, one level,
// `extra` words of [W, lambda] behind): the chunk's candidates and I^2, the mesh (x1, x2 and the
// ns x (D - 2) other columns), per level and cell a minimum (double) and a count (int64).
struct HmCellsWork {
  long long pts, i2, mesh, acc, extra;
  long long dev() const { return pts + i2 + mesh + 2 * acc + extra; }
  long long out_bytes() const { return 16 * acc; }
};
inline HmCellsWork hm_work_cells(long long cl, int D, int p, int maxno, long long g1, long long g2, long long ns,
                                 long long extra) {
  return HmCellsWork{cl * D, cl * (p ? p : 1), g1 + g2 + ns * (D - 2), (long long)maxno * g1 * g2, extra};
}
// gpe_hm_sample: the chunk's candidates and I^2, a rank per workgroup of HM_ACC_BLOCK candidates
// and the running total, the skip-ahead table, lo and hi, and `rows` = min(cap, m) accepted
// rows with their candidate numbers.
struct HmSampleWork {
  long long pts, i2, ranks, table, box, out_pts, out_idx;
  long long dev() const { return pts + i2 + ranks + table + box + out_pts + out_idx; }
};

// ---------------------------------------------------------------- PCG64 (numpy.random.PCG64)
// state <- state * HM_PCG_MULT + inc (mod 2^128); the output of a step is the new state's
// rotr64(hi ^ lo, hi >> 58); a double is (output >> 11) * 2^-53.
typedef unsigned __int128 hm_u128;
GPE_HM_HD inline hm_u128 hm_u128_of(uint64_t hi, uint64_t lo) { return ((hm_u128)hi << 64) | lo; }
GPE_HM_HD inline hm_u128 hm_pcg_mult() { return hm_u128_of(0x2360ED051FC65DA4ULL, 0x4385DF649FCCF645ULL); }
GPE_HM_HD inline hm_u128 hm_pcg_step(hm_u128 s, hm_u128 inc) { return s * hm_pcg_mult() + inc; }
GPE_HM_HD inline uint64_t hm_pcg_output(hm_u128 s) {
  const uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s, x = hi ^ lo;
  const unsigned r = (unsigned)(hi >> 58);
  return (x >> r) | (x << ((64 - r) & 63));
}
GPE_HM_HD inline double hm_pcg_double(uint64_t out) { return (double)(out >> 11) * (1.0 / 9007199254740992.0); }

// k steps at once: s -> mul * s + add.  With `add` already multiplied by the increment the
// jump costs one 128-bit product.
struct HmJump {
  hm_u128 mul, add;
};
GPE_HM_HD inline hm_u128 hm_pcg_apply(const HmJump& j, hm_u128 s) { return j.mul * s + j.add; }
// first a, then b
GPE_HM_HD inline HmJump hm_jump_then(const HmJump& a, const HmJump& b) { return HmJump{b.mul * a.mul, b.mul * a.add + b.add}; }
// the jump of k steps for increment inc, by squaring: O(log k)
inline HmJump hm_jump(uint64_t k, hm_u128 inc) {
  HmJump r{1, 0}, sq{hm_pcg_mult(), inc};
  for (; k; k >>= 1) {
    if (k & 1) r = hm_jump_then(r, sq);
    sq = hm_jump_then(sq, sq);
  }
  return r;
}

// The sampler's row table.  Row r of a chunk starts r * D steps behind the chunk's first row.
// r is read in digits of HM_DIGIT_BITS bits: entry [g][v] is the jump of v * D * 2^(8 g) steps,
// so a thread reaches its row with one product per digit (two at the default chunk of 65536
// rows), small beside the D steps that follow.
constexpr int HM_DIGIT_BITS = 8, HM_DIGIT = 1 << HM_DIGIT_BITS;
GPE_HM_HD inline int hm_digits(long long rows) {
  int g = 1;
  while (g < 8 && ((rows - 1) >> (HM_DIGIT_BITS * g)) > 0) ++g;
  return g;
}
// table: digits x HM_DIGIT entries of 4 words (mul hi, mul lo, add hi, add lo)
inline void hm_jump_table(int D, hm_u128 inc, int digits, uint64_t* table) {
  HmJump unit = hm_jump((uint64_t)D, inc);
  for (int g = 0; g < digits; ++g) {
    HmJump cur{1, 0};
    for (int v = 0; v < HM_DIGIT; ++v) {
      uint64_t* t = table + ((long long)g * HM_DIGIT + v) * 4;
      t[0] = (uint64_t)(cur.mul >> 64), t[1] = (uint64_t)cur.mul;
      t[2] = (uint64_t)(cur.add >> 64), t[3] = (uint64_t)cur.add;
      cur = hm_jump_then(cur, unit);
    }
    unit = cur;   // HM_DIGIT units: the next digit's unit
  }
}
// the state a row starts from: the chunk's first state advanced by r rows
GPE_HM_HD inline hm_u128 hm_row_state(const uint64_t* table, int digits, hm_u128 s, long long r) {
  for (int g = 0; g < digits; ++g) {
    const uint64_t* t = table + ((long long)g * HM_DIGIT + ((r >> (HM_DIGIT_BITS * g)) & (HM_DIGIT - 1))) * 4;
    s = hm_pcg_apply(HmJump{hm_u128_of(t[0], t[1]), hm_u128_of(t[2], t[3])}, s);
  }
  return s;
}
// x = lo + u (hi - lo), each operation rounded: NumPy's lo + random() * (hi - lo).  The pragma
// is clang's (the device build and a clang host build); a compiler that does not know it must be
// given -ffp-contract=off, as the host check's build is.
GPE_HM_HD inline double hm_affine(double lo, double hi, double u) {
#pragma clang fp contract(off)
  const double w = hi - lo;
  const double t = u * w;
  return lo + t;
}

inline HmSampleWork hm_work_sample(long long cl, int D, int p, long long rows) {
  return HmSampleWork{cl * D, cl * p, hm_acc_blocks(cl) + 1, (long long)hm_digits(cl) * HM_DIGIT * 4, 2LL * D,
                      rows * D, rows};
}

}  // namespace gpe
