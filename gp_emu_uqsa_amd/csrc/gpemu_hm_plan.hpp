// gpemu_hm_plan.hpp -- the layouts and sizes of the resident emulator set (gpe_hm_*, kernels in
// gpemu_hm.hpp): the packed copy of L^-1 with the [gamma, G] rows behind it, the tile shape, the
// tile list and the chunk and workspace sizes.  Host-checkable: no HIP header, so
// tests/host/hm_plan_check.cpp compiles it with any C++17 compiler; the kernels call the same
// functions on the device.
#pragma once

#if defined(__HIPCC__)
#define GPE_HM_HD __host__ __device__
#else
#define GPE_HM_HD
#endif

namespace gpe {

// limits of one emulator of a set, and of the set
constexpr int HM_MAX_N = 512, HM_MAX_D = 32, HM_MAX_Q = 16, HM_MAX_EMUL = 32;
// v_mfma_f64_16x16x4_f64: blocks of 16 rows, steps of 4 columns, 64 operand values per step
constexpr int HM_RB = 16, HM_KS = 4, HM_STEP = HM_RB * HM_KS;
constexpr int HM_LANES = 256, HM_WAVES = HM_LANES / 64;
// the point tile is a multiple of 16; chunks are multiples of the widest one
constexpr int HM_PT_WIDE = 64, HM_PT_NARROW = 32, HM_CHUNK_UNIT = 64;
constexpr long long HM_CHUNK_DEFAULT = 65536;
constexpr int HM_LDS_BYTES = 160 * 1024;

// rows padded to whole blocks, and the blocks
GPE_HM_HD inline int hm_n16(int n) { return ((n + HM_RB - 1) / HM_RB) * HM_RB; }
GPE_HM_HD inline int hm_nrb(int n) { return (n + HM_RB - 1) / HM_RB; }
// the blocks of 16 rows [gamma^T; G^T] takes (1 + q rows: two blocks at q = 16)
GPE_HM_HD inline int hm_nxb(int q) { return (1 + q + HM_RB - 1) / HM_RB; }
GPE_HM_HD inline int hm_nblocks(int n, int q) { return hm_nrb(n) + hm_nxb(q); }
// the same for `rows` rows behind L^-1's: 1 + q of a single emulator ([gamma, G]), p + q of a
// multi-output one ([Gamma, G]); at most HM_MAX_ROWS, the rows of yb
constexpr int HM_MAX_ROWS = 32;
GPE_HM_HD inline int hm_nxb_rows(int rows) { return (rows + HM_RB - 1) / HM_RB; }
GPE_HM_HD inline int hm_nblocks_rows(int n, int rows) { return hm_nrb(n) + hm_nxb_rows(rows); }

// The packed matrix, block by block.  Block b < nrb holds rows [16 b, 16 b + 16) of L^-1 over
// the columns [0, 16 (b + 1)): the lower blocks only, 4 (b + 1) steps.  Block nrb + x holds
// rows [16 x, 16 x + 16) of [gamma^T; G^T] (row 0 gamma, row 1 + j column j of G = A^-1 H) over
// all 16 nrb columns.  A step is the 64 values of one MFMA A operand in lane order: lane l holds
// (row l & 15, column 4 step + (l >> 4)), so a wave's load of a step is 512 contiguous bytes.
GPE_HM_HD inline int hm_block_steps(int nrb, int b) { return HM_KS * (b < nrb ? b + 1 : nrb); }
// first step of block b (steps of all earlier blocks)
GPE_HM_HD inline long long hm_block_first(int nrb, int b) {
  return b <= nrb ? 2LL * b * (b + 1) : 2LL * nrb * (nrb + 1) + (long long)(b - nrb) * HM_KS * nrb;
}
// index of (row r of the block, column k) of block b in the packed array
GPE_HM_HD inline long long hm_packed_index(int nrb, int b, int r, int k) {
  return (hm_block_first(nrb, b) + k / HM_KS) * HM_STEP + (k % HM_KS) * HM_RB + r;
}
// doubles of the packed array (the largest index + 1)
GPE_HM_HD inline long long hm_packed_size(int n, int q) {
  const int nrb = hm_nrb(n);
  return hm_block_first(nrb, nrb + hm_nxb(q)) * HM_STEP;
}
GPE_HM_HD inline long long hm_packed_size_rows(int n, int rows) {
  const int nrb = hm_nrb(n);
  return hm_block_first(nrb, nrb + hm_nxb_rows(rows)) * HM_STEP;
}

// Points per workgroup.  The tile's K* (16 nrb rows x PT) stays in LDS with 48 PT doubles of
// results behind it (32 rows of [gamma, G]^T K*, 16 partial sums of squares per point; the
// scaled points of the tile use that space first): 64 points up to n = 256 (152 KB of the
// 160 KB of a compute unit), 32 beyond (140 KB at n = 512).
GPE_HM_HD inline int hm_lds_doubles(int n, int pt) { return (hm_n16(n) + 48) * pt; }
GPE_HM_HD inline int hm_pt(int n) { return hm_n16(n) <= 256 ? HM_PT_WIDE : HM_PT_NARROW; }
static_assert((256 + 48) * HM_PT_WIDE * 8 <= HM_LDS_BYTES && (HM_MAX_N + 48) * HM_PT_NARROW * 8 <= HM_LDS_BYTES,
              "both tile shapes fit the LDS of a compute unit");

// The tiles of m points, pt each: tile t covers [pt t, min(m, pt (t + 1))).
struct HmTile {
  long long s0;
  int count;
};
inline long long hm_tiles(long long m, int pt) { return (m + pt - 1) / pt; }
inline HmTile hm_tile(long long m, int pt, long long t) {
  const long long s0 = t * pt;
  const long long left = m - s0;
  return HmTile{s0, (int)(left < pt ? left : pt)};
}

// The chunk length from GPEMU_HM_CHUNK's value (0: unset): a positive multiple of HM_CHUNK_UNIT
inline long long hm_chunk(long long env) {
  if (env <= 0) return HM_CHUNK_DEFAULT;
  const long long c = (env / HM_CHUNK_UNIT) * HM_CHUNK_UNIT;
  return c < HM_CHUNK_UNIT ? HM_CHUNK_UNIT : c;
}

// One chunk's buffers, in doubles, for cl points of D inputs, p emulators and maxno columns:
// the device holds the points, I^2, the parts and the selection; a pinned slot the points, and
// a pinned result slot the selection and the parts.
struct HmWork {
  long long pts, i2, parts, sel;
  long long dev() const { return pts + i2 + parts + sel; }
  long long pin_in() const { return pts; }
  long long pin_out() const { return sel + parts; }
};
inline HmWork hm_work(long long cl, int D, int p, int maxno, bool parts) {
  return HmWork{cl * D, cl * p, parts ? 2 * cl * p : 0, cl * maxno};
}
// The joint measure of one member of p outputs (gpe_hm_implausibility_mv): I^2 per point takes
// the selection's place (one column, copied out as it is); the parts are p means and c per point.
inline HmWork hm_work_mv(long long cl, int D, int p, bool parts) {
  return HmWork{cl * D, 0, parts ? (p + 1) * cl : 0, cl};
}

}  // namespace gpe
