// Stand-alone driver of csrc/gpemu_hm_plan.hpp for tests/test_implausibility_host.py: any C++17
// compiler, no HIP, no GPU.  Checks, for the shapes of the test's list and a sweep of every
// n <= 512:
//   - the packed index map of L^-1's lower 16 x 16 blocks and the [gamma, G] blocks is a
//     bijection onto [0, hm_packed_size): every (block, row, column) lands on an index of its
//     own, inside the array, and every index is hit; the size is the largest index + 1;
//   - a step of 4 columns of a block is 64 consecutive indices in MFMA lane order;
//   - the tile shape fits the LDS of a compute unit and the chunk unit is whole tiles;
//   - the tiles of a call, chunk by chunk, cover [0, m) exactly once, none empty;
//   - the chunk length's rounding and the workspace sizes.
// Prints "hm_plan_check OK" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpemu_hm_plan.hpp"

using namespace gpe;

static int fails = 0;
#define EXPECT(cond, ...)                  \
  do {                                     \
    if (!(cond)) {                         \
      std::fprintf(stderr, "FAIL %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);   \
      std::fprintf(stderr, "\n");          \
      if (++fails > 20) std::exit(1);      \
    }                                      \
  } while (0)

static void check_packed(int n, int q) {
  const int nrb = hm_nrb(n), nxb = hm_nxb(q), n16 = hm_n16(n);
  const long long size = hm_packed_size(n, q);
  EXPECT(n16 == 16 * nrb && n16 >= n && n16 - n < 16, "n %d n16 %d", n, n16);
  EXPECT(16 * nxb >= q + 1 && 16 * (nxb - 1) < q + 1, "q %d nxb %d", q, nxb);
  EXPECT(hm_nblocks(n, q) == nrb + nxb, "n %d q %d", n, q);
  std::vector<unsigned char> hit((size_t)size, 0);
  long long largest = -1, entries = 0;
  for (int b = 0; b < nrb + nxb; ++b) {
    const int cols = HM_KS * hm_block_steps(nrb, b);
    EXPECT(cols == (b < nrb ? 16 * (b + 1) : n16), "n %d block %d columns %d", n, b, cols);
    for (int r = 0; r < HM_RB; ++r)
      for (int k = 0; k < cols; ++k) {
        const long long i = hm_packed_index(nrb, b, r, k);
        EXPECT(i >= 0 && i < size, "n %d q %d block %d row %d column %d: index %lld of %lld", n, q, b, r, k, i, size);
        if (i < 0 || i >= size) return;
        EXPECT(!hit[(size_t)i], "n %d q %d block %d row %d column %d: index %lld taken", n, q, b, r, k, i);
        hit[(size_t)i] = 1;
        if (i > largest) largest = i;
        ++entries;
        // lane order inside the step: lane = 16 (k % 4) + r
        const long long step0 = (hm_block_first(nrb, b) + k / HM_KS) * HM_STEP;
        EXPECT(i - step0 == (k % HM_KS) * HM_RB + r, "n %d block %d row %d column %d: lane %lld", n, b, r, k, i - step0);
      }
  }
  EXPECT(entries == size, "n %d q %d: %lld entries, size %lld", n, q, entries, size);
  EXPECT(largest + 1 == size, "n %d q %d: largest index %lld, size %lld", n, q, largest, size);
  // every row and column of the lower triangle of L^-1 and of [gamma, G]^T has a block
  EXPECT(hm_block_steps(nrb, nrb - 1) * HM_KS >= n, "n %d: the last row block's columns", n);
}

static void check_tiles(long long m, int pt, long long chunk) {
  std::vector<int> cover((size_t)m, 0);
  for (long long s0 = 0; s0 < m; s0 += chunk) {
    const long long mc = m - s0 < chunk ? m - s0 : chunk;
    const long long nt = hm_tiles(mc, pt);
    EXPECT(nt >= 1 && (nt - 1) * pt < mc && nt * pt >= mc, "m %lld pt %d chunk %lld: %lld tiles of %lld points", m, pt, chunk, nt, mc);
    for (long long t = 0; t < nt; ++t) {
      const HmTile tl = hm_tile(mc, pt, t);
      EXPECT(tl.s0 == t * pt && tl.count >= 1 && tl.count <= pt && tl.s0 + tl.count <= mc, "m %lld pt %d tile %lld: [%lld, +%d)", m, pt, t, tl.s0, tl.count);
      for (int j = 0; j < tl.count && s0 + tl.s0 + j < m; ++j) ++cover[(size_t)(s0 + tl.s0 + j)];
    }
  }
  for (long long s = 0; s < m; ++s) EXPECT(cover[(size_t)s] == 1, "m %lld pt %d chunk %lld: point %lld covered %d times", m, pt, chunk, s, cover[(size_t)s]);
}

int main() {
  const int ns[] = {1, 15, 16, 17, 60, 128, 129, 300, 500, 512}, qs[] = {1, 4, 16};
  for (int n : ns)
    for (int q : qs) check_packed(n, q);
  for (int n = 1; n <= HM_MAX_N; ++n) {
    const int pt = hm_pt(n);
    EXPECT(pt == HM_PT_WIDE || pt == HM_PT_NARROW, "n %d pt %d", n, pt);
    EXPECT(pt % 16 == 0 && HM_CHUNK_UNIT % pt == 0, "n %d pt %d: whole MFMA groups, whole tiles per chunk", n, pt);
    EXPECT((long long)hm_lds_doubles(n, pt) * 8 <= HM_LDS_BYTES, "n %d pt %d: %d doubles of LDS", n, pt, hm_lds_doubles(n, pt));
    // the tile's scaled points (pt x 33 at most) fit the 48 pt doubles behind K*
    EXPECT(pt * (HM_MAX_D | 1) <= 48 * pt, "n %d pt %d", n, pt);
    EXPECT(hm_packed_size(n, HM_MAX_Q) >= (long long)n * (n + 1) / 2 + (long long)(HM_MAX_Q + 1) * n, "n %d", n);
    if (n % 37 == 0) check_packed(n, 7);
  }
  EXPECT(hm_pt(256) == HM_PT_WIDE && hm_pt(257) == HM_PT_NARROW, "the tile shapes' boundary");
  EXPECT(hm_packed_size(512, 16) * 8 <= 2 * 1024 * 1024, "n = 512 stays well inside an XCD's 4 MB of L2");
  for (int pt : {HM_PT_NARROW, HM_PT_WIDE})
    for (long long chunk : {(long long)HM_CHUNK_UNIT, 3LL * HM_CHUNK_UNIT, 1024LL})
      for (long long m : {1LL, (long long)pt - 1, (long long)pt, (long long)pt + 1, chunk, chunk + 1, 3LL * pt + 5})
        check_tiles(m, pt, chunk);
  EXPECT(hm_chunk(0) == HM_CHUNK_DEFAULT && hm_chunk(-5) == HM_CHUNK_DEFAULT, "the default chunk");
  EXPECT(hm_chunk(1) == 64 && hm_chunk(64) == 64 && hm_chunk(127) == 64 && hm_chunk(128) == 128 && hm_chunk(1000) == 960,
         "the chunk's rounding");
  EXPECT(HM_CHUNK_DEFAULT % HM_CHUNK_UNIT == 0, "the default chunk is whole tiles");
  for (bool parts : {false, true}) {
    const HmWork w = hm_work(960, 7, 5, 3, parts);
    EXPECT(w.pts == 960 * 7 && w.i2 == 960 * 5 && w.sel == 960 * 3 && w.parts == (parts ? 2 * 960 * 5 : 0), "hm_work");
    EXPECT(w.dev() == w.pts + w.i2 + w.parts + w.sel && w.pin_in() == w.pts && w.pin_out() == w.sel + w.parts, "hm_work sums");
  }
  if (fails) return 1;
  std::printf("hm_plan_check OK\n");
  return 0;
}
