// Stand-alone driver of csrc/gpemu_hm_cand_plan.hpp for tests/test_hm_candidates_host.py: any
// C++17 compiler, no HIP, no GPU.  For cells in {1, 6, 25}, ns in {1, 63, 64, 70, 150} and chunk
// in {64, 128, 65536}:
//   - the pieces of all chunks cover every cell's samples [0, ns) exactly once and in order;
//   - "starts at sample 0" (the piece overwrites the accumulators) holds for exactly one piece
//     per cell, the first one met;
//   - every piece lies inside its chunk, none is empty, and a chunk's pieces are consecutive cells;
//   - the workspace sums of the three entries hold.
// Prints "hm_cells_check OK" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpemu_hm_cand_plan.hpp"

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

static void check_pieces(long long cells, long long ns, long long chunk) {
  const long long M = cells * ns;
  std::vector<long long> next((size_t)cells, 0);   // the next sample each cell expects
  std::vector<int> starts((size_t)cells, 0);
  long long total = 0;
  for (long long s0 = 0; s0 < M; s0 += chunk) {
    const long long mc = M - s0 < chunk ? M - s0 : chunk;
    const long long np = hm_pieces(s0, mc, ns);
    EXPECT(np >= 1 && np <= mc, "cells %lld ns %lld chunk %lld s0 %lld: %lld pieces", cells, ns, chunk, s0, np);
    long long in_chunk = 0;
    for (long long k = 0; k < np; ++k) {
      const HmPiece pc = hm_piece(s0, mc, ns, k);
      EXPECT(pc.cell == s0 / ns + k && pc.cell >= 0 && pc.cell < cells, "cells %lld ns %lld chunk %lld s0 %lld piece %lld: cell %lld", cells, ns, chunk, s0, k, pc.cell);
      if (pc.cell < 0 || pc.cell >= cells) return;
      EXPECT(pc.t0 >= 0 && pc.t0 <= pc.t1 && pc.t1 < ns, "ns %lld chunk %lld s0 %lld piece %lld: samples [%lld, %lld]", ns, chunk, s0, k, pc.t0, pc.t1);
      // inside the chunk: the rows the reducer reads of I^2
      const long long a = pc.cell * ns + pc.t0 - s0, b = pc.cell * ns + pc.t1 - s0;
      EXPECT(a >= 0 && b < mc, "ns %lld chunk %lld s0 %lld piece %lld: rows [%lld, %lld] of %lld", ns, chunk, s0, k, a, b, mc);
      EXPECT(pc.t0 == next[(size_t)pc.cell], "cell %lld: piece starts at %lld, expected %lld", pc.cell, pc.t0, next[(size_t)pc.cell]);
      next[(size_t)pc.cell] = pc.t1 + 1;
      if (pc.t0 == 0) ++starts[(size_t)pc.cell];
      in_chunk += pc.t1 - pc.t0 + 1;
    }
    EXPECT(in_chunk == mc, "ns %lld chunk %lld s0 %lld: the pieces hold %lld of %lld rows", ns, chunk, s0, in_chunk, mc);
    total += in_chunk;
  }
  EXPECT(total == M, "cells %lld ns %lld chunk %lld: %lld of %lld candidates", cells, ns, chunk, total, M);
  for (long long c = 0; c < cells; ++c) {
    EXPECT(next[(size_t)c] == ns, "cell %lld covered up to %lld of %lld", c, next[(size_t)c], ns);
    EXPECT(starts[(size_t)c] == 1, "cell %lld: %d pieces start at sample 0", c, starts[(size_t)c]);
  }
}

int main() {
  for (long long cells : {1LL, 6LL, 25LL})
    for (long long ns : {1LL, 63LL, 64LL, 70LL, 150LL})
      for (long long chunk : {64LL, 128LL, 65536LL}) check_pieces(cells, ns, chunk);
  {
    const HmCellsWork w = hm_work_cells(960, 7, 5, 3, 4, 6, 70, 0);
    EXPECT(w.pts == 960 * 7 && w.i2 == 960 * 5 && w.mesh == 4 + 6 + 70 * 5 && w.acc == 3 * 24 && w.extra == 0, "hm_work_cells");
    EXPECT(w.dev() == w.pts + w.i2 + w.mesh + 2 * w.acc && w.out_bytes() == 16 * 3 * 24, "hm_work_cells sums");
    const HmCellsWork v = hm_work_cells(64, 2, 0, 1, 3, 2, 10, 20);   // the joint measure, D = 2
    EXPECT(v.pts == 128 && v.i2 == 64 && v.mesh == 5 && v.acc == 6 && v.extra == 20 && v.dev() == 128 + 64 + 5 + 12 + 20, "hm_work_cells (joint)");
  }
  {
    const HmSampleWork w = hm_work_sample(65536, 13, 4, 1000);
    EXPECT(w.pts == 65536LL * 13 && w.i2 == 65536LL * 4 && w.ranks == 257 && w.table == 2 * 256 * 4 && w.box == 26 && w.out_pts == 13000 && w.out_idx == 1000, "hm_work_sample");
    EXPECT(w.dev() == w.pts + w.i2 + w.ranks + w.table + w.box + w.out_pts + w.out_idx, "hm_work_sample sums");
    EXPECT(hm_acc_blocks(1) == 1 && hm_acc_blocks(256) == 1 && hm_acc_blocks(257) == 2, "hm_acc_blocks");
    EXPECT(hm_digits(1) == 1 && hm_digits(256) == 1 && hm_digits(257) == 2 && hm_digits(65536) == 2 && hm_digits(65537) == 3, "hm_digits");
  }
  if (fails) return 1;
  std::printf("hm_cells_check OK\n");
  return 0;
}
