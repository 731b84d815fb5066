// Stand-alone driver of the rows-based functions of csrc/gpemu_hm_plan.hpp (the blocks behind
// L^-1's of a member with `rows` = 1 + q or p + q result rows) for
// tests/test_implausibility_multi_host.py: any C++17 compiler, no HIP, no GPU.
//   - rows in {1, 16, 17, 32} (and every rows <= 32) at a list of n: the block count, the packed
//     size, and the index map over the extra blocks a bijection onto [end of L^-1's blocks,
//     hm_packed_size_rows);
//   - the q-based functions return what they returned: hm_nxb(q) = hm_nxb_rows(1 + q),
//     hm_nblocks and hm_packed_size likewise, for every q <= 16;
//   - hm_work_mv's sizes, and hm_work's unchanged.
// Prints "hm_plan_rows_check OK" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpemu_hm_plan.hpp"

using namespace gpe;

static int fails = 0;
#define EXPECT(cond, ...)                       \
  do {                                          \
    if (!(cond)) {                              \
      std::fprintf(stderr, "FAIL %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);        \
      std::fprintf(stderr, "\n");               \
      if (++fails > 20) std::exit(1);           \
    }                                           \
  } while (0)

static void check_rows(int n, int rows) {
  const int nrb = hm_nrb(n), nxb = hm_nxb_rows(rows), n16 = hm_n16(n);
  EXPECT(16 * nxb >= rows && 16 * (nxb - 1) < rows, "rows %d: %d blocks", rows, nxb);
  EXPECT(hm_nblocks_rows(n, rows) == nrb + nxb, "n %d rows %d", n, rows);
  const long long first = hm_block_first(nrb, nrb) * HM_STEP, size = hm_packed_size_rows(n, rows);
  EXPECT(first == 32LL * nrb * (nrb + 1) * 4, "n %d: L^-1's blocks end at %lld", n, first);
  EXPECT(size == first + (long long)nxb * 16 * n16, "n %d rows %d: size %lld", n, rows, size);
  std::vector<unsigned char> hit((size_t)(size - first), 0);
  long long entries = 0;
  for (int x = 0; x < nxb; ++x) {
    EXPECT(hm_block_steps(nrb, nrb + x) * HM_KS == n16, "n %d block %d", n, nrb + x);
    for (int r = 0; r < HM_RB; ++r)
      for (int k = 0; k < n16; ++k) {
        const long long i = hm_packed_index(nrb, nrb + x, r, k);
        EXPECT(i >= first && i < size, "n %d rows %d block %d row %d column %d: index %lld outside [%lld, %lld)", n, rows,
               x, r, k, i, first, size);
        if (i < first || i >= size) return;
        EXPECT(!hit[(size_t)(i - first)], "n %d rows %d block %d row %d column %d: index %lld taken", n, rows, x, r, k, i);
        hit[(size_t)(i - first)] = 1;
        ++entries;
      }
  }
  EXPECT(entries == size - first, "n %d rows %d: %lld entries for %lld places", n, rows, entries, size - first);
}

int main() {
  const int ns[] = {1, 16, 17, 60, 61, 129, 300, 512};
  for (int n : ns) {
    for (int rows : {1, 16, 17, 32}) check_rows(n, rows);
    for (int rows = 1; rows <= HM_MAX_ROWS; ++rows) {
      EXPECT(hm_nxb_rows(rows) == (rows <= 16 ? 1 : 2), "rows %d", rows);
      EXPECT(hm_packed_size_rows(n, rows) * 8 <= 2 * 1024 * 1024 + 2 * 16 * 512 * 8, "n %d rows %d", n, rows);
    }
    for (int q = 0; q <= HM_MAX_Q; ++q) {
      EXPECT(hm_nxb(q) == hm_nxb_rows(1 + q) && hm_nxb(q) == (q < 16 ? 1 : 2), "q %d", q);
      EXPECT(hm_nblocks(n, q) == hm_nblocks_rows(n, 1 + q), "n %d q %d", n, q);
      EXPECT(hm_packed_size(n, q) == hm_packed_size_rows(n, 1 + q), "n %d q %d", n, q);
    }
  }
  EXPECT(HM_MAX_ROWS == 32 && HM_MAX_ROWS * HM_PT_WIDE <= 48 * HM_PT_WIDE - 16 * HM_PT_WIDE, "yb's rows lie before ssb's");
  EXPECT(hm_nxb(4) == 1 && hm_nxb(15) == 1 && hm_nxb(16) == 2 && hm_nblocks(300, 11) == 20 && hm_nblocks(512, 16) == 34,
         "the q-based block counts");
  EXPECT(hm_packed_size(60, 4) == (2LL * 4 * 5 + 16) * 64 && hm_packed_size(512, 16) == (2LL * 32 * 33 + 2 * 128) * 64,
         "the q-based sizes");
  for (bool parts : {false, true}) {
    const HmWork w = hm_work_mv(960, 7, 5, parts);
    EXPECT(w.pts == 960 * 7 && w.i2 == 0 && w.sel == 960 && w.parts == (parts ? 960 * 6 : 0), "hm_work_mv");
    EXPECT(w.dev() == w.pts + w.parts + w.sel && w.pin_in() == w.pts && w.pin_out() == w.sel + w.parts, "hm_work_mv sums");
    const HmWork u = hm_work(960, 7, 5, 3, parts);
    EXPECT(u.pts == 960 * 7 && u.i2 == 960 * 5 && u.sel == 960 * 3 && u.parts == (parts ? 2 * 960 * 5 : 0), "hm_work");
  }
  if (fails) return 1;
  std::printf("hm_plan_rows_check OK\n");
  return 0;
}
