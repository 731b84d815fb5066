// Stand-alone driver of the PCG64 part of csrc/gpemu_hm_cand_plan.hpp for
// tests/test_hm_candidates_host.py: any C++17 compiler, no HIP, no GPU.  argv[1] names a text
// file the test wrote from numpy.random.default_rng(seed), every number a hexadecimal 64-bit
// word (doubles as their bits):
//   state_hi state_lo inc_hi inc_lo       the generator's initial state
//   k1 state1_hi state1_lo                the state after a first call of random(k1)
//   D R                                   then lo[D], hi[D]
//   N = R D doubles                       random(k1) followed by random(N - k1): one stream
//   N doubles                             lo + random((R, D)) * (hi - lo) of a fresh generator
// Checks stepping (every element), the O(log k) skip-ahead for elements {0, 1, 63, 64, 5000,
// last} and to the continued stream's state, the row table for every row and for rows beyond
// two digits, and the affine map, all bit for bit.
// Prints "hm_draw_check OK" and returns 0, or says what failed and returns 1.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static uint64_t word(FILE* f) {
  uint64_t v = 0;
  if (std::fscanf(f, "%" SCNx64, &v) != 1) {
    std::fprintf(stderr, "the input ends early\n");
    std::exit(1);
  }
  return v;
}
static uint64_t bits(double x) {
  uint64_t v;
  std::memcpy(&v, &x, sizeof v);
  return v;
}
static double from_bits(uint64_t v) {
  double x;
  std::memcpy(&x, &v, sizeof x);
  return x;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const uint64_t sh = word(f), sl = word(f), ih = word(f), il = word(f);
  const hm_u128 state = hm_u128_of(sh, sl), inc = hm_u128_of(ih, il);
  const uint64_t k1 = word(f);
  const uint64_t s1h = word(f), s1l = word(f);
  const hm_u128 state1 = hm_u128_of(s1h, s1l);
  const int D = (int)word(f);
  const long long R = (long long)word(f), N = R * D;
  std::vector<double> lo((size_t)D), hi((size_t)D);
  for (double& v : lo) v = from_bits(word(f));
  for (double& v : hi) v = from_bits(word(f));
  std::vector<uint64_t> u((size_t)N), x((size_t)N);
  for (uint64_t& v : u) v = word(f);
  for (uint64_t& v : x) v = word(f);
  std::fclose(f);
  EXPECT(N > 5000 && k1 > 0 && (long long)k1 < N, "the test's sizes: N %lld k1 %" PRIu64, N, k1);

  // stepping, and the affine map of every element
  hm_u128 s = state;
  for (long long e = 0; e < N; ++e) {
    s = hm_pcg_step(s, inc);
    const double d = hm_pcg_double(hm_pcg_output(s));
    EXPECT(bits(d) == u[(size_t)e], "element %lld: %016" PRIx64 " for %016" PRIx64, e, bits(d), u[(size_t)e]);
    const int k = (int)(e % D);
    EXPECT(bits(hm_affine(lo[(size_t)k], hi[(size_t)k], d)) == x[(size_t)e], "the affine map of element %lld", e);
    if ((uint64_t)(e + 1) == k1) EXPECT(s == state1, "the state after the first call's %" PRIu64 " elements", k1);
  }
  // skip-ahead to an element, and to the continued stream
  for (long long e : {0LL, 1LL, 63LL, 64LL, 5000LL, N - 1}) {
    const hm_u128 t = hm_pcg_step(hm_pcg_apply(hm_jump((uint64_t)e, inc), state), inc);
    EXPECT(bits(hm_pcg_double(hm_pcg_output(t))) == u[(size_t)e], "skip-ahead to element %lld", e);
  }
  EXPECT(hm_pcg_apply(hm_jump(k1, inc), state) == state1, "skip-ahead to the continued stream");
  {
    hm_u128 t = state1;
    for (uint64_t e = k1; e < k1 + 5; ++e) {
      t = hm_pcg_step(t, inc);
      EXPECT(bits(hm_pcg_double(hm_pcg_output(t))) == u[(size_t)e], "the continued stream's element %" PRIu64, e);
    }
  }
  // a composed jump is the jump of the sum
  {
    const HmJump a = hm_jump(12345, inc), b = hm_jump(678, inc), c = hm_jump(12345 + 678, inc), ab = hm_jump_then(a, b);
    EXPECT(ab.mul == c.mul && ab.add == c.add, "hm_jump_then");
  }
  // the row table: every row of the test, from the start and from a later chunk's start
  for (long long first : {0LL, 1000LL}) {
    const int digits = hm_digits(R);
    std::vector<uint64_t> table((size_t)digits * HM_DIGIT * 4);
    hm_jump_table(D, inc, digits, table.data());
    const hm_u128 start = hm_pcg_apply(hm_jump((uint64_t)first * D, inc), state);
    for (long long r = 0; r < R; ++r) {
      const hm_u128 got = hm_row_state(table.data(), digits, start, r);
      const hm_u128 want = hm_pcg_apply(hm_jump((uint64_t)(first + r) * D, inc), state);
      EXPECT(got == want, "row %lld behind candidate %lld", r, first);
      if (first == 0) {
        const hm_u128 t = hm_pcg_step(got, inc);
        EXPECT(bits(hm_pcg_double(hm_pcg_output(t))) == u[(size_t)(r * D)], "row %lld's first element", r);
      }
    }
  }
  {
    const int digits = hm_digits(70001);
    EXPECT(digits == 3, "three digits for 70001 rows");
    std::vector<uint64_t> table((size_t)digits * HM_DIGIT * 4);
    hm_jump_table(D, inc, digits, table.data());
    for (long long r : {255LL, 256LL, 65535LL, 65536LL, 70000LL})
      EXPECT(hm_row_state(table.data(), digits, state, r) == hm_pcg_apply(hm_jump((uint64_t)r * D, inc), state), "row %lld of three digits", r);
  }
  if (fails) return 1;
  std::printf("hm_draw_check OK\n");
  return 0;
}
