// oz_residue_check.cpp -- host-only check of the operand conversion's integer residue routine
// (gpemu_ozaki.hpp: oz_digits, oz_digit_sum, oz_reduce, oz_residues in their host form, and
// the weights oz_consts makes for them) against 128-bit integer arithmetic.  No HIP runtime
// call: it runs without a GPU.  Built and run by tests/test_oz_residue_host.py:
//   hipcc --offload-arch=gfx950 -std=c++17 -I gp_emu_uqsa_amd/csrc tests/host/oz_residue_check.cpp
// For nmod 8, 12 and 16 and every integer x tried (|x| <= 2^53, as the kernels' rint(ldexp(., e))):
//   - the seven balanced digits sum to x: sum_i d_i 256^i = x;
//   - for every modulus m: t = sum_i d_i w_i is congruent to x and |t| < 2^17; the byte r that
//     oz_residues returns is congruent to x, and for odd m it is the centred residue,
//     |r| <= (m - 1) / 2 (which makes it unique); as an int8 it is in [-128, 127] for m = 256 too.
// The weights: w_i = 256^i (mod m), |w_i| <= m / 2, (1, 0, ..) for 256, whi's top byte 0.
// Prints one line per failed check and "values=<count>"; exit status 0 and a last line
// "oz_residue_check OK" when every check holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpemu_kernels.hpp"
#include "gpemu_ozaki.hpp"

using namespace gpe;
typedef __int128 i128;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++g_fail <= 50) {                                \
        std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                          \
        std::printf("\n");                                 \
      }                                                    \
    }                                                      \
  } while (0)

static int weight(const OzConst& k, int l, int i) {
  return (int)(int8_t)((unsigned)(i < 4 ? k.wlo[l] : k.whi[l]) >> (8 * (i & 3)));
}

static void check_weights(const OzConst& k) {
  for (int l = 0; l < k.nmod; ++l) {
    const int m = k.m[l];
    i128 p = 1;
    for (int i = 0; i < 7; ++i, p *= 256) {
      const int w = weight(k, l, i);
      CHECK((p - w) % m == 0, "nmod %d m %d: w_%d = %d is not 256^%d", k.nmod, m, i, w, i);
      CHECK(2 * (w < 0 ? -w : w) <= m, "nmod %d m %d: w_%d = %d not centred", k.nmod, m, i, w);
      if (m == 256) CHECK(w == (i == 0 ? 1 : 0), "m 256: w_%d = %d", i, w);
    }
    CHECK(weight(k, l, 7) == 0, "nmod %d m %d: top weight %d", k.nmod, m, weight(k, l, 7));
    CHECK(k.inv[l] == 1.0f / (float)m, "nmod %d m %d: inv", k.nmod, m);
  }
}

static long long g_values = 0;
static void check_value(const OzConst& k, long long X) {
  ++g_values;
  const double x = (double)X;   // (|X| <= 2^53: exact)
  CHECK((long long)x == X, "%lld is not an fp64 integer", X);
  const OzDigits d = oz_digits(x);
  i128 sum = 0, p = 1;
  for (int i = 0; i < 8; ++i, p *= 256) sum += p * (int)(int8_t)((unsigned)(i < 4 ? d.lo : d.hi) >> (8 * (i & 3)));
  CHECK(sum == (i128)X, "x %lld: digits %08x %08x do not sum to it", X, (unsigned)d.hi, (unsigned)d.lo);
  CHECK(((unsigned)d.hi >> 24) == 0u, "x %lld: eighth digit %u", X, (unsigned)d.hi >> 24);
  int8_t r[OZ_MAXMOD];
  oz_residues(x, k, r);
  for (int l = 0; l < k.nmod; ++l) {
    const int m = k.m[l];
    const int t = oz_digit_sum(d, k.wlo[l], k.whi[l]);
    CHECK(((i128)t - (i128)X) % m == 0, "x %lld m %d: t = %d not congruent", X, m, t);
    CHECK(t > -(1 << 17) && t < (1 << 17), "x %lld m %d: t = %d", X, m, t);
    CHECK(((i128)r[l] - (i128)X) % m == 0, "x %lld m %d: r = %d not congruent", X, m, (int)r[l]);
    CHECK(r[l] >= -128 && r[l] <= 127, "x %lld m %d: r = %d", X, m, (int)r[l]);
    if (m & 1) CHECK(2 * (r[l] < 0 ? -r[l] : r[l]) <= m - 1, "x %lld m %d: r = %d is not the centred residue", X, m, (int)r[l]);
  }
}

int main() {
  const long long P53 = 1ll << 53;
  std::vector<long long> fixed = {0, 1, 127, 128, 129, 1ll << 31, (1ll << 32) - 1, 1ll << 52, P53 - 1, P53};
  for (int nmod : {8, 12, 16}) {
    const OzConst k = oz_consts(nmod, 16384);
    CHECK(k.nmod == nmod, "nmod %d", nmod);
    check_weights(k);
    for (long long v : fixed) {
      check_value(k, v);
      check_value(k, -v);
    }
    // 10^6 values over every magnitude: bit length 1 .. 54 in turn (54: 2^53 itself), either sign
    unsigned long long s = 0x9e3779b97f4a7c15ull + (unsigned)nmod;
    for (int i = 0; i < 1000000; ++i) {
      s ^= s << 13; s ^= s >> 7; s ^= s << 17;   // (xorshift64)
      const int bits = i % 54;                   // values in [2^bits, 2^(bits + 1)), capped at 2^53
      long long v = bits == 53 ? P53 : (long long)((1ull << bits) | ((s >> 8) & ((1ull << bits) - 1)));
      check_value(k, (s & 1) ? -v : v);
    }
    // next to the ties of every modulus: x = q m + c, c = +-(m - 1) / 2 and +-(m + 1) / 2, at a
    // small scale and at 2^52
    for (int l = 0; l < nmod; ++l) {
      const long long m = k.m[l];
      const long long qs[] = {0, 1, 2, 1000003, (1ll << 52) / m - 1, (1ll << 52) / m, (1ll << 52) / m + 1, P53 / m - 1};
      for (long long q : qs)
        for (long long c : {(m - 1) / 2, -((m - 1) / 2), (m + 1) / 2, -((m + 1) / 2)})
          for (int sg : {1, -1}) {
            const long long v = sg * q * m + c;
            if (v <= P53 && v >= -P53) check_value(k, v);
          }
    }
  }
  std::printf("values=%lld\n", g_values);
  if (g_fail) {
    std::printf("oz_residue_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("oz_residue_check OK\n");
  return 0;
}
