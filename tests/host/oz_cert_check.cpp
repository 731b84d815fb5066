// oz_cert_check.cpp -- host-only check of the 15-moduli certificate of the int8 products
// (gpemu_ozaki.hpp: oz_cert_term, oz_cert_ok and the constants OZ_T15_HI / OZ_T15_LO in their
// host form, oz_consts_cert) against 128-bit integer arithmetic.  No HIP runtime call: it runs
// without a GPU.  Built and run by tests/test_oz_cert_host.py:
//   hipcc --offload-arch=gfx950 -std=c++17 -I gp_emu_uqsa_amd/csrc tests/host/oz_cert_check.cpp
// Checks:
//   - T15 = floor(M15^2 / 2^130) recomputed from the first 15 moduli of oz_consts is the
//     header's constant and the decimal number of its comment;
//   - y^2 for |x'| at 0, 1, 2^32 - 1, 2^32, 2^32 + 1, 2^53 (either sign), and |x'| <= 2^32 y;
//   - A B just below and just above T15 for 10^5 values of A (oz_cert_ok is A B < T15; T15 has a
//     prime factor above 2^64, so A B = T15 has no solution in 64-bit sums), and the decision
//     against the 128-bit product on 2 10^5 seeded pairs;
//   - the largest possible sum, OZ_MAX_K terms of (2^21 + 1)^2, stays below 2^60;
//   - oz_consts_cert: 15 moduli, Md + Mlo = Md16 / 191 (M15 with the 16-moduli constant's own
//     rounding), beta the 16-moduli value, rhi + rlo = y / m;
//   - 10^5 seeded row pairs, entries |.| <= 2^53, K <= 2048: whenever the certificate holds for
//     the pair's sums, the exact |sum_k a'_k b'_k| < M15 / 2.
// Prints one line per failed check, "pairs=<count> certified=<count>"; exit status 0 and a last
// line "oz_cert_check OK" when every check holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpemu_kernels.hpp"
#include "gpemu_ozaki.hpp"

using namespace gpe;
typedef __int128 i128;
typedef unsigned __int128 u128;
typedef unsigned long long ull;

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

static u128 from_decimal(const char* s) {
  u128 v = 0;
  for (; *s; ++s) v = v * 10 + (unsigned)(*s - '0');
  return v;
}

static ull xorshift(ull& s) {
  s ^= s << 13; s ^= s >> 7; s ^= s << 17;
  return s;
}

int main() {
  const OzConst k16 = oz_consts(OZ_MAXMOD, 16384);
  // M15 ~ 2^117.4 fits 128 bits; M15^2 does not: floor(M15^2 / 2^130) from 64-bit limbs
  u128 M15 = 1;
  for (int l = 0; l < OZ_CERT_NMOD; ++l) M15 *= (unsigned)k16.m[l];
  CHECK(k16.m[OZ_CERT_NMOD] == 191, "the dropped modulus is %d", k16.m[OZ_CERT_NMOD]);
  u128 T15;
  {
    const ull lo = (ull)M15, hi = (ull)(M15 >> 64);
    // M15^2 = hi^2 2^128 + 2 hi lo 2^64 + lo^2, as four 64-bit limbs w[0..3]
    ull w[4] = {0, 0, 0, 0};
    const auto add = [&](u128 v, int limb) {   // w += v 2^(64 limb)
      for (int i = limb; i < 4 && v; ++i) {
        const u128 t = (u128)w[i] + (ull)v;
        w[i] = (ull)t;
        v = (v >> 64) + (t >> 64);
      }
    };
    add((u128)lo * lo, 0);
    add((u128)hi * lo, 1);
    add((u128)hi * lo, 1);
    add((u128)hi * hi, 2);
    // >> 130: limbs 2, 3 (bits 128 ..) shifted right by 2
    T15 = (((u128)w[3] << 64) | w[2]) >> 2;
  }
  const u128 T15h = ((u128)OZ_T15_HI << 64) | OZ_T15_LO;
  CHECK(T15 == T15h, "T15 recomputed differs from OZ_T15_HI / OZ_T15_LO");
  CHECK(T15 == from_decimal("34409203667017820043519436844158"), "T15 is not the comment's number");

  // y and y^2
  const long long P32 = 1ll << 32, P53 = 1ll << 53;
  const long long vals[] = {0, 1, P32 - 1, P32, P32 + 1, P53 - 1, P53};
  for (long long v : vals)
    for (int sg : {1, -1}) {
      const ull y = (ull)(v >> 32) + 1;
      const ull t = oz_cert_term((double)(sg * v));
      CHECK(t == y * y, "x' = %lld: term %llu, y = %llu", sg * v, t, y);
      CHECK((u128)v <= ((u128)y << 32), "x' = %lld: |x'| > 2^32 y", v);
    }
  CHECK(oz_cert_term((double)P53) == ((1ull << 21) + 1) * ((1ull << 21) + 1), "largest term");
  // the largest sum: no overflow, below 2^60
  {
    const u128 smax = (u128)OZ_MAX_K * (((1ull << 21) + 1) * ((1ull << 21) + 1));
    CHECK(smax < ((u128)1 << 60), "largest sum reaches 2^60");
    ull s = 0;
    for (int k = 0; k < OZ_MAX_K; ++k) s += oz_cert_term((double)P53);
    CHECK((u128)s == smax, "largest sum wrapped");
    CHECK(!oz_cert_ok(s, s), "largest sums certified");
  }
  // A B around T15.  T15 = 2 x 1277 x 301190441 x 44731405525778204147 and the last factor is
  // above 2^64, so no two 64-bit sums multiply to T15 itself: for every A the nearest products are
  // A floor(T15 / A) < T15 (certified) and A (floor(T15 / A) + 1) > T15 (refused)
  {
    const u128 big = from_decimal("44731405525778204147");
    CHECK(T15 % big == 0 && (big >> 64) != 0 && T15 / big == (u128)2 * 1277 * 301190441, "T15's factors");
    ull s = 0x6a09e667f3bcc909ull;
    for (int i = 0; i < 100000; ++i) {
      const ull A = i < 20 ? (1ull << (41 + i)) : ((xorshift(s) >> (i % 23)) | (1ull << 41));   // (T15 / A < 2^64)
      const ull B = (ull)(T15 / A);
      CHECK((T15 / A) >> 64 == 0, "A %llu too small", A);
      CHECK((u128)A * B < T15 && (u128)A * (B + 1) > T15, "bracket at A %llu", A);
      CHECK(oz_cert_ok(A, B) && oz_cert_ok(B, A), "A %llu: just below T15 refused", A);
      CHECK(!oz_cert_ok(A, B + 1) && !oz_cert_ok(B + 1, A), "A %llu: just above T15 certified", A);
    }
    CHECK(oz_cert_ok(0, ~0ull) && oz_cert_ok(~0ull, 0), "zero sums");
    CHECK(!oz_cert_ok(~0ull, ~0ull), "largest operands");
    CHECK(oz_cert_ok(1, (ull)~0ull), "2^64 - 1 < T15");
  }
  // the exact decision against 128-bit products on seeded pairs over every magnitude
  {
    ull s = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < 200000; ++i) {
      const ull A = xorshift(s) >> (4 + i % 56), B = xorshift(s) >> (4 + (i / 56) % 56);
      CHECK(oz_cert_ok(A, B) == ((u128)A * B < T15), "A %llu B %llu", A, B);
    }
  }
  // the 15-moduli constants
  {
    const OzConst k15 = oz_consts_cert(16384);
    CHECK(k15.nmod == OZ_CERT_NMOD, "nmod %d", k15.nmod);
    CHECK(k15.beta == k16.beta && k15.beta == 53, "beta %d against %d", k15.beta, k16.beta);
    CHECK(oz_consts(OZ_CERT_NMOD, 16384).beta < 53, "15 moduli alone carry 53 bits");
    // the scale: Md + Mlo = Md16 / 191 to double-double accuracy, so M15 with Md16's own rounding
    {
      const double last = (double)k16.m[OZ_CERT_NMOD];
      const double back = std::fma(k15.Md, last, k15.Mlo * last);   // (Md + Mlo) 191, one rounding
      CHECK(back == k16.Md, "(Md + Mlo) 191 = %.17g, Md16 = %.17g", back, k16.Md);
      CHECK(std::fabs(k15.Mlo) <= std::ldexp(k15.Md, -53), "Mlo above half an ulp of Md");
      CHECK(std::fabs(k15.Md / (double)M15 - 1.0) <= std::ldexp(1.0, -51), "Md is not M15");
      CHECK(k16.Mlo == 0.0 && oz_consts(12, 4096).Mlo == 0.0, "Mlo of the plain constants");
    }
    for (int l = 0; l < OZ_CERT_NMOD; ++l) {
      CHECK(k15.m[l] == k16.m[l] && k15.wlo[l] == k16.wlo[l] && k15.whi[l] == k16.whi[l] && k15.inv[l] == k16.inv[l] &&
                k15.c16[l] == k16.c16[l],
            "modulus %d differs from the 16-moduli context's", l);
      // y = round((rhi + rlo) m) is the inverse of M15 / m modulo m
      const long long y = (long long)((k15.rhi[l] + k15.rlo[l]) * k15.m[l] + 0.5);
      CHECK((u128)y * ((M15 / (unsigned)k15.m[l]) % (unsigned)k15.m[l]) % (unsigned)k15.m[l] == 1, "y of modulus %d", l);
    }
  }
  // random row pairs: certified => |sum a' b'| < M15 / 2
  long long pairs = 0, certified = 0;
  {
    ull s = 0x2545f4914f6cdd1dull;
    std::vector<long long> a, b;
    for (int it = 0; it < 100000; ++it) {
      const int K = 1 + (int)(xorshift(s) % 2048);
      // magnitudes: flat at the top (refused for long K), decaying, mixed; same or random signs
      const int kind = it % 4;
      a.assign((size_t)K, 0);
      b.assign((size_t)K, 0);
      ull sa = 0, sb = 0;
      i128 dot = 0;
      const int topbits = kind == 0 ? 53 : 44 + (int)(xorshift(s) % 10);   // 44 .. 53
      for (int k = 0; k < K; ++k) {
        for (int side = 0; side < 2; ++side) {
          int bits = topbits;
          if (kind == 1) bits = topbits - (k % 40);
          else if (kind == 2) bits = (int)(xorshift(s) % (unsigned)(topbits + 1));
          else if (kind == 3 && k > 0) bits = topbits - 12;
          if (bits < 0) bits = 0;
          long long v = bits >= 53 ? (xorshift(s) & 1 ? P53 : P53 - 1)
                                   : (long long)((1ull << bits) | (xorshift(s) & ((1ull << bits) - 1)));
          if (kind != 0 && (xorshift(s) & 1)) v = -v;
          (side ? b : a)[(size_t)k] = v;
        }
        sa += oz_cert_term((double)a[(size_t)k]);
        sb += oz_cert_term((double)b[(size_t)k]);
        dot += (i128)a[(size_t)k] * b[(size_t)k];
      }
      ++pairs;
      if (oz_cert_ok(sa, sb)) {
        ++certified;
        const u128 mag = dot < 0 ? (u128)(-dot) : (u128)dot;
        CHECK(2 * mag < M15, "pair %d (K %d, kind %d): certified and |dot| >= M15 / 2", it, K, kind);
      }
    }
  }
  std::printf("pairs=%lld certified=%lld\n", pairs, certified);
  CHECK(certified > pairs / 10 && certified < pairs, "the pairs do not exercise both decisions");
  if (g_fail) {
    std::printf("oz_cert_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("oz_cert_check OK\n");
  return 0;
}
