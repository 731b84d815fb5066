// Stand-alone driver of csrc/gpemu_hm_mv.hpp for tests/test_implausibility_multi_host.py: any
// C++17 compiler, no HIP, no GPU.  For p in {1, 2, 13, 31, 32} and symmetric positive definite
// Sigma and V of condition number 1e3 (2 seeds each):
//   - hm_mv_prepare's W and lambda: |W^T V W - I| and the off-diagonal of W^T Sigma W within
//     1e-10 (the products formed in long double, so that the figure is W's own), lambda ascending
//     and the diagonal of W^T Sigma W;
//   - I^2 = sum_j (W^T r)_j^2 / (c lambda_j + 1) in double against r^T (c Sigma + V)^-1 r by a
//     long double Cholesky solve, for c in {1e-6, 1e-3, 0.3, 1}: 1e-10 relative;
//   - "not positive definite" (return 1) for a V with a zero or a negative eigenvalue and for a
//     NaN on or off its diagonal.
// Prints the worst figures and "hm_mv_check OK" and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpemu_hm_mv.hpp"

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

typedef long double ld;

static unsigned long long rng_state = 1;
static double uniform() {   // (a 64-bit LCG's top 53 bits)
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}

// Q diag(e) Q^T with Q the Gram-Schmidt basis of a random matrix and e log-spaced over
// [scale / cond, scale] (p = 1: scale)
static std::vector<double> spd(int p, double scale, double cond) {
  const size_t P = (size_t)p;
  std::vector<ld> Q(P * P);
  for (ld& v : Q) v = (ld)uniform() - 0.5L;
  for (int j = 0; j < p; ++j) {
    for (int pass = 0; pass < 2; ++pass)
      for (int k = 0; k < j; ++k) {
        ld dot = 0;
        for (int i = 0; i < p; ++i) dot += Q[i * P + j] * Q[i * P + k];
        for (int i = 0; i < p; ++i) Q[i * P + j] -= dot * Q[i * P + k];
      }
    ld nrm = 0;
    for (int i = 0; i < p; ++i) nrm += Q[i * P + j] * Q[i * P + j];
    nrm = std::sqrt(nrm);
    for (int i = 0; i < p; ++i) Q[i * P + j] /= nrm;
  }
  std::vector<double> A(P * P);
  for (int a = 0; a < p; ++a)
    for (int b = 0; b <= a; ++b) {
      ld v = 0;
      for (int j = 0; j < p; ++j) {
        const ld e = p == 1 ? (ld)scale : (ld)scale * std::pow((ld)cond, -(ld)j / (ld)(p - 1));
        v += Q[a * P + j] * e * Q[b * P + j];
      }
      A[a * P + b] = A[b * P + a] = (double)v;
    }
  return A;
}

// r^T A^-1 r by a long double Cholesky of A (p x p row-major)
static ld solve_quad(int p, const std::vector<ld>& A, const std::vector<double>& r) {
  const size_t P = (size_t)p;
  std::vector<ld> L(P * P, 0.0L), y(P);
  for (int j = 0; j < p; ++j) {
    ld piv = A[j * P + j];
    for (int k = 0; k < j; ++k) piv -= L[j * P + k] * L[j * P + k];
    L[j * P + j] = std::sqrt(piv);
    for (int i = j + 1; i < p; ++i) {
      ld v = A[i * P + j];
      for (int k = 0; k < j; ++k) v -= L[i * P + k] * L[j * P + k];
      L[i * P + j] = v / L[j * P + j];
    }
  }
  ld q = 0;
  for (int i = 0; i < p; ++i) {
    ld v = r[i];
    for (int k = 0; k < i; ++k) v -= L[i * P + k] * y[k];
    y[i] = v / L[i * P + i];
    q += y[i] * y[i];
  }
  return q;
}

static double worst_id = 0.0, worst_off = 0.0, worst_i2 = 0.0;

static void check(int p, unsigned long long seed) {
  const size_t P = (size_t)p;
  rng_state = seed;
  const std::vector<double> Sigma = spd(p, 4.0, 1e3), V = spd(p, 1.0, 1e3);
  std::vector<double> W(P * P), lam(P);
  EXPECT(hm_mv_prepare(p, Sigma.data(), V.data(), W.data(), lam.data()) == 0, "p %d", p);
  for (int j = 0; j + 1 < p; ++j) EXPECT(lam[j] <= lam[j + 1], "p %d: lambda %d %g above lambda %d %g", p, j, lam[j], j + 1, lam[j + 1]);
  EXPECT(lam[0] > 0.0, "p %d: lambda_0 %g", p, lam[0]);
  for (int i = 0; i < p; ++i)
    for (int j = 0; j < p; ++j) {
      ld wv = 0, ws = 0;
      for (int a = 0; a < p; ++a)
        for (int b = 0; b < p; ++b) {
          wv += (ld)W[a * P + i] * (ld)V[a * P + b] * (ld)W[b * P + j];
          ws += (ld)W[a * P + i] * (ld)Sigma[a * P + b] * (ld)W[b * P + j];
        }
      const double eid = (double)std::fabs(wv - (i == j ? 1.0L : 0.0L));
      const double eoff = (double)std::fabs(ws - (i == j ? (ld)lam[i] : 0.0L));
      if (eid > worst_id) worst_id = eid;
      if (eoff > worst_off) worst_off = eoff;
      EXPECT(eid <= 1e-10, "p %d: (W^T V W - I)[%d, %d] = %g", p, i, j, eid);
      EXPECT(eoff <= 1e-10, "p %d: (W^T Sigma W - Lambda)[%d, %d] = %g", p, i, j, eoff);
    }
  std::vector<double> r(P);
  for (double c : {1e-6, 1e-3, 0.3, 1.0})
    for (int trial = 0; trial < 4; ++trial) {
      for (double& v : r) v = 4.0 * uniform() - 2.0;
      std::vector<ld> A(P * P);
      for (size_t e = 0; e < P * P; ++e) A[e] = (ld)c * (ld)Sigma[e] + (ld)V[e];
      const ld want = solve_quad(p, A, r);
      const double got = hm_mv_i2<double>(p, W.data(), lam.data(), r.data(), c);
      const double rel = (double)(std::fabs((ld)got - want) / want);
      if (rel > worst_i2) worst_i2 = rel;
      EXPECT(rel <= 1e-10, "p %d c %g: I^2 %.17g, the solve %.17Lg, relative %g", p, c, got, want, rel);
    }
}

static void check_not_pd() {
  double W[169], lam[13];
  const double S2[] = {2.0, 0.5, 0.5, 1.0};
  const double zero[] = {1.0, 1.0, 1.0, 1.0}, neg[] = {1.0, 2.0, 2.0, 1.0};
  const double nan_d[] = {NAN, 0.0, 0.0, 1.0}, nan_o[] = {1.0, NAN, NAN, 1.0}, nan_u[] = {1.0, NAN, 0.0, 1.0};
  const double ok[] = {1.0, 0.5, 0.5, 1.0}, z1[] = {0.0}, n1[] = {-1.0}, nn1[] = {NAN}, inf1[] = {INFINITY};
  EXPECT(hm_mv_prepare(2, S2, ok, W, lam) == 0, "a positive definite V");
  EXPECT(hm_mv_prepare(2, S2, zero, W, lam) == 1, "a zero eigenvalue");
  EXPECT(hm_mv_prepare(2, S2, neg, W, lam) == 1, "a negative eigenvalue");
  EXPECT(hm_mv_prepare(2, S2, nan_d, W, lam) == 1, "a NaN on the diagonal");
  EXPECT(hm_mv_prepare(2, S2, nan_o, W, lam) == 1, "a NaN off the diagonal");
  EXPECT(hm_mv_prepare(2, S2, nan_u, W, lam) == 1, "a NaN in the upper triangle alone");
  EXPECT(hm_mv_prepare(1, S2, z1, W, lam) == 1 && hm_mv_prepare(1, S2, n1, W, lam) == 1 &&
             hm_mv_prepare(1, S2, nn1, W, lam) == 1 && hm_mv_prepare(1, S2, inf1, W, lam) == 1,
         "p = 1");
  // p = 13: the identity with one diagonal entry 0, -1, NaN
  std::vector<double> S(169, 0.0), V(169, 0.0);
  for (int i = 0; i < 13; ++i) S[i * 13 + i] = 1.0 + i, V[i * 13 + i] = 1.0;
  EXPECT(hm_mv_prepare(13, S.data(), V.data(), W, lam) == 0 && lam[0] == 1.0 && lam[12] == 13.0, "p = 13 diagonal");
  for (double bad : {0.0, -1.0, (double)NAN}) {
    V[7 * 13 + 7] = bad;
    EXPECT(hm_mv_prepare(13, S.data(), V.data(), W, lam) == 1, "p = 13, V[7, 7] = %g", bad);
  }
}

int main() {
  for (int p : {1, 2, 13, 31, 32})
    for (unsigned long long seed : {11ULL, 12ULL}) check(p, seed + 100ULL * p);
  check_not_pd();
  std::printf("worst |W^T V W - I| %.3e, |W^T Sigma W - Lambda| %.3e, relative I^2 error %.3e\n", worst_id, worst_off,
              worst_i2);
  if (fails) return 1;
  std::printf("hm_mv_check OK\n");
  return 0;
}
