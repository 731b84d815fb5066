// gpemu_hm_mv.hpp -- the host algebra of the joint implausibility (gpe_hm_implausibility_mv):
// for a member of p outputs with between-output covariance Sigma and an observation covariance
// V, the measure at a candidate with emulator variance factor c is
//   I^2 = r^T (c Sigma + V)^-1 r,   r = mean - z.
// hm_mv_prepare finds W with W^T V W = I and W^T Sigma W = Lambda (the generalised eigenproblem
// Sigma w = lambda V w) once per call; then W^T (c Sigma + V) W = c Lambda + I for every c, so
//   (c Sigma + V)^-1 = W (c Lambda + I)^-1 W^T,   I^2 = sum_j (W^T r)_j^2 / (c lambda_j + 1):
// exact algebra, p dot products and p divisions per candidate and no factorisation there.
// Host-checkable: plain C++17, no HIP header, no LAPACK (tests/host/hm_mv_check.cpp).
#pragma once

#include <cmath>
#include <limits>
#include <utility>
#include <vector>

namespace gpe {

constexpr int HM_MV_SWEEPS = 60;   // cyclic Jacobi converges quadratically: about 10 at p = 32

// Sigma, V: p x p row-major, symmetric (the mean of the two triangles is used).  W (p x p
// row-major, column j the j-th generalised eigenvector) and lam (p, ascending) are written.
// Returns 0, or 1 when V is not positive definite (a Cholesky pivot <= 0 or NaN).
inline int hm_mv_prepare(int p, const double* Sigma, const double* V, double* W, double* lam) {
  const size_t P = (size_t)p;
  std::vector<double> C(P * P, 0.0), M(P * P), U(P * P, 0.0);
  // 1. V = C C^T
  for (int j = 0; j < p; ++j) {
    double piv = V[j * P + j];
    for (int k = 0; k < j; ++k) piv -= C[j * P + k] * C[j * P + k];
    if (!(piv > 0.0) || !std::isfinite(piv)) return 1;
    const double cjj = std::sqrt(piv);
    C[j * P + j] = cjj;
    for (int i = j + 1; i < p; ++i) {
      double v = 0.5 * (V[i * P + j] + V[j * P + i]);
      for (int k = 0; k < j; ++k) v -= C[i * P + k] * C[j * P + k];
      C[i * P + j] = v / cjj;
    }
  }
  // 2. M = C^-1 Sigma C^-T: X = C^-1 Sigma column by column, then M^T = C^-1 X^T; symmetrised
  std::vector<double> X(P * P);
  for (int i = 0; i < p; ++i)
    for (int j = 0; j < p; ++j) X[i * P + j] = 0.5 * (Sigma[i * P + j] + Sigma[j * P + i]);
  for (int col = 0; col < p; ++col)
    for (int i = 0; i < p; ++i) {
      double v = X[i * P + col];
      for (int k = 0; k < i; ++k) v -= C[i * P + k] * X[k * P + col];
      X[i * P + col] = v / C[i * P + i];
    }
  // (row `row` of X is a column of X^T)
  for (int row = 0; row < p; ++row)
    for (int i = 0; i < p; ++i) {
      double v = X[row * P + i];
      for (int k = 0; k < i; ++k) v -= C[i * P + k] * M[row * P + k];
      M[row * P + i] = v / C[i * P + i];
    }
  for (int i = 0; i < p; ++i)
    for (int j = 0; j < i; ++j) M[i * P + j] = M[j * P + i] = 0.5 * (M[i * P + j] + M[j * P + i]);
  // 3. cyclic Jacobi: M = U Lambda U^T
  for (int i = 0; i < p; ++i) U[i * P + i] = 1.0;
  double fro = 0.0;
  for (size_t e = 0; e < P * P; ++e) fro += M[e] * M[e];
  fro = std::sqrt(fro);
  const double eps = std::numeric_limits<double>::epsilon();
  for (int sweep = 0; sweep < HM_MV_SWEEPS; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < p; ++i)
      for (int j = 0; j < i; ++j) off += 2.0 * M[i * P + j] * M[i * P + j];
    if (!(std::sqrt(off) > eps * fro)) break;
    for (int a = 0; a + 1 < p; ++a)
      for (int b = a + 1; b < p; ++b) {
        const double mab = M[a * P + b];
        if (mab == 0.0) continue;
        const double theta = (M[b * P + b] - M[a * P + a]) / (2.0 * mab);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
        for (int k = 0; k < p; ++k) {   // columns a and b
          const double ka = M[k * P + a], kb = M[k * P + b];
          M[k * P + a] = cs * ka - sn * kb;
          M[k * P + b] = sn * ka + cs * kb;
        }
        for (int k = 0; k < p; ++k) {   // rows a and b
          const double ak = M[a * P + k], bk = M[b * P + k];
          M[a * P + k] = cs * ak - sn * bk;
          M[b * P + k] = sn * ak + cs * bk;
        }
        M[a * P + b] = M[b * P + a] = 0.0;
        for (int k = 0; k < p; ++k) {
          const double ka = U[k * P + a], kb = U[k * P + b];
          U[k * P + a] = cs * ka - sn * kb;
          U[k * P + b] = sn * ka + cs * kb;
        }
      }
  }
  // lambda ascending (an insertion sort of the column order; a NaN stays where it is)
  std::vector<int> ord(P);
  for (int j = 0; j < p; ++j) ord[j] = j;
  for (int j = 1; j < p; ++j)
    for (int k = j; k > 0 && M[ord[k] * P + ord[k]] < M[ord[k - 1] * P + ord[k - 1]]; --k) std::swap(ord[k], ord[k - 1]);
  // 4. W = C^-T U (the columns in lambda's order)
  for (int j = 0; j < p; ++j) {
    lam[j] = M[ord[j] * P + ord[j]];
    for (int i = p - 1; i >= 0; --i) {
      double v = U[i * P + ord[j]];
      for (int k = i + 1; k < p; ++k) v -= C[k * P + i] * W[k * P + j];
      W[i * P + j] = v / C[i * P + i];
    }
  }
  return 0;
}

// I^2 of one candidate from W and lambda in the order hm_point_multi (gpemu_hm.hpp) runs:
// y_j = sum_a W[a, j] r_a over a = 0 .. p - 1, then sum_j y_j^2 / (c lambda_j + 1) over j.
template <class T>
inline T hm_mv_i2(int p, const double* W, const double* lam, const T* r, T c) {
  T i2 = 0;
  for (int j = 0; j < p; ++j) {
    T y = 0;
    for (int a = 0; a < p; ++a) y += (T)W[(size_t)a * p + j] * r[a];
    i2 += y * y / (c * (T)lam[j] + (T)1);
  }
  return i2;
}

}  // namespace gpe
