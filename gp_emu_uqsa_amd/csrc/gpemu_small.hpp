// gpemu_small.hpp -- host-side q x q algebra on the Gram matrix of [L^-1 f, L^-1 H]
// (shared by the single-GPU and the distributed objective).
#pragma once
#include <cmath>
#include <limits>
#include <vector>

namespace gpe {

// dense Cholesky of a small SPD matrix (row-major), false if not PD
inline bool small_chol(std::vector<double>& a, int q) {
  for (int j = 0; j < q; ++j) {
    double s = a[j * q + j];
    for (int k = 0; k < j; ++k) s -= a[j * q + k] * a[j * q + k];
    if (!(s > 0.0)) return false;
    const double dj = std::sqrt(s);
    a[j * q + j] = dj;
    for (int i = j + 1; i < q; ++i) {
      double t = a[i * q + j];
      for (int k = 0; k < j; ++k) t -= a[i * q + k] * a[j * q + k];
      a[i * q + j] = t / dj;
    }
    for (int k = j + 1; k < q; ++k) a[j * q + k] = 0.0;
  }
  return true;
}

// solve K y = b (K lower, row-major)
inline void small_fwd(const std::vector<double>& K, int q, double* b) {
  for (int i = 0; i < q; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= K[i * q + k] * b[k];
    b[i] = s / K[i * q + i];
  }
}
inline void small_bwd(const std::vector<double>& K, int q, double* b) {
  for (int i = q - 1; i >= 0; --i) {
    double s = b[i];
    for (int k = i + 1; k < q; ++k) s -= K[k * q + i] * b[k];
    b[i] = s / K[i * q + i];
  }
}
// inverse of lower-triangular K (row-major)
inline std::vector<double> small_trinv(const std::vector<double>& K, int q) {
  std::vector<double> X((size_t)q * q, 0.0);
  for (int c0 = 0; c0 < q; ++c0) {
    std::vector<double> e(q, 0.0);
    e[c0] = 1.0;
    small_fwd(K, q, e.data());
    for (int i = 0; i < q; ++i) X[i * q + c0] = e[i];
  }
  return X;
}

struct SmallAlgebra {
  double zz = 0, quad = 0, logdetQ = 0;
  std::vector<double> Kq, beta;  // Kq row-major lower (q x q)
  bool ok = false;
};

inline SmallAlgebra small_from_gram(const std::vector<double>& G, int P) {
  // G over [z w]: zz = G00, wz = G[1:,0], Q = G[1:,1:]
  SmallAlgebra s;
  const int q = P - 1;
  s.zz = G[0];
  std::vector<double> Q((size_t)q * q), wz(q);
  for (int i = 0; i < q; ++i) {
    wz[i] = G[(i + 1) * P + 0];
    for (int j = 0; j < q; ++j) Q[i * q + j] = G[(i + 1) * P + (j + 1)];
  }
  if (!small_chol(Q, q)) return s;
  s.Kq = Q;
  s.beta = wz;
  small_fwd(Q, q, s.beta.data());
  small_bwd(Q, q, s.beta.data());
  double wzB = 0.0;
  for (int i = 0; i < q; ++i) wzB += wz[i] * s.beta[i];
  s.quad = s.zz - wzB;
  s.logdetQ = 0.0;
  for (int i = 0; i < q; ++i) s.logdetQ += 2.0 * std::log(Q[i * q + i]);
  s.ok = true;
  return s;
}

// T2 (P x P, column-major) with R2 = [z w] T2 = [sqrt(c)(z - w beta), w Kq^-T]:
// L^-T R2 = [sqrt(c) alpha, W], the two low-rank terms of the gradient's M
inline std::vector<double> small_t2(const SmallAlgebra& sa, int q, double cfac) {
  const int P = q + 1;
  std::vector<double> Kinv = small_trinv(sa.Kq, q);   // row-major
  std::vector<double> T2((size_t)P * P, 0.0);
  const double sc = std::sqrt(cfac);
  T2[0] = sc;
  for (int i = 0; i < q; ++i) T2[(i + 1) + 0 * P] = -sc * sa.beta[i];
  for (int o = 0; o < q; ++o)
    for (int i = 0; i < q; ++i) T2[(i + 1) + (o + 1) * P] = Kinv[o * q + i];   // (Kq^-T)(i,o)
  return T2;
}

// small_chol with a floor under each pivot (false if pivot j is not above floor[j])
inline bool small_chol_floor(std::vector<double>& a, int q, const std::vector<double>& floor) {
  for (int j = 0; j < q; ++j) {
    double s = a[j * q + j];
    for (int k = 0; k < j; ++k) s -= a[j * q + k] * a[j * q + k];
    if (!(s > floor[j])) return false;
    const double dj = std::sqrt(s);
    a[j * q + j] = dj;
    for (int i = j + 1; i < q; ++i) {
      double t = a[i * q + j];
      for (int k = 0; k < j; ++k) t -= a[i * q + k] * a[j * q + k];
      a[i * q + j] = t / dj;
    }
    for (int k = j + 1; k < q; ++k) a[j * q + k] = 0.0;
  }
  return true;
}

// The separable multi-output emulator's small algebra on the Gram matrix of
// Z = L^-1 [F H], F n x p and H n x q: Q = Z_H^T Z_H = Kq Kq^T, B = Q^-1 Z_H^T Z_F (the GLS
// coefficients, one column per output), S = F^T P F = Z_F^T Z_F - Y^T Y with Y = Kq^-1 Z_H^T Z_F
// (symmetric as formed) and its Cholesky factor C.
// A pivot of Q or S at or below 64 (p + q) eps times its column's diagonal entry of the Gram
// matrix is refused: a repeated basis column, or an output that is a linear combination of the
// others and H, leaves a pivot that is zero in exact arithmetic and a rounding residue of either
// sign here (S = Z_F^T Z_F - Y^T Y cancels against the Gram's diagonal, so that is its scale).
struct SmallMulti {
  int p = 0, q = 0;
  double logdetQ = 0, logdetS = 0;
  std::vector<double> Kq, B, S, C;   // row-major: Kq q x q lower, B q x p, S p x p, C p x p lower
  int refused = 0;                   // 0: fine; 1: Q is not positive definite; 2: S is not
  bool ok() const { return refused == 0; }
};

inline SmallMulti small_multi_from_gram(const std::vector<double>& G, int p, int q) {
  SmallMulti s;
  s.p = p;
  s.q = q;
  const int P = p + q;
  std::vector<double> Q((size_t)q * q);
  for (int i = 0; i < q; ++i)
    for (int j = 0; j < q; ++j) Q[i * q + j] = G[(size_t)(p + i) * P + (p + j)];
  const double rel = 64.0 * P * std::numeric_limits<double>::epsilon();
  std::vector<double> floorQ(q), floorS(p);
  for (int i = 0; i < q; ++i) floorQ[i] = rel * Q[i * q + i];
  for (int a = 0; a < p; ++a) floorS[a] = rel * G[(size_t)a * P + a];
  if (!small_chol_floor(Q, q, floorQ)) return s.refused = 1, s;
  s.Kq = Q;
  // Y = Kq^-1 Z_H^T Z_F column by column, B = Kq^-T Y
  std::vector<double> Y((size_t)q * p), col(q);
  s.B.assign((size_t)q * p, 0.0);
  for (int a = 0; a < p; ++a) {
    for (int i = 0; i < q; ++i) col[i] = G[(size_t)(p + i) * P + a];
    small_fwd(Q, q, col.data());
    for (int i = 0; i < q; ++i) Y[i * p + a] = col[i];
    small_bwd(Q, q, col.data());
    for (int i = 0; i < q; ++i) s.B[i * p + a] = col[i];
  }
  s.S.assign((size_t)p * p, 0.0);
  for (int a = 0; a < p; ++a)
    for (int b = 0; b <= a; ++b) {
      double yy = 0.0;
      for (int i = 0; i < q; ++i) yy += Y[i * p + a] * Y[i * p + b];
      s.S[a * p + b] = s.S[b * p + a] = G[(size_t)a * P + b] - yy;
    }
  s.C = s.S;
  if (!small_chol_floor(s.C, p, floorS)) return s.refused = 2, s;
  for (int i = 0; i < q; ++i) s.logdetQ += 2.0 * std::log(Q[i * q + i]);
  for (int a = 0; a < p; ++a) s.logdetS += 2.0 * std::log(s.C[a * p + a]);
  return s;
}

// small_t2 for p outputs: T2 ((p + q)-square, column-major) with
// Z T2 = [sqrt(cfac) (Z_F - Z_H B) C^-T, Z_H Kq^-T], so L^-T Z T2 = [sqrt(cfac) P F C^-T, G Kq^-T]
inline std::vector<double> small_multi_t2(const SmallMulti& sm, double cfac) {
  const int p = sm.p, q = sm.q, P = p + q;
  const std::vector<double> Kinv = small_trinv(sm.Kq, q), Cinv = small_trinv(sm.C, p);   // row-major
  std::vector<double> T2((size_t)P * P, 0.0);
  const double sc = std::sqrt(cfac);
  for (int c = 0; c < p; ++c) {
    for (int a = 0; a <= c; ++a) T2[a + (size_t)c * P] = sc * Cinv[c * p + a];   // (C^-T)(a, c) = Cinv(c, a)
    for (int i = 0; i < q; ++i) {
      double v = 0.0;
      for (int a = 0; a <= c; ++a) v += sm.B[i * p + a] * Cinv[c * p + a];
      T2[(p + i) + (size_t)c * P] = -sc * v;
    }
  }
  for (int o = 0; o < q; ++o)
    for (int i = 0; i < q; ++i) T2[(p + i) + (size_t)(p + o) * P] = Kinv[o * q + i];   // (Kq^-T)(i, o)
  return T2;
}

// gradient from the contraction sums red[0:d] = sum M E dx_k^2, red[d] = sum_{i>j} M E,
// red[d+1] = tr M (the d+2 outputs of k_contract); coff/cdiag as the K-build's
// red = [S_1..S_d, E, T, R] from k_contract; std_r: the std kernel with a per-point r,
// whose sigma derivative the reference takes as A - diag(r) although A carries no r
// (_emulatoroptimise.py:476-478 vs _emulatorclasses.py:572-575): -1/2 sum_i M_ii r_i
inline void small_grad(const double* red, int d, bool alt_nug, double nu, bool fitnug, bool gp4ml,
                       double gscale, double s2, double coff, double cdiag, int n_hp, double* grad,
                       bool std_r = false) {
  const double pref = alt_nug ? 1.0 : (1.0 - nu);
  const double SE = 2.0 * red[d], Tr = red[d + 1];
  for (int k = 0; k < d; ++k) grad[k] = 0.5 * gscale * pref * 2.0 * red[k];
  if (fitnug) grad[d] = alt_nug ? 0.5 * gscale * nu * nu * Tr : 0.5 * gscale * (-0.5 * nu) * SE;
  if (gp4ml) grad[n_hp - 1] = 0.5 * s2 * (coff * SE + cdiag * Tr) - (std_r ? 0.5 * red[d + 2] : 0.0);
}

}  // namespace gpe
