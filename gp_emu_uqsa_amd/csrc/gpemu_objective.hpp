// gpemu_objective.hpp -- the objective's host arithmetic, shared by every path to it (k_tiny,
// k_snb, the general single-GPU path and the row-block one): kernel codes, the argument
// split, the length-scale check, the closed form of LLH / sigma^2 / gradient scale, the
// failure messages and the reader of the one-launch kernels' result buffer.  Host only (no
// HIP or kernel header), so tests/host/objective_check.cpp runs it without a GPU.
#pragma once
#include <cmath>
#include <string>

#include "../../include/gpemu.h"
#include "gpemu_small.hpp"

namespace gpe {

// the device kernels' correlation families (described in gpemu_kernels.hpp)
enum : int { FAM_GAUSS = 0, FAM_MATERN32 = 1, FAM_MATERN52 = 2 };

// A kernel code is the nugget convention (bit 0) OR-ed with the correlation family
// (GPE_KERNEL_MATERN32 / GPE_KERNEL_MATERN52, 0 = Gaussian).
constexpr int KERNEL_FAMILY_BITS = GPE_KERNEL_MATERN32 | GPE_KERNEL_MATERN52;
inline bool kernel_ok(int kernel) {
  return (kernel & ~(KERNEL_FAMILY_BITS | GPE_KERNEL_ALT_NUG)) == 0 &&
         (kernel & KERNEL_FAMILY_BITS) != KERNEL_FAMILY_BITS;
}
inline bool kernel_alt(int kernel) { return (kernel & GPE_KERNEL_ALT_NUG) != 0; }
// the device kernels' FAM_* of a valid kernel code
inline int kernel_fam(int kernel) {
  return (kernel & GPE_KERNEL_MATERN32) ? FAM_MATERN32 : (kernel & GPE_KERNEL_MATERN52) ? FAM_MATERN52 : FAM_GAUSS;
}

inline void kernel_consts(int kernel, double nu, bool predict, double* coff, double* cdiag) {
  if (kernel_alt(kernel)) {
    *coff = 1.0;
    *cdiag = predict ? 1.0 + nu * nu : 1.0;
  } else {
    *coff = 1.0 - nu;
    *cdiag = predict ? 1.0 : 1.0 - nu;
  }
}

// What an objective call's variant, kernel and hyperparameter vector hp = [delta (d), nu if
// fitted, sigma if gp4ml] say (the kernel code itself is checked by the caller).
struct ObjArgs {
  bool gp4ml = false, fitnug = false;
  double nu = 0.0, s2 = 1.0, rscale = 0.0;
};
inline int objective_args(int variant, int kernel, int d, const double* hp, int n_hp, double nu_fixed,
                          ObjArgs* a, std::string* err) {
  if (variant != GPE_GP4ML && variant != GPE_MUCM) return *err = "bad variant", GPE_ERR_ARG;
  a->gp4ml = variant == GPE_GP4ML;
  const int base = a->gp4ml ? d + 1 : d;
  if (n_hp != base && n_hp != base + 1) return *err = "n_hp inconsistent with d", GPE_ERR_ARG;
  a->fitnug = n_hp == base + 1;
  a->nu = a->fitnug ? hp[d] : nu_fixed;
  const double sigma = a->gp4ml ? hp[n_hp - 1] : 1.0;
  a->s2 = a->gp4ml ? sigma * sigma : 1.0;
  a->rscale = (a->gp4ml && kernel_alt(kernel)) ? 1.0 : 0.0;
  return GPE_OK;
}

// out[k] = 1 / hp[k] up to the first k whose length scale is zero or NaN (neither > 0 nor
// < 0), which is returned; -1: none.  There the reference's covariance is NaN and its Cholesky
// raises LinAlgError (-> `return None`, _emulatoroptimise.py:374-376, :489-491): GPE_NOT_PD.
inline int inv_length_scales(const double* hp, int d, double* out) {
  for (int k = 0; k < d; ++k) {
    if (!(hp[k] > 0.0) && !(hp[k] < 0.0)) return k;
    out[k] = 1.0 / hp[k];
  }
  return -1;
}
inline std::string bad_length_scale(int k) { return "length scale delta[" + std::to_string(k) + "] is zero or NaN"; }

// the two GPE_NOT_PD messages: the Cholesky's failed column, and Q = H^T A^-1 H
inline std::string not_pd_pivot(int info) { return "matrix not positive definite (pivot " + std::to_string(info) + ")"; }
constexpr const char* Q_NOT_PD = "H^T A^-1 H not positive definite";

// LLH, sigma^2 (gp4ml: the given one; MUCM: its estimate), the factor of alpha's column of T2
// (small_t2) and the gradient's scale, from the q x q algebra and log|A|
struct ObjValue {
  double llh, sig2, cfac, gscale;
};
inline ObjValue objective_value(const SmallAlgebra& sa, double logdetA, double n, int q, bool gp4ml, double s2) {
  ObjValue v;
  if (gp4ml) {
    v.llh = 0.5 * (sa.quad + logdetA + sa.logdetQ + (n - q) * std::log(2.0 * M_PI));
    v.sig2 = s2;
    v.cfac = 1.0;
    v.gscale = s2;
  } else {
    v.sig2 = sa.quad / (n - q - 2.0);
    v.llh = 0.5 * ((n - q) * std::log(v.sig2) + logdetA + sa.logdetQ);
    v.cfac = (n - q) / (v.sig2 * (n - q - 2.0));
    v.gscale = v.sig2;
  }
  return v;
}

// The separable multi-output objective (gpe_objective_multi) from the small
// algebra and log|A|: Sigma-hat = S / (n - q - 2) (p x p row-major),
// llh = 1/2 [(n - q) log|Sigma-hat| + p log|A| + p log|Q|], the factor of the first p columns
// of T2 (small_multi_t2) and the gradient's scale: the gradient is p times small_grad's (gscale
// 1) of the contraction sums, the plain derivative of llh.
constexpr const char* S_NOT_PD = "F^T P F not positive definite";
struct ObjValueMulti {
  double llh, cfac, gscale;
  std::vector<double> Sigma;
};
inline ObjValueMulti objective_value_multi(const SmallMulti& sm, double logdetA, double n) {
  ObjValueMulti v;
  const int p = sm.p, q = sm.q;
  const double dof = n - q - 2.0;
  v.Sigma.resize((size_t)p * p);
  for (size_t e = 0; e < v.Sigma.size(); ++e) v.Sigma[e] = sm.S[e] / dof;
  const double logdetSigma = sm.logdetS - p * std::log(dof);
  v.llh = 0.5 * ((n - q) * logdetSigma + p * logdetA + p * sm.logdetQ);
  v.cfac = (n - q) / p;
  v.gscale = p;
  return v;
}

// the gradient from the d + 3 contraction sums (small_grad with the K-build's constants)
inline void objective_grad(const double* red, int d, int kernel, double nu, bool fitnug, bool gp4ml, double gscale,
                           double s2, int n_hp, double* grad, bool std_r) {
  double coff, cdiag;
  kernel_consts(kernel, nu, true, &coff, &cdiag);
  small_grad(red, d, kernel_alt(kernel), nu, fitnug, gp4ml, gscale, s2, coff, cdiag, n_hp, grad, std_r);
}

// The pinned result buffer of the one-launch kernels (k_tiny: nld = 1; k_snb: nld = NB), as
// TinyArgs::small / SnbArgs::small lay it out: Gram (P x P) | nld log|L| parts | info (the
// failed column; -1: a wait ran out; -2: workgroup 0 never reported) | d + 3 | Q refused by
// the device's own Cholesky | nh helpers' partial sums (64 each, slot 63 the call's tag once
// the helper's sums are in).
struct OneLaunchResult {
  const double* h;
  int P, d, nld, nh;
  double tag;
  const char* name;   // "k_tiny" / "k_snb", for the messages

  // GPE_OK, or the kernel's failure (neither negative info is the matrix's doing)
  int status(std::string* err) const {
    const int info = (int)h[P * P + nld];
    if (info == 0) return GPE_OK;
    *err = info == -1  ? std::string(name) + ": a workgroup wait timed out"
           : info < 0 ? std::string(name) + ": workgroup 0 did not complete"
                      : not_pd_pivot(info);
    return info < 0 ? GPE_ERR_HIP : GPE_NOT_PD;
  }
  double logdetA() const {
    double s = 0.0;
    for (int k = 0; k < nld; ++k) s += h[P * P + k];
    return 2.0 * s;
  }
  bool q_refused() const { return h[P * P + nld + 1 + d + 3] != 0.0; }
  // red[0 : d+3] = the helpers' partials summed in helper order, once every helper's sums
  // are this call's (a helper that gave up a wait never tags them)
  int sums(double* red, std::string* err) const {
    const double* part = h + (size_t)P * P + nld + 1 + d + 4;
    for (int g = 0; g < nh; ++g)
      if (part[g * 64 + 63] != tag) {
        *err = std::string(name) + ": helper " + std::to_string(g) + " did not finish (a wait timed out)";
        return GPE_ERR_HIP;
      }
    for (int k = 0; k < d + 3; ++k) {
      double v = 0.0;
      for (int g = 0; g < nh; ++g) v += part[g * 64 + k];
      red[k] = v;
    }
    return GPE_OK;
  }
};

}  // namespace gpe
