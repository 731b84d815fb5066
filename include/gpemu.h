/*
 * gpemu.h -- C-ABI of libgpemu.so, the MI355X (gfx950) GP-emulator hot path.
 *
 * The reference (MathThyMod/GP_emu_UQSA) is pure Python and has no FFI: its
 * seams are duck-typed Python objects.  Each entry point below
 * replaces one of them; the reference interface it stands in for is cited.
 * The library is bound by the package's own ctypes layer
 * (gp_emu_uqsa_amd/native.py); INTEGRATION.md shows the binding a reference
 * maintainer would add.
 *
 * Conventions
 *  - All host buffers are caller-owned, C-contiguous (row-major) fp64 and are
 *    only read/written during the call.  Device buffers belong to the context.
 *  - Calls are synchronous: the context's HIP stream is drained before return.
 *  - One context per host thread, one GPU per context.  No callbacks.
 *  - Return codes: GPE_OK (0); GPE_NOT_PD (1) = Cholesky met a non-positive or
 *    NaN pivot, or a length scale is zero / NaN (the reference's covariance is NaN
 *    there) -- the host maps it to the reference's `return None`
 *    (_emulatoroptimise.py:374-376, :489-491); negative = error, text in
 *    gpe_last_error().
 *  - Hyperparameters are UNtransformed (delta, nu, sigma); transform /
 *    untransform x = 2 log(hp) stays on the host (_emulatorkernels.py:31-36).
 */
#ifndef GPEMU_H
#define GPEMU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_ABI_VERSION 10  /* 3: gpe_dist_objective gained want_grad / grad_out; 4: sensitivity;
                                5: gpe_noise_sample (noise_fit); 6: gpe_kernel_grad;
                                7: gpe_lhc_maximin; 8: gpe_dist_rank_bytes,
                                gpe_device_synchronize, gpe_build_id;
                                9: gpe_dist_local_rows takes the basis width q;
                                10: gpe_ozaki_stats (gpe_loo, gpe_posterior_pivchol,
                                gpe_posterior_imse, gpe_posterior_grad, gpe_posterior_mean, gpe_posterior_groups,
                                gpe_set_outputs, gpe_objective_multi, gpe_beta_multi, gpe_posterior_mean_multi, the gpe_hm_* set (with gpe_hm_add_multi, gpe_hm_outputs,
                                gpe_hm_member_outputs, gpe_hm_implausibility_mv, gpe_hm_cells, gpe_hm_cells_mv
                                and gpe_hm_sample) and the test
                                hooks gpe_test_oz_product, gpe_test_oz_planes and gpe_test_gemm_group were
                                added within 10: additions, nothing existing changed) */

enum gpe_status {
    GPE_OK = 0,
    GPE_NOT_PD = 1,
    GPE_ERR_ARG = -1,
    GPE_ERR_HIP = -2,
    GPE_ERR_ALLOC = -3,
    GPE_ERR_STATE = -4,
    GPE_ERR_UNSUPPORTED = -5
};

/* kernel: the nugget convention, _emulatorkernels.py:10 (kernel) and :83 (kernel_alt_nug),
 * OR-ed with a correlation family (an addition within ABI 10; the reference has only the
 * Gaussian one, which is family bits 0, so the codes 0 and 1 mean what they always did).
 * With s = sum_k ((x_k - x'_k) / delta_k)^2 and r = sqrt(s):
 *   Gaussian    rho = exp(-s)
 *   MATERN32    rho = (1 + sqrt(3) r) exp(-sqrt(3) r)
 *   MATERN52    rho = (1 + sqrt(5) r + (5/3) s) exp(-sqrt(5) r)
 * The off-diagonal is (1 - nu) rho (std) or rho (alt); the diagonal, the r / s2 rules and
 * the nugget and sigma derivatives are those of the Gaussian kernels with exp(-s) read as
 * rho.  Accepted by gpe_objective, gpe_factor (and through the resident factor by gpe_beta,
 * gpe_loo, gpe_solve, gpe_posterior, gpe_noise_sample, gpe_posterior_pivchol),
 * gpe_kernel_var, gpe_kernel_covar and gpe_kernel_grad_k.  A Matern objective takes
 * the one-launch paths at n <= 512 as a Gaussian one does (same limits, same pivot floor as
 * on the general path).  gpe_dist_objective answers GPE_ERR_UNSUPPORTED to a
 * Matern code; gpe_sense_pairs / gpe_gauss_transform are Gaussian closed forms.  Any other
 * bit, or both family bits, is GPE_ERR_ARG.
 * GPE_NOT_PD for a Matern code: besides a non-positive or NaN pivot, a pivot at or below
 * 4 n_pad eps times its diagonal entry of A (n_pad = n rounded up to 128), i.e. within the
 * factorisation's own backward error of zero: a matrix made singular by coincident points
 * without a nugget is refused whatever the rounding of its zero pivot.  The Gaussian codes keep
 * the plain rule, whose decisions are pinned to the reference's. */
enum gpe_kernel {
    GPE_KERNEL_STD = 0,
    GPE_KERNEL_ALT_NUG = 1,
    GPE_KERNEL_MATERN32 = 0x10,
    GPE_KERNEL_MATERN52 = 0x20
};
/* objective: _emulatoroptimise.py:412 (gp4ml) and :305 (mucm) */
enum gpe_variant { GPE_GP4ML = 0, GPE_MUCM = 1 };

/* Input dimensions d and columns q + 1 of [f H] (the reference's linear mean has
 * q = d + 1) take any value, as in the reference (_emulatorkernels.py:39-50): the
 * kernels for d <= 32 and q + 1 <= 33 keep coordinates and basis rows in registers,
 * beyond that they stage them through LDS in chunks of 32.  The two constants below
 * are only the sizes a context's small per-dimension / per-column buffers start at
 * (they grow with the data); they are no longer limits (ABI version 8 and later). */
#define GPE_MAX_DIMS 128
#define GPE_MAX_COLS 128

typedef struct gpe_ctx gpe_ctx;

int gpe_abi_version(void);
/* SHA-256 (hex) of the sources the library was built from (gp_emu_uqsa_amd/buildinfo.py). */
const char* gpe_build_id(void);
int gpe_device_count(void);
/* Wait for all work on GPU `device` (the timed-region bracket of bench.py). */
int gpe_device_synchronize(int32_t device);

/* Create a context on one GPU (device index as HIP sees it). NULL on failure;
 * the reason is then available from gpe_last_error(NULL). */
gpe_ctx* gpe_create(int32_t device);
void gpe_destroy(gpe_ctx* ctx);
const char* gpe_last_error(const gpe_ctx* ctx);

/* Training data: replaces Data.inputs/.outputs/.H/.r (_emulatorclasses.py:540-550,
 * :577-584).  X n x d (already active-column-selected and [0,1]-scaled, as
 * All_Data leaves it), f n, H n x q, r n or NULL (r = 0).  Copies to HBM. */
int gpe_set_data(gpe_ctx* ctx, int64_t n, int32_t d, int32_t q,
                 const double* X, const double* f, const double* H, const double* r);

/* Objective: replaces Optimize.loglikelihood_gp4ml (_emulatoroptimise.py:412-493)
 * and Optimize.loglikelihood_mucm (:305-378).
 * hp = untransformed [delta(d), nu (if fitted), sigma (gp4ml only)], n_hp its
 * length; the nugget is fitted iff n_hp == d+2 (gp4ml) / d+1 (mucm), exactly the
 * reference's `x.size` test (:463, :360).  nu_fixed is used otherwise.
 * Outputs: *llh_out = the reference's LLH (negative log marginal likelihood);
 * grad_out (n_hp, may be NULL when want_grad == 0) = its gradient w.r.t.
 * x = 2 log(hp), including the MUCM sigma-hat^2 scaling the reference applies;
 * *sigma2_out = sigma^2 (gp4ml) or the analytic sigma-hat^2 (mucm, :324-327).
 * want_grad == 0 (sigma_analytic_mucm, :382-408) runs K-build, Cholesky and a forward
 * substitution for L^-1 [f H] only: no triangular inverse and no A^-1. */
int gpe_objective(gpe_ctx* ctx, int32_t variant, int32_t kernel,
                  const double* hp, int32_t n_hp, double nu_fixed, int32_t want_grad,
                  double* llh_out, double* grad_out, double* sigma2_out);

/* Factor A = s2 * K.var(X_train, predict=True) + r_scale * diag(r) and keep the
 * Cholesky factor and its inverse resident for gpe_beta / gpe_posterior.
 * Replaces the factorisations inside Optimize.optimalbeta (:497-504) and the
 * three scipy.linalg.solve(A, .) LU solves of Posterior (_emulatorclasses.py:613,
 * :623, :628).  r_scale is 1/s2 after training's make_A(s2) and 1 after remake(). */
int gpe_factor(gpe_ctx* ctx, int32_t kernel, const double* delta, double nu,
               double s2, double r_scale);

/* GLS beta = Q^-1 H^T A^-1 f with the resident factor (optimalbeta, :497-504).  Needs
 * only L: L^-1 [f H] by forward substitution with the Cholesky's diagonal-tile inverses
 * (no n^3/3 triangular inverse; that runs on demand for the posterior-side entries). */
int gpe_beta(gpe_ctx* ctx, double* beta_out);

/* Leave-one-out cross-validation of the resident factor (an addition within ABI 10; the
 * reference has no such entry).  For every training point i, the posterior at x_i given the
 * other n - 1 points with the hyperparameters held fixed: what n calls of Posterior
 * (_emulatorclasses.py:607-631) give, each on the n - 1 other points (Dold.A the submatrix
 * of the resident A), with beta re-estimated on them by Optimize.optimalbeta
 * (_emulatoroptimise.py:497-504) and Dnew.A = K.var(x_i, predict=True).  In closed form,
 * with P = A^-1 - A^-1 H (H^T A^-1 H)^-1 H^T A^-1:
 *   mean_out[i] = f_i - (P f)_i / P_ii,   var_out[i] = sigma^2 (1 / P_ii - r_scale r_i)
 * (r_scale that of gpe_factor; the r term is zero without r).  One pass over L^-1 (run on
 * demand, as for gpe_solve) gives diag(A^-1) and A^-1 [f H] together; P_ii, the mean and the
 * variance are formed on the device.  Repeated calls on one factor return the same bits.
 * mean_out, var_out: n values; beta_out: q values (the GLS beta of all n points, as gpe_beta)
 * or NULL.  GPE_ERR_STATE without a resident factor, GPE_ERR_ARG if n < q + 2, GPE_NOT_PD if
 * H^T A^-1 H is not positive definite. */
int gpe_loo(gpe_ctx* ctx, double sigma, double* mean_out, double* var_out, double* beta_out);

/* Posterior at m points: replaces Posterior.make_covar/make_mean/make_var
 * (_emulatorclasses.py:607-631) with the resident factor.  Xs m x d, Hs m x q.
 * mean_out m; var_out m x m (row-major) when full_var != 0, else its diagonal
 * (m values); any m, in chunks of 16384 points (full: blocks of the m x m result
 * formed on the device and written to the host).  sigma is par.sigma.
 * precision 64: fp64 accuracy; for 4096 <= n_pad <= 32768 the dominant product
 * L^-1 K* (n^2 m flops) runs as exact int8 products of 53-bit operands (16 moduli).
 * precision 32 (diagonal only; SURVEY 8b/8d, BASELINE config C5): that product from
 * 24-bit operands (8 moduli; GPEMU_OZAKI=0 or n_pad outside that range: fp32 MFMA on
 * fp32 copies of L^-1 and K*); the mean and the q x q terms stay fp64. */
int gpe_posterior(gpe_ctx* ctx, int64_t m, const double* Xs, const double* Hs,
                  const double* beta, double sigma, int32_t full_var, int32_t precision,
                  double* mean_out, double* var_out);

/* Posterior mean and diagonal variance at m points with their gradients in the point (an
 * addition within ABI 10; the reference has no counterpart).  Coordinates are those of
 * gpe_posterior's Xs.  mean_out (m) and var_out (m) are bit for bit what
 * gpe_posterior(full_var = 0, precision = 64) returns for the same arguments; dmean_out
 * (m x d row-major) is d mean / d x_k and dvar_out (m x d, or NULL) d var / d x_k.
 * With s_i = sum_k ((x_k - x_ik) / delta_k)^2, K*_i = coff rho(s_i) (coff = 1 - nu std, 1
 * alt) and g the family's derivative factor (Gaussian exp(-s), MATERN32 (3/2) exp(-sqrt(3) r),
 * MATERN52 (5/6)(1 + sqrt(5) r) exp(-sqrt(5) r)):
 *   d K*_i / d x_k = -2 coff g(s_i) (x_k - x_ik) / delta_k^2
 *   d mean / d x_k = d_k h . beta + sum_i gamma_i d_k K*_i,    gamma = A^-1 (f - H beta)
 *   d var / d x_k  = sigma^2 (-2 sum_i u_i d_k K*_i + 2 tau . d_k h),
 *   tau = (H^T A^-1 H)^-1 (h - G^T K*),  u = A^-1 K* + G tau,  G = A^-1 H.
 * Nothing divides by r: a point on a training point is fine (MATERN32 is C^1).  Every basis
 * column depends on one input: dHs (m x q) is each column's derivative in its own input
 * hdim[j] (q values in [-1, d), -1 a constant column; columns may share an input), so
 * (d_k h)_j = dHs[., j] if hdim[j] = k, else 0.
 * Any m, in chunks of 8192 points through the diagonal posterior's two-slot pipeline; per
 * chunk one more triangular n^2 m product (U = L^-T V, fp64 MFMA; skipped with dvar_out NULL)
 * and one fused kernel (gpemu_postgrad.hpp).  Every family and nugget kind, with or without
 * r.  Fixed summation order, no floating-point atomics: repeated calls on one factor return
 * the same bits, and the resident factor stays usable.
 * GPE_ERR_STATE without a resident factor; GPE_ERR_ARG for m <= 0, a NULL among Xs, Hs, dHs,
 * hdim, beta, mean_out, var_out, dmean_out, or hdim[j] outside [-1, d). */
int gpe_posterior_grad(gpe_ctx* ctx, int64_t m, const double* Xs, const double* Hs,
                       const double* dHs, const int32_t* hdim, const double* beta, double sigma,
                       double* mean_out, double* var_out, double* dmean_out, double* dvar_out);

/* Posterior mean alone at m points (an addition within ABI 10; the reference has no entry
 * that skips the variance).  Xs, Hs, beta as for gpe_posterior; mean_out (m):
 *   mean_s = hs . beta + sum_i gamma_i K*_is,   gamma = A^-1 (f - H beta),
 * with gamma bit for bit the one gpe_posterior uses and every term gamma_i K*_is formed with
 * the arithmetic of gpe_posterior's K*; only the order of the sum over i differs, so the two
 * means agree to the rounding of an n-term sum.  One fused kernel (gpemu_postmean.hpp) reads
 * the training rows and sums on the fly: no n x m block is formed and no n^2 m product runs;
 * the work is n m (2 d + one exp) and the device workspace (2 d + n / 192 + 2) doubles per
 * point of a chunk.  Any m, in chunks of 65536 points (GPEMU_MEAN_CHUNK, a multiple of 128,
 * read when the context is created) through two pinned slots: the next chunk's upload is
 * queued before the host finishes the previous one.  The training rows are summed in segments
 * of 192 whose sums are added in index order whatever m and the chunk length are: the result
 * does not depend on the chunk length, repeated calls return the same bits, and there are no
 * floating-point atomics.  Every family and nugget kind, with or without r; the resident
 * factor and what other entries keep of it stay as they are.
 * GPE_ERR_STATE without a resident factor; GPE_ERR_ARG for m <= 0 or a NULL pointer;
 * GPE_NOT_PD if H^T A^-1 H is not positive definite, as gpe_posterior. */
int gpe_posterior_mean(gpe_ctx* ctx, int64_t m, const double* Xs, const double* Hs,
                       const double* beta, double* mean_out);

/* ---- Separable multi-output emulator (additions within ABI 10; MUCM's ProcBuildMultiOutputGPSep,
 * Conti & O'Hagan 2010): p outputs F (n x p) share one correlation matrix A = what
 * gpe_objective(GPE_MUCM, kernel, hp, nu_fixed) factors (s2 = 1, the same treatment of r), the
 * p x p between-output covariance Sigma is estimated in closed form as MUCM's sigma-hat^2 is.
 * With G = A^-1 H, Q = H^T G, P = A^-1 - G Q^-1 G^T, S = F^T P F, x = 2 log hp:
 *   B = Q^-1 G^T F (q x p, the GLS coefficients, one column per output),
 *   Sigma-hat = S / (n - q - 2),
 *   llh = 1/2 [(n - q) log|Sigma-hat| + p log|A| + p log|Q|],
 *   d llh / d x_k = 1/2 tr(M dA/dx_k),  M = p [A^-1 - W W^T],
 *   W = [sqrt((n - q) / p) P F C^-T, G Kq^-T],  S = C C^T, Q = Kq Kq^T.
 * At p = 1: llh and Sigma-hat are gpe_objective's llh_out and sigma2_out, and the gradient is its
 * MUCM grad_out divided by sigma2_out (the plain derivative of llh, without the reference's
 * sigma-hat^2 scaling).  Posterior at x with the factor gpe_factor(kernel, delta, nu, 1, r_scale):
 * mean (p values) = h(x)^T B + K*(x)^T Gamma, Gamma = A^-1 (F - H B); the covariance of output a
 * at x and output b at x' is Sigma-hat_ab c(x, x') with c what gpe_posterior(sigma = 1) returns.
 * The existing entries are unaffected by resident outputs (same bits with and without). */

/* The outputs: F n x p row-major for the resident data of gpe_set_data (whose own f stays as
 * it is), 1 <= p <= 64.  Dropped by the next gpe_set_data.  GPE_ERR_STATE without data;
 * GPE_ERR_ARG for a bad p, a NULL pointer or n < p + q + 3. */
int gpe_set_outputs(gpe_ctx* ctx, int32_t p, const double* F);

/* The objective above.  hp, n_hp and nu_fixed are read as gpe_objective reads them for GPE_MUCM
 * (hp = [delta (d), nu if fitted]); every kernel code gpe_objective accepts.  Runs
 * gpe_objective's general path (the K-build, the Cholesky with its int8 products, the skinny
 * solves, the Gram, the contraction) at every n on the p + q columns of [F H]; want_grad == 0:
 * no triangular inverse and no A^-1.  *llh_out; grad_out (n_hp, may be NULL when want_grad == 0);
 * Sigma_out p x p row-major; B_out q x p row-major or NULL.
 * GPE_NOT_PD as gpe_objective (failed pivot, bad length scale, H^T A^-1 H), and with
 * "F^T P F not positive definite" when S is not: outputs linearly dependent given H.  For Q and
 * S a pivot at or below 64 (p + q) eps times its column's diagonal entry of the Gram matrix of
 * L^-1 [F H] counts as not positive: a repeated basis column or a duplicated output leaves a
 * rounding residue of either sign where the exact pivot is zero.
 * GPE_ERR_STATE without outputs. */
int gpe_objective_multi(gpe_ctx* ctx, int32_t kernel, const double* hp, int32_t n_hp, double nu_fixed,
                        int32_t want_grad, double* llh_out, double* grad_out, double* Sigma_out,
                        double* B_out);

/* B (q x p row-major) for the resident factor, as gpe_beta gives beta for f. */
int gpe_beta_multi(gpe_ctx* ctx, double* B_out);

/* The posterior means of the p outputs at m points: mean_out m x p row-major,
 *   mean_sc = hs . B[:, c] + sum_i Gamma_ic K*_is,   Gamma = A^-1 (F - H B)
 * from the resident factor (B q x p row-major, Xs and Hs as for gpe_posterior_mean).  One fused
 * kernel (gpemu_postmean_multi.hpp) forms every K*_is once, with gpe_posterior_mean's arithmetic,
 * and uses it for all p outputs on the fp64 matrix cores; nothing of size n x m is written.
 * Any m; chunks (GPEMU_MEAN_CHUNK), the two pinned slots and the summation contract are
 * gpe_posterior_mean's: segments of 192 training rows added in index order, a result that does not
 * depend on the chunk length, the same bits on every call, no floating-point atomics.  The device
 * workspace is (2 d + (n / 192 + 2) p) doubles per point of a chunk.
 * GPE_ERR_STATE without a resident factor or without outputs; GPE_ERR_ARG for m <= 0 or a NULL
 * pointer. */
int gpe_posterior_mean_multi(gpe_ctx* ctx, int64_t m, const double* Xs, const double* Hs,
                             const double* B, double* mean_out);

/* Posterior covariance inside groups of G consecutive points (an addition within ABI 10): the
 * block diagonal of the m x m covariance in blocks of G, which the m^2 entries of full_var = 1
 * cannot give at the 10^5 .. 10^6 points of a Sobol' design.  The m points form m / G groups;
 * mean_out (m); cov_out (m / G) x G x G row-major, block g entry (a, b) = the posterior
 * covariance of points g G + a and g G + b with gpe_posterior(full_var = 1, precision = 64)'s
 * conventions:
 *   a == b   s2 (cdiag - |v_a|^2 + |t_a|^2)
 *   a != b   s2 (coff rho(s_ab) - v_a . v_b + t_a . t_b),   v = L^-1 K*, t = T Kq^-T
 * "diagonal" by index, never by coordinates: two different points of a group with equal
 * coordinates get the off-diagonal form.  The lower triangle is formed and mirrored, so every
 * block is exactly symmetric.  fp64 accuracy only (V from the int8 product where gpe_posterior
 * would take it there, from the fp64 GEMM otherwise); every family and nugget kind, with or
 * without r.  Any m: chunks of floor(8192 / G) G points (a group never straddles two) go
 * through the diagonal pipeline's two slots, the host part of one chunk beside the device work
 * of the next.  Per chunk two kernels (gpemu_postgroup.hpp) read V once in place of the
 * column norms: the G x G Grams on the fp64 matrix cores, then their finish with rho from the
 * scaled points.  Every Gram sum runs over the training rows in segments of 1024 added in
 * index order whatever m, G and the group's place are: a group's block does not depend on the
 * other groups of the call, repeated calls return the same bits, there are no floating-point
 * atomics and no waits between workgroups.  The resident factor and what other entries keep
 * of it stay as they are.
 * GPE_ERR_STATE without a resident factor; GPE_ERR_ARG for m <= 0, G outside [1, 64], m not a
 * multiple of G or a NULL pointer; GPE_NOT_PD as gpe_posterior. */
int gpe_posterior_groups(gpe_ctx* ctx, int64_t m, int32_t G, const double* Xs, const double* Hs,
                         const double* beta, double sigma, double* mean_out, double* cov_out);

/* ---- History matching over a resident set of emulators (additions within ABI 10; the
 * reference forms one Posterior per emulator and grid cell, history_match.py:91-121).  A wave
 * has p emulators of a few hundred design points each and rules out input space at 10^6 and
 * more candidates.  A set keeps p emulators on one GPU together; per emulator one fused kernel
 * (gpemu_hm.hpp) goes from the candidates to I^2 without K* or L^-1 K* in memory (L^-1 of
 * n <= 512 rows is at most 1 MB and stays in L2), and one selection kernel follows.  One set
 * per host thread; its calls are synchronous on a stream of its own. */
typedef struct gpe_hm gpe_hm;

/* A set on one GPU.  NULL on failure; the reason is then in gpe_hm_last_error(NULL).
 * GPEMU_HM_CHUNK (read here; default 65536, rounded down to a multiple of 64, at least 64) is
 * the number of candidates per chunk. */
gpe_hm* gpe_hm_create(int32_t device);
void gpe_hm_destroy(gpe_hm* set);
const char* gpe_hm_last_error(const gpe_hm* set);

/* Snapshot ctx's resident factor (gpe_factor) as the next emulator of the set; returns its
 * number (>= 0), or a negative status.  The triangular inverse runs on demand, as for
 * gpe_solve.  Copied into buffers the set owns: the scaled training rows, 1 / delta, L^-1 and
 * [gamma, G] = A^-1 [f - H beta, H] in MFMA operand order (lower 16 x 16 blocks only), Kq^-1
 * with Kq Kq^T = H^T A^-1 H, beta, sigma^2 and the kernel's family, coff and cdiag: exactly what
 * gpe_posterior(beta, sigma) would use.  The copies are ordered behind the context's stream,
 * and the context's stream behind them, by events; the context keeps its factor and everything
 * other entries keep of it, and is free for the next emulator on return.
 * d and q are those of ctx's data.  active[d]: the columns of the D-wide candidate rows this
 * emulator reads, in the order of its inputs.  Basis column j of a candidate is the constant
 * hval[j] when hdim[j] == -1, else the value of the emulator's input hdim[j] (0 <= hdim[j] < d):
 * the reference's default forms.
 * Limits: n <= 512, d <= 32, q <= 16, 32 emulators per set; beyond, GPE_ERR_UNSUPPORTED and the
 * set is unchanged.  GPE_ERR_STATE without a resident factor; GPE_ERR_ARG for a NULL pointer, a
 * d or q other than the context's, a negative active index, hdim[j] outside [-1, d) or a
 * context on another device; GPE_NOT_PD if H^T A^-1 H is not positive definite. */
int gpe_hm_add(gpe_hm* set, gpe_ctx* ctx, int32_t d, const int32_t* active, int32_t q,
               const int32_t* hdim, const double* hval, const double* beta, double sigma);
int gpe_hm_count(const gpe_hm* set);

/* Implausibilities of m candidates.  Xs m x D row-major in the scaled coordinates
 * gpe_posterior takes, uploaded once per chunk for all emulators; z and var_extra p values
 * (p = gpe_hm_count).  For emulator o and candidate s, with K* and h of the candidate,
 *   mean = h . beta + sum_i gamma_i K*_i,
 *   var  = sigma^2 (cdiag - |L^-1 K*|^2 + |(h - G^T K*) Kq^-T|^2)
 * (gpe_posterior(full_var = 0, precision = 64)'s formulas) and
 *   I^2 = (mean - z_o)^2 / (var + var_extra_o),
 * IEEE arithmetic with no clamping.  imax_out (m x maxno): per candidate the maxno largest
 * sqrt(I^2) over the emulators in ascending order, a NaN counted above every number (numpy's
 * sort order); 1 <= maxno <= p.  mean_out and var_out (p x m each, row o emulator o; both or
 * neither): the parts.
 * Any m: chunks of GPEMU_HM_CHUNK candidates through two pinned slots, the next chunk's work
 * queued before the host copies the previous one's results.  The sums over the training rows
 * run in an order that depends on n alone and there are no floating-point atomics: the result
 * of a candidate does not depend on m, on the chunk length or on the other candidates, and
 * repeated calls return the same bits.
 * GPE_ERR_STATE for an empty set; GPE_ERR_ARG for m <= 0, a NULL among Xs, z, var_extra and
 * imax_out, one of mean_out / var_out without the other, D smaller than an emulator's largest
 * active index + 1, or maxno outside [1, p]. */
int gpe_hm_implausibility(gpe_hm* set, int64_t m, int32_t D, const double* Xs, const double* z,
                          const double* var_extra, int32_t maxno, double* imax_out,
                          double* mean_out, double* var_out);

/* A member of p outputs: the separable multi-output emulator (gpe_set_outputs) as one member,
 * with one copy of L^-1 and one pass over K* and L^-1 K* for all p outputs.
 * ctx: data, outputs (gpe_set_outputs, p of them) and the factor gpe_factor(kernel, delta, nu, 1,
 * r_scale) resident.  B q x p row-major (gpe_beta_multi's), Sigma p x p row-major (symmetric).
 * The member contributes p outputs to the set, in order; returns the member's number.  It
 * snapshots what gpe_hm_add snapshots, with [Gamma (p columns), G (q columns)],
 * Gamma = A^-1 (F - H B) by gpe_posterior_mean_multi's route, in place of [gamma, G], and B,
 * Sigma and p besides; the context keeps its factor, its outputs and every bit other entries
 * return.  active, hdim, hval as gpe_hm_add.
 * In gpe_hm_implausibility "p" is then gpe_hm_outputs: z and var_extra have that many values,
 * maxno lies in [1, outputs], mean_out / var_out have one row per output, and output a of this
 * member has mean mu_a = h . B[:, a] + sum_i Gamma_ia K*_i and variance Sigma_aa c, with
 *   c = cdiag - |L^-1 K*|^2 + |(h - G^T K*) Kq^-T|^2   (gpe_posterior's variance at sigma = 1).
 * gpe_hm_count still counts members; a set of gpe_hm_add members behaves as before.
 * Limits: n <= 512, d <= 32, q <= 16, 1 <= p, p + q <= 32, and 32 outputs per set in all (a
 * gpe_hm_add member counts 1); beyond, GPE_ERR_UNSUPPORTED and the set is unchanged.
 * GPE_ERR_STATE without a resident factor or without outputs; GPE_ERR_ARG for a NULL pointer, p
 * other than the context's, a d or q other than the context's, a negative active index, hdim[j]
 * outside [-1, d) or a context on another device; GPE_NOT_PD as gpe_hm_add. */
int gpe_hm_add_multi(gpe_hm* set, gpe_ctx* ctx, int32_t d, const int32_t* active, int32_t q,
                     const int32_t* hdim, const double* hval, int32_t p, const double* B,
                     const double* Sigma);
int gpe_hm_outputs(const gpe_hm* set);      /* sum of the members' outputs (a gpe_hm_add member: 1) */
int gpe_hm_member_outputs(const gpe_hm* set, int32_t member);

/* Joint (multivariate) implausibility of one multi-output member (Vernon, Goldstein & Bower
 * 2010): z (p), V (p x p row-major, symmetric positive definite: observation error + model
 * discrepancy),
 *   I^2 = (z - mu)^T (c Sigma + V)^-1 (z - mu)
 * per candidate, with the between-output covariance Sigma of gpe_hm_add_multi.  W with
 * W^T V W = I and W^T Sigma W = Lambda is found once per call on the host (a Cholesky of V and a
 * Jacobi eigendecomposition; exact algebra), so that per candidate
 *   I^2 = sum_j (W^T (mu - z))_j^2 / (c lambda_j + 1).
 * i2_out (m) = I^2, no square root, no clamping; mean_out (p x m, row a output a) and c_out (m):
 * both or neither.  Chunks, order of the sums and repeatability as gpe_hm_implausibility.
 * GPE_ERR_ARG for a member that is not multi-output, m <= 0, a NULL among Xs, z, V and i2_out,
 * one of mean_out / c_out without the other, or D smaller than the member's largest active
 * index + 1; GPE_NOT_PD (with text in gpe_hm_last_error) when V is not positive definite. */
int gpe_hm_implausibility_mv(gpe_hm* set, int32_t member, int64_t m, int32_t D, const double* Xs,
                             const double* z, const double* V, double* i2_out, double* mean_out,
                             double* c_out);

/* ---- Candidates made and reduced on the device (additions within ABI 10; kernels in
 * gpemu_hm_cand.hpp).  The entries above take every candidate row from the host and return a
 * value per candidate; these write the chunk's rows into the same device buffer by a kernel,
 * run the same post kernels on it, and reduce I^2 on the device, so that the arguments go up
 * and only the answer comes back.  A candidate's I^2 has the bits gpe_hm_implausibility gives
 * for the same row.
 *
 * Maps over a mesh of two inputs.  Candidate s = (i g2 + j) ns + t is the row with x1[i] in
 * column ca, x2[j] in column cb and others[t, :] (ns x (D - 2) row-major; NULL iff D == 2) in
 * the remaining columns in ascending order; the values are copied.  use (one flag per output, or
 * NULL: all on): an output switched off has no kernel launched and enters the selection with
 * I^2 = 0 exactly; a multi-output member has one flag, its first output's.  Level l (0-based)
 * of a candidate is the (l + 1)-th largest sqrt(I^2) over the outputs, a NaN above every number.
 * imp_out[l, c] (maxno x g1 g2, cell c = i g2 + j): the minimum of level l over the cell's ns
 * samples, NaN if any of them is NaN (numpy's min); below_out[l, c]: the samples with level
 * l < cm (a NaN is not below).  The candidate index is cut into chunks of GPEMU_HM_CHUNK; a
 * cell may lie across any number of them.  Minima and integer counts do not depend on the order
 * of combination and the launches are ordered on the set's stream: no atomics, the chunk length
 * does not show, repeated calls return the same bits.
 * GPE_ERR_STATE for an empty set; GPE_ERR_ARG, before any device work, for g1, g2 or ns < 1,
 * ca == cb or either outside [0, D), D < 2, D not above every member's largest active index,
 * others NULL with D > 2, a NULL among x1, x2, z, var_extra, imp_out and below_out, maxno
 * outside [1, outputs], or g1 g2 ns >= 2^40. */
int gpe_hm_cells(gpe_hm* set, int32_t D, int32_t ca, int32_t cb, int32_t g1, const double* x1,
                 int32_t g2, const double* x2, int64_t ns, const double* others,
                 const int32_t* use, const double* z, const double* var_extra, int32_t maxno,
                 double cm, double* imp_out, int64_t* below_out);

/* The same maps for the joint measure of one multi-output member: one level, I = sqrt(I^2) with
 * I^2 as gpe_hm_implausibility_mv forms it; imp_out and below_out have g1 g2 entries.  Errors as
 * gpe_hm_cells and gpe_hm_implausibility_mv (GPE_NOT_PD for V). */
int gpe_hm_cells_mv(gpe_hm* set, int32_t member, int32_t D, int32_t ca, int32_t cb, int32_t g1,
                    const double* x1, int32_t g2, const double* x2, int64_t ns,
                    const double* others, const double* z, const double* V, double cm,
                    double* imp_out, int64_t* below_out);

/* Rejection sampling from numpy's PCG64 stream.  state and inc are the generator's 128-bit state
 * and increment (numpy's bit_generator.state), high word first.  Candidates number
 * c in [first, first + m) are tried: coordinate k of candidate c comes from element e = c D + k,
 * the output after e + 1 steps from state (state <- state * 0x2360ED051FC65DA44385DF649FCCF645
 * + inc mod 2^128; output rotr64(hi ^ lo, hi >> 58) of the new state; u = (output >> 11) 2^-53),
 * x_k = lo_k + u (hi_k - lo_k) with the difference, the product and the sum each rounded: the
 * bits of lo + default_rng(seed).random((., D)) * (hi - lo).  A thread reaches its row through a
 * host-made table of jumps, one 128-bit product per 8 bits of the row's number in the chunk.
 * A candidate is accepted when the maxno-th largest sqrt(I^2) over the outputs is < cm (a NaN
 * is not).  The accepted rows and their candidate numbers go to pts_out (cap x D) and idx_out
 * (cap) in stream order, by a scan; storing stops at cap rows and *accepted_out counts all
 * accepted.  Nothing is uploaded but the arguments, and only accepted rows come back.
 * GPE_ERR_STATE for an empty set; GPE_ERR_ARG for m < 1, first < 0, (first + m) D >= 2^63,
 * cap < 0, a NULL among lo, hi, state, inc, z, var_extra and accepted_out (and pts_out,
 * idx_out when cap > 0), D not above every member's largest active index, or maxno outside
 * [1, outputs]. */
int gpe_hm_sample(gpe_hm* set, int32_t D, const double* lo, const double* hi,
                  const uint64_t state[2], const uint64_t inc[2], int64_t first, int64_t m,
                  const double* z, const double* var_extra, int32_t maxno, double cm, int64_t cap,
                  double* pts_out, int64_t* idx_out, int64_t* accepted_out);

/* ---- Sensitivity / UQ building blocks, resident factor --------
 * Replace the O(n^2) parts of sensitivity/_sensitivityclasses.py (case2): the
 * solves with emul.training.A (:40-44, :187-189, :436-441, :451-454) and the n x n
 * pair matrices Rtt (:90-102) and Pw (:599-626), which are never formed here.
 * Host arrays are row-major; x below is the resident raw training inputs (n x d). */

/* X = A^-1 B  (B, X: n x ncols). */
int gpe_solve(gpe_ctx* ctx, int32_t ncols, const double* B, double* X);

/* J Gaussian pair kernels K_j(k,l) = u[j,k] u[j,l] exp(-sum_i w[j,i] (x_ki - x_li)^2)
 * (w: J x d, u: J x n).  trace_out[j] = sum_kl (A^-1)_kl K_j(k,l) = tr(A^-1 K_j);
 * quad_out[j] = Z^T K_j Z (p x p; Z: n x p).  Any p (Z columns in chunks of 32, one
 * launch each) and any d the context holds (d > 32: coordinates staged through LDS in
 * chunks of 32 dimensions), as the reference's Pw / Rtt loops (:90-102, :599-626). */
int gpe_sense_pairs(gpe_ctx* ctx, int32_t J, const double* w, const double* u, int32_t p,
                    const double* Z, double* trace_out, double* quad_out);

/* out[t] = sum_k a[k] exp(-sum_s c[s] (Y[t,s] - x[k, dims[s]])^2), t < m, ns <= 4
 * (Y: m x ns): the Tw . e sums of main effects (:277-285, ns = 1) and interaction
 * effects (:353-373, ns = 2).  Needs set_data only. */
int gpe_gauss_transform(gpe_ctx* ctx, int64_t m, int32_t ns, const int32_t* dims,
                        const double* c, const double* Y, const double* a, double* out);

/* K.var(X, predict) materialised (m x m, symmetric): _emulatorkernels.py:39-50 /
 * :112-123, plus make_A's r/s2 diagonal (r_scale * r, r may be NULL). */
int gpe_kernel_var(gpe_ctx* ctx, int32_t kernel, const double* delta, int32_t d,
                   double nu, int32_t predict, int64_t m, const double* X,
                   const double* r, double r_scale, double* A_out);

/* The reference's dense derivative matrices, m x m row-major, zero diagonal:
 *   G(k,l) = pre * ((col_k - col_l) * col_scale)^2 * exp(-sum_i ((X_ki - X_li)/delta_i)^2)
 * (col NULL: the squared factor is 1).  kernel.grad_delta_A(X[:,i], i, s2)
 * (_emulatorkernels.py:53-63, alt :126-136): col = X[:,i], col_scale = 1/delta_i,
 * pre = s2 (1 - nu) (alt: s2), delta / X those of the preceding var() (its exp_save).
 * kernel.grad_nugget_A (std :66-71): col NULL, pre = -nu s2 / 2.  (The alt-nugget
 * form, s2 nu^2 I, is diagonal and built by the host.) */
int gpe_kernel_grad(gpe_ctx* ctx, const double* delta, int32_t d, int64_t m, const double* X,
                    const double* col, double col_scale, double pre, double* G_out);

/* gpe_kernel_grad for any correlation family (an addition within ABI 10); only the family
 * bits of `kernel` are read.  With col:
 *   G(k,l) = pre * ((col_k - col_l) * col_scale)^2 * g(s_kl),
 * g the family's derivative factor, d rho / d(2 log delta_i) = g(s) ((x_i - x'_i) / delta_i)^2:
 * exp(-s) (Gaussian), (3/2) exp(-sqrt(3) r) (MATERN32), (5/6)(1 + sqrt(5) r) exp(-sqrt(5) r)
 * (MATERN52).  Without col: G(k,l) = pre * rho(s_kl) (grad_nugget_A).  Zero diagonal.
 * Family bits 0 return the bits gpe_kernel_grad returns for the same arguments. */
int gpe_kernel_grad_k(gpe_ctx* ctx, int32_t kernel, const double* delta, int32_t d, int64_t m,
                      const double* X, const double* col, double col_scale, double pre,
                      double* G_out);

/* The oLHC generator's selection statistic (design_inputs.py:54-64): for each of the N
 * candidate designs (designs: N x n x dim row-major, design k at k*n*dim),
 * idx_out[k] = np.argmin(scipy pdist(xt, 'sqeuclidean')) with xt = [design k; fextra]
 * (fextra: ne x dim row-major, ne may be 0 / NULL): the condensed index of the closest
 * pair, first occurrence on ties, NaN distances count as the minimum.  Distances are
 * summed over dimensions in order without FMA, bit-identical to pdist's.  The caller
 * keeps the reference's rule (largest index wins, :62-67).  n + ne >= 2. */
int gpe_lhc_maximin(gpe_ctx* ctx, int32_t N, int64_t n, int32_t dim, const double* designs,
                    int64_t ne, const double* fextra, int64_t* idx_out);

/* K.covar(XT, XV) -> n x m row-major: _emulatorkernels.py:75-79 / :148-152. */
int gpe_kernel_covar(gpe_ctx* ctx, int32_t kernel, const double* delta, int32_t d,
                     double nu, int64_t n, const double* XT, int64_t m,
                     const double* XV, double* C_out);

/* Cholesky factor, inverse factor and inverse of an arbitrary SPD matrix
 * (row-major m x m, lower triangle read).  Replaces the np.linalg.cholesky of the
 * posterior covariance in posterior_sample (emulatorfunctions.py:283) and serves
 * as the unit-test entry of the blocked factorisation.  Any output may be NULL.
 * L_out / Linv_out are lower-triangular with zero upper part. */
int gpe_cholesky(gpe_ctx* ctx, int64_t m, const double* A, double* L_out,
                 double* Linv_out, double* Ainv_out, double* logdet_out);

/* Test hook for the grouped MFMA GEMM building block on one problem:
 * C = alpha * opA x opB + beta * C with opA M x K, opB K x N (row-major host
 * arrays A (M x K), B (K x N), C (M x N)); trans_a / trans_b choose the device
 * storage orientation exercised (0: M-/N-contiguous, 1: K-contiguous).
 * M, N multiples of 128, K multiple of 16. */
int gpe_test_gemm(gpe_ctx* ctx, int32_t trans_a, int32_t trans_b, int64_t M, int64_t N,
                  int64_t K, const double* A, const double* B, double* C,
                  double alpha, double beta);

/* Test hook for one exact int8 product (gpemu_ozaki.hpp), an addition within ABI 10; the
 * reference has no counterpart.  C = alpha op(A) op(B)^T (+ C with acc) through the
 * production sequence -- exponents, split into int8 planes, k_oz_gemm, k_oz_crt -- on device
 * buffers of its own, freed on exit; the context's resident factor and cached plans are not
 * touched.  The constants come from oz_consts(nmod, K); the operand conversion, the tile list
 * with its k ranges and the two product launches are calls of the launch layer every
 * production product goes through (oz_operand / oz_operand_packed, OzShape, oz_product_launch).
 *
 * An operand is a window of a host fp64 array `src` of `len` doubles, copied to the device
 * as it is: op(r, k) = src[offset + k + r ld] (trans 0) or src[offset + r + k ld] (trans 1)
 * for r < R, k < Kv, zero outside, and zero where k < r (mask 1) or k > r (mask 2).  Rows are
 * padded to a multiple of 256 (Pa, Pb) and k to K.
 *
 * Rectangular form (packed 0): a and b (b NULL: B is A, one set of planes and one exponent
 * array) and the product's parameters, passed on as they are to OzGemm / OzCrt: K (a
 * multiple of 64 in [64, 2^17 - 128], >= both Kv), kbeg 0 to 3, kend 0 / 1, kdiv >= 1,
 * ti0 (first tile row: the product covers tile rows [ti0, Pa / 256)), tri (only tiles tj <= ti; with
 * Pb < Pa, which needs ti0 = 0, the triangle capped at B's Pb / 256 tile columns: the nested
 * split Cholesky's trapezoid), lower128, alpha, acc, nmod in [6, 16].  C is column-major, c_len
 * doubles, read first and written back whole: entry (i, j) of the product, i < rows <= Pa,
 * j < cols <= Pb, goes to C[i - 256 ti0 + j ldc]; nothing else changes.
 * Packed form (packed 1; the A^-1 = X^T X of the objective's gradient): a describes X, R x R
 * column-major lower-triangular (R a multiple of 128, trans / Kv / mask ignored, entries above
 * the diagonal never read), through k_oz_colexp and k_oz_split; K, kbeg, kend, tri, lower128,
 * ti0, rows and cols are fixed to the production call's (kbeg 1, tri, lower128, rows = cols = R)
 * and only alpha, acc, nmod, ldc and res_mod are read from p.
 *
 * Optional outputs (NULL: skipped): exa_out (Pa ints) / exb_out (Pb ints; with B = A a copy
 * of exa) the row exponents; res_out the centred residues of modulus number res_mod as
 * int8, (Pa - 256 ti0) x Pb row-major in the product's own (row, column) order (tiles the
 * product does not cover: 0).
 * GPE_ERR_ARG for anything outside the above (K not a multiple of 64 included: the kernel
 * would drop the remainder silently). */
typedef struct gpe_oz_operand {
    const double* src;
    int64_t len, offset, ld;
    int32_t trans, R, Kv, mask;
} gpe_oz_operand;
typedef struct gpe_oz_params {
    int32_t packed, K, kbeg, kend, kdiv, ti0, tri, lower128, acc, nmod, rows, cols, res_mod;
    int64_t ldc, c_len;
    double alpha;
} gpe_oz_params;
int gpe_test_oz_product(gpe_ctx* ctx, const gpe_oz_operand* a, const gpe_oz_operand* b,
                        const gpe_oz_params* p, double* C, int32_t* exa_out, int32_t* exb_out,
                        int8_t* res_out);

/* The same product with a 15-moduli certificate (gpemu_ozaki.hpp: OzCert), an addition within
 * ABI 10: the operand conversions also form the row sums, k_oz_cert decides, and k_oz_gemm and
 * k_oz_crt_cert run as the objective's products do.  nmod must be 16.  nmod_used_out (required):
 * 15 where the certificate held, 16 where it was refused. */
int gpe_test_oz_product_cert(gpe_ctx* ctx, const gpe_oz_operand* a, const gpe_oz_operand* b,
                             const gpe_oz_params* p, double* C, int32_t* exa_out, int32_t* exb_out,
                             int8_t* res_out, int32_t* nmod_used_out);

/* Test hook for one operand's conversion (gpemu_ozaki.hpp), an addition within ABI 10; the
 * reference has no counterpart.  The operand a (as gpe_test_oz_product's: a window of a host
 * array, R rows padded to P, a multiple of 256) goes through the production oz_operand
 * (packed 0: k_oz_rowexp<trans> and k_oz_split_rect<trans>, k padded to K, a multiple of 64 in
 * [64, 2^17 - 128], >= Kv) or oz_operand_packed (packed 1: X is R x R lower-triangular, R a
 * multiple of 128, ld and offset even, K ignored and taken as P; k_oz_colexp and k_oz_split)
 * on device buffers of its own, freed on exit, with the constants of oz_consts(nmod, K).
 * Outputs: ex_out, the P row (packed: column) exponents, and planes_out, the int8 planes of
 * all nmod moduli, [modulus][row][k]: nmod x P x K bytes; packed: nmod x P x P bytes, row j the
 * column j of X over k = the rows of X, the bytes with k < 256 (j / 256) -- above column j's
 * panel, which the planes do not hold -- 0.  The planes are filled with 0x55 before the
 * conversion: a byte the kernels fail to write shows. */
int gpe_test_oz_planes(gpe_ctx* ctx, const gpe_oz_operand* a, int32_t packed, int32_t K,
                       int32_t nmod, int32_t* ex_out, int8_t* planes_out);

/* Test hook for one launch of the plain (non-fused) grouped fp64 GEMM k_gemm on a group of
 * problems, an addition within ABI 10; the reference has no counterpart.  Descriptors come
 * from mkprob and push_prob, split K from split_k, the tile list from order_tiles
 * (csrc/gpemu_gemm_sched.hpp, through add_launch on a plan of the hook's own) and the launch
 * from launch_gemm_range, so launch_k_gemm: the routines every production GEMM, single-GPU or
 * row-block, goes through.  Device memory is the hook's own and freed on every way out; the context's
 * resident factor and cached plans are not touched.
 *
 * Buffers: nbuf host fp64 arrays bufs[i] of lens[i] doubles, copied to the device as they are
 * and copied back whole afterwards.  Problem p names its operands by buffer index, element
 * offset and leading dimension; operands may share a buffer, and C may live in the buffer of
 * A and B (that the tiles read and the tiles written are disjoint is the caller's business).
 * With kind = 0..3 (GemmKind: 0 <A M-contiguous, B N-contiguous>, 1 <A K-contiguous>,
 * 2 <both K-contiguous>, 3 <B K-contiguous>), over 128 x 128 tiles (ti, tj), ti < mt, tj < nt
 * (tj <= ti only under GPE_G_CLOWER):
 *   opA(m, k) = A[k + m lda] (K-contiguous) or A[m + k lda];  opB(k, n) likewise with ldb;
 *   C[m + n ldc] = alpha sum_{kbeg <= k < kend} opA(m, k) opB(k, n) + beta C[m + n ldc],
 *   kbeg = 128 ti under GPE_G_KBEG_TI (else 0),
 *   kend = min(K, 128 (ti kti_mul + kti_off + 1)) under GPE_G_KEND_TI (else K);
 * an empty range leaves C = beta C.  With beta = 0, C is not read.
 *
 * launch: kind; split (1: split_k on the group, with scratch and counters of the hook's own,
 * the counters zeroed once at allocation); listed (1: the tile list of order_tiles where
 * add_launch finds the group listable; 0: the implicit order); reps >= 1 identical launches
 * back to back on the context's stream, C's buffers restored from the inputs (on the device)
 * before every launch after the first.
 *
 * Outputs: ksplit_out[nprob] the split each problem got (1: none); info_out[0] 1 if the launch
 * had a tile list, info_out[1] 1 if the CDEF instance ran, info_out[2] the workgroups of one
 * launch; tiles_out (tiles_cap entries, may be NULL with tiles_cap 0) the tile list, codes
 * p << 24 | ti << 12 | tj, when there is one.
 *
 * GPE_ERR_ARG, with text and nothing launched, for: a flag other than the three above (the
 * fused Cholesky's in-launch hand-offs are out of reach); K not a positive multiple of 16;
 * alpha == 0 or not finite (the kernel forms beta / alpha); an odd or negative offset or an
 * odd leading dimension (16-byte loads and stores); ldc > 2^21 (the kernel's other path for
 * C, not reached here); mt or nt outside [1, 4096], more than 65536 tiles, 1024 problems or
 * 64 buffers; a buffer index that names no buffer;
 * negative kti_mul / kti_off; a tile whose operand window over its own K range, or whose C
 * window, leaves its buffer; listed with 256 or more problems; a tile list that does not fit
 * tiles_cap; kind, split, listed or reps (1..16) out of range. */
enum { GPE_G_CLOWER = 1, GPE_G_KBEG_TI = 2, GPE_G_KEND_TI = 4 };
typedef struct gpe_gemm_group_prob {
    int32_t a_buf, b_buf, c_buf;
    int32_t mt, nt, K, flags, kti_mul, kti_off;
    int64_t a_off, lda, b_off, ldb, c_off, ldc;
    double alpha, beta;
} gpe_gemm_group_prob;
typedef struct gpe_gemm_group_launch {
    int32_t kind, split, listed, reps;
} gpe_gemm_group_launch;
int gpe_test_gemm_group(gpe_ctx* ctx, int32_t nbuf, double* const* bufs, const int64_t* lens,
                        int32_t nprob, const gpe_gemm_group_prob* probs,
                        const gpe_gemm_group_launch* launch, int32_t* ksplit_out,
                        int32_t* info_out, uint32_t* tiles_out, int64_t tiles_cap);

/* Benchmark hook: time `reps` launches of the grouped GEMM on device-resident
 * random operands: C (mt*128 x nt*128, lower tiles only if lower) += -A B^T-style
 * update with K, in storage orientation (trans_a, trans_b).  Returns average
 * ms per launch in *ms_out.  Uses its own device buffers. */
int gpe_bench_gemm(gpe_ctx* ctx, int32_t trans_a, int32_t trans_b, int32_t mt, int32_t nt,
                   int32_t K, int32_t lower, double beta, int32_t reps, double* ms_out);

/* noise_fit's noise-estimation step (noise_fit/noise_fit.py:130-139, :142-150):
 * the posterior at Xs (m x d, Hs m x q; full m x m covariance V, built on the
 * device with Dnew's own r/s2 diagonal: r_new (m, or NULL) times r_scale, as in
 * Dnew.make_A(s2) after Dnew.set_r, _emulatorclasses.py:572-575), L = chol(V),
 * and for the s draws u_j = U[j, :] (U row-major s x m: the reference's successive
 * np.random.randn(m) calls) z_out[i] = sum_j 0.5 (t_i - mean_i - (L u_j)_i)^2
 * (the caller divides by s and applies the log transform).  mean_out (m) is the
 * posterior mean.  Needs the resident factor of gpe_factor.  Any m up to 2^20 (the
 * reference has no bound): m <= 16384 forms V in one chunk, beyond it V is formed
 * chunk pair by chunk pair straight into the factorisation workspace (V and its
 * factor take 2 x m_pad^2 x 8 bytes of HBM: 2 x 8.6 GB at m = 32768).
 * GPE_NOT_PD when V is not positive definite (np.linalg.cholesky's LinAlgError). */
int gpe_noise_sample(gpe_ctx* ctx, int64_t m, const double* Xs, const double* Hs,
                     const double* beta, double sigma, const double* r_new, double r_scale,
                     const double* t, int32_t s, const double* U, double* mean_out,
                     double* z_out);

/* Greedy pivoted Cholesky S = P L L^T P^T of the posterior covariance at m points (an
 * addition within ABI 10; the reference has no counterpart).  It extends the seam of
 * gpe_posterior, Posterior.make_covar/make_mean/make_var (_emulatorclasses.py:607-631): S is
 * the `var` of that Posterior, exactly what gpe_posterior(full_var = 1, precision = 64)
 * returns for the same arguments, plus sigma^2 r_scale r_new on its diagonal (r_new m values
 * or NULL) as gpe_noise_sample forms it; mean_out (m) is its mean.
 * With d^0 = diag S, step t takes p = argmax of d over the points not yet chosen (lowest
 * index on ties; a NaN is never greater) and stops before the step if t = k or
 * d_p <= tol max(d^0); else piv_out[t] = p, pivvar_out[t] = d_p, column
 * c = S[:, p] - L[:, :t] L[p, :t]^T, L[p, t] = sqrt(d_p), L[i, t] = c_i / sqrt(d_p) for
 * unchosen i and exactly 0 for rows chosen earlier, d_i -= L[i, t]^2.  *rank_out = steps
 * taken.  The pivots are the greedy maximum-variance batch (each the point with the largest
 * posterior variance given the training set and the points picked before it); L^-1 P^T
 * (y - mean) are the pivoted-Cholesky errors of Bastos & O'Hagan (2009).
 * L_out (m x k row-major, or NULL) is in the original point order (S = L L^T when
 * rank = m), columns >= rank zero; piv_out / pivvar_out (k values) are -1 / 0 from rank on.
 * 1 <= k <= m <= 16384 (one chunk of gpe_posterior): beyond, GPE_ERR_UNSUPPORTED; bad k,
 * tol < 0 or a NULL output: GPE_ERR_ARG; GPE_ERR_STATE without a resident factor.  Repeated
 * calls on one factor return the same bits; the resident factor stays usable.
 * One launch per pivot in panels of 128 columns (gpemu_pivchol.hpp), a grouped MFMA GEMM
 * S -= W W^T after each full panel; no synchronisation before the end. */
int gpe_posterior_pivchol(gpe_ctx* ctx, int64_t m, const double* Xs, const double* Hs,
                          const double* beta, double sigma, const double* r_new, double r_scale,
                          int64_t k, double tol, double* mean_out, int64_t* piv_out,
                          double* pivvar_out, double* L_out, int64_t* rank_out);

/* Greedy integrated-variance (IMSE, Cohn's ALC) batch design (an addition within ABI 10; the
 * reference has no counterpart).  Xs holds m = mc + mr points: the first mc rows are the
 * candidates, the last mr = m - mc rows a reference sample of the input distribution.  S is
 * exactly the matrix gpe_posterior_pivchol works on: gpe_posterior(full_var = 1,
 * precision = 64)'s covariance plus sigma^2 r_scale r_new on its diagonal (r_new m values or
 * NULL; "diagonal" by index); mean_out (m) is its mean.  w holds mr weights >= 0, NULL
 * meaning 1 / mr each.  Each step picks the candidate whose run most reduces the posterior
 * variance averaged (with w) over the reference points.
 * State, for candidates c and reference rows r: d_c = S_cc, C_rc = S[mc + r, c],
 * thr = tol max_c d^0_c (over the candidates only), *imse0_out = sum_r w_r S[mc + r, mc + r].
 * Step t = 0, 1, ...:
 *   q_c = sum_r w_r C_rc^2 and score_c = q_c / d_c; candidate c is eligible if it is unchosen,
 *   d_c > thr and its score is not NaN; stop before the step if t = k or nobody is eligible;
 *   p = the eligible candidate with the largest score (lowest index on ties; a NaN never wins);
 *   piv_out[t] = p, gain_out[t] = score_p, pivvar_out[t] = d_p;
 *   l_c = (S_cp - sum_{s<t} L_cs L_ps) / sqrt(d_p) for unchosen c (exactly 0 for candidates
 *   chosen earlier, sqrt(d_p) at c = p), lambda_r = C_rp / sqrt(d_p);
 *   C_rc -= lambda_r l_c and d_c -= l_c^2 for unchosen c.
 * gain_out[t] is the reduction of sum_r w_r Var(reference r) bought by observing candidate p
 * with the variance on S's diagonal: the integrated variance left after t picks is
 * imse0 - sum_{s<t} gain[s].  *rank_out = picks taken; piv_out / gain_out / pivvar_out (k
 * values) are -1 / 0 / 0 from rank on.
 * 1 <= mc < m <= 16384 (one chunk of gpe_posterior): beyond, GPE_ERR_UNSUPPORTED; mc < 1,
 * m - mc < 1, k outside [1, mc], tol < 0, a negative or NaN weight or a NULL among the
 * required pointers (all but r_new and w): GPE_ERR_ARG, before any device work;
 * GPE_ERR_STATE without a resident factor.  Repeated calls on one factor return the same
 * bits; the resident factor stays usable.
 * Two launches per pick (gpemu_imse.hpp: the column of L over the candidates, then one
 * streaming pass over C that downdates it and forms the next scores) in panels of 128 picks,
 * a grouped MFMA GEMM S -= W W^T over the candidates after each full panel; no
 * synchronisation before the end. */
int gpe_posterior_imse(gpe_ctx* ctx, int64_t m, int64_t mc, const double* Xs, const double* Hs,
                       const double* beta, double sigma, const double* r_new, double r_scale,
                       const double* w, int64_t k, double tol, double* mean_out,
                       int64_t* piv_out, double* gain_out, double* pivvar_out,
                       double* imse0_out, int64_t* rank_out);

/* Per-phase device time of the most recent gpe_objective call, in ms:
 * [0] K-build, [1] Cholesky, [2] triangular inverse, [3] A^-1 (L^-T L^-1),
 * [4] skinny solves / small algebra, [5] gradient contraction, [6] total.
 * After gpe_posterior_pivchol: [0] forming the covariance, [1] the pivot steps, [2] the
 * trailing updates and panel copies, [6] their sum (one synchronisation per panel is added).
 * After gpe_posterior_imse: [0] forming the covariance and copying C, [1] the column and
 * sweep kernels, [2] the trailing updates, [6] their sum (one synchronisation per panel is added).
 * After gpe_posterior_grad: [0] k_post_grad's device time summed over the chunks, [1] the
 * number of chunks (one synchronisation per chunk is added).
 * After gpe_posterior_mean: [0] k_post_mean's device time summed over the chunks, [1] the
 * number of chunks (one synchronisation per chunk is added).
 * After gpe_posterior_mean_multi: [0] k_post_mean_multi's device time summed over the chunks, [1] the
 * number of chunks (one synchronisation per chunk is added).  After gpe_objective_multi: as after
 * gpe_objective.
 * After gpe_posterior_groups: [0] the device time of k_post_groupgram and k_post_groupcov
 * summed over the chunks, [1] the number of chunks (one synchronisation per chunk is added).
 * Only filled when profiling is on. */
int gpe_set_profiling(gpe_ctx* ctx, int32_t on);
int gpe_phase_times(gpe_ctx* ctx, double* ms_out, int32_t n);

/* Aggregate device time (ms) and call count of the MFMA GEMM launches of the most
 * recent objective (profiling on), and their algorithmic flop count. */
int gpe_gemm_stats(gpe_ctx* ctx, double* ms_out, double* launches_out,
                   double* flops_out);

/* The same for the int8 products of the objective's A^-1 and of the top TRTRI level
 * (gpemu_ozaki.hpp: the fp64 products emulated exactly on the i8 MFMA, N moduli): their
 * device time (ms), launch count, int8 multiply-add ops (2 per multiply-add, every modulus that ran: 15 for a certified product)
 * and the fp64 flops of the products they replace.  Internal instrumentation for bench.py;
 * the reference has no counterpart. */
int gpe_ozaki_stats(gpe_ctx* ctx, double* ms_out, double* launches_out, double* int8_ops_out,
                    double* fp64_flops_out);

/* The 15-moduli certificates of the int8 products of the most recent factorisation or
 * objective (an addition within ABI 10; no profiling needed): how many products carried a
 * certificate (0 with GPEMU_OZAKI_CERT=0, fewer than 16 moduli or no int8 product) and how
 * many of those were certified and ran on 15 moduli.  Waits for the context's streams. */
int gpe_oz_cert_stats(gpe_ctx* ctx, int32_t* products_out, int32_t* certified_out);

/* The same products' row-sum maxima, in launch order (an addition within ABI 10; a debug
 * read-back, outside timed runs): A = max_r s_a and B = max_r s_b of the first min(cap,
 * products) products; a product is certified iff A B < T15 (gpemu_ozaki.hpp). */
int gpe_oz_cert_sums(gpe_ctx* ctx, int32_t cap, uint64_t* a_out, uint64_t* b_out);

#ifdef __cplusplus
}
#endif

#endif /* GPEMU_H */
