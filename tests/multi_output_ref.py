"""Dense NumPy / LAPACK reference of the separable multi-output emulator (test infrastructure;
imports nothing from the package).

p outputs F (n x p) share one correlation matrix A = K(X, X; delta, nu), the matrix the MUCM
objective factors (sigma^2 = 1; r does not enter).  With H n x q, G = A^-1 H, Q = H^T G,
P = A^-1 - G Q^-1 G^T, S = F^T P F and x = 2 log hp (hp = [delta (d), nu if fitted]):

  B         = Q^-1 G^T F                       (q x p)
  Sigma-hat = S / (n - q - 2)                  (p x p)
  llh       = 1/2 [(n - q) log|Sigma-hat| + p log|A| + p log|Q|]
  d llh / d x_k = 1/2 tr(M dA/dx_k),  M = p A^-1 - p G Q^-1 G^T - (n - q) P F S^-1 F^T P

Posterior at x: mean = h(x)^T B + K*(x)^T A^-1 (F - H B); cov(output a at x, output b at x') =
Sigma-hat_ab c(x, x') with c the single-output posterior covariance at sigma = 1.

A, rho and g come from tests/matern_ref.py, which runs oracle.gp_oracle.kernel_var_ref's own
operations for the gaussian family; the derivative matrices are the oracle's grad_delta_ref and
grad_nugget_ref (s2 = 1) on the family's g and rho.
"""
import numpy as np
from scipy import linalg as sla

import matern_ref as mr
from oracle import gp_oracle as orc


def outputs(X, p, seed=3):
    """p smooth, linearly independent outputs of the inputs X (n x d) plus a little noise."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(d, p))
    ph = rs.uniform(0, 2 * np.pi, size=p)
    F = np.sin(X @ W * 1.5 + ph) + 0.3 * (X ** 2) @ rs.normal(size=(d, p)) + 0.02 * rs.normal(size=(n, p))
    return F * (1.0 + 0.5 * np.arange(p))


def algebra(A, F, H):
    """(L, logdetA, G, Q, B, P F, S) of the model above; np.linalg.LinAlgError where a Cholesky
    fails (A, Q)."""
    L = np.linalg.cholesky(A)
    logdetA = 2.0 * np.sum(np.log(np.diag(L)))
    G = sla.cho_solve((L, True), H)
    Q = H.T @ G
    Kq = np.linalg.cholesky(Q)
    B = sla.cho_solve((Kq, True), G.T @ F)
    PF = sla.cho_solve((L, True), F - H @ B)
    S = F.T @ PF
    S = 0.5 * (S + S.T)
    return L, logdetA, G, Q, B, PF, S


def objective(X, F, H, hp, kind, fit_nugget, family="gaussian", nu_fixed=0.0, want_grad=True):
    """(llh, grad or None, Sigma-hat, B), or None when A, Q or S is not positive definite."""
    X = np.asarray(X, np.float64)
    F = np.asarray(F, np.float64).reshape(X.shape[0], -1)
    H = np.asarray(H, np.float64)
    n, d = X.shape
    q, p = H.shape[1], F.shape[1]
    hp = np.asarray(hp, np.float64)
    delta = hp[:d]
    nu = float(hp[d]) if fit_nugget else float(nu_fixed)
    A, rho, g = mr.make_A(X, delta, nu, kind, family, None, 1.0)
    try:
        L, logdetA, G, Q, B, PF, S = algebra(A, F, H)
        C = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None
    Sigma = S / (n - q - 2.0)
    logdetS = 2.0 * np.sum(np.log(np.diag(C)))
    logdetQ = np.linalg.slogdet(Q)[1]
    llh = 0.5 * ((n - q) * (logdetS - p * np.log(n - q - 2.0)) + p * logdetA + p * logdetQ)
    if not want_grad:
        return llh, None, Sigma, B
    Ainv = sla.cho_solve((L, True), np.eye(n))
    M = p * Ainv - p * G @ sla.solve(Q, G.T) - (n - q) * PF @ sla.solve(S, PF.T)
    grad = np.empty(hp.size)
    for k in range(d):
        dA = orc.grad_delta_ref(X[:, k], delta[k], nu, g, 1.0, kind)
        grad[k] = 0.5 * np.sum(M * dA)
    if fit_nugget:
        dA = orc.grad_nugget_ref(n, nu, rho, 1.0, kind)
        grad[d] = 0.5 * np.sum(M * dA)
    return llh, grad, Sigma, B


def conditioning(X, delta, nu, kind, family="gaussian"):
    """(cond(A), median off-diagonal rho)."""
    A, rho, _ = mr.kernel_var(X, delta, nu, kind, family)
    return float(np.linalg.cond(A)), float(np.median(rho))


def posterior(X, F, H, Xs, Hs, delta, nu, kind, family="gaussian", r=None, r_scale=0.0, full=True):
    """(mean m x p, c (m x m, or its diagonal), Sigma-hat, B) for the factor
    gpe_factor(kernel, delta, nu, 1, r_scale)."""
    X = np.asarray(X, np.float64)
    F = np.asarray(F, np.float64).reshape(X.shape[0], -1)
    n, q = X.shape[0], H.shape[1]
    A = mr.kernel_var(X, delta, nu, kind, family, True)[0]
    if r is not None and r_scale != 0.0:
        A[np.diag_indices_from(A)] += r_scale * np.asarray(r, np.float64)
    L, _, G, Q, B, PF, S = algebra(A, F, H)
    Ks = mr.kernel_covar(X, Xs, delta, nu, kind, family)
    mean = Hs @ B + Ks.T @ PF
    t1 = Hs - Ks.T @ G
    Ass = mr.kernel_var(Xs, delta, nu, kind, family, True)[0]
    c = Ass - Ks.T @ sla.cho_solve((L, True), Ks) + t1 @ sla.solve(Q, t1.T)
    return mean, (c if full else np.diag(c).copy()), S / (n - q - 2.0), B
