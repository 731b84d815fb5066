"""Dense NumPy reference for the resident emulator set (gpe_hm_*): per emulator the posterior
mean and diagonal variance from L^-1 by the formulas of include/gpemu.h, the implausibility
and the selection of the largest ones (test infrastructure, NumPy / SciPy only).

For emulator o with training matrix A = K.var(X, predict) + diag(r_diag) = L L^T, K* the
n x m cross-covariance, gamma = A^-1 (f - H beta), G = A^-1 H and Kq Kq^T = H^T A^-1 H:

    mean = h . beta + sum_i gamma_i K*_i
    var  = sigma^2 (cdiag - |L^-1 K*|^2 + |(h - G^T K*) Kq^-T|^2)
    I^2  = (mean - z)^2 / (var + var_extra)

cdiag is K.var's diagonal for prediction: 1 (std nugget), 1 + nu^2 (alt nugget).  ``dtype``
np.longdouble evaluates the same formulas in extended precision (the triangular solves by
substitution in NumPy, since LAPACK has no such type): the yardstick for comparing two fp64
routes to one posterior.
"""
import numpy as np
from scipy import linalg as sla

import matern_ref as mref
from oracle import gp_oracle as orc


def _chol(A):
    """Lower Cholesky factor in A's dtype (column by column: works for np.longdouble)."""
    if A.dtype == np.float64:
        return np.linalg.cholesky(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j].dot(L[j, :j]))
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    return L


def _forward(L, B):
    """L^-1 B in L's dtype."""
    if L.dtype == np.float64:
        return sla.solve_triangular(L, B, lower=True)
    Y = np.array(B, dtype=L.dtype)
    for i in range(L.shape[0]):
        Y[i] = (Y[i] - L[i, :i].dot(Y[:i])) / L[i, i]
    return Y


def _backward(L, B):
    """L^-T B in L's dtype."""
    if L.dtype == np.float64:
        return sla.solve_triangular(L, B, lower=True, trans="T")
    Y = np.array(B, dtype=L.dtype)
    for i in range(L.shape[0] - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i].dot(Y[i + 1:])) / L[i, i]
    return Y


def posterior_diag(XT, fT, HT, Xs, Hs, beta, sigma, delta, nu, kind, family="gaussian", r_diag=None,
                   dtype=np.float64):
    """(mean, var) at the m points Xs (in the emulator's own inputs), both of length m."""
    A = mref.kernel_var(XT, delta, nu, kind, family, True)[0]
    if r_diag is not None:
        A[np.diag_indices_from(A)] += np.asarray(r_diag, dtype=np.float64)
    Ks = mref.kernel_covar(XT, Xs, delta, nu, kind, family)
    A, Ks = A.astype(dtype), Ks.astype(dtype)
    fT, HT, Hs, beta = (np.asarray(a, dtype=dtype) for a in (fT, HT, Hs, beta))
    L = _chol(A)
    V = _forward(L, Ks)                                   # L^-1 K*
    Z = _forward(L, np.column_stack([fT - HT.dot(beta), HT]))
    W = _backward(L, Z)                                   # [gamma, G]
    gamma, G = W[:, 0], W[:, 1:]
    Kq = _chol(Z[:, 1:].T.dot(Z[:, 1:]))                  # H^T A^-1 H = Kq Kq^T
    T = Hs - Ks.T.dot(G)
    U = _forward(Kq, T.T)                                 # ((h - G^T K*) Kq^-T)^T
    cdiag = dtype(1.0) + dtype(nu) ** 2 if kind == orc.ALT else dtype(1.0)
    mean = Hs.dot(beta) + Ks.T.dot(gamma)
    var = dtype(sigma) ** 2 * (cdiag - np.sum(V * V, axis=0) + np.sum(U * U, axis=0))
    return mean, var


def imaxes(I2, maxno):
    """Per point (row) the maxno largest sqrt(I2) over the emulators (columns), ascending; a NaN
    counts as larger than every number."""
    I2 = np.asarray(I2, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        I = np.sqrt(I2)
    out = np.empty((I.shape[0], maxno))
    for s in range(I.shape[0]):
        row = I[s]
        nan = row[np.isnan(row)]
        num = np.sort(row[~np.isnan(row)])
        out[s] = np.concatenate([num, nan])[-maxno:]
    return out


def implausibility(emulators, Xs, zs, var_extra, maxno=1):
    """(imax (m x maxno), mean (p x m), var (p x m)).  Each emulator is a dict with XT, fT, HT,
    beta, sigma, delta, nu, kind and optionally family, r_diag, and ``active``: the columns of
    Xs it reads; its basis at a point is [1, its inputs] (``oracle.gp_oracle.linear_basis``)
    cut to HT's width."""
    Xs = np.asarray(Xs, dtype=np.float64)
    means, vars_ = [], []
    for e in emulators:
        x = Xs[:, list(e["active"])]
        hs = orc.linear_basis(x)[:, :np.asarray(e["HT"]).shape[1]]
        mean, var = posterior_diag(e["XT"], e["fT"], e["HT"], x, hs, e["beta"], e["sigma"], e["delta"], e["nu"],
                                   e["kind"], e.get("family", "gaussian"), e.get("r_diag"))
        means.append(mean)
        vars_.append(var)
    mean, var = np.array(means), np.array(vars_)
    with np.errstate(invalid="ignore", divide="ignore"):
        I2 = (mean - np.asarray(zs)[:, None]) ** 2 / (var + np.asarray(var_extra)[:, None])
    return imaxes(I2.T, maxno), mean, var
