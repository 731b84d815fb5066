"""Dense NumPy / SciPy reference for the gradient of the posterior in the point (test
infrastructure; checked against central differences of matern_ref.posterior in
test_posterior_grad_host.py).

With s_i = sum_k ((x_k - x_ik) / delta_k)^2, K*_i = coff rho(s_i) (coff = 1 - nu for the std
kernel, 1 for the alt one) and g the family's derivative factor (matern_ref.rho_g):

  d K*_i / d x_k = -2 coff g(s_i) (x_k - x_ik) / delta_k^2
  d mean / d x_k = d_k h . beta + sum_i gamma_i d_k K*_i,      gamma = A^-1 (f - H beta)
  d var / d x_k  = sigma^2 (-2 sum_i u_i d_k K*_i + 2 tau . d_k h)
  tau = (H^T A^-1 H)^-1 (h - G^T K*),   u = A^-1 K* + G tau,   G = A^-1 H

(d_k h)_j = dHs[., j] if hdim[j] = k, else 0: every basis column depends on one input.
"""
import numpy as np
from scipy import linalg as sla
from scipy.spatial import distance as dist

import matern_ref as mr
from oracle import gp_oracle as orc


def linear_basis_deriv(Xs):
    """(dHs, hdim) of oracle.gp_oracle.linear_basis: H = [1, x_0, ..., x_{d-1}]."""
    m, d = Xs.shape
    dHs = np.ones((m, d + 1))
    dHs[:, 0] = 0.0
    return dHs, np.arange(-1, d, dtype=np.int32)


def gls_beta(A, H, f):
    """beta = (H^T A^-1 H)^-1 H^T A^-1 f from one Cholesky factorisation (what
    oracle.gp_oracle.optimal_beta_ref computes; that one is slow at n in the thousands)."""
    G = sla.cho_solve(sla.cho_factor(A, lower=True), H)
    return sla.solve(H.T.dot(G), G.T.dot(f), assume_a="pos")


def grad(XT, fT, HT, A, Xs, Hs, dHs, hdim, beta, sigma, delta, nu, kind, family):
    """(dmean, dvar), m x d each, of matern_ref.posterior's mean and diagonal variance."""
    XT = np.asarray(XT, dtype=np.float64)
    Xs = np.asarray(Xs, dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    hdim = np.asarray(hdim)
    m, d = Xs.shape
    rho, g = mr.rho_g(dist.cdist(XT / delta, Xs / delta, "sqeuclidean"), family)
    coff = 1.0 if kind == orc.ALT else 1.0 - nu
    Ks = coff * rho                                   # n x m
    cA = sla.cho_factor(A, lower=True)                # (one factorisation for the three solves)
    gamma = sla.cho_solve(cA, fT - HT.dot(beta))
    G = sla.cho_solve(cA, HT)
    T = Hs - Ks.T.dot(G)                              # m x q
    tau = sla.solve(HT.T.dot(G), T.T, assume_a="pos").T
    U = sla.cho_solve(cA, Ks) + G.dot(tau.T)          # n x m
    dmean = np.empty((m, d))
    dvar = np.empty((m, d))
    for k in range(d):
        dK = -2.0 * coff * g * (Xs[:, k][None, :] - XT[:, k][:, None]) / delta[k] ** 2
        dh = dHs * (hdim == k)[None, :]
        dmean[:, k] = dh.dot(beta) + dK.T.dot(gamma)
        dvar[:, k] = sigma ** 2 * (-2.0 * np.sum(U * dK, axis=0) + 2.0 * np.sum(tau * dh, axis=1))
    return dmean, dvar
