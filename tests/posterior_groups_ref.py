"""A numpy statement of gpe_posterior_groups (no GPU): the posterior covariance inside groups of
G consecutive points, with the conventions of the full posterior covariance.

With A = L L^T the training matrix, K* the n x m cross-covariance, v = L^-1 K*,
T = Hs - K*^T A^-1 H, Kq Kq^T = H^T A^-1 H and t = T Kq^-T (one row per point):

    a == b   sigma^2 (cdiag - |v_a|^2 + |t_a|^2)
    a != b   sigma^2 (coff rho(s_ab) - v_a . v_b + t_a . t_b)

where "a == b" is decided by index: two different points with equal coordinates get the
off-diagonal form.  coff = 1 - nu and cdiag = 1 for the std nugget, coff = 1 and
cdiag = 1 + nu^2 for the alt one (K.var(predict=True) of the reference).
"""
import numpy as np
import scipy.linalg as sla

import matern_ref as mr
from oracle import gp_oracle as orc


def consts(nu, kind):
    """(coff, cdiag) of the posterior's own covariance term."""
    return (1.0, 1.0 + nu ** 2) if kind == orc.ALT else (1.0 - nu, 1.0)


def _parts(XT, fT, HT, A, Xs, Hs, beta, delta, nu, kind, family):
    """(mean, v (n x m), t (m x q)) of the points Xs."""
    L = np.linalg.cholesky(A)
    Ks = mr.kernel_covar(XT, Xs, delta, nu, kind, family)
    v = sla.solve_triangular(L, Ks, lower=True)
    z = sla.solve_triangular(L, np.column_stack([fT - HT.dot(beta), HT]), lower=True)
    mean = Hs.dot(beta) + v.T.dot(z[:, 0])
    T = Hs - v.T.dot(z[:, 1:])
    Kq = np.linalg.cholesky(z[:, 1:].T.dot(z[:, 1:]))
    t = sla.solve_triangular(Kq, T.T, lower=True).T
    return mean, v, t


def group_blocks(XT, fT, HT, A, Xs, Hs, beta, sigma, delta, nu, kind, family, group):
    """(mean (m), cov (m // group, group, group))."""
    m, G = len(Xs), int(group)
    assert 1 <= G and m % G == 0
    mean, v, t = _parts(XT, fT, HT, A, Xs, Hs, beta, delta, nu, kind, family)
    coff, cdiag = consts(nu, kind)
    ng = m // G
    xw = (np.asarray(Xs, dtype=float) / np.asarray(delta, dtype=float)).reshape(ng, G, -1)
    s = ((xw[:, :, None, :] - xw[:, None, :, :]) ** 2).sum(axis=-1)
    own = coff * mr.rho_g(s, family)[0]
    own[:, np.arange(G), np.arange(G)] = cdiag
    vg = v.reshape(v.shape[0], ng, G)
    tg = t.reshape(ng, G, -1)
    cov = sigma ** 2 * (own - np.einsum("iga,igb->gab", vg, vg) + np.einsum("gaq,gbq->gab", tg, tg))
    return mean, cov


def full_cov(XT, fT, HT, A, Xs, Hs, beta, sigma, delta, nu, kind, family):
    """(mean, m x m covariance): the one group of all the points."""
    mean, cov = group_blocks(XT, fT, HT, A, Xs, Hs, beta, sigma, delta, nu, kind, family, len(Xs))
    return mean, cov[0]
