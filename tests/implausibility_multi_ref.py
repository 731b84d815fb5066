"""Dense NumPy reference for a multi-output member of the resident emulator set
(gpe_hm_add_multi, gpe_hm_implausibility_mv): test infrastructure, NumPy / SciPy only.

p outputs F (n x p) share A = K.var(X, predict) + diag(r_diag).  B (q x p) and Sigma-hat (p x p)
are multi_output_ref.algebra's (the formulas of include/gpemu.h); per output a the mean and
c, the variance at sigma = 1, are implausibility_ref.posterior_diag's with f = F[:, a] and
beta = B[:, a] (c does not depend on a: it is taken from output 0).  Then

    univariate  I^2_a = (mean_a - z_a)^2 / (Sigma_aa c + var_extra_a)
    joint       I^2   = (mean - z)^T (c Sigma + V)^-1 (mean - z)      by np.linalg.solve
"""
import numpy as np

import implausibility_ref as iref
import matern_ref as mref
import multi_output_ref as mo


def estimates(XT, F, HT, delta, nu, kind, family="gaussian", r_diag=None):
    """(B q x p, Sigma-hat p x p) on the factor's matrix."""
    F = np.asarray(F, np.float64).reshape(np.asarray(XT).shape[0], -1)
    A = mref.kernel_var(XT, delta, nu, kind, family, True)[0]
    if r_diag is not None:
        A[np.diag_indices_from(A)] += np.asarray(r_diag, np.float64)
    _, _, _, _, B, _, S = mo.algebra(A, F, np.asarray(HT, np.float64))
    return B, S / (F.shape[0] - np.asarray(HT).shape[1] - 2.0)


def parts(XT, F, HT, Xs, Hs, B, delta, nu, kind, family="gaussian", r_diag=None):
    """(mean p x m, c m) at the m points Xs (in the member's own inputs)."""
    F = np.asarray(F, np.float64).reshape(np.asarray(XT).shape[0], -1)
    means, c = [], None
    for a in range(F.shape[1]):
        mean, var = iref.posterior_diag(XT, F[:, a], HT, Xs, Hs, B[:, a], 1.0, delta, nu, kind, family, r_diag)
        means.append(mean)
        c = var if c is None else c
    return np.array(means), c


def univariate(mean, c, Sigma, zs, var_extra):
    """I^2 (p x m) output by output."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (mean - np.asarray(zs)[:, None]) ** 2 / (np.diag(Sigma)[:, None] * c[None, :]
                                                        + np.asarray(var_extra)[:, None])


def joint(mean, c, Sigma, z, V):
    """I^2 (m): a dense solve of c Sigma + V per point."""
    r = (mean - np.asarray(z)[:, None]).T                          # m x p
    A = c[:, None, None] * np.asarray(Sigma)[None] + np.asarray(V)[None]
    return np.einsum("sa,sa->s", r, np.linalg.solve(A, r[:, :, None])[:, :, 0])


def spd(p, cond, seed, scale=1.0):
    """A random symmetric positive definite p x p matrix with the condition number cond
    (eigenvalues log-spaced over [scale / cond, scale]; p = 1: scale)."""
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.normal(size=(p, p)))
    e = scale * np.logspace(0.0, -np.log10(cond), p) if p > 1 else np.array([scale])
    A = (Q * e) @ Q.T
    return 0.5 * (A + A.T)
