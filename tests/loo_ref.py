"""Leave-one-out references for gpe_loo (test infrastructure, NumPy / SciPy only).

``closed_form`` is the one-factorisation formula of DESIGN.md; ``brute_force`` is what it
replaces: n refits through the oracle's ``posterior_ref`` and ``optimal_beta_ref``, each on
the n - 1 other points.  ``CASES`` are the problems both test files use.
"""
import functools

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as orc

SIGMA = 0.7

# name -> (n, d, kernel, nu, delta, with r)
CASES = {
    "n60_std": (60, 3, orc.STD, 1e-3, [0.6, 0.9, 1.1], False),                  # one tile, padded
    "n60_alt_r": (60, 3, orc.ALT, 3e-2, [0.6, 0.9, 1.1], True),                 # the r term
    "n129_std": (129, 2, orc.STD, 1e-4, [1.0, 1.0], False),                     # one row in a second tile
    "n300_alt_r": (300, 10, orc.ALT, 3e-2, np.linspace(0.5, 1.1, 10), True),    # three tiles, ragged
    "n300_d33": (300, 33, orc.STD, 1e-3, np.linspace(0.8, 2.0, 33), False),     # q + 1 = 35: two column chunks
    "n1000_std": (1000, 5, orc.STD, 1e-3, np.linspace(0.5, 1.1, 5), False),     # 8 tile rows: several k chunks
    "n1100_alt_r": (1100, 5, orc.ALT, 3e-2, np.linspace(0.5, 1.1, 5), True),    # 9 tile rows: ragged TRTRI pairs
}
BRUTE_CASES = ("n60_std", "n60_alt_r", "n129_std")   # the brute force stays under a second in total


def problem(name):
    """(X, f, H, r or None, kernel, delta, nu, A) of a case; A as gpe_factor(s2 = 1, r_scale = 1) holds it."""
    n, d, kind, nu, delta, with_r = CASES[name]
    X, f, H = orc.synthetic_problem(n, d, seed=0)
    r = np.random.RandomState(5).uniform(0, 0.02, n) if with_r else None
    delta = np.asarray(delta, dtype=float)
    A, _ = orc.make_A_ref(X, delta, nu, kind, r=r, s2=1.0, predict=True)
    return X, f, H, r, kind, delta, nu, A


def closed_form(A, H, f, sigma, r=None, r_scale=1.0):
    """(mean, var, beta): mean_i = f_i - (P f)_i / P_ii, var_i = sigma^2 (1 / P_ii - r_scale r_i)
    with P = A^-1 - A^-1 H (H^T A^-1 H)^-1 H^T A^-1, from one Cholesky of A."""
    n = f.size
    L = np.linalg.cholesky(A)
    Xi = sla.solve_triangular(L, np.eye(n), lower=True)
    a = np.sum(Xi * Xi, axis=0)                              # (A^-1)_ii
    Z = Xi.dot(np.column_stack([f, H]))
    U = Xi.T.dot(Z)                                          # A^-1 [f H]
    G = Z[:, 1:].T.dot(Z[:, 1:])
    beta = np.linalg.solve(G, Z[:, 1:].T.dot(Z[:, 0]))
    UH = U[:, 1:]
    pii = a - np.einsum("ij,ji->i", UH, np.linalg.solve(G, UH.T))
    pf = U[:, 0] - UH.dot(beta)
    rr = 0.0 if r is None else r_scale * np.asarray(r, dtype=float)
    return f - pf / pii, sigma ** 2 * (1.0 / pii - rr), beta


def brute_force(X, f, H, A, sigma, delta, nu, kind):
    """The n refits: Posterior at x_i from the other n - 1 points, beta by optimalbeta on them."""
    n = f.size
    mean = np.empty(n)
    var = np.empty(n)
    for i in range(n):
        o = np.delete(np.arange(n), i)
        Ao = A[np.ix_(o, o)]
        beta = orc.optimal_beta_ref(Ao, H[o], f[o])
        m, v = orc.posterior_ref(X[o], f[o], H[o], Ao, X[i:i + 1], H[i:i + 1], beta, sigma, delta, nu, kind)
        mean[i] = m[0]
        var[i] = v[0, 0]
    return mean, var


@functools.lru_cache(maxsize=None)
def reference(name):
    """closed_form of a case, computed once and shared; callers must not modify it."""
    X, f, H, r, kind, delta, nu, A = problem(name)
    out = closed_form(A, H, f, SIGMA, r=r, r_scale=1.0)
    for a in out:
        a.setflags(write=False)
    return out


def errors(mean, var, ref_mean, ref_var, f):
    """(max |d mean| / max |f|, max relative error of the variance): the figures the tests bound."""
    return (float(np.max(np.abs(mean - ref_mean)) / np.max(np.abs(f))),
            float(np.max(np.abs(var - ref_var) / np.abs(ref_var))))
