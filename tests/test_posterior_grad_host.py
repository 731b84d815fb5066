"""CPU checks behind gpe_posterior_grad: the dense reference (tests/posterior_grad_ref.py)
against central differences of matern_ref.posterior, and Basis.design_matrix_deriv.

Central differences of step h = 1e-5 carry a truncation error of h^2 f''' / 6 ~ 1e-11 and a
rounding error of about eps cond(A) |f| / h; at cond(A) <= 9e4 that is ~ 1e-9 (the largest
difference seen over these cases was 8.9e-9), so 1e-7 max(1, max |d|) holds with room and
still catches a wrong sign, factor or term.  None of the random points is a training point:
Matern 3/2 is only C^1 there, and a central difference across the kink is O(h) off.
"""
import numpy as np
import pytest

import matern_ref as mr
import posterior_grad_ref as pgr
from gp_emu_uqsa_amd import model
from oracle import gp_oracle as orc

STEP = 1e-5


def central_differences(X, f, H, A, Xs, beta, delta, nu, kind, family):
    m, d = Xs.shape
    dmean = np.empty((m, d))
    dvar = np.empty((m, d))
    for k in range(d):
        out = []
        for sgn in (1.0, -1.0):
            Xp = Xs.copy()
            Xp[:, k] += sgn * STEP
            mean, S = mr.posterior(X, f, H, A, Xp, orc.linear_basis(Xp), beta, mr.SIGMA, delta, nu, kind, family)
            out.append((mean, np.diag(S)))
        dmean[:, k] = (out[0][0] - out[1][0]) / (2.0 * STEP)
        dvar[:, k] = (out[0][1] - out[1][1]) / (2.0 * STEP)
    return dmean, dvar


@pytest.mark.parametrize("kind", [orc.STD, orc.ALT], ids=["std", "alt"])
@pytest.mark.parametrize("n,d", [(300, 5), (129, 2)])
@pytest.mark.parametrize("family", mr.FAMILIES)
def test_reference_against_central_differences(family, n, d, kind):
    X, f, H = orc.synthetic_problem(n, d, seed=9)
    delta, nu = mr.deltas(d), mr.NU[kind]
    A = mr.make_A(X, delta, nu, kind, family)[0]
    assert np.linalg.cond(A) <= 1e6
    beta = orc.optimal_beta_ref(A, H, f)
    Xs = np.random.RandomState(3).uniform(0.05, 0.95, (40, d))
    Hs = orc.linear_basis(Xs)
    dHs, hdim = pgr.linear_basis_deriv(Xs)
    dmean, dvar = pgr.grad(X, f, H, A, Xs, Hs, dHs, hdim, beta, mr.SIGMA, delta, nu, kind, family)
    fm, fv = central_differences(X, f, H, A, Xs, beta, delta, nu, kind, family)
    em = np.max(np.abs(dmean - fm)) / max(1.0, np.max(np.abs(fm)))
    ev = np.max(np.abs(dvar - fv)) / max(1.0, np.max(np.abs(fv)))
    print(family, n, d, kind, "d mean", em, "d var", ev, "max |d mean|", np.max(np.abs(fm)),
          "max |d var|", np.max(np.abs(fv)))
    assert np.max(np.abs(fm)) > 1e-2 and np.max(np.abs(fv)) > 1e-4   # (no comparison of zeros)
    assert em <= 1e-7 and ev <= 1e-7


class _Beliefs:
    def __init__(self, basis_str, basis_inf):
        self.active = []
        self.basis_str = list(basis_str)
        self.basis_inf = list(basis_inf)


def test_design_matrix_deriv_is_analytic():
    """x, x**2, np.cos(x) and a constant, by complex step: the analytic derivatives to 1e-12."""
    basis = model.Basis(_Beliefs(["1.0", "x", "x**2", "np.cos(x)", "0.0*x+2.5"], [0, 1, 2, 3]))
    X = np.random.RandomState(1).uniform(size=(50, 4))
    dH, hdim = basis.design_matrix_deriv(X)
    assert hdim.dtype == np.int32
    np.testing.assert_array_equal(hdim, [-1, 0, 1, 2, 3])
    want = np.stack([np.zeros(50), np.ones(50), 2.0 * X[:, 1], -np.sin(X[:, 2]), np.zeros(50)], axis=1)
    assert np.max(np.abs(dH - want)) <= 1e-12
    H = basis.design_matrix(X)
    assert dH.shape == H.shape


def test_design_matrix_deriv_falls_back_to_central_differences():
    """np.abs returns a real number for a complex argument, np.floor refuses one, and a plain
    number has no imaginary part to read: each takes the central difference, to 1e-6."""
    basis = model.Basis(_Beliefs(["1.0", "np.abs(x - 0.5)**3", "np.floor(x) + x**2", "3.0"], [0, 1, 2]))
    X = np.random.RandomState(2).uniform(size=(40, 3))
    dH, hdim = basis.design_matrix_deriv(X)
    np.testing.assert_array_equal(hdim, [-1, 0, 1, 2])
    u = X[:, 0] - 0.5
    want = np.stack([np.zeros(40), 3.0 * np.abs(u) * u, 2.0 * X[:, 1], np.zeros(40)], axis=1)
    assert np.max(np.abs(dH - want)) <= 1e-6
