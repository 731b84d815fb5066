"""CPU checks of the pivoted-Cholesky reference (tests/pivchol_ref.py) that the GPU tests of
gpe_posterior_pivchol lean on: the reference against LAPACK's dpstrf, the conditions of the
cases (pivot gaps, stop-rule margins) and the greedy maximum-variance equivalence.
"""
import numpy as np
import pytest
from scipy.linalg import lapack

import pivchol_ref as pr

GAP = 1e-6   # a pivot is compared only where the top two variances differ by this much of max diag S


@pytest.mark.parametrize("name,with_r", pr.VARIANTS)
def test_reference_matches_dpstrf(name, with_r):
    S = pr.covariance(name, with_r)
    piv, pivvar, L, rank, g = pr.reference(name, with_r)
    m = S.shape[0]
    assert rank == m
    assert sorted(piv.tolist()) == list(range(m))
    recon = np.max(np.abs(L.dot(L.T) - S)) / np.max(np.diag(S))
    _, lp, lrank, info = lapack.dpstrf(np.array(S), lower=1)
    assert info == 0 and lrank == m
    k = pr.safe_prefix(g, GAP)
    print(name, with_r, "reconstruction", recon, "gap-safe prefix", k, "cond", np.linalg.cond(S))
    assert recon <= 1e-10
    np.testing.assert_array_equal(lp[:k] - 1, piv[:k])


@pytest.mark.parametrize("name,with_r", pr.VARIANTS)
def test_first_32_pivots_are_well_separated(name, with_r):
    """The GPU's pivot-order test compares 32 pivots with the reference's on the oracle's
    covariance; the device's covariance differs from it by up to 1e-8 of its scale."""
    g = pr.reference(name, with_r)[4]
    print(name, with_r, "smallest gap of the first 32 steps", g[:32].min())
    assert g[:32].min() >= GAP


def test_gap_safe_prefixes_of_the_cases():
    got = [pr.safe_prefix(pr.reference(name)[4], GAP) for name in pr.CASES]
    assert got == [59, 129, 300, 71, 312]


@pytest.mark.parametrize("key", sorted(pr.STOP_CASES))
def test_stop_rule_cases_have_a_margin(key):
    name, tol = key
    S = pr.case(name)["S"]
    full = pr.reference(name)[1]
    piv, pivvar, L, rank = pr.pivchol(S, None, tol)
    assert rank == pr.STOP_CASES[key]
    scale = np.max(np.diag(S))
    kept = (full[rank - 1] - tol * scale) / scale
    dropped = (tol * scale - full[rank]) / scale
    print(name, tol, "rank", rank, "margins", kept, dropped)
    assert kept >= 1e-4 and dropped >= 1e-4
    # untrimmed outputs: the first rank steps of the full factorisation, then -1 / 0 / zero columns
    np.testing.assert_array_equal(piv[:rank], pr.reference(name)[0][:rank])
    assert np.all(piv[rank:] == -1) and np.all(pivvar[rank:] == 0.0) and not L[:, rank:].any()


def test_pivots_are_the_greedy_maximum_variance_batch():
    from oracle import gp_oracle as orc
    c, cand, Hc, picks = pr.design_problem()
    idx, var, gap = pr.brute_force_design(c, cand, picks)
    _, S = orc.posterior_ref(c["X"], c["f"], c["H"], c["A"], cand, Hc, c["beta"], pr.SIGMA, c["delta"], c["nu"],
                             c["kind"])
    piv, pivvar, _, rank = pr.pivchol(S, picks)
    err = np.max(np.abs(pivvar - var) / var)
    print("picks", idx, "worst variance difference", err, "smallest gap", gap)
    assert rank == picks
    np.testing.assert_array_equal(piv, idx)
    assert err <= 1e-10
    assert gap >= 1e-6


def test_ties_nan_and_the_stop_at_zero():
    S = np.diag([2.0, 3.0, 3.0, 1.0])
    piv, pivvar, L, rank = pr.pivchol(S)
    assert piv.tolist() == [1, 2, 0, 3] and rank == 4
    S = np.diag([2.0, np.nan, 1.0])
    piv, _, _, rank = pr.pivchol(S)
    assert piv.tolist() == [0, 2, -1] and rank == 2
    S = np.ones((3, 3))   # rank one: the second pivot's variance is exactly 0 <= 0 * max
    piv, pivvar, L, rank = pr.pivchol(S)
    assert rank == 1 and piv.tolist() == [0, -1, -1]
