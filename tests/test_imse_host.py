"""CPU checks of the integrated-variance design reference (tests/imse_ref.py) that the GPU
tests of gpe_posterior_imse lean on: the conditions of the cases (score gaps, eligibility
margins, ranks of the stop cases), the gain identity, a brute-force refit, and the argument
checks of design_inputs.imse_design that need no device.
"""
import types

import numpy as np
import pytest

import imse_ref as ir
import pivchol_ref as pr
from gp_emu_uqsa_amd import design_inputs
from oracle import gp_oracle as orc

ALL = ir.VARIANTS + ir.STOP_VARIANTS
STOP_RANKS = {("n300_alt_r", 0.5): 72, ("n1000_std", 0.5): 10, ("n1000_std", 0.3): 36}


@pytest.mark.parametrize("name,with_r,weighted,tol", ALL)
def test_every_step_is_well_separated(name, with_r, weighted, tol):
    """The GPU tests compare picks with the reference's: every step's best score must stand
    clear of the second best."""
    piv, gain, pivvar, imse0, rank, gaps, margin = ir.reference(name, with_r, weighted, tol)
    print(name, with_r, weighted, tol, "rank", rank, "smallest gap", gaps.min(), "margin", margin)
    assert gaps.size == rank and gaps.min() >= ir.GAP
    assert len(set(piv[:rank].tolist())) == rank and np.all(piv[:rank] < ir.CASES[name][0])
    assert np.all(piv[rank:] == -1) and np.all(gain[rank:] == 0.0) and np.all(pivvar[rank:] == 0.0)
    if tol == 0.0:
        assert rank == ir.CASES[name][1]


@pytest.mark.parametrize("name,with_r,weighted,tol", ir.STOP_VARIANTS)
def test_stop_cases_have_a_margin(name, with_r, weighted, tol):
    rank, margin = ir.reference(name, with_r, weighted, tol)[4], ir.reference(name, with_r, weighted, tol)[6]
    assert rank == STOP_RANKS[(name, tol)]
    assert rank < ir.CASES[name][1]
    assert margin >= 1e-6


@pytest.mark.parametrize("name,with_r,weighted,tol", ALL)
def test_gain_identity(name, with_r, weighted, tol):
    """imse0 - sum(gain) is the weighted variance of the reference block conditioned directly
    on the picks."""
    S = ir.covariance(name, with_r)
    mc = ir.CASES[name][0]
    w = ir.weights(name, weighted)
    piv, gain, _, imse0, rank, _, _ = ir.reference(name, with_r, weighted, tol)
    left = imse0 - np.sum(gain[:rank])
    direct = ir.conditioned_imse(S, mc, piv[:rank], w)
    rel = abs(left - direct) / direct
    print(name, with_r, weighted, tol, "imse0", imse0, "left", left, "direct", direct, "relative difference", rel)
    assert rel <= 1e-12


def test_brute_force_refit():
    """n60_std, 8 picks: the picks join the training set (any output: the variance does not
    depend on it; beta = 0) and the posterior variance of the reference points is recomputed."""
    name, picks = "n60_std", 8
    c = pr.case(name)
    mc = ir.CASES[name][0]
    piv, gain, _, imse0, rank, _, _ = ir.imse(c["S"], mc, picks)
    assert rank == picks
    cand, ref = c["Xs"][:mc], c["Xs"][mc:]
    X = np.vstack([c["X"], cand[piv]])
    H = np.vstack([c["H"], orc.linear_basis(cand[piv])])
    A, _ = orc.make_A_ref(X, c["delta"], c["nu"], c["kind"], r=None, s2=1.0, predict=True)
    _, V = orc.posterior_ref(X, np.zeros(X.shape[0]), H, A, ref, orc.linear_basis(ref), np.zeros(H.shape[1]),
                             ir.SIGMA, c["delta"], c["nu"], c["kind"])
    refit = np.mean(np.diag(V))
    left = imse0 - np.sum(gain)
    rel = abs(left - refit) / refit
    print("imse0", imse0, "left after 8 picks", left, "refit", refit, "relative difference", rel)
    assert rel <= 1e-8


def test_picks_differ_from_the_maximum_variance_rule():
    differ = []
    for name, (mc, k) in ir.CASES.items():
        S = pr.case(name)["S"]
        piv = ir.reference(name)[0]
        mv = pr.pivchol(S[:mc, :mc], k)[0]
        differ.append(not np.array_equal(piv, mv))
    print("cases whose picks differ from the maximum-variance batch:", differ)
    assert any(differ)


def test_ties_nan_and_the_threshold():
    # two identical candidates: the lowest index wins, and the other's variance falls to 0
    # exactly (every number is a small integer or a power of two): 0 > tol * 4 = 0 fails
    S = np.array([[4.0, 4.0, 0.0, 2.0], [4.0, 4.0, 0.0, 2.0], [0.0, 0.0, 1.0, 0.5], [2.0, 2.0, 0.5, 3.0]])
    piv, gain, pivvar, imse0, rank, _, _ = ir.imse(S, 3, 3)
    assert piv.tolist() == [0, 2, -1] and rank == 2 and imse0 == 3.0
    assert gain.tolist() == [1.0, 0.25, 0.0] and pivvar.tolist() == [4.0, 1.0, 0.0]
    # a NaN score never wins
    S = np.array([[np.nan, 0.0, 1.0], [0.0, 1.0, 0.5], [1.0, 0.5, 2.0]])
    piv, _, _, _, rank, _, _ = ir.imse(S, 2, 2)
    assert piv.tolist() == [1, -1] and rank == 1


def _emulator(dim):
    return types.SimpleNamespace(training=types.SimpleNamespace(inputs=np.zeros((4, dim))))


def test_imse_design_checks_its_arguments():
    """Refused before any device work: more than 16384 points together, k beyond the candidates."""
    E = _emulator(3)
    with pytest.raises(ValueError, match="16384"):
        design_inputs.imse_design(E, np.zeros((16000, 3)), np.zeros((385, 3)), 5)
    with pytest.raises(ValueError, match="k = 41"):
        design_inputs.imse_design(E, np.zeros((40, 3)), np.zeros((60, 3)), 41)
    with pytest.raises(ValueError, match="k = 0"):
        design_inputs.imse_design(E, np.zeros((40, 3)), np.zeros((60, 3)), 0)
    with pytest.raises(ValueError, match="weight"):
        design_inputs.imse_design(E, np.zeros((40, 3)), np.zeros((60, 3)), 5, weights=-np.ones(60))
