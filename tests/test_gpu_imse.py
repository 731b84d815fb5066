"""gpe_posterior_imse on the GPU against the NumPy reference (tests/imse_ref.py, itself checked
against a direct conditioning and a brute-force refit in test_imse_host.py).

Bounds.  Against the reference run on the device's own covariance only the order of the sums
differs: picks equal, gains and pick variances within 1e-11 relative (the reference's own
rounding against an extended-precision replay is <= 2.5e-15 in the gains), imse0 within 1e-13.
A step whose score gap on the device covariance is below 1e-6 ends the compared prefix, which
must cover min(32, rank) steps (two of the cases have fewer than 32 steps).  Against the
oracle's covariance, which the device's matches to 1e-8 of its scale: the same picks over the
first min(32, rank) steps and gains within 1e-5 relative.
The gain identity on the device covariance (the API tests, 8 picks): 1e-10 relative.  The
identity holds to 1e-12 for the reference, the device's gains are within 1e-11 of the
reference's, and imse0 - sum(gain) keeps more than half of imse0 after 8 picks, so the
cancellation at most doubles those.
"""
import ctypes
import os
import shutil

import numpy as np
import pytest

import gp_emu_uqsa_amd as g
import imse_ref as ir
import loo_ref
import pivchol_ref as pr
from gp_emu_uqsa_amd import design_inputs, native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(__file__), "golden", "examples")
_I64 = ctypes.POINTER(ctypes.c_int64)
ALL = ir.VARIANTS + ir.STOP_VARIANTS
STOP_RANKS = {("n300_alt_r", 0.5): 72, ("n1000_std", 0.5): 10, ("n1000_std", 0.3): 36}


def _factor(ctx, name):
    c = pr.case(name)
    ctx.set_data(c["X"], c["f"], c["H"], c["r"])
    ctx.factor(c["kind"], c["delta"], c["nu"], 1.0, 0.0 if c["r"] is None else 1.0)
    return c


def _rargs(c, with_r):
    return dict(r_new=c["r_new"], r_scale=c["r_scale"]) if with_r else {}


def _imse(ctx, c, name, with_r=False, weighted=False, tol=0.0, k=None):
    mc, kk = ir.CASES[name]
    return ctx.posterior_imse(c["Xs"], c["Hs"], c["beta"], pr.SIGMA, mc, kk if k is None else k,
                              w=ir.weights(name, weighted), tol=tol, **_rargs(c, with_r))


def _device_cov(ctx, c, with_r=False):
    mean, S = ctx.posterior(c["Xs"], c["Hs"], c["beta"], pr.SIGMA, full_var=True)
    if with_r:
        S = S + np.diag(pr.SIGMA ** 2 * c["r_scale"] * c["r_new"])
    return mean, S


@pytest.fixture(scope="module")
def runs(ctx):
    """Every variant's call, the device's own covariance and the reference run on it: computed
    once, shared by the tests below (read-only)."""
    out = {}
    for key in ALL:
        name, with_r, weighted, tol = key
        c = _factor(ctx, name)
        res = _imse(ctx, c, name, with_r, weighted, tol)
        mean_dev, S_dev = _device_cov(ctx, c, with_r)
        mc, k = ir.CASES[name]
        ref = ir.imse(S_dev, mc, k, ir.weights(name, weighted), tol)
        out[key] = (res, mean_dev, S_dev, ref)
    return out


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b))) if len(b) else 0.0


@pytest.mark.parametrize("key", ALL)
def test_picks_and_gains_on_the_device_covariance(runs, key):
    (mean, piv, gain, pivvar, imse0, rank), _, _, ref = runs[key]
    rpiv, rgain, rvar, rimse0, rrank, rgaps, _ = ref
    n = pr.safe_prefix(rgaps, ir.GAP)
    eg, ev, e0 = _rel(gain[:n], rgain[:n]), _rel(pivvar[:n], rvar[:n]), abs(imse0 - rimse0) / rimse0
    print(key, "rank", rank, rrank, "compared prefix", n, "gain error", eg, "variance error", ev, "imse0 error", e0)
    assert n >= min(32, rrank)
    np.testing.assert_array_equal(piv[:n], rpiv[:n])
    if n == rrank:
        assert rank == rrank and piv.shape == gain.shape == pivvar.shape == (rank,)
    assert eg <= 1e-11 and ev <= 1e-11
    assert e0 <= 1e-13


@pytest.mark.parametrize("key", ALL)
def test_first_picks_match_the_reference_on_the_oracle_covariance(runs, key):
    name, with_r, weighted, tol = key
    _, piv, gain = runs[key][0][:3]
    rpiv, rgain, _, _, rrank, _, _ = ir.reference(name, with_r, weighted, tol)
    n = min(32, rrank)
    eg = _rel(gain[:n], rgain[:n])
    print(key, "gain error against the oracle covariance", eg)
    np.testing.assert_array_equal(piv[:n], rpiv[:n])
    assert eg <= 1e-5


@pytest.mark.parametrize("key", ALL)
def test_structure(runs, key):
    name = key[0]
    (mean, piv, gain, pivvar, imse0, rank), mean_dev, S_dev, _ = runs[key]
    mc = ir.CASES[name][0]
    assert len(set(piv.tolist())) == rank and np.all(piv >= 0) and np.all(piv < mc)
    assert mean.tobytes() == mean_dev.tobytes()    # the posterior's own mean
    print(key, "pivvar[0]", repr(pivvar[0]), "device diagonal", repr(S_dev[piv[0], piv[0]]))
    if key[1]:
        # with r_new the device forms sigma^2 r_scale r_new inside its covariance kernel, and no
        # call returns that matrix: S_dev carries the term added on the host, in another order
        # (measured: 3.8e-15 relative apart).  Only the rounding of that one sum differs.
        assert abs(pivvar[0] - S_dev[piv[0], piv[0]]) <= 1e-13 * pivvar[0]
    else:
        assert pivvar[0] == S_dev[piv[0], piv[0]]      # bit for bit
    assert np.all(gain > 0.0) and np.all(pivvar > 0.0) and imse0 - gain.sum() > 0.0
    if name == "n129_std":
        assert rank == mc and sorted(piv.tolist()) == list(range(mc))


def test_prefix(ctx):
    """k = 8: the bits of the first 8 steps of the k = 140 call on the same factor."""
    name = "n300_alt_r"
    c = _factor(ctx, name)
    full = _imse(ctx, c, name)
    assert full[5] == 140
    mean, piv, gain, pivvar, imse0, rank = _imse(ctx, c, name, k=8)
    assert rank == 8
    np.testing.assert_array_equal(piv, full[1][:8])
    assert gain.tobytes() == full[2][:8].tobytes() and pivvar.tobytes() == full[3][:8].tobytes()
    assert imse0 == full[4] and mean.tobytes() == full[0].tobytes()


def test_repeat_and_the_resident_factor(ctx):
    name = "n1000_std"
    c = _factor(ctx, name)
    post0 = ctx.posterior(c["Xs"], c["Hs"], c["beta"], pr.SIGMA, full_var=True)
    a = _imse(ctx, c, name, weighted=True)
    b = _imse(ctx, c, name, weighted=True)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4:] == b[4:] and a[5] == ir.CASES[name][1]
    post1 = ctx.posterior(c["Xs"], c["Hs"], c["beta"], pr.SIGMA, full_var=True)
    for x, y in zip(post0, post1):
        assert x.tobytes() == y.tobytes()
    # capacity reuse: m = 100 right after m = 700, and the pivoted Cholesky that shares the panel
    small = "n60_std"
    cs = _factor(ctx, small)
    res = _imse(ctx, cs, small)
    ref = ir.imse(_device_cov(ctx, cs)[1], *ir.CASES[small])
    np.testing.assert_array_equal(res[1], ref[0])
    assert ctx.posterior_pivchol(cs["Xs"], cs["Hs"], cs["beta"], pr.SIGMA, k=8, want_L=False)[4] == 8


@pytest.mark.parametrize("key", ir.STOP_VARIANTS)
def test_stop_rule(ctx, runs, key):
    """The reference's rank; at the C-ABI the trailing entries are -1 / 0 / 0."""
    name, with_r, weighted, tol = key
    want = STOP_RANKS[(name, tol)]
    assert runs[key][3][4] == want and runs[key][0][5] == want
    c = _factor(ctx, name)
    m = pr.CASES[name][0]
    mc, k = ir.CASES[name]
    Xs, Hs, beta = (np.ascontiguousarray(c[x], dtype=np.float64) for x in ("Xs", "Hs", "beta"))
    mean, gain, pivvar = np.zeros(m), np.full(k, 7.0), np.full(k, 7.0)
    piv = np.full(k, 7, dtype=np.int64)
    rank, imse0 = ctypes.c_int64(-5), ctypes.c_double(-1.0)
    D = native._D
    rc = ctx.lib.gpe_posterior_imse(ctx._h, m, mc, Xs.ctypes.data_as(D), Hs.ctypes.data_as(D), beta.ctypes.data_as(D),
                                    pr.SIGMA, None, 0.0, None, k, tol, mean.ctypes.data_as(D),
                                    piv.ctypes.data_as(_I64), gain.ctypes.data_as(D), pivvar.ctypes.data_as(D),
                                    ctypes.byref(imse0), ctypes.byref(rank))
    assert rc == 0 and rank.value == want
    np.testing.assert_array_equal(piv[:want], runs[key][0][1])
    assert np.all(piv[want:] == -1) and np.all(gain[want:] == 0.0) and np.all(pivvar[want:] == 0.0)
    assert np.all(gain[:want] > 0.0) and np.all(pivvar[:want] > 0.0)
    assert imse0.value == runs[key][0][4]


def test_without_a_factor_is_a_state_error():
    c = native.Context(0)
    try:
        X, f, H = orc.synthetic_problem(60, 3, seed=0)
        c.set_data(X, f, H)
        with pytest.raises(RuntimeError,
                           match=r"gpe_posterior_imse failed \(-4\): no resident factor \(call gpe_factor\)"):
            c.posterior_imse(X[:8], H[:8], np.zeros(4), loo_ref.SIGMA, 5, 2)
    finally:
        c.close()


def test_argument_and_size_errors(ctx):
    name = "n60_std"
    c = _factor(ctx, name)
    m = pr.CASES[name][0]
    mc = ir.CASES[name][0]
    args = (c["Xs"], c["Hs"], c["beta"], pr.SIGMA)
    bad_w = np.full(m - mc, 1.0)
    bad_w[5] = -1e-3
    nan_w = np.full(m - mc, 1.0)
    nan_w[0] = np.nan
    for a, kw in (((m, 4), {}), ((0, 1), {}), ((mc, mc + 1), {}), ((mc, 0), {}), ((mc, 4), dict(tol=-1.0)),
                  ((mc, 4), dict(w=bad_w)), ((mc, 4), dict(w=nan_w))):
        with pytest.raises(RuntimeError, match=r"gpe_posterior_imse failed \(-1\)"):
            ctx.posterior_imse(*args, *a, **kw)
    big = np.zeros((16385, 3))
    with pytest.raises(RuntimeError, match=r"gpe_posterior_imse failed \(-5\).*16384"):
        ctx.posterior_imse(big, orc.linear_basis(big), c["beta"], pr.SIGMA, 16000, 4)
    # the context is still usable
    assert _imse(ctx, c, name, k=4)[5] == 4


def _toy_sim(tmp_path, monkeypatch, extra=None):
    d = tmp_path / "toy-sim"
    shutil.copytree(os.path.join(EX, "toy-sim"), d)
    monkeypatch.chdir(d)
    if extra:
        with open("toy-sim_beliefs", "a") as fh:
            fh.write(extra)
    np.random.seed(0)
    E = g.setup("toy-sim_config")
    dim = E.training.inputs.shape[1]
    rs = np.random.RandomState(4)
    return E, rs.uniform(size=(40, dim)), rs.uniform(size=(60, dim))


def _check_gain_identity(S, mc, idx, gains, imse0, w=None):
    left = imse0 - np.sum(gains)
    direct = ir.conditioned_imse(S, mc, idx, w)
    rel = abs(left - direct) / direct
    print("imse0", imse0, "left", left, "conditioned directly", direct, "relative difference", rel)
    assert left > 0.5 * imse0
    assert rel <= 1e-10


def test_imse_design_on_the_toy_sim_example(tmp_path, monkeypatch):
    E, cand, ref = _toy_sim(tmp_path, monkeypatch)
    idx, gains, imse0 = design_inputs.imse_design(E, cand, ref, 8)
    S = g.posterior(E, np.vstack([cand, ref]))[1]
    rpiv, rgain, _, rimse0, rrank, rgaps, _ = ir.imse(S, 40, 8, None, 1e-8)
    print("picks", idx, "reference", rpiv, "smallest gap", rgaps.min(), "gain error", _rel(gains, rgain))
    assert rrank == 8 and rgaps.min() >= ir.GAP
    assert idx.shape == gains.shape == (8,)
    np.testing.assert_array_equal(idx, rpiv)
    assert _rel(gains, rgain) <= 1e-11 and abs(imse0 - rimse0) <= 1e-13 * rimse0
    # weighted, and the maximum-variance rule beside it
    w = np.random.RandomState(31).uniform(0.0, 1.0, 60)
    idx_w, gains_w, imse0_w = design_inputs.imse_design(E, cand, ref, 8, weights=w / w.sum())
    _check_gain_identity(S, 40, idx_w, gains_w, imse0_w, w / w.sum())
    with pytest.raises(ValueError, match="16384"):
        design_inputs.imse_design(E, np.zeros((16000, cand.shape[1])), np.zeros((385, cand.shape[1])), 5)
    with pytest.raises(ValueError, match="k = 41"):
        design_inputs.imse_design(E, cand, ref, 41)


def test_imse_design_with_a_matern52_emulator(tmp_path, monkeypatch):
    from gp_emu_uqsa_amd import kernels
    E, cand, ref = _toy_sim(tmp_path, monkeypatch, "kernel matern52\n")
    assert type(E.K) is kernels.kernel_matern52
    idx, gains, imse0 = design_inputs.imse_design(E, cand, ref, 8)
    assert len(set(idx.tolist())) == 8 and np.all(idx < 40)
    S = g.posterior(E, np.vstack([cand, ref]))[1]
    _check_gain_identity(S, 40, idx, gains, imse0)
