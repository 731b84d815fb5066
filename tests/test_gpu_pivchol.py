"""gpe_posterior_pivchol on the GPU against the NumPy reference (tests/pivchol_ref.py, itself
checked against LAPACK's dpstrf and a brute-force greedy design in test_pivchol_host.py).

Bounds.  L L^T against the device's own posterior covariance: 1e-9 of max diag S (the
reference attains 5.3e-12 on these cases; the device sums in another order).  Against the
oracle's S: 1e-8, what the suite holds the posterior to.  Pivots are compared over the first
32 steps, where the reference's top-two gap is >= 1e-6 of max diag S (asserted on the CPU
side), 100x the posterior tolerance.  sum D_PC^2 against e^T S^-1 e: 1e-10 relative
(cond S <= 150 times fp64 epsilon with four orders of margin).
"""
import ctypes
import os
import shutil

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import gp_emu_uqsa_amd as g
import loo_ref
import pivchol_ref as pr
from gp_emu_uqsa_amd import design_inputs, native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(__file__), "golden", "examples")
_I64 = ctypes.POINTER(ctypes.c_int64)


def _factor(ctx, name):
    c = pr.case(name)
    ctx.set_data(c["X"], c["f"], c["H"], c["r"])
    ctx.factor(c["kind"], c["delta"], c["nu"], 1.0, 0.0 if c["r"] is None else 1.0)
    return c


def _rargs(c, with_r):
    return dict(r_new=c["r_new"], r_scale=c["r_scale"]) if with_r else {}


def _pivchol(ctx, c, with_r=False, **kw):
    return ctx.posterior_pivchol(c["Xs"], c["Hs"], c["beta"], pr.SIGMA, **_rargs(c, with_r), **kw)


def _device_cov(ctx, c, with_r=False):
    mean, S = ctx.posterior(c["Xs"], c["Hs"], c["beta"], pr.SIGMA, full_var=True)
    if with_r:
        S = S + np.diag(pr.SIGMA ** 2 * c["r_scale"] * c["r_new"])
    return mean, S


def _check_reconstruction(name, L, S_dev, S_ref):
    scale = np.max(np.diag(S_dev))
    own = np.max(np.abs(L.dot(L.T) - S_dev)) / scale
    print(name, "L L^T against the device covariance", own)
    assert own <= 1e-9
    if S_ref is not None:
        ref = np.max(np.abs(L.dot(L.T) - S_ref)) / np.max(np.diag(S_ref))
        print(name, "L L^T against the oracle covariance", ref)
        assert ref <= 1e-8


@pytest.fixture(scope="module")
def full(ctx):
    """The k = m, tol = 0 call of every variant, with the device's own covariance: computed
    once, shared by the tests below (read-only)."""
    out = {}
    for name, with_r in pr.VARIANTS:
        c = _factor(ctx, name)
        res = _pivchol(ctx, c, with_r)
        mean_dev, S_dev = _device_cov(ctx, c, with_r)
        out[(name, with_r)] = res + (mean_dev, S_dev)
    return out


@pytest.mark.parametrize("name,with_r", pr.VARIANTS)
def test_structure_of_the_full_factor(full, name, with_r):
    mean, piv, pivvar, L, rank, mean_dev, _ = full[(name, with_r)]
    m = pr.CASES[name][0]
    assert rank == m and piv.shape == (m,) and pivvar.shape == (m,) and L.shape == (m, m)
    assert sorted(piv.tolist()) == list(range(m))
    assert np.all(np.diff(pivvar) <= 0.0)          # d only ever decreases: exact
    np.testing.assert_array_equal(L[piv, np.arange(m)], np.sqrt(pivvar))
    assert not np.triu(L[piv], 1).any()            # rows chosen earlier: exactly 0
    assert mean.tobytes() == mean_dev.tobytes()    # the posterior's own mean


@pytest.mark.parametrize("name,with_r", pr.VARIANTS)
def test_reconstructs_the_covariance(full, name, with_r):
    L, S_dev = full[(name, with_r)][3], full[(name, with_r)][6]
    _check_reconstruction(name, L, S_dev, pr.covariance(name, with_r))


@pytest.mark.parametrize("name,with_r", pr.VARIANTS)
def test_first_32_pivots_match_the_reference(full, name, with_r):
    piv, pivvar = full[(name, with_r)][1:3]
    rpiv, rvar = pr.reference(name, with_r)[:2]
    err = np.max(np.abs(pivvar[:32] - rvar[:32])) / rvar[0]
    print(name, with_r, "pivot variance error", err)
    np.testing.assert_array_equal(piv[:32], rpiv[:32])
    assert err <= 1e-8


@pytest.mark.parametrize("name,with_r", pr.VARIANTS)
def test_errors_sum_to_the_mahalanobis_distance(full, name, with_r):
    mean, piv, _, L, _, _, S_dev = full[(name, with_r)]
    e = pr.case(name)["y"] - mean
    dpc = solve_triangular(L[piv], e[piv], lower=True)
    md = e.dot(np.linalg.solve(S_dev, e))
    rel = abs(np.sum(dpc ** 2) - md) / md
    print(name, with_r, "sum D_PC^2", np.sum(dpc ** 2), "Mahalanobis", md, "relative difference", rel)
    assert rel <= 1e-10


@pytest.mark.parametrize("name", ["n300_alt_r", "n1000_std"])
def test_prefix(ctx, name):
    """k = 8: no panel boundary, the same bits as the first 8 steps of k = m on the same
    factor.  k = 129: one trailing update, then one step in the second panel."""
    c = _factor(ctx, name)
    _, fpiv, fvar, fL, _ = _pivchol(ctx, c)
    scale = np.max(fvar)
    for k in (8, 129):
        _, piv, pivvar, L, rank = _pivchol(ctx, c, k=k)
        assert rank == k and L.shape == (fL.shape[0], k)
        np.testing.assert_array_equal(piv, fpiv[:k])
        dv, dl = np.max(np.abs(pivvar - fvar[:k])) / scale, np.max(np.abs(L - fL[:, :k])) / scale
        print(name, k, "difference of pivvar", dv, "of L", dl)
        if k <= 128:
            assert pivvar.tobytes() == fvar[:k].tobytes()
            assert L.tobytes() == np.ascontiguousarray(fL[:, :k]).tobytes()
        else:
            assert dv <= 1e-13 and dl <= 1e-13


@pytest.mark.parametrize("key", sorted(pr.STOP_CASES))
def test_stop_rule(ctx, key):
    """The reference's rank; at the C-ABI the trailing entries are -1 / 0 and the trailing
    columns of L zero."""
    name, tol = key
    c = _factor(ctx, name)
    m = pr.CASES[name][0]
    want = pr.STOP_CASES[key]
    k = m
    Xs, Hs, beta = (np.ascontiguousarray(c[x], dtype=np.float64) for x in ("Xs", "Hs", "beta"))
    mean, pivvar, L = np.zeros(m), np.full(k, 7.0), np.full((m, k), 7.0)
    piv = np.full(k, 7, dtype=np.int64)
    rank = ctypes.c_int64(-5)
    D = native._D
    rc = ctx.lib.gpe_posterior_pivchol(ctx._h, m, Xs.ctypes.data_as(D), Hs.ctypes.data_as(D), beta.ctypes.data_as(D),
                                       pr.SIGMA, None, 0.0, k, tol, mean.ctypes.data_as(D),
                                       piv.ctypes.data_as(_I64), pivvar.ctypes.data_as(D), L.ctypes.data_as(D),
                                       ctypes.byref(rank))
    assert rc == 0
    assert rank.value == want
    rpiv = pr.pivchol(c["S"], None, tol)[0]
    np.testing.assert_array_equal(piv, rpiv)
    assert np.all(piv[want:] == -1) and np.all(pivvar[want:] == 0.0) and np.all(pivvar[:want] > 0.0)
    assert not L[:, want:].any()
    # the wrapper trims to the rank
    _, tpiv, tvar, tL, trank = _pivchol(ctx, c, tol=tol)
    assert trank == want and tpiv.shape == (want,) and tvar.shape == (want,) and tL.shape == (m, want)
    assert tL.tobytes() == np.ascontiguousarray(L[:, :want]).tobytes()
    _, _, _, noL, nrank = _pivchol(ctx, c, tol=tol, want_L=False)
    assert noL is None and nrank == want


def test_repeat_and_workspace(ctx):
    name = "n1000_std"
    c = _factor(ctx, name)
    rs = np.random.RandomState(3)
    m = pr.CASES[name][0]
    t, U = c["y"], rs.standard_normal((4, m))
    post0 = ctx.posterior(c["Xs"], c["Hs"], c["beta"], pr.SIGMA, full_var=True)
    noise0 = ctx.noise_sample(c["Xs"], c["Hs"], c["beta"], pr.SIGMA, t, U)
    a = _pivchol(ctx, c)
    b = _pivchol(ctx, c)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4] == b[4] == m
    post1 = ctx.posterior(c["Xs"], c["Hs"], c["beta"], pr.SIGMA, full_var=True)
    noise1 = ctx.noise_sample(c["Xs"], c["Hs"], c["beta"], pr.SIGMA, t, U)
    for x, y in zip(post0 + noise0, post1 + noise1):
        assert x.tobytes() == y.tobytes()
    # capacity reuse: m = 100 right after m = 700
    small = "n60_std"
    cs = _factor(ctx, small)
    res = _pivchol(ctx, cs)
    assert res[4] == pr.CASES[small][0]
    _check_reconstruction(small, res[3], _device_cov(ctx, cs)[1], cs["S"])


def test_after_a_gradient_objective_and_a_new_factor(ctx):
    name = "n1000_std"
    c = pr.case(name)
    ctx.set_data(c["X"], c["f"], c["H"], c["r"])
    hp = np.concatenate([1.3 * c["delta"], [5e-3, 0.9]])   # other hyperparameters than the factor's
    ctx.objective(native.GP4ML, c["kind"], hp, want_grad=True)
    ctx.factor(c["kind"], c["delta"], c["nu"], 1.0, 0.0)
    res = _pivchol(ctx, c)
    assert res[4] == pr.CASES[name][0]
    _check_reconstruction(name, res[3], _device_cov(ctx, c)[1], c["S"])


def test_design_picks_the_brute_force_batch(ctx):
    c, cand, Hc, picks = pr.design_problem()
    _factor(ctx, pr.DESIGN[0])
    idx, var, _ = pr.brute_force_design(c, cand, picks)
    _, piv, pivvar, L, rank = ctx.posterior_pivchol(cand, Hc, c["beta"], pr.SIGMA, k=picks, want_L=False)
    err = np.max(np.abs(pivvar - var) / var)
    print("picks", piv, "variance error", err)
    assert rank == picks and L is None
    np.testing.assert_array_equal(piv, idx)
    assert err <= 1e-8


def test_public_surface_on_the_toy_sim_example(tmp_path, monkeypatch, capsys):
    d = tmp_path / "toy-sim"
    shutil.copytree(os.path.join(EX, "toy-sim"), d)
    monkeypatch.chdir(d)
    np.random.seed(0)
    E = g.setup("toy-sim_config")
    dim = E.training.inputs.shape[1]
    cand = np.random.RandomState(4).uniform(size=(30, dim))
    idx, cvar = design_inputs.max_variance_design(E, cand, 5)
    var = np.diag(g.posterior(E, cand)[1])
    assert idx.shape == cvar.shape == (5,)
    assert idx[0] == np.argmax(var)
    assert cvar[0] == pytest.approx(var[idx[0]], rel=1e-12)
    assert len(set(idx.tolist())) == 5 and np.all(np.diff(cvar) <= 0.0)
    # the validation diagnostics
    resid = E.post.Dnew.outputs - E.post.mean
    md = resid.dot(np.linalg.solve(E.post.var, resid))
    capsys.readouterr()
    e = E.post.pivoted_cholesky_errors(ise=0)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("  Bad predictions:")]
    m = resid.size
    assert e.shape == (m,) and E.post.rank_pc == m and len(lines) == m
    p0 = E.post.piv[0]
    assert lines[0] == ("  Bad predictions: " + str(E.post.Dnew.inputs[p0, :]) + " pivot: 0 pce: " +
                        str(np.round(e[0], decimals=4)))
    rel = abs(np.sum(e ** 2) - md) / md
    print("sum D_PC^2", np.sum(e ** 2), "Mahalanobis", md, "relative difference", rel)
    assert rel <= 1e-10
    assert E.post.piv[0] == np.argmax(np.diag(E.post.var))
    with pytest.raises(ValueError, match="16384"):
        design_inputs.max_variance_design(E, np.zeros((16385, dim)), 5)


def test_without_a_factor_is_a_state_error():
    c = native.Context(0)
    try:
        X, f, H = orc.synthetic_problem(60, 3, seed=0)
        c.set_data(X, f, H)
        with pytest.raises(RuntimeError,
                           match=r"gpe_posterior_pivchol failed \(-4\): no resident factor \(call gpe_factor\)"):
            c.posterior_pivchol(X[:5], H[:5], np.zeros(4), loo_ref.SIGMA)
    finally:
        c.close()


def test_argument_and_size_errors(ctx):
    c = _factor(ctx, "n60_std")
    m = pr.CASES["n60_std"][0]
    for kw in (dict(k=0), dict(k=m + 1), dict(tol=-1.0)):
        with pytest.raises(RuntimeError, match=r"gpe_posterior_pivchol failed \(-1\)"):
            _pivchol(ctx, c, **kw)
    big = np.zeros((16385, 3))
    with pytest.raises(RuntimeError, match=r"gpe_posterior_pivchol failed \(-5\).*16384"):
        ctx.posterior_pivchol(big, orc.linear_basis(big), c["beta"], pr.SIGMA, k=4)
    # the context is still usable
    assert _pivchol(ctx, c, k=4)[4] == 4
