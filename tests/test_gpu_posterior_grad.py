"""gpe_posterior_grad on the GPU against the dense reference tests/posterior_grad_ref.py
(itself checked against central differences on the CPU in test_posterior_grad_host.py).

Shapes are test_gpu_matern.py's posterior cases and their shared references: (300, 5, 200),
(260, 40, 130) for the d > 32 kernel, (129, 2, 200) with one valid row in the second tile;
ten of the points are training points.  Tolerance: that of test_gpu_matern.test_posterior,
max |error| <= 1e-8 max(1, max |reference|), for d mean and for d var; every case asserts
cond(A) <= 1e6.  mean and var must be the bits of ctx.posterior(full_var=False).
"""
import functools

import numpy as np
import pytest

import matern_ref as mr
import posterior_grad_ref as pgr
import test_gpu_matern as tm
from gp_emu_uqsa_amd import native, synthetic
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
SHAPES = [(300, 5, 200), (260, 40, 130), (129, 2, 200)]
KINDS = pytest.mark.parametrize("kind", [orc.STD, orc.ALT], ids=["std", "alt"])


def errors(dmean, dvar, rmean, rvar):
    em = np.max(np.abs(dmean - rmean)) / max(1.0, np.max(np.abs(rmean)))
    ev = np.max(np.abs(dvar - rvar)) / max(1.0, np.max(np.abs(rvar)))
    return em, ev


@functools.lru_cache(maxsize=None)
def grad_case(family, n, d, m, kind):
    """test_gpu_matern.post_case with the linear basis' derivative and the reference's
    gradients (shared, read-only)."""
    X, f, H = tm.problem(n, d)
    A, beta, Xs, Hs, _, _ = tm.post_case(family, n, d, m, kind)
    dHs, hdim = pgr.linear_basis_deriv(Xs)
    rmean, rvar = pgr.grad(X, f, H, A, Xs, Hs, dHs, hdim, beta, mr.SIGMA, mr.deltas(d), mr.NU[kind], kind, family)
    return tm._frozen(beta, Xs, Hs, dHs, hdim, rmean, rvar)


@KINDS
@pytest.mark.parametrize("n,d,m", SHAPES)
@pytest.mark.parametrize("family", mr.FAMILIES)
def test_parity_and_bits(ctx, family, n, d, m, kind):
    """The gradients against the reference; mean and var the bits of the posterior; a second
    call the same bits; the posterior afterwards the bits it returned before."""
    beta, Xs, Hs, dHs, hdim, rmean, rvar = grad_case(family, n, d, m, kind)
    assert tm.conditioning(family, n, d, kind)[0] <= 1e6
    tm._factor(ctx, family, n, d, kind)
    pm, pv = ctx.posterior(Xs, Hs, beta, mr.SIGMA, full_var=False)
    mean, var, dmean, dvar = ctx.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA)
    em, ev = errors(dmean, dvar, rmean, rvar)
    print(family, n, d, m, kind, "d mean error", em, "d var error", ev, "max |d mean|", np.max(np.abs(rmean)),
          "max |d var|", np.max(np.abs(rvar)))
    assert dmean.shape == dvar.shape == (m, d)
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)
    assert em <= 1e-8 and ev <= 1e-8
    again = ctx.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA)
    for a, b in zip(again, (mean, var, dmean, dvar)):
        assert np.array_equal(a, b)
    pm2, pv2 = ctx.posterior(Xs, Hs, beta, mr.SIGMA, full_var=False)
    assert np.array_equal(pm2, pm) and np.array_equal(pv2, pv)


@pytest.mark.parametrize("n,d,m", SHAPES)
def test_without_the_variance_gradient(ctx, n, d, m):
    family, kind = "matern52", orc.STD
    beta, Xs, Hs, dHs, hdim, rmean, _ = grad_case(family, n, d, m, kind)
    tm._factor(ctx, family, n, d, kind)
    _, _, dmean, dvar = ctx.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA)
    mean0, var0, dmean0, dvar0 = ctx.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA, want_var=False)
    pm, pv = ctx.posterior(Xs, Hs, beta, mr.SIGMA, full_var=False)
    assert dvar0 is None and dvar is not None
    assert np.array_equal(dmean0, dmean)
    assert np.array_equal(mean0, pm) and np.array_equal(var0, pv)


@pytest.mark.parametrize("family", mr.FAMILIES)
def test_more_than_one_chunk(ctx, family):
    """8192 + 130 points: a full chunk and a ragged one through the two-slot pipeline; 200 of
    them, from both chunks and from both ends of each, against the reference."""
    n, d, m, kind = 129, 2, 8192 + 130, orc.ALT
    X, f, H = tm.problem(n, d)
    delta, nu = mr.deltas(d), mr.NU[kind]
    assert tm.conditioning(family, n, d, kind)[0] <= 1e6
    A = mr.make_A(X, delta, nu, kind, family)[0]
    beta = orc.optimal_beta_ref(A, H, f)
    Xs = np.random.RandomState(11).uniform(size=(m, d))
    Xs[8190:8200] = X[:10]   # training points on both sides of the chunk boundary
    Hs = orc.linear_basis(Xs)
    dHs, hdim = pgr.linear_basis_deriv(Xs)
    sel = np.concatenate([np.arange(0, 60), np.arange(8150, 8250), np.arange(m - 40, m)])
    assert sel.size == 200
    rmean, rvar = pgr.grad(X, f, H, A, Xs[sel], Hs[sel], dHs[sel], hdim, beta, mr.SIGMA, delta, nu, kind, family)
    tm._factor(ctx, family, n, d, kind)
    mean, var, dmean, dvar = ctx.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA)
    pm, pv = ctx.posterior(Xs, Hs, beta, mr.SIGMA, full_var=False)
    em, ev = errors(dmean[sel], dvar[sel], rmean, rvar)
    print(family, "two chunks: d mean error", em, "d var error", ev)
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)
    assert em <= 1e-8 and ev <= 1e-8
    assert np.all(np.isfinite(dmean)) and np.all(np.isfinite(dvar))


def test_profiling_counts_the_chunks(ctx):
    """The same two chunks with profiling on: phase_times() slot [1] is the chunk count and
    slot [0] k_post_grad's device time, and the outputs are the bits of the unprofiled call."""
    n, d, m, kind, family = 129, 2, 8192 + 130, orc.ALT, "gaussian"
    Xs = np.random.RandomState(11).uniform(size=(m, d))
    Hs = orc.linear_basis(Xs)
    dHs, hdim = pgr.linear_basis_deriv(Xs)
    tm._factor(ctx, family, n, d, kind)
    beta = ctx.beta()
    plain = ctx.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA)
    ctx.set_profiling(True)
    try:
        timed = ctx.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA)
        times = ctx.phase_times()
    finally:
        ctx.set_profiling(False)
    print("chunks", times["cholesky"], "k_post_grad ms", times["kbuild"])
    assert times["cholesky"] == 2 and times["kbuild"] > 0.0      # slots [1] and [0]
    for a, b in zip(timed, plain):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("family", mr.FAMILIES)
def test_with_r(ctx, family):
    """The alt kernel with r on the diagonal of the resident A (r_scale = 1)."""
    n, d, m, kind = 300, 5, 200, orc.ALT
    X, f, H = tm.problem(n, d)
    r = tm.r_of(n)
    delta, nu = mr.deltas(d), mr.NU[kind]
    A = mr.make_A(X, delta, nu, kind, family, r=r, s2=1.0)[0]
    assert np.linalg.cond(A) <= 1e6
    beta = orc.optimal_beta_ref(A, H, f)
    _, Xs, Hs, dHs, hdim, _, _ = grad_case(family, n, d, m, kind)
    rmean, rvar = pgr.grad(X, f, H, A, Xs, Hs, dHs, hdim, beta, mr.SIGMA, delta, nu, kind, family)
    tm._factor(ctx, family, n, d, kind, r)
    mean, var, dmean, dvar = ctx.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA)
    pm, pv = ctx.posterior(Xs, Hs, beta, mr.SIGMA, full_var=False)
    em, ev = errors(dmean, dvar, rmean, rvar)
    print(family, "with r: d mean error", em, "d var error", ev)
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)
    assert em <= 1e-8 and ev <= 1e-8


def _basis_case(ctx, family, kind, H_of, dH_of, hdim):
    n, d, m = 300, 3, 200
    X, f, _ = tm.problem(n, d)
    H = H_of(X)
    delta, nu = mr.deltas(d), mr.NU[kind]
    A = mr.make_A(X, delta, nu, kind, family)[0]
    assert np.linalg.cond(A) <= 1e6
    beta = orc.optimal_beta_ref(A, H, f)
    Xs = orc.olhc_design(m, d, 4)
    Xs[:10] = X[:: n // 10][:10]
    Hs, dHs = H_of(Xs), dH_of(Xs)
    hdim = np.array(hdim, dtype=np.int32)
    rmean, rvar = pgr.grad(X, f, H, A, Xs, Hs, dHs, hdim, beta, mr.SIGMA, delta, nu, kind, family)
    ctx.set_data(X, f, H)
    ctx.factor(tm.code(family, kind), delta, nu, 1.0, 0.0)
    mean, var, dmean, dvar = ctx.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA)
    pm, pv = ctx.posterior(Xs, Hs, beta, mr.SIGMA, full_var=False)
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)
    return errors(dmean, dvar, rmean, rvar)


@KINDS
@pytest.mark.parametrize("family", mr.FAMILIES)
def test_basis_columns_sharing_an_input(ctx, family, kind):
    """H = [1, x0, x0^2, cos(x1), x2]: two columns on input 0."""
    def H_of(X):
        return np.stack([np.ones(len(X)), X[:, 0], X[:, 0] ** 2, np.cos(X[:, 1]), X[:, 2]], axis=1)

    def dH_of(X):
        return np.stack([np.zeros(len(X)), np.ones(len(X)), 2.0 * X[:, 0], -np.sin(X[:, 1]), np.ones(len(X))], axis=1)
    em, ev = _basis_case(ctx, family, kind, H_of, dH_of, [-1, 0, 0, 1, 2])
    print(family, kind, "shared input: d mean error", em, "d var error", ev)
    assert em <= 1e-8 and ev <= 1e-8


@pytest.mark.parametrize("family", mr.FAMILIES)
def test_constant_basis_alone(ctx, family):
    """H = [1], q = 1: no basis term in either gradient."""
    em, ev = _basis_case(ctx, family, orc.STD, lambda X: np.ones((len(X), 1)), lambda X: np.zeros((len(X), 1)), [-1])
    print(family, "constant basis: d mean error", em, "d var error", ev)
    assert em <= 1e-8 and ev <= 1e-8


@pytest.mark.parametrize("family", ["gaussian", "matern52"])
def test_int8_v_path(monkeypatch, family):
    """n = 4096: V = L^-1 K* comes from the int8 cores under the default settings and from the
    fp64 GEMM under GPEMU_OZAKI=0 (as test_posterior_int8_matches_fp64 sets them up, with its
    threshold override); U = L^-T V is an fp64 product either way.  Both against the reference.
    cond(A) <= (largest row sum) / nu for the std kernel, A = (1 - nu) R + nu I with R positive
    semi-definite: asserted <= 1e6 from that bound (an SVD of 4096^2 would take longer than
    the rest of the test)."""
    n, d, m, kind, nu, sigma = 4096, 3, 300, orc.STD, 1e-2, 0.9
    X, f, H = synthetic.problem(n, d, seed=5)
    delta = np.full(d, 0.2)
    A = mr.make_A(X, delta, nu, kind, family)[0]
    assert np.max(np.sum(np.abs(A), axis=1)) / nu <= 1e6
    beta = pgr.gls_beta(A, H, f)
    Xs = synthetic.design(m, d, seed=8)
    Xs[:10] = X[:: n // 10][:10]
    Hs = synthetic.linear_basis(Xs)
    dHs, hdim = pgr.linear_basis_deriv(Xs)
    rmean, rvar = pgr.grad(X, f, H, A, Xs, Hs, dHs, hdim, beta, sigma, delta, nu, kind, family)
    monkeypatch.setenv("GPEMU_OZAKI_MIN_NP", "2048")   # (the int8 product's default start: 4096)
    for oz in (None, "0"):
        if oz is None:
            monkeypatch.delenv("GPEMU_OZAKI", raising=False)
        else:
            monkeypatch.setenv("GPEMU_OZAKI", oz)
        c = native.Context(0)
        c.set_data(X, f, H)
        c.factor(tm.code(family, kind), delta, nu, 1.0, 0.0)
        mean, var, dmean, dvar = c.posterior_grad(Xs, Hs, dHs, hdim, beta, sigma)
        pm, pv = c.posterior(Xs, Hs, beta, sigma, full_var=False)
        c.close()
        em, ev = errors(dmean, dvar, rmean, rvar)
        print(family, "GPEMU_OZAKI", oz, "d mean error", em, "d var error", ev, "max |d mean|",
              np.max(np.abs(rmean)), "max |d var|", np.max(np.abs(rvar)))
        assert np.array_equal(mean, pm) and np.array_equal(var, pv)
        assert em <= 1e-8 and ev <= 1e-8


def test_errors(ctx):
    n, d, m = 129, 2, 200
    X, f, H = tm.problem(n, d)
    beta, Xs, Hs, dHs, hdim, _, _ = grad_case("gaussian", n, d, m, orc.STD)
    c = native.Context(0)
    c.set_data(X, f, H)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):   # GPE_ERR_STATE: no resident factor
        c.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA)
    c.close()
    tm._factor(ctx, "gaussian", n, d, orc.STD)
    for bad in (d, -2):
        h = hdim.copy()
        h[1] = bad
        with pytest.raises(RuntimeError, match=r"\(-1\)"):   # GPE_ERR_ARG
            ctx.posterior_grad(Xs, Hs, dHs, h, beta, mr.SIGMA)
    # the factor is still usable
    mean, var, _, _ = ctx.posterior_grad(Xs, Hs, dHs, hdim, beta, mr.SIGMA)
    pm, pv = ctx.posterior(Xs, Hs, beta, mr.SIGMA, full_var=False)
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)
