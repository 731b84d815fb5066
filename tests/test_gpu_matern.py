"""The Matern 3/2 and 5/2 correlation families on the GPU against the dense NumPy reference
(tests/matern_ref.py, itself checked on the CPU in test_matern_host.py).

Shapes: 129 is two tiles with one valid row in the second, d = 10 the k_contract<10, 13>
instantiation, d = 40 the _wide kernels, 520 five tile rows with csplit off.  A Matern
objective takes the general path at every n (the one-launch paths are Gaussian only).

Tolerances are those of test_gpu_objective.py: LLH max(1e-10, 4 eps cond(A)) relative,
gradient 1e-7 (|g_ref| + max |g_ref|), sigma^2 1e-10 relative, value-only against gradient
LLH 1e-12 relative.  Every case asserts cond(A) <= 1e6 and a median off-diagonal correlation
>= 0.05 of its own inputs, so the cond term cannot widen silently and no case compares zeros.
Kernel matrices: 4e-15 absolute for rho <= 1, the bound the Gaussian ones are held to.
Posterior: 1e-8 (max(1, max |v|)); precision 32 within 2e-5 sigma^2 of precision 64.
"""
import functools
import glob
import os
import shutil

import numpy as np
import pytest

import gp_emu_uqsa_amd as g
import loo_ref
import matern_ref as mr
import pivchol_ref as pr
from gp_emu_uqsa_amd import files, kernels, native, sensitivity
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(__file__), "golden", "examples")
EPS = np.finfo(float).eps
MATERN = ["matern32", "matern52"]
# (kind, variant): MUCM with the std nugget only (the beliefs refuse mucm with alt_nugget)
KV = [(orc.STD, orc.GP4ML), (orc.ALT, orc.GP4ML), (orc.STD, orc.MUCM)]
GAP = 1e-6   # as test_pivchol_host.py: pivots are compared where the top two variances differ by this


def code(family, kind):
    return mr.FAMILY_CODE[family] | kind


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def problem(n, d, coincident=False):
    """(X, f, H) of a shape (shared, read-only); coincident: row 7 copied over row 250 and
    row 3 over row 131, a pair inside one tile column and a pair that straddles tiles."""
    X, f, H = orc.synthetic_problem(n, d, seed=9)
    if coincident:
        X = X.copy()
        X[250] = X[7]
        X[131] = X[3]
        H = orc.linear_basis(X)
    return _frozen(X, f, H)


@functools.lru_cache(maxsize=None)
def r_of(n):
    return _frozen(np.random.RandomState(5).uniform(0, 0.02, n))[0]


@functools.lru_cache(maxsize=None)
def conditioning(family, n, d, kind, coincident=False):
    """(cond(A), median off-diagonal rho) of a case's correlation matrix."""
    X = problem(n, d, coincident)[0]
    A, rho, _ = mr.kernel_var(X, mr.deltas(d), mr.NU[kind], kind, family)
    return float(np.linalg.cond(A)), float(np.median(rho))


@functools.lru_cache(maxsize=None)
def ref_objective(family, n, d, kind, variant, fit, with_r=False, coincident=False):
    """matern_ref.objective of a case (shared, read-only)."""
    X, f, H = problem(n, d, coincident)
    hp = mr.hyperparams(d, variant, kind, fit)
    out = mr.objective(X, f, H, hp, variant, kind, fit, family, r=r_of(n) if with_r else None,
                       nu_fixed=mr.NU[kind])
    _frozen(*out)
    return out


def check_objective(ctx, family, n, d, kind, variant, fit, with_r=False, coincident=False):
    X, f, H = problem(n, d, coincident)
    cond, med = conditioning(family, n, d, kind, coincident)
    assert cond <= 1e6 and med >= 0.05
    rtol = max(1e-10, 4 * EPS * cond)
    hp = mr.hyperparams(d, variant, kind, fit)
    rl, rg, rs2 = ref_objective(family, n, d, kind, variant, fit, with_r, coincident)
    ctx.set_data(X, f, H, r_of(n) if with_r else None)
    llh, grad, s2 = ctx.objective(variant, code(family, kind), hp, nu_fixed=mr.NU[kind], want_grad=True)
    vllh, vgrad, vs2 = ctx.objective(variant, code(family, kind), hp, nu_fixed=mr.NU[kind], want_grad=False)
    gerr = np.abs(grad - rg) / (np.abs(rg) + np.max(np.abs(rg)))
    print(family, n, d, kind, variant, fit, "cond", cond, "LLH error", abs(llh - rl) / abs(rl),
          "value-only", abs(vllh - rl) / abs(rl), "gradient error", np.max(gerr),
          "sigma^2 error", abs(s2 - rs2) / abs(rs2))
    assert np.isfinite(llh) and np.all(np.isfinite(grad))
    assert abs(llh - rl) <= rtol * abs(rl)
    assert abs(vllh - rl) <= rtol * abs(rl)
    assert np.max(gerr) <= 1e-7
    assert abs(s2 - rs2) <= 1e-10 * abs(rs2) and abs(vs2 - rs2) <= 1e-10 * abs(rs2)
    assert vgrad is None
    assert abs(vllh - llh) <= 1e-12 * abs(llh)


@pytest.mark.parametrize("fit", [True, False], ids=["fit", "fixed"])
@pytest.mark.parametrize("kind,variant", KV, ids=["std-gp4ml", "alt-gp4ml", "std-mucm"])
@pytest.mark.parametrize("n,d", mr.SHAPES)
@pytest.mark.parametrize("family", MATERN)
def test_objective(ctx, family, n, d, kind, variant, fit):
    """LLH, gradient and sigma^2, with the gradient and value only."""
    check_objective(ctx, family, n, d, kind, variant, fit)


@pytest.mark.parametrize("kind", [orc.STD, orc.ALT], ids=["std", "alt"])
@pytest.mark.parametrize("family", MATERN)
def test_objective_with_r(ctx, family, kind):
    """r set: on the diagonal of A for the alt nugget, in the sigma gradient for both."""
    check_objective(ctx, family, 300, 5, kind, orc.GP4ML, True, with_r=True)


@pytest.mark.parametrize("kind", [orc.STD, orc.ALT], ids=["std", "alt"])
@pytest.mark.parametrize("family", MATERN)
def test_coincident_points(ctx, family, kind):
    """s = 0 off the diagonal: rho = 1 and g = 3/2 or 5/6 there, nothing divides by r."""
    check_objective(ctx, family, 300, 5, kind, orc.GP4ML, True, coincident=True)


@pytest.mark.parametrize("family", MATERN)
def test_duplicated_rows_without_a_nugget_are_not_positive_definite(ctx, family):
    """Two equal rows with nu = 0: A is exactly singular and the dense reference returns None.

    The copied row's pivot is zero in exact arithmetic and a rounding residue of either sign
    in fp64 (without the pivot floor the device returned a finite LLH = 2.85e15 for matern32
    and stopped at pivot 132 for matern52), so the Matern families hold every pivot against
    4 n_pad eps of its diagonal entry (k_pivot_floor): the lower copy of the first pair,
    row 131, is reported."""
    X, f, H = problem(300, 5, True)
    hp = mr.hyperparams(5, orc.GP4ML, orc.STD, False)
    assert mr.objective(X, f, H, hp, orc.GP4ML, orc.STD, False, family, nu_fixed=0.0) is None
    ctx.set_data(X, f, H)
    try:
        got = ctx.objective(orc.GP4ML, code(family, orc.STD), hp, nu_fixed=0.0)
    except native.NotPositiveDefinite as e:
        got = None
        print(family, "raised:", e)
    print(family, "objective with two pairs of equal rows and nu = 0:", got)
    assert got is None, "did not raise NotPositiveDefinite"
    with pytest.raises(native.NotPositiveDefinite, match=r"pivot 132\)"):
        ctx.objective(orc.GP4ML, code(family, orc.STD), hp, nu_fixed=0.0, want_grad=False)
    with pytest.raises(native.NotPositiveDefinite, match=r"pivot 132\)"):
        ctx.factor(code(family, orc.STD), hp[:5], 0.0, 1.0, 0.0)


@pytest.mark.parametrize("family", MATERN)
def test_zero_length_scale_is_not_positive_definite(ctx, family):
    """The reference's covariance is NaN there."""
    X, f, H = problem(300, 5)
    ctx.set_data(X, f, H)
    hp = mr.hyperparams(5, orc.GP4ML, orc.STD, True)
    hp[0] = 0.0
    for want_grad in (True, False):
        with pytest.raises(native.NotPositiveDefinite):
            ctx.objective(orc.GP4ML, code(family, orc.STD), hp, want_grad=want_grad)
    with pytest.raises(native.NotPositiveDefinite):
        ctx.factor(code(family, orc.STD), hp[:5], 1e-3, 1.0, 0.0)


KSHAPES = [(129, 2), (200, 10), (260, 40)]


@pytest.mark.parametrize("kind", [orc.STD, orc.ALT], ids=["std", "alt"])
@pytest.mark.parametrize("n,d", KSHAPES)
@pytest.mark.parametrize("family", MATERN)
def test_kernel_matrices(ctx, family, n, d, kind):
    """gpe_kernel_var (predict T / F), gpe_kernel_covar and gpe_kernel_grad_k."""
    X = problem(n, d)[0]
    delta, nu, k = mr.deltas(d), mr.NU[kind], code(family, kind)
    assert conditioning(family, n, d, kind)[1] >= 0.05
    for predict in (True, False):
        A = ctx.kernel_var(k, delta, nu, X, predict=predict)
        err = np.max(np.abs(A - mr.kernel_var(X, delta, nu, kind, family, predict)[0]))
        print(family, n, d, kind, "kernel_var predict", predict, err)
        assert err <= 4e-15
    XV = orc.olhc_design(70, d, 3)
    C = ctx.kernel_covar(k, delta, nu, X, XV)
    err = np.max(np.abs(C - mr.kernel_covar(X, XV, delta, nu, kind, family)))
    print(family, n, d, kind, "kernel_covar", err)
    assert C.shape == (n, 70) and err <= 4e-15
    pre = 1.0 if kind == orc.ALT else 1.0 - nu
    G = ctx.kernel_grad_k(k, delta, X, X[:, 1], 1.0 / delta[1], pre)
    err = np.max(np.abs(G - mr.kernel_grad(X, delta, X[:, 1], 1.0 / delta[1], pre, family)))
    print(family, n, d, kind, "kernel_grad_k with a column", err)
    assert err <= 4e-15 and not np.diag(G).any()
    G = ctx.kernel_grad_k(k, delta, X, None, 0.0, -0.7)
    err = np.max(np.abs(G - mr.kernel_grad(X, delta, None, 0.0, -0.7, family)))
    print(family, n, d, kind, "kernel_grad_k without a column", err)
    assert err <= 4e-15 and not np.diag(G).any()


@pytest.mark.parametrize("n,d", [(129, 2), (260, 40)])
def test_kernel_grad_k_gaussian_is_kernel_grad(ctx, n, d):
    X = problem(n, d)[0]
    delta = mr.deltas(d)
    for col, scale, pre in ((X[:, 1], 1.0 / delta[1], 0.999), (None, 0.0, -0.0005)):
        old = ctx.kernel_grad(delta, X, col, scale, pre)
        for kind in (native.KERNEL_STD, native.KERNEL_ALT_NUG):
            assert ctx.kernel_grad_k(kind, delta, X, col, scale, pre).tobytes() == old.tobytes()
        assert old.any()


def test_python_kernel_classes(ctx):
    """var / covar / grad_delta_A / grad_nugget_A of the classes against the reference's forms."""
    X = problem(129, 2)[0]
    delta, s2 = mr.deltas(2), 1.3 ** 2
    for family, alt, cls in (("matern32", False, kernels.kernel_matern32),
                             ("matern52", True, kernels.kernel_matern52_alt_nug)):
        kind = orc.ALT if alt else orc.STD
        nu = mr.NU[kind]
        K = cls(2, type("par", (), dict(delta=delta, nugget=nu)))
        A, rho, gg = mr.kernel_var(X, delta, nu, kind, family)
        assert np.max(np.abs(K.var(X) - A)) <= 4e-15
        assert np.max(np.abs(K.covar(X, X[:50]) - mr.kernel_covar(X, X[:50], delta, nu, kind, family))) <= 4e-15
        ref = orc.grad_delta_ref(X[:, 1], delta[1], nu, gg, s2, kind)
        assert np.max(np.abs(K.grad_delta_A(X[:, 1], 1, s2) - ref)) <= 4e-15 * s2
        ref = orc.grad_nugget_ref(129, nu, rho, s2, kind)
        assert np.max(np.abs(K.grad_nugget_A(X, s2) - ref)) <= 4e-15 * s2


@pytest.mark.parametrize("call", ["objective", "factor", "kernel_var", "kernel_covar", "kernel_grad_k"])
@pytest.mark.parametrize("bad", [0x30, 0x31, 0x40, 2, 0x12])
def test_unknown_kernel_codes_are_argument_errors(ctx, call, bad):
    X, f, H = problem(129, 2)
    ctx.set_data(X, f, H)
    delta = mr.deltas(2)
    with pytest.raises(RuntimeError, match=r"failed \(-1\): bad kernel"):
        if call == "objective":
            ctx.objective(orc.GP4ML, bad, mr.hyperparams(2, orc.GP4ML, orc.STD, True))
        elif call == "factor":
            ctx.factor(bad, delta, 1e-3, 1.0, 0.0)
        elif call == "kernel_var":
            ctx.kernel_var(bad, delta, 1e-3, X)
        elif call == "kernel_covar":
            ctx.kernel_covar(bad, delta, 1e-3, X, X[:5])
        else:
            ctx.kernel_grad_k(bad, delta, X, None, 0.0, 1.0)


# ---- through the resident factor ---------------------------------------------------------
POST = [(300, 5, 200), (260, 40, 130)]


@functools.lru_cache(maxsize=None)
def post_case(family, n, d, m, kind):
    """Training side, m test points of which ten are training points, and the reference's
    beta, posterior mean and covariance (shared, read-only)."""
    X, f, H = problem(n, d)
    delta, nu = mr.deltas(d), mr.NU[kind]
    A = mr.make_A(X, delta, nu, kind, family)[0]
    beta = orc.optimal_beta_ref(A, H, f)
    Xs = orc.olhc_design(m, d, 4)
    Xs[:10] = X[:: n // 10][:10]
    Hs = orc.linear_basis(Xs)
    mean, S = mr.posterior(X, f, H, A, Xs, Hs, beta, mr.SIGMA, delta, nu, kind, family)
    return _frozen(A, beta, Xs, Hs, mean, S)


def _factor(ctx, family, n, d, kind, r=None):
    X, f, H = problem(n, d)
    ctx.set_data(X, f, H, r)
    ctx.factor(code(family, kind), mr.deltas(d), mr.NU[kind], 1.0, 0.0 if r is None else 1.0)


@pytest.mark.parametrize("kind", [orc.STD, orc.ALT], ids=["std", "alt"])
@pytest.mark.parametrize("n,d,m", POST)
@pytest.mark.parametrize("family", MATERN)
def test_posterior(ctx, family, n, d, m, kind):
    A, beta, Xs, Hs, rmean, S = post_case(family, n, d, m, kind)
    assert conditioning(family, n, d, kind)[0] <= 1e6
    _factor(ctx, family, n, d, kind)
    gb = ctx.beta()
    assert np.max(np.abs(gb - beta)) <= 1e-8 * np.max(np.abs(beta))
    mean, var = ctx.posterior(Xs, Hs, beta, mr.SIGMA, full_var=True)
    mean_d, diag = ctx.posterior(Xs, Hs, beta, mr.SIGMA, full_var=False)
    _, diag32 = ctx.posterior(Xs, Hs, beta, mr.SIGMA, full_var=False, precision=32)
    em = np.max(np.abs(mean - rmean)) / max(1.0, np.max(np.abs(rmean)))
    ev = np.max(np.abs(var - S)) / max(1.0, np.max(np.abs(S)))
    ed = np.max(np.abs(diag - np.diag(S))) / max(1.0, np.max(np.abs(S)))
    e32 = np.max(np.abs(diag32 - diag)) / mr.SIGMA ** 2
    print(family, n, d, m, kind, "mean", em, "covariance", ev, "diagonal", ed, "precision 32", e32)
    assert em <= 1e-8 and ev <= 1e-8 and ed <= 1e-8
    assert np.max(np.abs(mean_d - rmean)) <= 1e-8 * max(1.0, np.max(np.abs(rmean)))
    assert e32 <= 2e-5


@pytest.mark.parametrize("kind", [orc.STD, orc.ALT], ids=["std", "alt-r"])
@pytest.mark.parametrize("family", MATERN)
def test_loo(ctx, family, kind):
    """gpe_loo against loo_ref.closed_form with the Matern A (alt: with r)."""
    n, d = 300, 5
    X, f, H = problem(n, d)
    r = r_of(n) if kind == orc.ALT else None
    A = mr.make_A(X, mr.deltas(d), mr.NU[kind], kind, family, r=r, s2=1.0)[0]
    rm, rv, rbeta = loo_ref.closed_form(A, H, f, loo_ref.SIGMA, r=r, r_scale=1.0)
    _factor(ctx, family, n, d, kind, r)
    mean, var, beta = ctx.loo(loo_ref.SIGMA)
    em, ev = loo_ref.errors(mean, var, rm, rv, f)
    print(family, kind, "LOO mean error", em, "variance error", ev)
    assert em < 1e-8 and ev < 1e-8
    assert np.max(np.abs(beta - rbeta)) <= 1e-8 * np.max(np.abs(rbeta))


@pytest.mark.parametrize("kind", [orc.STD, orc.ALT], ids=["std", "alt"])
@pytest.mark.parametrize("family", MATERN)
def test_posterior_pivchol(ctx, family, kind):
    n, d, m = POST[0]
    A, beta, Xs, Hs, rmean, S = post_case(family, n, d, m, kind)
    rpiv, rvar, rL, rrank = pr.pivchol(S)
    k = pr.safe_prefix(pr.gaps(S), GAP)
    _factor(ctx, family, n, d, kind)
    mean, piv, pivvar, L, rank = ctx.posterior_pivchol(Xs, Hs, beta, mr.SIGMA)
    scale = np.max(np.diag(S))
    recon = np.max(np.abs(L.dot(L.T) - S)) / scale
    verr = np.max(np.abs(pivvar[:k] - rvar[:k])) / rvar[0]
    print(family, kind, "gap-safe prefix", k, "L L^T against the reference covariance", recon,
          "pivot variance error", verr)
    assert rank == rrank == m and k >= 32
    np.testing.assert_array_equal(piv[:k], rpiv[:k])
    assert verr <= 1e-8 and recon <= 1e-8
    assert np.max(np.abs(mean - rmean)) <= 1e-8 * max(1.0, np.max(np.abs(rmean)))


# ---- end to end -----------------------------------------------------------------------------
def test_train_toy_sim_with_matern52(tmp_path, monkeypatch):
    """setup + train on the toy-sim example with `kernel matern52` in its beliefs (MUCM, fixed
    nugget): the final beliefs carry the line and read back to the same class, the LLH train
    ended at is the reference's at the written hyperparameters, the posterior at the training
    inputs is the reference's and reproduces the outputs at the nugget's scale; sensitivity
    refuses the emulator."""
    d = tmp_path / "toy-sim"
    shutil.copytree(os.path.join(EX, "toy-sim"), d)
    monkeypatch.chdir(d)
    with open("toy-sim_beliefs", "a") as fh:
        fh.write("kernel matern52\n")
    np.random.seed(0)
    E = g.setup("toy-sim_config")
    assert type(E.K) is kernels.kernel_matern52
    calls = []
    orig = E.opt_T.loglikelihood_mucm

    def rec(x):
        res = orig(x)
        if res is not None:
            calls.append((E.K.untransform(np.array(x, float)), res[0], E.training.inputs.shape[0]))
        return res
    monkeypatch.setattr(E.opt_T, "loglikelihood_mucm", rec)
    g.train(E, auto=True)
    finals = sorted(glob.glob("toy-sim_beliefs-*f"))
    assert len(finals) == 1
    lines = open(finals[0]).read().splitlines()
    assert lines[-1] == "kernel matern52"
    b = files.Beliefs(finals[0])
    assert b.kernel == "matern52"
    assert kernels.for_beliefs(b.kernel, b.alt_nugget == "T") is type(E.K)
    # the call train ended at: the last one at the written length scales, on the final set
    delta, nu, sigma = np.array(b.delta), b.nugget, b.sigma
    X, f, H = E.training.inputs, E.training.outputs, E.training.H
    at = [c for c in calls if c[2] == X.shape[0] and np.max(np.abs(c[0] - delta)) <= 1e-12 * np.max(delta)]
    assert at
    ref = mr.objective(X, f, H, delta, orc.MUCM, orc.STD, False, "matern52", nu_fixed=nu)
    print("LLH train ended at", at[-1][1], "reference", ref[0], "sigma", sigma, "reference", np.sqrt(ref[2]))
    assert abs(at[-1][1] - ref[0]) <= 1e-8 * abs(ref[0])
    assert abs(sigma - np.sqrt(ref[2])) <= 1e-8 * sigma
    # posterior at the training inputs
    pm, pv = g.posterior(E, X)
    A = mr.make_A(X, delta, nu, orc.STD, "matern52")[0]
    rm, rv = mr.posterior(X, f, H, A, X, H, np.array(b.beta), sigma, delta, nu, orc.STD, "matern52")
    assert np.max(np.abs(pm - rm)) <= 1e-8 * max(1.0, np.max(np.abs(rm)))
    assert np.max(np.abs(pv - rv)) <= 1e-8 * max(1.0, np.max(np.abs(rv)))
    # the nugget gives each output the variance sigma^2 nu about the smooth part, and the
    # posterior at a training point keeps about that much (predict = True): four standard
    # deviations of sigma^2 2 nu bound the residuals
    print("largest residual at the training inputs", np.max(np.abs(pm - f)), "sigma sqrt(2 nu)", sigma * np.sqrt(2 * nu))
    assert np.max(np.abs(pm - f)) <= 4.0 * sigma * np.sqrt(2.0 * nu)
    with pytest.raises(sensitivity.NonGaussianKernel, match="gaussian kernel"):
        sensitivity.setup(E, [0.5, 0.5], [0.02, 0.02])


@pytest.mark.parametrize("family", MATERN)
def test_distributed_objective_refuses_matern(family):
    X, f, H = problem(129, 2)
    hp = mr.hyperparams(2, orc.GP4ML, orc.STD, True)
    dc = native.DistContext(0, 1)
    try:
        dc.set_data(X, f, H)
        for kind in (orc.STD, orc.ALT):
            with pytest.raises(RuntimeError, match=r"gpe_dist_objective failed \(-5\): .*Gaussian"):
                dc.objective(orc.GP4ML, code(family, kind), hp)
        with pytest.raises(RuntimeError, match=r"gpe_dist_objective failed \(-1\): bad kernel"):
            dc.objective(orc.GP4ML, 0x30, hp)
        llh, _ = dc.objective(orc.GP4ML, native.KERNEL_STD, hp)   # the Gaussian codes as before
        ref = orc.objective_ref(X, f, H, hp, orc.GP4ML, orc.STD, True, want_grad=False)[0]
        assert abs(llh - ref) <= 1e-10 * abs(ref)
    finally:
        dc.close()
