"""The separable multi-output emulator on the GPU (gpe_set_outputs, gpe_objective_multi,
gpe_beta_multi, gpe_posterior_mean_multi, gp_emu_uqsa_amd.multioutput) against the dense NumPy
reference tests/multi_output_ref.py, itself checked on the CPU in test_multi_output_host.py.

Objective shapes: n = 129 is two tiles with one valid row in the second, 520 five tile rows, 300
a size at which gpe_objective takes k_snb (the multi entry runs the general path at every n);
d = 40 the _wide kernels; p + q = 35 columns k_contract_wide with a narrow d, 58 columns with a
wide one; p + q <= 33 the register-resident k_contract buckets.

Tolerances are those of test_gpu_matern.py's header: llh max(1e-10, 4 eps cond(A)) relative,
gradient 1e-7 (|g_ref| + max |g_ref|), Sigma-hat 1e-10 relative to max |Sigma-hat|, value-only
against gradient llh 1e-12 relative; every case asserts cond(A) <= 1e6 and a median off-diagonal
correlation >= 0.05 of its own inputs.  B (a GLS solve) and the posterior means: 1e-8 max(1,
max |v|), that file's posterior tolerance.
"""
import functools
import os
import shutil

import numpy as np
import pytest

import matern_ref as mr
import multi_output_ref as mo
from gp_emu_uqsa_amd import native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(__file__), "golden", "examples")
EPS = np.finfo(float).eps
ERR_ARG, ERR_STATE = -1, -4      # include/gpemu.h


def code(family, kind):
    return mr.FAMILY_CODE[family] | kind


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def problem(n, d, p, basis="linear"):
    """(X, F, H) of a shape (shared, read-only); basis: linear (q = d + 1) or const (q = 1)."""
    X, _, H = orc.synthetic_problem(n, d, seed=9)
    if basis == "const":
        H = np.ones((n, 1))
    return _frozen(X, mo.outputs(X, p), H)


@functools.lru_cache(maxsize=None)
def r_of(n):
    return _frozen(np.random.RandomState(5).uniform(0, 0.02, n))[0]


@functools.lru_cache(maxsize=None)
def reference(n, d, p, family, kind, fit, basis="linear"):
    """(cond(A), median rho, llh, grad, Sigma, B) of a case (shared, read-only)."""
    X, F, H = problem(n, d, p, basis)
    hp = mr.hyperparams(d, orc.MUCM, kind, fit)
    cond, med = mo.conditioning(X, mr.deltas(d), mr.NU[kind], kind, family)
    out = mo.objective(X, F, H, hp, kind, fit, family, nu_fixed=mr.NU[kind])
    return (cond, med) + _frozen(*out)


def check_objective(ctx, n, d, p, family, kind, fit, basis="linear", with_r=False):
    X, F, H = problem(n, d, p, basis)
    cond, med, rl, rg, rS, rB = reference(n, d, p, family, kind, fit, basis)
    assert cond <= 1e6 and med >= 0.05, (cond, med)
    rtol = max(1e-10, 4 * EPS * cond)
    hp = mr.hyperparams(d, orc.MUCM, kind, fit)
    # (r is resident but, as for the MUCM objective, no part of A)
    ctx.set_data(X, F[:, 0], H, r_of(n) if with_r else None)
    ctx.set_outputs(F)
    llh, grad, S, B = ctx.objective_multi(code(family, kind), hp, nu_fixed=mr.NU[kind], want_grad=True)
    vllh, vgrad, vS, vB = ctx.objective_multi(code(family, kind), hp, nu_fixed=mr.NU[kind], want_grad=False)
    gerr = np.abs(grad - rg) / (np.abs(rg) + np.max(np.abs(rg)))
    serr = np.max(np.abs(S - rS)) / np.max(np.abs(rS))
    berr = np.max(np.abs(B - rB)) / max(1.0, np.max(np.abs(rB)))
    print(n, d, p, family, kind, fit, basis, "cond", cond, "llh error", abs(llh - rl) / abs(rl), "value-only",
          abs(vllh - rl) / abs(rl), "gradient error", np.max(gerr), "Sigma error", serr, "B error", berr)
    assert np.isfinite(llh) and np.all(np.isfinite(grad))
    assert abs(llh - rl) <= rtol * abs(rl)
    assert abs(vllh - rl) <= rtol * abs(rl)
    assert np.max(gerr) <= 1e-7
    assert serr <= 1e-10 and np.max(np.abs(vS - rS)) <= 1e-10 * np.max(np.abs(rS))
    assert np.array_equal(S, S.T)
    assert berr <= 1e-8 and np.max(np.abs(vB - rB)) <= 1e-8 * max(1.0, np.max(np.abs(rB)))
    assert vgrad is None
    assert abs(vllh - llh) <= 1e-12 * abs(llh)


OBJECTIVE_CASES = [   # (n, d, p, family, kind, fit nugget, basis, with r)
    (129, 3, 3, "gaussian", orc.STD, True, "linear", False),
    (129, 10, 17, "matern32", orc.ALT, True, "linear", False),
    (520, 3, 17, "gaussian", orc.STD, True, "linear", False),
    (520, 10, 1, "matern52", orc.STD, True, "linear", False),
    (300, 3, 1, "gaussian", orc.STD, True, "linear", False),
    (300, 10, 3, "matern52", orc.STD, False, "linear", False),
    (300, 5, 3, "gaussian", orc.STD, True, "const", False),
    (300, 5, 3, "gaussian", orc.ALT, False, "linear", True),
    (300, 5, 3, "matern32", orc.STD, True, "linear", True),
    (260, 40, 3, "matern32", orc.STD, True, "linear", False),
    (200, 3, 30, "gaussian", orc.ALT, True, "linear", False),      # 35 columns, d = 3
    (260, 40, 17, "gaussian", orc.STD, True, "linear", False),     # 58 columns, d = 40
    (260, 40, 1, "gaussian", orc.ALT, False, "const", False),
]


@pytest.mark.parametrize("case", OBJECTIVE_CASES, ids=["-".join(str(v) for v in c) for c in OBJECTIVE_CASES])
def test_objective_against_the_reference(ctx, case):
    check_objective(ctx, *case)


@pytest.mark.parametrize("n,d,family,kind,fit", [(129, 3, "gaussian", orc.STD, True),
                                                 (300, 10, "matern52", orc.STD, False),
                                                 (520, 5, "gaussian", orc.ALT, True),
                                                 (260, 40, "matern32", orc.STD, True)])
def test_one_output_is_the_mucm_objective(ctx, n, d, family, kind, fit):
    """llh and Sigma-hat are gpe_objective(GPE_MUCM)'s llh and sigma2, the gradient its grad /
    sigma2 (n = 129 and 300 are one-launch sizes there, the general path here)."""
    X, F, H = problem(n, d, 1)
    cond, med = mo.conditioning(X, mr.deltas(d), mr.NU[kind], kind, family)
    assert cond <= 1e6 and med >= 0.05
    rtol = max(1e-10, 4 * EPS * cond)
    hp = mr.hyperparams(d, orc.MUCM, kind, fit)
    ctx.set_data(X, F[:, 0], H)
    ctx.set_outputs(F)
    for want_grad in (True, False):
        l1, g1, s2 = ctx.objective(orc.MUCM, code(family, kind), hp, nu_fixed=mr.NU[kind], want_grad=want_grad)
        lm, gm, S, B = ctx.objective_multi(code(family, kind), hp, nu_fixed=mr.NU[kind], want_grad=want_grad)
        print(n, d, family, kind, fit, want_grad, "llh", abs(lm - l1) / abs(l1), "sigma2", abs(S[0, 0] - s2) / s2)
        assert abs(lm - l1) <= rtol * abs(l1)
        assert S.shape == (1, 1) and abs(S[0, 0] - s2) <= 1e-10 * s2
        if want_grad:
            ref = g1 / s2
            assert np.max(np.abs(gm - ref) / (np.abs(ref) + np.max(np.abs(ref)))) <= 1e-7
    ctx.ensure_factor(code(family, kind), hp[:d], hp[d] if fit else mr.NU[kind], 1.0, 0.0)
    assert np.max(np.abs(ctx.beta_multi()[:, 0] - ctx.beta())) <= 1e-8 * max(1.0, np.max(np.abs(B)))


# ------------------------------------------------------------------ the int8 paths
@pytest.fixture(scope="module")
def oz_pair():
    """(a context with the int8 products from n_pad 2048, one with GPEMU_OZAKI=0), as
    test_gpu_ozaki.py's."""
    mp = pytest.MonkeyPatch()
    mp.setenv("GPEMU_OZAKI_MIN_NP", "2048")
    a = native.Context(0)
    mp.undo()
    mp.setenv("GPEMU_OZAKI", "0")
    b = native.Context(0)
    mp.undo()
    yield a, b
    a.close()
    b.close()


def test_int8_products(oz_pair):
    """n = 2048, p = 3: A^-1 = L^-T L^-1 on the int8 cores against the fp64 LAUUM.  The llh and
    Sigma-hat do not depend on A^-1: equal bits; gradient 1e-10 of scale (test_gpu_ozaki.py)."""
    oz, fp64 = oz_pair
    n, d, p = 2048, 10, 3
    X, F, H = problem(n, d, p)
    hp = np.concatenate([np.linspace(0.5, 1.1, d), [1e-3]])
    out = []
    for c in (oz, fp64):
        c.set_data(X, F[:, 0], H)
        c.set_outputs(F)
        out.append(c.objective_multi(orc.STD, hp))
    (l, g, S, B), (l64, g64, S64, B64) = out
    err = np.max(np.abs(g - g64) / (np.abs(g64) + np.max(np.abs(g64))))
    print("int8 against fp64: gradient", err)
    assert l == l64 and np.array_equal(S, S64) and np.array_equal(B, B64)
    assert err <= 1e-10


# ------------------------------------------------------------------ refusals and state
def _status(ctx, call):
    """(code, message) of a native call that must fail."""
    with pytest.raises((RuntimeError, ArithmeticError)) as e:
        call()
    text = str(e.value)
    if isinstance(e.value, native.NotPositiveDefinite):
        return native.GPE_NOT_PD, text
    return int(text.split("failed (")[1].split(")")[0]), text


@pytest.mark.parametrize("family", ["matern32", "matern52"])
def test_coincident_points_without_a_nugget(ctx, family):
    """The same status as gpe_objective on the same data (the Matern pivot floor included)."""
    X, F, H = problem(300, 5, 3)
    X = X.copy()
    X[250] = X[7]
    hp = mr.deltas(5)
    ctx.set_data(X, F[:, 0], orc.linear_basis(X))
    ctx.set_outputs(F)
    one = _status(ctx, lambda: ctx.objective(orc.MUCM, code(family, orc.STD), hp, nu_fixed=0.0))
    multi = _status(ctx, lambda: ctx.objective_multi(code(family, orc.STD), hp, nu_fixed=0.0))
    assert one[0] == multi[0] == native.GPE_NOT_PD
    assert "not positive definite (pivot" in one[1] and "not positive definite (pivot" in multi[1]


def test_dependent_outputs_and_basis(ctx):
    X, F, H = problem(300, 5, 3)
    hp = mr.hyperparams(5, orc.MUCM, orc.STD, True)
    Fdup = F.copy()
    Fdup[:, 2] = Fdup[:, 0]
    ctx.set_data(X, F[:, 0], H)
    ctx.set_outputs(Fdup)
    for want_grad in (True, False):
        st = _status(ctx, lambda: ctx.objective_multi(orc.STD, hp, want_grad=want_grad))
        assert st[0] == native.GPE_NOT_PD and st[1].endswith("F^T P F not positive definite"), st
    ctx.set_data(X, F[:, 0], np.column_stack([H, H[:, 1]]))
    ctx.set_outputs(F)
    st = _status(ctx, lambda: ctx.objective_multi(orc.STD, hp))
    assert st[0] == native.GPE_NOT_PD and st[1].endswith("H^T A^-1 H not positive definite"), st
    st = _status(ctx, lambda: ctx.objective_multi(orc.STD, np.array([0.5, 0.0, 0.7, 0.8, 0.9, 1e-3])))
    assert st[0] == native.GPE_NOT_PD and st[1].endswith("length scale delta[1] is zero or NaN"), st


def test_state_and_arguments():
    c = native.Context(0)
    try:
        X, F, H = problem(129, 3, 3)
        hp = mr.hyperparams(3, orc.MUCM, orc.STD, True)
        assert _status(c, lambda: c.set_outputs(F))[0] == ERR_STATE           # no data
        c.set_data(X, F[:, 0], H)
        assert _status(c, lambda: c.objective_multi(orc.STD, hp))[0] == ERR_STATE      # no outputs
        assert _status(c, lambda: c.beta_multi())[0] == ERR_STATE                      # no factor
        c.factor(orc.STD, hp[:3], hp[3])
        assert _status(c, lambda: c.beta_multi())[0] == ERR_STATE                      # no outputs
        assert _status(c, lambda: c.posterior_mean_multi(X[:5], H[:5], np.zeros((4, 1))))[0] == ERR_STATE
        for bad in (np.zeros((129, 0)), np.zeros((129, 65))):
            assert _status(c, lambda: c.set_outputs(bad))[0] == ERR_ARG
        assert c.lib.gpe_set_outputs(c._h, 3, None) == ERR_ARG
        c.set_outputs(np.column_stack([F] * 22)[:, :64])     # p = 64 is accepted
        # n < p + q + 3: n = 9 with p = 3, q = 4 needs 10
        c.set_data(X[:9], F[:9, 0], H[:9])
        assert _status(c, lambda: c.set_outputs(F[:9]))[0] == ERR_ARG
        c.set_outputs(F[:9, :2])
        # a new gpe_set_data drops the outputs
        c.set_data(X, F[:, 0], H)
        assert _status(c, lambda: c.objective_multi(orc.STD, hp))[0] == ERR_STATE
        c.set_outputs(F)
        assert _status(c, lambda: c.objective_multi(orc.STD | 0x30, hp))[0] == ERR_ARG
        assert _status(c, lambda: c.objective_multi(orc.STD, hp[:2]))[0] == ERR_ARG
        c.objective_multi(orc.STD, hp)
    finally:
        c.close()


def test_single_output_entries_keep_their_bits():
    """gpe_objective, gpe_posterior_mean and gpe_posterior before and after gpe_set_outputs (and
    after the multi entries have run) in one context."""
    c = native.Context(0)
    try:
        n, d = 520, 3
        X, F, H = problem(n, d, 17)
        hp = mr.hyperparams(d, orc.GP4ML, orc.STD, True)
        Xs = np.random.RandomState(2).uniform(size=(300, d))
        Hs = orc.linear_basis(Xs)

        def run():
            o = c.objective(orc.GP4ML, orc.STD, hp)
            v = c.objective(orc.MUCM, orc.STD, hp[:-1], want_grad=False)
            c.factor(orc.STD, hp[:d], hp[d])
            beta = c.beta()
            return (o[0], o[1], o[2], v[0], v[2], beta, c.posterior_mean(Xs, Hs, beta),
                    *c.posterior(Xs, Hs, beta, 1.3, full_var=False))
        c.set_data(X, F[:, 0], H)
        before = run()
        c.set_outputs(F)
        with_outputs = run()
        _, _, _, B = c.objective_multi(orc.STD, hp[:-1])
        c.factor(orc.STD, hp[:d], hp[d])
        c.posterior_mean_multi(Xs, Hs, B)
        after = run()
        for a, b, e in zip(before, with_outputs, after):
            assert np.array_equal(a, b) and np.array_equal(a, e)
    finally:
        c.close()


# ------------------------------------------------------------------ the posterior means
MEAN_CASES = [   # (n, m, p, d, family, kind)
    (200, 1000, 1, 3, "gaussian", orc.STD),
    (200, 1000, 3, 3, "matern32", orc.ALT),
    (200, 1, 17, 3, "matern52", orc.STD),
    (200, 1000, 16, 3, "matern52", orc.STD),
    (200, 1000, 40, 8, "gaussian", orc.STD),       # three blocks of 16 outputs
    (200, 1000, 64, 10, "matern32", orc.STD),      # four
    (700, 1000, 16, 3, "gaussian", orc.ALT),
    (700, 1000, 17, 40, "gaussian", orc.STD),
    (700, 1000, 1, 40, "matern32", orc.STD),
    (700, 1, 3, 40, "matern52", orc.ALT),
    (700, 1000, 3, 16, "gaussian", orc.STD),
    (700, 1000, 3, 20, "matern52", orc.STD),
]


@functools.lru_cache(maxsize=None)
def mean_reference(n, m, p, d, family, kind):
    X, F, H = problem(n, d, p)
    Xs = np.random.RandomState(7).uniform(size=(m, d))
    Hs = orc.linear_basis(Xs)
    mean, _, _, B = mo.posterior(X, F, H, Xs, Hs, mr.deltas(d), mr.NU[kind], kind, family, full=False)
    return _frozen(Xs, Hs, mean, B)


def _resident(c, n, p, d, family, kind):
    X, F, H = problem(n, d, p)
    c.set_data(X, F[:, 0], H)
    c.set_outputs(F)
    c.factor(code(family, kind), mr.deltas(d), mr.NU[kind], 1.0, 0.0)


@pytest.mark.parametrize("case", MEAN_CASES, ids=["-".join(str(v) for v in c) for c in MEAN_CASES])
def test_posterior_means_against_the_reference(ctx, case):
    n, m, p, d, family, kind = case
    X, F, H = problem(n, d, p)
    Xs, Hs, rmean, rB = mean_reference(*case)
    _resident(ctx, n, p, d, family, kind)
    B = ctx.beta_multi()
    berr = np.max(np.abs(B - rB)) / max(1.0, np.max(np.abs(rB)))
    mean = ctx.posterior_mean_multi(Xs, Hs, B)
    again = ctx.posterior_mean_multi(Xs, Hs, B)
    tol = 1e-8 * max(1.0, np.max(np.abs(rmean)))
    print(case, "B error", berr, "mean error", np.max(np.abs(mean - rmean)), "tol", tol)
    assert berr <= 1e-8
    assert mean.shape == (m, p) and np.all(np.isfinite(mean))
    assert np.max(np.abs(mean - rmean)) <= tol
    assert np.array_equal(mean, again)                    # a repeated call: equal bits
    # column by column against gpe_posterior_mean (a new gpe_set_data each: the outputs go)
    cols = np.empty_like(mean)
    for j in range(p):
        ctx.set_data(X, F[:, j], H)
        ctx.factor(code(family, kind), mr.deltas(d), mr.NU[kind], 1.0, 0.0)
        cols[:, j] = ctx.posterior_mean(Xs, Hs, B[:, j])
    print(case, "against gpe_posterior_mean", np.max(np.abs(mean - cols)))
    assert np.max(np.abs(mean - cols)) <= tol


@pytest.mark.parametrize("case", [c for c in MEAN_CASES if c[2] == 1], ids=lambda c: "-".join(str(v) for v in c))
def test_one_output_returns_the_single_mean_bits(ctx, case):
    """p = 1: gpe_posterior_mean_multi and gpe_posterior_mean share the route to gamma, the order
    of the n-term sum and the host's hs . beta, so they return the same bits (the register
    widths with d = 3, the wide instance with d = 40)."""
    n, m, p, d, family, kind = case
    X, F, H = problem(n, d, p)
    Xs, Hs, _, _ = mean_reference(*case)
    _resident(ctx, n, p, d, family, kind)
    B = ctx.beta_multi()
    multi = ctx.posterior_mean_multi(Xs, Hs, B)
    single = ctx.posterior_mean(Xs, Hs, B[:, 0])
    assert multi.shape == (m, 1) and np.array_equal(multi[:, 0], single)


@pytest.mark.parametrize("m,p,d", [(1000, 17, 3), (257, 3, 40)])
def test_chunks_return_the_same_bits(ctx, monkeypatch, m, p, d):
    """GPEMU_MEAN_CHUNK=256 in a context of its own: 4 chunks (m = 1000), and 2 with the last of
    one point (m = 257), bit for bit the single chunk's result."""
    n, family, kind = 700, "matern32", orc.STD
    Xs = np.random.RandomState(8).uniform(size=(m, d))
    Hs = orc.linear_basis(Xs)
    _resident(ctx, n, p, d, family, kind)
    B = ctx.beta_multi()
    one = ctx.posterior_mean_multi(Xs, Hs, B)
    monkeypatch.setenv("GPEMU_MEAN_CHUNK", "256")
    c = native.Context(0)
    try:
        _resident(c, n, p, d, family, kind)
        many = c.posterior_mean_multi(Xs, Hs, B)
        c.set_profiling(True)
        c.posterior_mean_multi(Xs, Hs, B)
        assert c.phase_times()["cholesky"] == -(-m // 256) and c.phase_times()["kbuild"] > 0.0   # [1] chunks, [0] ms
    finally:
        c.close()
    assert np.array_equal(many, one)


def test_posterior_mean_arguments(ctx):
    _resident(ctx, 200, 3, 3, "gaussian", orc.STD)
    Xs, Hs, _, B = mean_reference(200, 1000, 3, 3, "matern32", orc.ALT)
    out = np.zeros((5, 3))
    D = native._ptr
    lib, h = ctx.lib, ctx._h
    assert lib.gpe_posterior_mean_multi(h, 0, D(Xs), D(Hs), D(B), D(out)) == ERR_ARG
    assert lib.gpe_posterior_mean_multi(h, 5, None, D(Hs), D(B), D(out)) == ERR_ARG
    assert lib.gpe_posterior_mean_multi(h, 5, D(Xs), D(Hs), None, D(out)) == ERR_ARG
    assert lib.gpe_posterior_mean_multi(h, 5, D(Xs), D(Hs), D(B), None) == ERR_ARG
    assert lib.gpe_beta_multi(h, None) == ERR_ARG


# ------------------------------------------------------------------ the Python layer
@pytest.fixture()
def toysim3d(tmp_path, monkeypatch):
    """The toysim3D example in a directory of its own, with 4 tries."""
    for f in os.listdir(os.path.join(EX, "toysim3D")):
        shutil.copy(os.path.join(EX, "toysim3D", f), tmp_path)
    cfg = tmp_path / "toysim3D_config0"
    cfg.write_text(cfg.read_text().replace("tries 20", "tries 4"))
    monkeypatch.chdir(tmp_path)
    return tmp_path


def test_python_setup_train_posterior(toysim3d, monkeypatch):
    import gp_emu_uqsa_amd as g
    from gp_emu_uqsa_amd import multioutput, optimize
    seen = []
    orig = optimize.Optimize._run_try

    def run_try(self, x_guess):
        r = orig(self, x_guess)
        seen.append((r, np.array(self.cons, dtype=float)))
        return r
    monkeypatch.setattr(optimize.Optimize, "_run_try", run_try)
    np.random.seed(0)
    M = multioutput.setup("toysim3D_config0", outputs=[0, 1], datashuffle=True)
    assert M.p == 2 and M.F.shape == (M.training.inputs.shape[0], 2)
    before = sorted(os.listdir("."))
    multioutput.train(M)
    assert sorted(os.listdir(".")) == before                         # no files are written
    assert len(seen) == 4 and all(r is not None for r, _ in seen)
    for (fun, x, res), bounds in seen:
        # the stop L-BFGS-B reported: the two test_gpu_headline.py accepts.  Its bound on the
        # projected gradient after an ftol stop (10 ftol |f|) is scaled to |f| ~ 1e4; at
        # |f| ~ 1e2 it lies below pgtol itself and says nothing, so the figure is printed: a
        # last step that lowers f by <= ftol max(1, |f|) = 2.2e-7 leaves |pg|^2 ~ 2 h 2.2e-7 for
        # a curvature h along it (measured: 3.3e-4 at f = -101.5)
        msg = res.message if isinstance(res.message, str) else res.message.decode()
        pg = np.clip(x - res.jac, bounds[:, 0], bounds[:, 1]) - x
        print(res.nfev, "evaluations,", msg, "llh", -fun, "max |projected grad|", np.max(np.abs(pg)))
        assert res.success, msg
        if "PROJECTED GRADIENT" in msg:
            assert np.max(np.abs(pg)) <= 1e-5, pg
        else:
            assert "RELATIVE REDUCTION OF F" in msg, msg
    # the trained state against the reference at the optimum
    X, F, H = M.training.inputs, M.F, M.training.H
    delta, nu = np.asarray(M.par.delta, float), float(M.par.nugget)
    kind = M.K.kind & 1
    ref = mo.objective(X, F, H, delta, kind, False, nu_fixed=nu, want_grad=False)
    assert np.max(np.abs(M.Sigma - ref[2])) <= 1e-8 * np.max(np.abs(ref[2]))
    assert np.max(np.abs(M.B - ref[3])) <= 1e-8 * max(1.0, np.max(np.abs(ref[3])))
    assert min(seen, key=lambda s: s[0][0])[0][2].nfev >= 2       # (a chain from a flat corner stops at once)
    assert abs(min(fun for (fun, _, _), _ in seen) - ref[0]) <= 1e-8 * max(1.0, abs(ref[0]))
    # posterior: c symmetric and gpe_posterior(sigma = 1)'s, the means the reference's
    xs = np.random.RandomState(3).uniform(size=(40, X.shape[1]))
    hs = M.basis.design_matrix(xs)
    mean, c, Sigma = multioutput.posterior(M, xs, full=True)
    rmean, rc, rS, _ = mo.posterior(X, F, H, xs, hs, delta, nu, kind, full=True)
    tol = 1e-8 * max(1.0, np.max(np.abs(rmean)))
    assert mean.shape == (40, 2) and np.max(np.abs(mean - rmean)) <= tol
    assert np.array_equal(c, c.T) and np.max(np.abs(c - rc)) <= 1e-8
    ctx = native.default_context()
    _, c1 = ctx.posterior(xs, hs, M.B[:, 0], 1.0, full_var=True)
    assert np.array_equal(c, c1) and np.array_equal(Sigma, M.Sigma)
    m2, cd, _ = multioutput.posterior(M, xs)
    assert np.array_equal(m2, mean) and np.max(np.abs(cd - np.diag(c))) <= 1e-8
    assert np.array_equal(multioutput.posterior_mean(M, xs), mean)
    # output j alone is an ordinary emulator
    for j in (0, 1):
        E = M.single(j)
        mj, vj = g.posterior(E, xs)
        assert np.max(np.abs(mj - mean[:, j])) <= tol
        assert np.max(np.abs(vj - M.Sigma[j, j] * c)) <= 1e-8 * max(1.0, M.Sigma[j, j])
        loo = g.loo(E)
        assert loo.mean.shape == (X.shape[0],) and np.all(np.isfinite(loo.error)) and np.all(loo.var > 0)
