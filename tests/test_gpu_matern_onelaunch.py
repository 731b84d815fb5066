"""The Matern 3/2 and 5/2 families in the one-launch objectives (k_tiny<DM, FAM>, n <= 128;
k_snb<DM, FAM>, 128 < n <= 512) against the dense NumPy reference (tests/matern_ref.py) and
against the general path of the same library (a GPEMU_TINY=0 context).

Shapes: the smallest that reach every instantiation and edge.  k_tiny: (5, 1) almost all
padding, (100, 3) DM 4, (60, 6) DM 8, (128, 10) DM 12 and a full tile, (97, 16) DM 16,
(128, 30) DM 32.  k_snb: (129, 5) one valid row in the second tile, (300, 10) three ragged
tiles, (512, 16) four full tiles, (450, 30) DM 32.

Inputs: orc.synthetic_problem(n, d, seed=9), delta = linspace(0.5, 1.1, d) sqrt(max(d, 5) / 5),
nu = matern_ref.NU[kind], sigma = matern_ref.SIGMA.  Every case asserts cond(A) <= 1e6 and a
median off-diagonal correlation >= 0.05 of its own inputs, so no case compares zeros or
widens its own tolerance.

Tolerances (the project's existing ones).  Against matern_ref.objective: LLH
max(1e-10, 4 eps cond(A)) relative, gradient |g - g_ref| <= 1e-7 (|g_ref| + max |g_ref|),
sigma^2 1e-10 relative, value-only LLH within 1e-12 of the gradient call's.  Against the
general path on the same inputs (the bounds of test_gpu_tiny.py / test_gpu_snb.py): LLH and
sigma^2 1e-11, gradient 1e-9 (1 + max |g|).
"""
import functools
import glob
import os
import shutil

import numpy as np
import pytest

import gp_emu_uqsa_amd as g
import matern_ref as mr
from gp_emu_uqsa_amd import files, kernels, native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(__file__), "golden", "examples")
EPS = np.finfo(float).eps
MATERN = ["matern32", "matern52"]
# (kind, variant): MUCM with the std nugget only (the beliefs refuse mucm with alt_nugget)
KV = [(orc.STD, orc.GP4ML), (orc.ALT, orc.GP4ML), (orc.STD, orc.MUCM)]
TINY_SHAPES = [(5, 1), (100, 3), (60, 6), (128, 10), (97, 16), (128, 30)]
SNB_SHAPES = [(129, 5), (300, 10), (512, 16), (450, 30)]
PHASES = ["kbuild", "cholesky", "trtri", "inverse", "skinny", "contract"]


@pytest.fixture(scope="module")
def general():
    """A context on the general path (GPEMU_TINY=0 is read when the context is created)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("GPEMU_TINY", "0")
    c = native.Context(0)
    mp.undo()
    yield c
    c.close()


def code(family, kind):
    return mr.FAMILY_CODE[family] | kind


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def deltas(d):
    return np.linspace(0.5, 1.1, d) * np.sqrt(max(d, 5) / 5.0)


def hyperparams(d, variant, kind, fit):
    hp = list(deltas(d))
    if fit:
        hp.append(mr.NU[kind])
    if variant == orc.GP4ML:
        hp.append(mr.SIGMA)
    return np.array(hp)


@functools.lru_cache(maxsize=None)
def problem(n, d, coincident=False):
    """(X, f, H) of a shape (shared, read-only).  coincident, n = 100: row 7 copied over row
    60 (a pair inside k_tiny); n = 300: row 7 over row 250 and row 3 over row 131 (a pair
    inside a tile and one that straddles tiles, as test_gpu_matern.py's)."""
    X, f, H = orc.synthetic_problem(n, d, seed=9)
    if coincident:
        X = X.copy()
        if n == 100:
            X[60] = X[7]
        else:
            assert n == 300
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
    A, rho, _ = mr.kernel_var(X, deltas(d), mr.NU[kind], kind, family)
    return float(np.linalg.cond(A)), float(np.median(rho)) if rho.size else 1.0


@functools.lru_cache(maxsize=None)
def ref_objective(family, n, d, kind, variant, fit, with_r=False, coincident=False):
    """matern_ref.objective of a case (computed once, shared, read-only)."""
    X, f, H = problem(n, d, coincident)
    hp = hyperparams(d, variant, kind, fit)
    out = mr.objective(X, f, H, hp, variant, kind, fit, family, r=r_of(n) if with_r else None,
                       nu_fixed=mr.NU[kind])
    _frozen(*out)
    return out


def assert_matches_reference(got, ref, rtol, what):
    """(llh, grad, s2) of a gradient call against the reference's."""
    llh, grad, s2 = got
    rl, rg, rs2 = ref
    gerr = np.abs(grad - rg) / (np.abs(rg) + np.max(np.abs(rg)))
    print(*what, "LLH error", abs(llh - rl) / abs(rl), "gradient error", np.max(gerr), "sigma^2 error",
          abs(s2 - rs2) / abs(rs2))
    assert np.isfinite(llh) and np.all(np.isfinite(grad))
    assert abs(llh - rl) <= rtol * abs(rl)
    assert np.max(gerr) <= 1e-7
    assert abs(s2 - rs2) <= 1e-10 * abs(rs2)


def check_objective(ctx, general, family, n, d, kind, variant, fit, with_r=False, coincident=False):
    X, f, H = problem(n, d, coincident)
    cond, med = conditioning(family, n, d, kind, coincident)
    print(family, n, d, kind, variant, fit, "cond", cond, "median rho", med)
    assert cond <= 1e6 and med >= 0.05
    rtol = max(1e-10, 4 * EPS * cond)
    hp = hyperparams(d, variant, kind, fit)
    k, nu = code(family, kind), mr.NU[kind]
    r = r_of(n) if with_r else None
    ref = ref_objective(family, n, d, kind, variant, fit, with_r, coincident)
    ctx.set_data(X, f, H, r)
    llh, grad, s2 = ctx.objective(variant, k, hp, nu_fixed=nu, want_grad=True)
    vllh, vgrad, vs2 = ctx.objective(variant, k, hp, nu_fixed=nu, want_grad=False)
    assert_matches_reference((llh, grad, s2), ref, rtol, (family, n, d, kind, variant, fit))
    assert abs(vllh - ref[0]) <= rtol * abs(ref[0]) and abs(vs2 - ref[2]) <= 1e-10 * abs(ref[2])
    assert vgrad is None
    assert abs(vllh - llh) <= 1e-12 * abs(llh)
    general.set_data(X, f, H, r)
    gl, gg, gs2 = general.objective(variant, k, hp, nu_fixed=nu, want_grad=True)
    print("against the general path: LLH", abs(llh - gl) / max(1.0, abs(gl)), "gradient",
          np.max(np.abs(grad - gg)) / (1.0 + np.max(np.abs(gg))), "sigma^2", abs(s2 - gs2) / gs2)
    assert abs(llh - gl) <= 1e-11 * max(1.0, abs(gl))
    assert np.max(np.abs(grad - gg)) <= 1e-9 * (1.0 + np.max(np.abs(gg)))
    assert abs(s2 - gs2) <= 1e-11 * gs2


# ---- a. the path taken ----------------------------------------------------------------------
def _profile(c, family, n, d, want_grad):
    """(gemm launches, phase times) of one profiled Matern objective on context c."""
    X, f, H = problem(n, d)
    c.set_data(X, f, H)
    hp = hyperparams(d, orc.GP4ML, orc.STD, True)
    c.set_profiling(True)
    try:
        c.objective(orc.GP4ML, code(family, orc.STD), hp, want_grad=want_grad)
        return c.gemm_stats()["launches"], c.phase_times()
    finally:
        c.set_profiling(False)


@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "value"])
@pytest.mark.parametrize("n,d", [(100, 3), (300, 10)])
@pytest.mark.parametrize("family", MATERN)
def test_matern_objective_is_one_launch(ctx, general, family, n, d, want_grad):
    """What tiny_objective / snb_objective leave behind with profiling on: no GEMM-range
    launch, every phase but the total exactly 0.  The same call on the GPEMU_TINY=0 context
    reports at least one launch, so the check is not vacuous."""
    launches, ph = _profile(ctx, family, n, d, want_grad)
    glaunches, gph = _profile(general, family, n, d, want_grad)
    print(family, n, d, want_grad, "launches", launches, ph, "general path: launches", glaunches, gph)
    assert launches == 0
    assert all(ph[p] == 0.0 for p in PHASES) and ph["total"] > 0.0
    assert glaunches >= 1 and gph["cholesky"] > 0.0


@pytest.mark.parametrize("n,d", [(128, 31), (513, 3)])
@pytest.mark.parametrize("family", MATERN)
def test_past_the_one_launch_limits(ctx, family, n, d):
    """q + 1 = 33 basis columns and n = 513 take the general path on the default context."""
    launches, ph = _profile(ctx, family, n, d, True)
    print(family, n, d, "launches", launches, ph)
    assert launches >= 1


# ---- b. values ------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [True, False], ids=["fit", "fixed"])
@pytest.mark.parametrize("kind,variant", KV, ids=["std-gp4ml", "alt-gp4ml", "std-mucm"])
@pytest.mark.parametrize("n,d", TINY_SHAPES + SNB_SHAPES)
@pytest.mark.parametrize("family", MATERN)
def test_objective(ctx, general, family, n, d, kind, variant, fit):
    """LLH, gradient and sigma^2, with the gradient and value only."""
    check_objective(ctx, general, family, n, d, kind, variant, fit)


# ---- c. per-point r -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [orc.STD, orc.ALT], ids=["std", "alt"])
@pytest.mark.parametrize("n,d", [(100, 3), (300, 5)])
@pytest.mark.parametrize("family", MATERN)
def test_objective_with_r(ctx, general, family, n, d, kind):
    """r set: on the diagonal of A for the alt nugget, in the sigma gradient for both (the
    hosts of the one-launch paths must read the nugget bit of the kernel code, not the code)."""
    check_objective(ctx, general, family, n, d, kind, orc.GP4ML, True, with_r=True)


# ---- d. coincident points with a nugget ------------------------------------------------------
@pytest.mark.parametrize("kind", [orc.STD, orc.ALT], ids=["std", "alt"])
@pytest.mark.parametrize("n,d", [(100, 3), (300, 5)])
@pytest.mark.parametrize("family", MATERN)
def test_coincident_points(ctx, general, family, n, d, kind):
    """s = 0 off the diagonal: rho = 1 and g = 3/2 or 5/6 there, nothing divides by r."""
    check_objective(ctx, general, family, n, d, kind, orc.GP4ML, True, coincident=True)


# ---- e. not positive definite ----------------------------------------------------------------
def _not_pd_message(c, family, n, d, want_grad):
    X, f, H = problem(n, d, True)
    hp = hyperparams(d, orc.GP4ML, orc.STD, False)
    c.set_data(X, f, H)
    with pytest.raises(native.NotPositiveDefinite) as e:
        c.objective(orc.GP4ML, code(family, orc.STD), hp, nu_fixed=0.0, want_grad=want_grad)
    return str(e.value)


@pytest.mark.parametrize("family", MATERN)
def test_duplicated_row_without_a_nugget_in_k_tiny(ctx, general, family):
    """(100, 3) with row 7 copied over row 60 and nu = 0: A is exactly singular, the dense
    reference returns None, and the pivot floor inside the launch names the copy's column,
    as the general path's k_pivot_floor does."""
    X, f, H = problem(100, 3, True)
    hp = hyperparams(3, orc.GP4ML, orc.STD, False)
    assert mr.objective(X, f, H, hp, orc.GP4ML, orc.STD, False, family, nu_fixed=0.0) is None
    for want_grad in (True, False):
        msg = _not_pd_message(ctx, family, 100, 3, want_grad)
        gmsg = _not_pd_message(general, family, 100, 3, want_grad)
        print(family, want_grad, "one launch:", msg, "| general path:", gmsg)
        assert "pivot 61)" in msg
        assert "pivot 61)" in gmsg


@pytest.mark.parametrize("family", MATERN)
def test_duplicated_rows_without_a_nugget_in_k_snb(ctx, general, family):
    """n = 300 with two pairs (the pivot is pinned in test_gpu_matern.py): the one-launch and
    the general path give the same message."""
    for want_grad in (True, False):
        msg = _not_pd_message(ctx, family, 300, 5, want_grad)
        gmsg = _not_pd_message(general, family, 300, 5, want_grad)
        print(family, want_grad, "one launch:", msg, "| general path:", gmsg)
        assert msg == gmsg


@pytest.mark.parametrize("n,d", [(100, 3), (300, 5)])
@pytest.mark.parametrize("family", MATERN)
def test_not_pd_then_usable(ctx, family, n, d):
    """After a refused matrix the same context gives a good objective, and the resident-factor
    calls (gpe_factor, beta, posterior at 9 points) run after a one-launch objective."""
    _not_pd_message(ctx, family, n, d, True)
    X, f, H = problem(n, d, True)
    kind = orc.STD
    cond, med = conditioning(family, n, d, kind, True)
    assert cond <= 1e6 and med >= 0.05
    hp = hyperparams(d, orc.GP4ML, kind, True)
    got = ctx.objective(orc.GP4ML, code(family, kind), hp)
    ref = ref_objective(family, n, d, kind, orc.GP4ML, True, False, True)
    assert_matches_reference(got, ref, max(1e-10, 4 * EPS * cond), (family, n, d, "after not-PD"))
    delta, nu = deltas(d), mr.NU[kind]
    ctx.factor(code(family, kind), delta, nu, 1.0, 0.0)
    beta = ctx.beta()
    A = mr.make_A(X, delta, nu, kind, family)[0]
    assert np.max(np.abs(beta - orc.optimal_beta_ref(A, H, f))) <= 1e-8 * (1 + np.max(np.abs(beta)))
    xs = np.random.RandomState(1).uniform(size=(9, d))
    hs = orc.linear_basis(xs)
    mean, var = ctx.posterior(xs, hs, beta, mr.SIGMA, full_var=True)
    rm, rv = mr.posterior(X, f, H, A, xs, hs, beta, mr.SIGMA, delta, nu, kind, family)
    assert np.max(np.abs(mean - rm)) <= 1e-8 * max(1.0, np.max(np.abs(rm)))
    assert np.max(np.abs(var - rv)) <= 1e-8 * max(1.0, np.max(np.abs(rv)))


# ---- f. families interleaved on one context ---------------------------------------------------
@pytest.mark.parametrize("n,d", [(128, 10), (300, 10)])
def test_families_interleaved(ctx, n, d):
    """Gaussian, matern32, matern52 and Gaussian again without set_data in between: the sync
    counters run on across the instantiations, each result is its own reference's and the
    two Gaussian results are bit-identical."""
    X, f, H = problem(n, d)
    kind, variant = orc.STD, orc.GP4ML
    hp = hyperparams(d, variant, kind, True)
    ctx.set_data(X, f, H)
    got = []
    for family in ("gaussian", "matern32", "matern52", "gaussian"):
        got.append((family, ctx.objective(variant, code(family, kind), hp, want_grad=True),
                    ctx.objective(variant, code(family, kind), hp, want_grad=False)))
    for family, wg, vo in got:
        cond, med = conditioning(family, n, d, kind)
        assert cond <= 1e6 and med >= 0.05
        ref = ref_objective(family, n, d, kind, variant, True)
        assert_matches_reference(wg, ref, max(1e-10, 4 * EPS * cond), (family, n, d, "interleaved"))
        assert abs(vo[0] - wg[0]) <= 1e-12 * abs(wg[0])
    (_, a, av), (_, b, bv) = got[0], got[3]
    assert a[0] == b[0] and a[2] == b[2] and a[1].tobytes() == b[1].tobytes()
    assert av[0] == bv[0] and av[2] == bv[2]


# ---- g. end to end ----------------------------------------------------------------------------
def test_train_toy_sim_with_matern52_one_launch(ctx, tmp_path, monkeypatch):
    """setup + train on the toy-sim example (60 points: k_tiny) with `kernel matern52` in its
    beliefs: it completes, and at the hyperparameters it writes the context's objective is
    one launch and gives matern_ref.objective's LLH and sigma^2."""
    d = tmp_path / "toy-sim"
    shutil.copytree(os.path.join(EX, "toy-sim"), d)
    monkeypatch.chdir(d)
    with open("toy-sim_beliefs", "a") as fh:
        fh.write("kernel matern52\n")
    np.random.seed(0)
    E = g.setup("toy-sim_config")
    assert type(E.K) is kernels.kernel_matern52
    g.train(E, auto=True)
    finals = sorted(glob.glob("toy-sim_beliefs-*f"))
    assert len(finals) == 1
    b = files.Beliefs(finals[0])
    assert b.kernel == "matern52"
    delta, nu = np.array(b.delta), b.nugget
    X, f, H = E.training.inputs, E.training.outputs, E.training.H
    assert X.shape[0] <= 128
    A = mr.make_A(X, delta, nu, orc.STD, "matern52")[0]
    cond = float(np.linalg.cond(A))
    assert cond <= 1e6
    rtol = max(1e-10, 4 * EPS * cond)
    ref = mr.objective(X, f, H, delta, orc.MUCM, orc.STD, False, "matern52", nu_fixed=nu)
    ctx.set_data(X, f, H)
    ctx.set_profiling(True)
    try:
        got = ctx.objective(orc.MUCM, code("matern52", orc.STD), delta, nu_fixed=nu)
        launches, ph = ctx.gemm_stats()["launches"], ctx.phase_times()
    finally:
        ctx.set_profiling(False)
    assert launches == 0 and all(ph[p] == 0.0 for p in PHASES) and ph["total"] > 0.0
    # (LLH and sigma^2 only: at the optimum the gradient is a rounding-level remainder)
    print("toy-sim matern52 cond", cond, "LLH", got[0], "reference", ref[0], "sigma^2", got[2], "reference", ref[2])
    assert abs(got[0] - ref[0]) <= rtol * abs(ref[0])
    assert abs(got[2] - ref[2]) <= 1e-10 * abs(ref[2])
    assert abs(b.sigma - np.sqrt(ref[2])) <= 1e-8 * b.sigma
