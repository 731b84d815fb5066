"""gpe_posterior_mean on the GPU: the posterior mean alone from the fused kernel k_post_mean
(gpemu_postmean.hpp), against ctx.posterior's mean and against a np.longdouble evaluation.

The bound.  Both means are h . beta + sum_i gamma_i K*_i with the same gamma and the same
terms; only the order of the n-term sum differs, and the q-term tail is identical.  With
t = sum_i |gamma_i K*_i| and hb = sum_i |hs_i beta_i|, two such sums cannot differ by more than
    B = 2 n eps t + 2 (q + 1) eps (t + hb),
and either is within B / 2 + eps |mean| of the exact value.  A dropped, doubled or padded-in
term is a whole gamma_i K*_i: orders of magnitude above B.  gamma comes from ctx.solve(f - H beta)
and K* from gpe_kernel_covar (which includes the factor 1 - nu of the std kernel); both are
computed once per case and shared.

The cases cover n in {100, 129, 700}, d in {1, 3, 10, 32, 33, 40} (33 and 40, the LDS-staged
instance, with every family), q in {1, d + 1}, m in {1, 127, 128, 129, 1000}, the three families
with both nugget kinds, and one case with r; every case ends on a training point.
"""
import ctypes

import numpy as np
import pytest

import matern_ref as mr
from gp_emu_uqsa_amd import native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps

# (n, d, q, m, family, kind, with r)
CASES = [
    (100, 1, 2, 1, "gaussian", orc.STD, False),
    (129, 3, 1, 127, "matern32", orc.ALT, False),
    (700, 10, 11, 128, "matern52", orc.STD, False),
    (100, 32, 33, 129, "gaussian", orc.ALT, False),
    (129, 33, 34, 1000, "gaussian", orc.STD, False),
    (700, 33, 1, 129, "matern32", orc.STD, False),
    (100, 33, 34, 128, "matern52", orc.ALT, False),
    (129, 40, 1, 127, "gaussian", orc.ALT, False),
    (100, 40, 41, 1, "matern32", orc.ALT, False),
    (700, 40, 41, 1000, "matern52", orc.STD, False),
    (129, 3, 4, 1000, "matern32", orc.STD, False),
    (700, 10, 11, 129, "matern52", orc.ALT, True),
]
IDS = ["-".join(str(v) for v in c) for c in CASES]


def test_cases_cover_every_value():
    assert {c[0] for c in CASES} == {100, 129, 700}
    assert {c[1] for c in CASES} == {1, 3, 10, 32, 33, 40}
    assert {c[2] == 1 for c in CASES} == {True, False} and all(c[2] in (1, c[1] + 1) for c in CASES)
    assert {c[3] for c in CASES} == {1, 127, 128, 129, 1000}
    assert {(c[4], c[5]) for c in CASES} == {(f, k) for f in mr.FAMILIES for k in (orc.STD, orc.ALT)}
    for d in (33, 40):
        assert {c[4] for c in CASES if c[1] == d} == set(mr.FAMILIES)
    assert sum(c[6] for c in CASES) == 1


def deltas(d):
    """Length scales at which the correlations are not all ~ 0 (longer from d = 32 on)."""
    return np.linspace(2.5, 4.0, d) if d >= 32 else np.linspace(0.5, 1.1, d)


def basis(X, q):
    return np.ones((len(X), 1)) if q == 1 else orc.linear_basis(X)


_problems = {}


def problem(n, d, q, m, family, kind, with_r):
    """(X, f, H, r, Xs, Hs, kernel code, delta, nu) of a case: shared, read-only."""
    key = (n, d, q, m, family, kind, with_r)
    if key not in _problems:
        X, f, _ = orc.synthetic_problem(n, d, seed=9)
        Xs = np.random.RandomState(100 + m).uniform(size=(m, d))
        Xs[-1] = X[min(n - 1, 128)]   # a training point (with n = 129 the one in the second tile)
        if m == n:                    # (test_coinciding_points: every point a training point)
            Xs = X.copy()
        r = np.random.RandomState(5).uniform(0, 0.02, n) if with_r else None
        out = (X, f, basis(X, q), r, Xs, basis(Xs, q), mr.FAMILY_CODE[family] | kind, deltas(d), mr.NU[kind])
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _problems[key] = out
    return _problems[key]


def factor(ctx, case):
    X, f, H, r, _, _, code, delta, nu = problem(*case)
    ctx.set_data(X, f, H, r)
    ctx.factor(code, delta, nu, 1.0, 0.0 if r is None else 1.0)


_refs = {}


def reference(ctx, case):
    """With the case's factor resident: (beta, long-double mean, |mean| scale, B), computed once."""
    if case not in _refs:
        X, f, H, r, Xs, Hs, code, delta, nu = problem(*case)
        n, q = H.shape
        beta = ctx.beta()
        gamma = ctx.solve(f - H.dot(beta))
        Ks = ctx.kernel_covar(code, delta, nu, X, Xs)          # n x m, the kernel's factor included
        t = np.abs(Ks * gamma[:, None]).sum(axis=0)
        hb = np.abs(Hs * beta[None, :]).sum(axis=1)
        B = 2 * n * EPS * t + 2 * (q + 1) * EPS * (t + hb)
        ld = np.longdouble
        exact = (Hs.astype(ld) * beta.astype(ld)[None, :]).sum(axis=1) \
            + (Ks.astype(ld) * gamma.astype(ld)[:, None]).sum(axis=0)
        out = (beta, exact, B)
        for a in out:
            a.setflags(write=False)
        _refs[case] = out
    return _refs[case]


def check(ctx, case, what=""):
    """The mean of the resident case against the posterior's and the long-double one."""
    _, _, _, _, Xs, Hs, _, _, _ = problem(*case)
    beta, exact, B = reference(ctx, case)
    pm, _ = ctx.posterior(Xs, Hs, beta, 1.3, full_var=False)
    mean = ctx.posterior_mean(Xs, Hs, beta)
    assert mean.shape == pm.shape == (len(Xs),) and np.all(np.isfinite(mean))
    e1 = np.abs(mean - pm)
    e2 = np.abs(mean.astype(np.longdouble) - exact).astype(np.float64)
    lim2 = B / 2 + EPS * np.abs(mean)
    print(what, case, "max |mean - posterior| / B", np.max(e1 / B), "max |mean - exact| / (B/2 + eps |mean|)",
          np.max(e2 / lim2), "max B", np.max(B), "max |mean|", np.max(np.abs(mean)))
    assert np.all(B > 0)
    assert np.all(e1 <= B)
    assert np.all(e2 <= lim2)
    return mean


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mean_against_posterior_and_long_double(ctx, case):
    factor(ctx, case)
    check(ctx, case)


def test_row_split(ctx):
    """n = 2000 rows for 5 points: 64 row tiles in segments of 6, ten full ones and a ragged
    one of 4, each with a workgroup of its own, added by the finishing kernel."""
    case = (2000, 3, 4, 5, "gaussian", orc.STD, False)
    factor(ctx, case)
    check(ctx, case, "row split")


def test_row_split_with_several_columns(ctx):
    """The same rows for 2 x 512 + 3 points: three columns of workgroups, the last nearly empty."""
    case = (2000, 3, 4, 1027, "matern52", orc.STD, False)
    factor(ctx, case)
    check(ctx, case, "row split, three columns")


@pytest.mark.parametrize("m", [1000, 257])
def test_chunks_return_the_same_bits(ctx, monkeypatch, m):
    """GPEMU_MEAN_CHUNK=256 in a fresh context: 4 (m = 1000) and 2 (m = 257, the last of one
    point) chunks through the two-slot pipeline, bit for bit the single chunk's result."""
    case = (700, 10, 11, m, "matern32", orc.STD, False)
    X, f, H, r, Xs, Hs, code, delta, nu = problem(*case)
    factor(ctx, case)
    one = check(ctx, case, "one chunk")
    beta = reference(ctx, case)[0]
    monkeypatch.setenv("GPEMU_MEAN_CHUNK", "256")
    c = native.Context(0)
    try:
        c.set_data(X, f, H, r)
        c.factor(code, delta, nu, 1.0, 0.0)
        c.set_profiling(True)
        many = c.posterior_mean(Xs, Hs, beta)
        times = np.zeros(8)
        assert c.lib.gpe_phase_times(c._h, times.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 8) == 0
    finally:
        c.close()
    assert times[1] == (m + 255) // 256 and times[0] > 0.0
    assert np.array_equal(many, one)


def test_determinism_and_factor_intact(ctx):
    case = (700, 33, 1, 129, "matern32", orc.STD, False)
    _, _, _, _, Xs, Hs, _, _, _ = problem(*case)
    factor(ctx, case)
    beta = reference(ctx, case)[0]
    before = ctx.posterior(Xs, Hs, beta, 1.3, full_var=False)
    a = ctx.posterior_mean(Xs, Hs, beta)
    b = ctx.posterior_mean(Xs, Hs, beta)
    after = ctx.posterior(Xs, Hs, beta, 1.3, full_var=False)
    assert np.array_equal(a, b)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(ctx.posterior_mean(Xs, Hs, beta), a)


@pytest.mark.parametrize("family", mr.FAMILIES)
def test_coinciding_points(ctx, family):
    """Every point is a training point (s = 0 for one row each): finite, within the bound."""
    case = (129, 3, 4, 129, family, orc.ALT, False)   # m = n: the points are the training points
    assert np.array_equal(problem(*case)[4], problem(*case)[0])
    factor(ctx, case)
    mean = check(ctx, case, "coinciding")
    assert np.all(np.isfinite(mean))


def test_errors(ctx):
    case = (129, 3, 4, 127, "gaussian", orc.STD, False)
    X, f, H, r, Xs, Hs, code, delta, nu = problem(*case)
    c = native.Context(0)
    try:
        c.set_data(X, f, H)
        with pytest.raises(RuntimeError, match=r"\(-4\).*factor"):   # GPE_ERR_STATE
            c.posterior_mean(Xs, Hs, np.zeros(H.shape[1]))
    finally:
        c.close()
    factor(ctx, case)
    beta = reference(ctx, case)[0]
    D = ctypes.POINTER(ctypes.c_double)
    out = np.zeros(len(Xs))
    good = [Xs.ctypes.data_as(D), Hs.ctypes.data_as(D), beta.ctypes.data_as(D), out.ctypes.data_as(D)]
    calls = [(0, good), (-3, good)]
    for i in range(4):
        calls.append((len(Xs), [None if j == i else p for j, p in enumerate(good)]))
    for m, ptrs in calls:
        assert ctx.lib.gpe_posterior_mean(ctx._h, m, *ptrs) == -1   # GPE_ERR_ARG
        assert b"posterior_mean" in ctx.lib.gpe_last_error(ctx._h)
    assert np.all(out == 0.0)
    # the next good call is right
    check(ctx, case, "after errors")
