"""gpe_posterior_groups on the GPU: the posterior covariance inside groups of G consecutive
points (k_post_groupgram / k_post_groupcov, gpemu_postgroup.hpp) against the entries that
ctx.posterior(full_var=True) returns for the same points.

The bound is the project's for a device-against-device posterior, 1e-11 sigma^2 max(1, cdiag)
(cdiag = 1 for the std nugget, 1 + nu^2 for the alt one): both sides form
sigma^2 (own - v_a . v_b + t_a . t_b) from the same V = L^-1 K* and the same T; only the order
of the n-term sums differs, n eps |v_a| |v_b| <= 520 * 2.2e-16 ~ 1.2e-13 here.  A dropped or
misplaced column of V is a whole v_a . v_b: many orders above it.

Shapes and kernels are test_gpu_matern.py's; the (G, m) cases:
  (1, 7) the smallest; (2, 256); (5, 265) groups of 5 side by side in one MFMA tile and a group
  across a 128-point tile; (16, 256) the last group ends on the padded chunk's last column;
  (17, 34) two tiles; (42, 84) three tiles, with d = 40 among the shapes; (64, 128) four tiles.
"""
import ctypes

import numpy as np
import pytest

import matern_ref as mr
from gp_emu_uqsa_amd import native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
SIGMA = mr.SIGMA
GM = [(1, 7), (2, 256), (5, 265), (16, 256), (17, 34), (42, 84), (64, 128)]
SHAPES = [(129, 2), (300, 5), (520, 3), (260, 40)]
# (family, kind, with r)
KERNELS = [("gaussian", orc.STD, False), ("gaussian", orc.ALT, False), ("matern32", orc.STD, False),
           ("matern52", orc.ALT, False)]
CONFIGS = [(n, d) + k for (n, d) in SHAPES for k in KERNELS] + [(300, 5, "matern52", orc.ALT, True)]
IDS = ["-".join(str(v) for v in c) for c in CONFIGS]

_cache = {}


def problem(n, d):
    """(X, f, H) of a shape, as test_gpu_matern.py builds it (shared, read-only)."""
    if (n, d) not in _cache:
        out = orc.synthetic_problem(n, d, seed=9)
        for a in out:
            a.setflags(write=False)
        _cache[(n, d)] = out
    return _cache[(n, d)]


def points(n, d, m):
    """m points (shared, read-only), every 11th a training point."""
    key = ("pts", n, d, m)
    if key not in _cache:
        X = problem(n, d)[0]
        Xs = np.random.RandomState(50 + m).uniform(size=(m, d))
        Xs[::11] = X[np.arange(0, m, 11) % n]
        Hs = orc.linear_basis(Xs)
        Xs.setflags(write=False)
        Hs.setflags(write=False)
        _cache[key] = (Xs, Hs)
    return _cache[key]


def bound(kind):
    cdiag = 1.0 + mr.NU[kind] ** 2 if kind == orc.ALT else 1.0
    return 1e-11 * SIGMA ** 2 * max(1.0, cdiag)


def factor(ctx, n, d, family, kind, with_r=False):
    X, f, H = problem(n, d)
    r = np.random.RandomState(5).uniform(0, 0.02, n) if with_r else None
    ctx.set_data(X, f, H, r)
    ctx.factor(mr.FAMILY_CODE[family] | kind, mr.deltas(d), mr.NU[kind], 1.0, 1.0 if with_r else 0.0)
    return ctx.beta()


def blocks_of(full, G):
    m = full.shape[0]
    return np.stack([full[g * G:(g + 1) * G, g * G:(g + 1) * G] for g in range(m // G)])


def check(ctx, Xs, Hs, beta, G, lim, what):
    """Blocks, diagonal and mean of the resident case against gpe_posterior's."""
    m = len(Xs)
    mean, cov = ctx.posterior_groups(Xs, Hs, beta, SIGMA, G)
    fm, full = ctx.posterior(Xs, Hs, beta, SIGMA, full_var=True)
    dm, diag = ctx.posterior(Xs, Hs, beta, SIGMA, full_var=False)
    assert mean.shape == (m,) and cov.shape == (m // G, G, G) and np.all(np.isfinite(cov))
    eb = np.max(np.abs(cov - blocks_of(full, G)))
    ed = np.max(np.abs(np.diagonal(cov, axis1=1, axis2=2).ravel() - diag))
    print(what, "G", G, "m", m, "max |block - full| / bound", eb / lim, "max |diagonal - diag| / bound", ed / lim)
    assert eb <= lim and ed <= lim
    # (the same chunk through the same kernels: the means are gpe_posterior's)
    assert np.array_equal(mean, dm) and np.array_equal(mean, fm)
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    return mean, cov


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_blocks_against_the_full_covariance(ctx, cfg):
    n, d, family, kind, with_r = cfg
    beta = factor(ctx, n, d, family, kind, with_r)
    for G, m in GM:
        Xs, Hs = points(n, d, m)
        check(ctx, Xs, Hs, beta, G, bound(kind), cfg)


def test_configs_cover_the_cases():
    assert {(c[0], c[1]) for c in CONFIGS} == set(SHAPES) and (42, 84) in GM and (260, 40) in SHAPES
    assert {c[2] for c in CONFIGS} == set(mr.FAMILIES)
    assert {(c[2], c[3]) for c in CONFIGS} >= {("gaussian", orc.STD), ("gaussian", orc.ALT)}
    assert sum(c[4] for c in CONFIGS) == 1 and all(mr.NU[k] > 0 for k in (orc.STD, orc.ALT))


@pytest.mark.parametrize("family", mr.FAMILIES)
def test_a_group_with_the_same_point_twice(ctx, family):
    """Equal coordinates at different indices: the off-diagonal form, as the full covariance."""
    n, d, kind = 129, 2, orc.ALT
    beta = factor(ctx, n, d, family, kind)
    Xs = points(n, d, 34)[0].copy()
    Xs[3] = Xs[1]          # inside the first group of 17
    Xs[33] = Xs[17]        # first and last of the second
    Xs[20] = problem(n, d)[0][128]
    Xs[21] = Xs[20]        # a training point twice
    _, cov = check(ctx, Xs, orc.linear_basis(Xs), beta, 17, bound(kind), "twice " + family)
    # the pair's covariance is the off-diagonal form (no nugget term), so below the variances
    assert cov[0, 3, 1] < min(cov[0, 1, 1], cov[0, 3, 3])


def test_more_than_one_chunk(ctx):
    """n = 129, G = 5, m = 8500: chunks of 8190 and 310 points."""
    n, d, G, m, kind = 129, 2, 5, 8500, orc.STD
    beta = factor(ctx, n, d, "matern32", kind)
    Xs, Hs = points(n, d, m)
    ctx.set_profiling(True)
    try:
        mean, cov = ctx.posterior_groups(Xs, Hs, beta, SIGMA, G)
        times = np.zeros(8)
        assert ctx.lib.gpe_phase_times(ctx._h, times.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 8) == 0
    finally:
        ctx.set_profiling(False)
    assert times[1] == 2 and times[0] > 0.0
    dm, diag = ctx.posterior(Xs, Hs, beta, SIGMA, full_var=False)
    lim = bound(kind)
    ed = np.max(np.abs(np.diagonal(cov, axis1=1, axis2=2).ravel() - diag))
    # (the chunks are cut elsewhere than gpe_posterior's: the means to rounding)
    assert np.max(np.abs(mean - dm)) <= 1e-12 * max(1.0, np.max(np.abs(dm))) and ed <= lim
    gs = [0, 8190 // G - 1, 8190 // G, m // G - 1]     # first, both sides of point 8190, last
    idx = np.concatenate([np.arange(g * G, (g + 1) * G) for g in gs])
    _, full = ctx.posterior(Xs[idx], Hs[idx], beta, SIGMA, full_var=True)
    eb = max(np.max(np.abs(cov[g] - full[k * G:(k + 1) * G, k * G:(k + 1) * G])) for k, g in enumerate(gs))
    print("two chunks: max |diagonal - diag| / bound", ed / lim, "max |block - full| / bound", eb / lim)
    assert eb <= lim
    assert np.array_equal(cov, cov.transpose(0, 2, 1))


@pytest.mark.parametrize("G,m,pick", [(5, 265, [0, 1, 2, 25, 52]), (17, 34, [1]), (12, 8400, [0, 682, 699])])
def test_independence_and_repeatability(ctx, G, m, pick):
    """A group's block from a one-group call equals, bit for bit, its block inside a larger call
    at another position (another place in its MFMA tile, another workgroup, the second chunk);
    two identical calls are bit-equal; ctx.posterior afterwards is unchanged."""
    n, d = 300, 5
    beta = factor(ctx, n, d, "matern52", orc.ALT)
    Xs, Hs = points(n, d, m)
    before = ctx.posterior(Xs[:200], Hs[:200], beta, SIGMA, full_var=True)
    mean, cov = ctx.posterior_groups(Xs, Hs, beta, SIGMA, G)
    again = ctx.posterior_groups(Xs, Hs, beta, SIGMA, G)
    assert np.array_equal(mean, again[0]) and np.array_equal(cov, again[1])
    for g in pick:
        sl = slice(g * G, (g + 1) * G)
        m1, c1 = ctx.posterior_groups(Xs[sl], Hs[sl], beta, SIGMA, G)
        assert np.array_equal(c1[0], cov[g]) and np.array_equal(m1, mean[sl]), g
    after = ctx.posterior(Xs[:200], Hs[:200], beta, SIGMA, full_var=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_int8_product(monkeypatch):
    """V from the int8 product (started from n_pad 2048 here, as test_gpu_posterior.py does):
    against that context's full covariance, and against a GPEMU_OZAKI=0 context's blocks."""
    from gp_emu_uqsa_amd import synthetic
    n, d, G, m, sigma = 2048, 5, 12, 240, 0.9
    X, f, H = synthetic.problem(n, d, seed=5)
    delta = np.full(d, 0.7)
    xs = synthetic.design(m, d, seed=8)
    hs = synthetic.linear_basis(xs)
    out = {}
    monkeypatch.setenv("GPEMU_OZAKI_MIN_NP", "2048")
    for oz in ("0", "1"):
        monkeypatch.setenv("GPEMU_OZAKI", oz)
        c = native.Context(0)
        try:
            c.set_data(X, f, H)
            c.factor(native.KERNEL_STD, delta, 1e-3, 1.0, 0.0)
            beta = c.beta()
            out[oz] = (c.posterior_groups(xs, hs, beta, sigma, G), c.posterior(xs, hs, beta, sigma, full_var=True))
        finally:
            c.close()
    lim = 1e-11 * sigma ** 2
    (m1, c1), (fm1, full1) = out["1"]
    (m0, c0), _ = out["0"]
    e_full = np.max(np.abs(c1 - blocks_of(full1, G)))
    e_fp64 = np.max(np.abs(c1 - c0))
    print("int8: max |block - full| / bound", e_full / lim, "max |int8 - fp64| / bound", e_fp64 / lim)
    assert np.array_equal(m1, fm1) and np.array_equal(m1, m0)
    assert e_full <= lim and e_fp64 <= lim


def test_errors(ctx):
    n, d, G, m = 129, 2, 2, 256
    X, f, H = problem(n, d)
    Xs, Hs = points(n, d, m)
    c = native.Context(0)
    try:
        c.set_data(X, f, H)
        with pytest.raises(RuntimeError, match=r"\(-4\).*factor"):   # GPE_ERR_STATE
            c.posterior_groups(Xs, Hs, np.zeros(H.shape[1]), SIGMA, G)
    finally:
        c.close()
    beta = factor(ctx, n, d, "gaussian", orc.STD)
    D = ctypes.POINTER(ctypes.c_double)
    mean, cov = np.zeros(m), np.zeros((m // G, G, G))
    good = [Xs.ctypes.data_as(D), Hs.ctypes.data_as(D), beta.ctypes.data_as(D), SIGMA, mean.ctypes.data_as(D),
            cov.ctypes.data_as(D)]
    calls = [(m, 0, good), (m, 65, good), (m, -1, good), (255, 2, good), (m, 3, good), (0, 2, good), (-4, 2, good)]
    for i in (0, 1, 2, 4, 5):
        calls.append((m, G, [None if j == i else p for j, p in enumerate(good)]))
    for mm, gg, args in calls:
        assert ctx.lib.gpe_posterior_groups(ctx._h, mm, gg, *args) == -1, (mm, gg)   # GPE_ERR_ARG
        assert b"posterior" in ctx.lib.gpe_last_error(ctx._h)
    assert np.all(mean == 0.0) and np.all(cov == 0.0)
    check(ctx, Xs, Hs, beta, G, bound(orc.STD), "after errors")
