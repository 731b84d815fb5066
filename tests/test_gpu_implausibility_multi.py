"""A multi-output member of the resident emulator set (gpe_hm_add_multi, gpe_hm_outputs,
gpe_hm_implausibility_mv; native.EmulatorSet.add_multi / implausibility_mv; MultiEmulator items
of history_match.EmulatorSet) on the GPU.

Emulators come from synthetic_problem at delta in [0.5, 1.1] and nu = 1e-3 with the p outputs of
multi_output_ref.outputs, each column divided by its factor 1 + a / 2 so that cond(Sigma-hat) <=
1e3 (computed on the CPU: 1, 125, 4.3, 6.7, 3.1, 9.0 for the six cases; asserted below).
Bounds, the project's own (test_gpu_implausibility.py, test_gpu_posterior.py): two routes to one
variance on one factor 1e-11 sigma^2 (here sigma^2 = Sigma_aa), means 1e-11 (1 + max|mean|), the
NumPy reference 1e-8.  The joint I^2: 1e-10 relative against NumPy's solve on the GPU's own mean
and c (p eps cond(V) = 3.4e-12, see test_implausibility_multi_host.py), 1e-7 relative against
the reference.
Shapes: p + q = 16 is one block of [Gamma, G] rows with a ragged n, 17 rows two blocks, n = 300
the narrow tile, (512, 28 + 4) 32 rows and n at the limit.
"""
import functools
import os
import shutil

import numpy as np
import pytest

import implausibility_multi_ref as mhr
import implausibility_ref as iref
import multi_output_ref as mo
from gp_emu_uqsa_amd import native
from gp_emu_uqsa_amd.history_match import _imaxes
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EX = os.path.join(HERE, "golden", "examples")
NU = 1e-3
FAMILY = {"gaussian": 0x00, "matern32": native.KERNEL_MATERN32, "matern52": native.KERNEL_MATERN52}
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5
PT = 64


def _forms(q):
    return [-1] + list(range(q - 1)), [1.0] + [0.0] * (q - 1)


def _hs(q, xs):
    return np.ascontiguousarray(orc.linear_basis(xs)[:, :q])


@functools.lru_cache(maxsize=None)
def _problem(n, d, q, p, kind=orc.STD, family="gaussian", with_r=False):
    """A case's data and its reference estimates (shared, read-only)."""
    X, _, H = orc.synthetic_problem(n, d, seed=9)
    H = np.ascontiguousarray(H[:, :q])
    F = np.ascontiguousarray(mo.outputs(X, p) / (1.0 + 0.5 * np.arange(p)))
    r = np.random.RandomState(n + 1).uniform(0.0, 0.02, n) if with_r else None
    delta = np.linspace(0.5, 1.1, d)
    B_ref, S_ref = mhr.estimates(X, F, H, delta, NU, kind, family, r)
    for a in (X, H, F, B_ref, S_ref):
        a.setflags(write=False)
    return dict(X=X, H=H, F=F, r=r, delta=delta, kind=kind, family=family, n=n, d=d, q=q, p=p, B_ref=B_ref,
                S_ref=S_ref)


def _resident(ctx, e):
    """Make e the context's resident data, outputs and factor; returns B from the factor."""
    ctx.set_data(e["X"], e["F"][:, 0], e["H"], e["r"])
    ctx.set_outputs(e["F"])
    ctx.factor(e["kind"] | FAMILY[e["family"]], e["delta"], NU, 1.0, 1.0 if e["r"] is not None else 0.0)
    return ctx.beta_multi()


def _add_multi(hset, ctx, e, B, Sigma, active=None):
    hdim, hval = _forms(e["q"])
    return hset.add_multi(ctx, list(range(e["d"])) if active is None else list(active), hdim, hval, B, Sigma)


def _status(excinfo):
    return getattr(excinfo.value, "status", None)


CASES = [(60, 3, 4, 1, orc.STD, "gaussian", False), (61, 3, 4, 12, orc.ALT, "gaussian", False),
         (129, 10, 11, 6, orc.STD, "matern32", False), (300, 10, 11, 8, orc.STD, "matern52", False),
         (512, 3, 4, 28, orc.STD, "gaussian", False), (17, 1, 2, 3, orc.ALT, "gaussian", True)]
IDS = ["-".join(str(v) for v in c) for c in CASES]


# ------------------------------------------------------------------ 1. parts, case by case
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parts_against_the_existing_paths(ctx, case):
    n, d, q, p = case[:4]
    e = _problem(*case)
    B = _resident(ctx, e)
    Sigma = e["S_ref"]
    xs = np.random.RandomState(n + 7).uniform(size=(200, d))
    hs = _hs(q, xs)
    m0 = ctx.posterior_mean_multi(xs, hs, B)                                    # 200 x p
    _, c0 = ctx.posterior(xs, hs, B[:, 0], 1.0, full_var=False, precision=64)
    zs, ve = np.linspace(0.5, 1.5, p), np.linspace(0.01, 0.02, p)
    hset = native.EmulatorSet(0)
    try:
        assert _add_multi(hset, ctx, e, B, Sigma) == 0 and len(hset) == 1 and hset.outputs == p
        assert hset.member_outputs(0) == p
        imax, mean, var = hset.implausibility(xs, zs, ve, maxno=p, parts=True)
        imax1 = hset.implausibility(xs, zs, ve, maxno=1)
    finally:
        hset.close()
    assert mean.shape == var.shape == (p, 200) and imax.shape == (200, p) and imax1.shape == (200, 1)
    sd = np.diag(Sigma)
    dm = np.max(np.abs(mean.T - m0))
    dv = np.max(np.abs(var - sd[:, None] * c0[None, :]) / sd[:, None])
    m_ref, c_ref = mhr.parts(e["X"], e["F"], e["H"], xs, hs, B, e["delta"], NU, e["kind"], e["family"], e["r"])
    rm, rv = np.max(np.abs(mean - m_ref)), np.max(np.abs(var - sd[:, None] * c_ref[None, :]))
    print(f"{case}: |dmean| {dm:.3e} (bound {1e-11 * (1 + np.max(np.abs(m0))):.3e}) |dvar| / Sigma_aa {dv:.3e} "
          f"(bound 1e-11); against the reference {rm:.3e} {rv:.3e}; B against the reference "
          f"{np.max(np.abs(B - e['B_ref'])):.3e}")
    assert dm < 1e-11 * (1.0 + np.max(np.abs(m0)))
    assert dv < 1e-11
    assert rm < 1e-8 and rv < 1e-8
    with np.errstate(invalid="ignore"):
        I2 = (mean - zs[:, None]) ** 2 / (var + ve[:, None])
        assert np.array_equal(imax, _imaxes(I2.T, p), equal_nan=True)
        assert np.array_equal(imax1, _imaxes(I2.T, 1), equal_nan=True)


# ------------------------------------------------------------------ 2. the joint measure
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_joint_measure(ctx, case):
    n, d, q, p = case[:4]
    e = _problem(*case)
    B = _resident(ctx, e)
    Sigma = e["S_ref"]
    cond = np.linalg.cond(Sigma)
    assert cond <= 1e3, cond
    xs = np.random.RandomState(n + 8).uniform(size=(200, d))
    hs = _hs(q, xs)
    V = mhr.spd(p, 1e3, seed=n, scale=0.05)
    assert np.linalg.cond(V) <= 1.0001e3
    z = np.linspace(0.5, 1.5, p)
    vd = np.linspace(0.01, 0.02, p)
    hset, diag = native.EmulatorSet(0), native.EmulatorSet(0)
    try:
        _add_multi(hset, ctx, e, B, Sigma)
        _add_multi(diag, ctx, e, B, np.diag(np.diag(Sigma)))
        I2, mean, c = hset.implausibility_mv(0, xs, z, V, parts=True)
        assert np.array_equal(hset.implausibility_mv(0, xs, z, V), I2)           # without the parts: the same bits
        _, mean_u, var_u = hset.implausibility(xs, z, vd, maxno=1, parts=True)
        I2d = diag.implausibility_mv(0, xs, z, np.diag(vd))
        imax_d, mean_d, var_d = diag.implausibility(xs, z, vd, maxno=p, parts=True)
        for bad in (np.diag(np.r_[0.0, np.ones(p - 1)]), -np.eye(p), np.full((p, p), np.nan)):
            with pytest.raises(native.NotPositiveDefinite) as ei:
                hset.implausibility_mv(0, xs, z, bad)
            assert "V is not positive definite" in str(ei.value)
        assert np.array_equal(hset.implausibility_mv(0, xs, z, V), I2)           # the set still works
    finally:
        hset.close()
        diag.close()
    assert I2.shape == (200,) and mean.shape == (p, 200) and c.shape == (200,)
    assert np.array_equal(mean, mean_u) and np.array_equal(np.diag(Sigma)[:, None] * c[None, :], var_u)
    want = mhr.joint(mean, c, Sigma, z, V)
    own = np.max(np.abs(I2 - want) / want)
    m_ref, c_ref = mhr.parts(e["X"], e["F"], e["H"], xs, hs, B, e["delta"], NU, e["kind"], e["family"], e["r"])
    ref = mhr.joint(m_ref, c_ref, Sigma, z, V)
    rel = np.max(np.abs(I2 - ref) / ref)
    uni = np.sum((mean_d - z[:, None]) ** 2 / (var_d + vd[:, None]), axis=0)
    du = np.max(np.abs(I2d - uni) / uni)
    print(f"{case}: cond(Sigma) {cond:.1f}; joint I^2 against NumPy's solve on the GPU's parts {own:.3e} (bound 1e-10), "
          f"against the reference {rel:.3e} (bound 1e-7); diagonal Sigma and V against the univariate sum {du:.3e} "
          f"(bound 1e-12)")
    assert own <= 1e-10
    assert rel <= 1e-7
    assert du <= 1e-12
    if p == 1:
        assert np.max(np.abs(I2d - imax_d[:, 0] ** 2) / I2d) <= 1e-13


# ------------------------------------------------------------------ 3. a mixed set
def _single(n, d, q, seed, kind=orc.STD, family="gaussian"):
    X, f, H = orc.synthetic_problem(n, d, seed=seed)
    return dict(XT=X, fT=f, HT=np.ascontiguousarray(H[:, :q]), delta=np.linspace(0.5, 1.1, d), nu=NU, kind=kind,
                family=family, sigma=0.9, r=None, r_diag=None, n=n, d=d, q=q)


def _add_single(hset, ctx, e, active):
    ctx.set_data(e["XT"], e["fT"], e["HT"], None)
    ctx.factor(e["kind"] | FAMILY[e["family"]], e["delta"], NU, 1.0, 0.0)
    e["beta"] = ctx.beta()
    e["active"] = list(active)
    return hset.add(ctx, e["active"], *_forms(e["q"]), e["beta"], e["sigma"])


def test_mixed_set(ctx):
    s0, s2 = _single(60, 3, 4, 11), _single(300, 1, 2, 13, family="matern32")
    em = _problem(130, 2, 3, 3, orc.ALT, "matern52", False)
    xs = np.random.RandomState(5).uniform(size=(150, 4))
    xs[40, [0, 1, 2]] = s0["XT"][7]
    zs = np.array([2.0, 0.5, 1.0, 1.5, 2.5])
    ve = np.array([0.01, 0.02, 0.03, 0.04, 0.05])
    mixed, alone = native.EmulatorSet(0), native.EmulatorSet(0)
    try:
        assert _add_single(mixed, ctx, s0, [0, 1, 2]) == 0
        B = _resident(ctx, em)
        assert _add_multi(mixed, ctx, em, B, em["S_ref"], active=[3, 0]) == 1
        assert _add_single(mixed, ctx, s2, [2]) == 2
        assert mixed.outputs == 5 and len(mixed) == 3
        assert [mixed.member_outputs(i) for i in range(3)] == [1, 3, 1]
        _add_single(alone, ctx, s0, [0, 1, 2])
        _add_single(alone, ctx, s2, [2])
        assert alone.outputs == 2 and len(alone) == 2
        imax, mean, var = mixed.implausibility(xs, zs, ve, maxno=5, parts=True)
        _, mean_a, var_a = alone.implausibility(xs, zs[[0, 4]], ve[[0, 4]], maxno=2, parts=True)
        assert np.array_equal(mean[[0, 4]], mean_a) and np.array_equal(var[[0, 4]], var_a)
        # the member's rows against the reference, through its own columns of the candidates
        x = np.ascontiguousarray(xs[:, [3, 0]])
        m_ref, c_ref = mhr.parts(em["X"], em["F"], em["H"], x, _hs(3, x), B, em["delta"], NU, em["kind"], em["family"])
        assert np.max(np.abs(mean[1:4] - m_ref)) < 1e-8
        assert np.max(np.abs(var[1:4] - np.diag(em["S_ref"])[:, None] * c_ref[None, :])) < 1e-8
        _, m_s, v_s = iref.implausibility([s0, s2], xs, zs[[0, 4]], ve[[0, 4]], maxno=1)
        assert np.max(np.abs(mean[[0, 4]] - m_s)) < 1e-8 and np.max(np.abs(var[[0, 4]] - v_s)) < 1e-8
        for k in range(1, 6):
            got = mixed.implausibility(xs, zs, ve, maxno=k)
            I2 = (mean - zs[:, None]) ** 2 / (var + ve[:, None])
            assert got.shape == (150, k) and np.array_equal(got, _imaxes(I2.T, k)), k
        assert np.array_equal(imax, _imaxes(I2.T, 5))
        # var + var_extra < 0 at one point for output 1 of the member: a NaN that sorts last
        order = np.argsort(var[2])
        pt = int(order[0])
        ve2 = ve.copy()
        ve2[2] = -0.5 * (var[2, order[0]] + var[2, order[1]])
        assert var[2, order[1]] > var[2, pt] > 0.0
        for k in (1, 3, 5):
            got = mixed.implausibility(xs, zs, ve2, maxno=k)
            with np.errstate(invalid="ignore"):
                I2 = (mean - zs[:, None]) ** 2 / (var + ve2[:, None])
                want = _imaxes(I2.T, k)
            assert I2[2, pt] < 0.0 and np.sum(I2 < 0.0) == 1
            assert np.array_equal(got, want, equal_nan=True)
            assert np.isnan(got[pt, -1]) and not np.any(np.isnan(np.delete(got, pt, axis=0)))
            assert not np.any(np.isnan(got[pt, :-1]))
        with pytest.raises(RuntimeError) as ei:                  # the joint measure of a single member
            mixed.implausibility_mv(0, xs, [1.0], np.eye(1))
        assert _status(ei) == ERR_ARG
        with pytest.raises(RuntimeError) as ei:                  # maxno = outputs + 1
            mixed.implausibility(xs, zs, ve, maxno=6)
        assert _status(ei) == ERR_ARG
        with pytest.raises(ValueError):                          # one z per output, checked before the call
            mixed.implausibility(xs, zs[:3], ve[:3])
        with pytest.raises(ValueError):
            mixed.implausibility_mv(1, xs, zs[:2], np.eye(2))
    finally:
        mixed.close()
        alone.close()


# ------------------------------------------------------------------ 4. p = 1 against the single member
def test_one_output_against_the_single_member(ctx):
    e = _problem(129, 3, 4, 1)
    s2 = 0.81
    xs = np.random.RandomState(2).uniform(size=(200, 3))
    hset = native.EmulatorSet(0)
    try:
        ctx.set_data(e["X"], e["F"][:, 0], e["H"], None)
        ctx.factor(orc.STD, e["delta"], NU, 1.0, 0.0)
        beta = ctx.beta()
        assert hset.add(ctx, [0, 1, 2], *_forms(4), beta, np.sqrt(s2)) == 0
        ctx.set_outputs(e["F"])
        assert hset.add_multi(ctx, [0, 1, 2], *_forms(4), beta[:, None], [[s2]]) == 1
        imax, mean, var = hset.implausibility(xs, [1.0, 1.0], [0.01, 0.01], maxno=2, parts=True)
    finally:
        hset.close()
    dm, dv = np.max(np.abs(mean[0] - mean[1])), np.max(np.abs(var[0] - var[1]))
    print(f"p = 1 against gpe_hm_add: |dmean| {dm:.3e} |dvar| {dv:.3e}")
    assert dm < 1e-11 * (1.0 + np.max(np.abs(mean[0])))
    assert dv < 1e-11 * s2


# ------------------------------------------------------------------ 5. independence
def _pair(ctx, hset):
    """A set of one multi-output member per tile shape: n = 61 (64 points per workgroup), n = 300 (32)."""
    es = [_problem(61, 3, 4, 12, orc.ALT), _problem(300, 3, 4, 5, orc.STD, "matern52")]
    Bs = []
    for e in es:
        Bs.append(_resident(ctx, e))
        _add_multi(hset, ctx, e, Bs[-1], e["S_ref"])
    return es, Bs


def test_independence_of_tiling(ctx, monkeypatch):
    m = 3 * PT + 5
    xs = np.random.RandomState(9).uniform(size=(m, 3))
    zs, ve = np.linspace(0.5, 1.5, 17), np.linspace(0.01, 0.02, 17)
    one = native.EmulatorSet(0)
    monkeypatch.setenv("GPEMU_HM_CHUNK", str(PT))
    many = native.EmulatorSet(0)
    monkeypatch.delenv("GPEMU_HM_CHUNK")
    try:
        es, Bs = _pair(ctx, one)
        xs[PT + 2] = es[1]["X"][100]                             # a candidate on a training point
        _pair(ctx, many)
        V = [mhr.spd(12, 1e3, 1, 0.05), mhr.spd(5, 1e3, 2, 0.05)]
        a = one.implausibility(xs, zs, ve, maxno=3, parts=True)
        b = many.implausibility(xs, zs, ve, maxno=3, parts=True)
        for u, v in zip(a, b):
            assert np.array_equal(u, v, equal_nan=True)          # the chunk length does not show
        for u, v in zip(a, one.implausibility(xs, zs, ve, maxno=3, parts=True)):
            assert np.array_equal(u, v, equal_nan=True)          # nor does the call
        ja = [one.implausibility_mv(i, xs, zs[o:o + k], V[i], parts=True) for i, (o, k) in enumerate([(0, 12), (12, 5)])]
        jb = [many.implausibility_mv(i, xs, zs[o:o + k], V[i], parts=True) for i, (o, k) in enumerate([(0, 12), (12, 5)])]
        for i, (o, k) in enumerate([(0, 12), (12, 5)]):
            for u, v in zip(ja[i], jb[i]):
                assert np.array_equal(u, v)
            for u, v in zip(ja[i], one.implausibility_mv(i, xs, zs[o:o + k], V[i], parts=True)):
                assert np.array_equal(u, v)
            assert np.array_equal(ja[i][1], a[1][o:o + k])       # both entries: the same means
            assert np.all(np.isfinite(ja[i][0]))
        for mm in (1, PT + 1):
            for hset in (one, many):
                c = hset.implausibility(xs[:mm], zs, ve, maxno=3, parts=True)
                assert np.array_equal(c[0], a[0][:mm]) and np.array_equal(c[1], a[1][:, :mm]) \
                    and np.array_equal(c[2], a[2][:, :mm]), mm  # nor does m
                for i, (o, k) in enumerate([(0, 12), (12, 5)]):
                    j = hset.implausibility_mv(i, xs[:mm], zs[o:o + k], V[i], parts=True)
                    assert np.array_equal(j[0], ja[i][0][:mm]) and np.array_equal(j[1], ja[i][1][:, :mm]) \
                        and np.array_equal(j[2], ja[i][2][:mm]), mm
        assert np.all(np.isfinite(a[1][:, PT + 2])) and np.all(np.isfinite(a[2][:, PT + 2]))
    finally:
        one.close()
        many.close()


# ------------------------------------------------------------------ 6. the context stays intact
def test_context_left_intact(ctx):
    e = _problem(129, 3, 4, 6)
    other = _problem(200, 2, 3, 2, orc.STD, "matern32")
    xs = np.random.RandomState(3).uniform(size=(70, 3))
    hs = _hs(4, xs)
    B = _resident(ctx, e)

    def state():
        return (ctx.posterior_mean_multi(xs, hs, B), *ctx.posterior(xs, hs, B[:, 0], 1.0, full_var=False), *ctx.loo(1.0),
                ctx.beta_multi())
    before = state()
    hset = native.EmulatorSet(0)
    try:
        _add_multi(hset, ctx, e, B, e["S_ref"])
        for u, v in zip(state(), before):
            assert np.array_equal(u, v)
        z, V = np.linspace(0.5, 1.5, 6), mhr.spd(6, 1e3, 4, 0.05)
        out = hset.implausibility(xs, z, np.full(6, 0.01), maxno=2, parts=True) + hset.implausibility_mv(0, xs, z, V, True)
        _resident(ctx, other)                                    # the context moves on to other data
        xo = np.random.RandomState(4).uniform(size=(30, 2))
        ctx.posterior_mean_multi(xo, _hs(3, xo), ctx.beta_multi())
        again = hset.implausibility(xs, z, np.full(6, 0.01), maxno=2, parts=True) + hset.implausibility_mv(0, xs, z, V, True)
        for u, v in zip(out, again):
            assert np.array_equal(u, v)
    finally:
        hset.close()


# ------------------------------------------------------------------ 7. errors
def test_errors(ctx):
    hset = native.EmulatorSet(0)
    fresh = native.Context(0)
    try:
        e = _problem(60, 3, 4, 3)
        forms = _forms(4)
        fresh.set_data(e["X"], e["F"][:, 0], e["H"])
        fresh.set_outputs(e["F"])
        with pytest.raises(RuntimeError) as ei:                  # no factor
            hset.add_multi(fresh, [0, 1, 2], *forms, np.zeros((4, 3)), np.eye(3))
        assert _status(ei) == ERR_STATE and len(hset) == 0 and hset.outputs == 0
        fresh.set_data(e["X"], e["F"][:, 0], e["H"])             # (a new gpe_set_data drops the outputs)
        fresh.factor(orc.STD, e["delta"], NU, 1.0, 0.0)
        with pytest.raises(RuntimeError) as ei:                  # no outputs
            hset.add_multi(fresh, [0, 1, 2], *forms, np.zeros((4, 3)), np.eye(3))
        assert _status(ei) == ERR_STATE and len(hset) == 0
        B = _resident(ctx, e)
        with pytest.raises(RuntimeError) as ei:                  # p other than the context's
            hset.add_multi(ctx, [0, 1, 2], *forms, B[:, :2], np.eye(2))
        assert _status(ei) == ERR_ARG and len(hset) == 0
        with pytest.raises(RuntimeError) as ei:                  # hdim names an input the emulator has not
            hset.add_multi(ctx, [0, 1, 2], [-1, 0, 1, 3], forms[1], B, e["S_ref"])
        assert _status(ei) == ERR_ARG and len(hset) == 0
        wide = _problem(60, 3, 4, 29)                            # p + q = 33
        Bw = _resident(ctx, wide)
        with pytest.raises(RuntimeError) as ei:
            _add_multi(hset, ctx, wide, Bw, wide["S_ref"])
        assert _status(ei) == ERR_UNSUPPORTED and len(hset) == 0 and hset.outputs == 0
        big = _problem(513, 2, 3, 2)                             # n = 513
        Bb = _resident(ctx, big)
        with pytest.raises(RuntimeError) as ei:
            _add_multi(hset, ctx, big, Bb, big["S_ref"])
        assert _status(ei) == ERR_UNSUPPORTED and len(hset) == 0
        full = _problem(60, 3, 4, 16)                            # 16 + 16 outputs fill the set
        Bf = _resident(ctx, full)
        assert _add_multi(hset, ctx, full, Bf, full["S_ref"]) == 0
        assert _add_multi(hset, ctx, full, Bf, full["S_ref"]) == 1 and hset.outputs == 32
        with pytest.raises(RuntimeError) as ei:                  # a 33rd output, by either entry
            hset.add(ctx, [0, 1, 2], *forms, Bf[:, 0], 1.0)
        assert _status(ei) == ERR_UNSUPPORTED and len(hset) == 2 and hset.outputs == 32
        B3 = _resident(ctx, e)
        with pytest.raises(RuntimeError) as ei:
            _add_multi(hset, ctx, e, B3, e["S_ref"])
        assert _status(ei) == ERR_UNSUPPORTED and len(hset) == 2 and hset.outputs == 32
        xs = np.random.RandomState(1).uniform(size=(5, 3))
        with pytest.raises(ValueError):                          # z / var_extra: one entry per output
            hset.implausibility(xs, np.ones(2), np.ones(2))
        with pytest.raises(RuntimeError) as ei:
            hset.implausibility(xs, np.ones(32), np.ones(32), maxno=33)
        assert _status(ei) == ERR_ARG
        lib, D = hset.lib, native._ptr
        i2, z, V = np.zeros(5), np.ones(16), np.eye(16)
        assert lib.gpe_hm_implausibility_mv(hset._h, 0, 0, 3, D(xs), D(z), D(V), D(i2), None, None) == ERR_ARG
        assert lib.gpe_hm_implausibility_mv(hset._h, 0, 5, 3, None, D(z), D(V), D(i2), None, None) == ERR_ARG
        assert lib.gpe_hm_implausibility_mv(hset._h, 0, 5, 3, D(xs), D(z), D(V), None, None, None) == ERR_ARG
        assert lib.gpe_hm_implausibility_mv(hset._h, 0, 5, 3, D(xs), D(z), D(V), D(i2), D(np.zeros((16, 5))), None) == ERR_ARG
        assert lib.gpe_hm_implausibility_mv(hset._h, 0, 5, 2, D(xs), D(z), D(V), D(i2), None, None) == ERR_ARG
        assert lib.gpe_hm_implausibility_mv(hset._h, 2, 5, 3, D(xs), D(z), D(V), D(i2), None, None) == ERR_ARG
        assert lib.gpe_hm_member_outputs(hset._h, 2) == ERR_ARG
        out = hset.implausibility(xs, np.ones(32), np.full(32, 0.1), maxno=32)     # the set still works
        assert out.shape == (5, 32) and np.all(np.isfinite(out)) and np.all(np.diff(out, axis=1) >= 0.0)
        assert np.all(np.isfinite(hset.implausibility_mv(1, xs, z, V)))
    finally:
        hset.close()
        fresh.close()


# ------------------------------------------------------------------ 8. the Python layer
@pytest.fixture()
def toysim3d(tmp_path, monkeypatch):
    """The toysim3D example of test_gpu_multi_output.py (4 tries) beside the two trained
    toysim3D emulators of test_gpu_history_match.py."""
    for f in os.listdir(os.path.join(EX, "toysim3D")):
        shutil.copy(os.path.join(EX, "toysim3D", f), tmp_path)
    cfg = tmp_path / "toysim3D_config0"
    cfg.write_text(cfg.read_text().replace("tries 20", "tries 4"))
    shutil.copytree(os.path.join(EX, "sensitivity_recon"), tmp_path / "w", copy_function=shutil.copyfile)
    os.chmod(tmp_path / "w", 0o755)
    with open(tmp_path / "w" / "toysim3D_beliefs0-1f", "a") as fh:
        fh.write("active_index 0 1 2\n")
    monkeypatch.chdir(tmp_path)
    return tmp_path


def test_python_layer(toysim3d, monkeypatch):
    import gp_emu_uqsa_amd as g
    from gp_emu_uqsa_amd import history_match as hm
    from gp_emu_uqsa_amd import multioutput
    np.random.seed(0)
    M = multioutput.setup("toysim3D_config0", outputs=[0, 1], datashuffle=True)
    with pytest.raises(RuntimeError):
        hm.EmulatorSet([M])                                      # not trained yet
    multioutput.train(M)
    x = np.random.RandomState(6).uniform(size=(250, 3))
    mean, c, Sigma = multioutput.posterior(M, x)
    zs = np.array([float(np.median(mean[:, 0])), float(np.median(mean[:, 1]))])
    ve = np.array([0.02 * Sigma[0, 0], 0.03 * Sigma[1, 1]])
    V = np.array([[ve[0], 0.3 * np.sqrt(ve[0] * ve[1])], [0.3 * np.sqrt(ve[0] * ve[1]), ve[1]]])
    I2u = (mean - zs) ** 2 / (np.diag(Sigma) * c[:, None] + ve)
    r = mean - zs
    I2j = np.einsum("sa,sa->s", r, np.linalg.solve(c[:, None, None] * Sigma + V, r[:, :, None])[:, :, 0])
    S = hm.EmulatorSet([M])
    try:
        assert S.fused is True and S.D == 3 and S.outputs == 2
        got = S.implausibility(zs, ve, x, maxno=2)
        assert got.shape == (250, 2) and np.allclose(got, _imaxes(I2u, 2), rtol=1e-7, atol=0.0)
        I, pm, pc = S.implausibility_mv(0, zs, V, x, parts=True)
        assert np.allclose(I, np.sqrt(I2j), rtol=1e-7, atol=0.0)
        assert pm.shape == (250, 2) and np.allclose(pm, mean, rtol=0, atol=1e-8 * max(1.0, np.max(np.abs(mean))))
        assert np.allclose(pc, c, rtol=0, atol=1e-8)
        assert np.array_equal(hm.implausibility_mv(S, zs, V, x), I)
        assert np.array_equal(hm.implausibility_mv(M, zs, V, x), I)              # a MultiEmulator makes its own set
        Id = hm.implausibility_mv(S, zs, ve, x)                                  # a vector: V's diagonal
        I2d = np.einsum("sa,sa->s", r, np.linalg.solve(c[:, None, None] * Sigma + np.diag(ve), r[:, :, None])[:, :, 0])
        assert np.allclose(Id ** 2, I2d, rtol=1e-7, atol=0.0)
    finally:
        S.close()
    # an Emulator beside it: its row is what it gives alone
    monkeypatch.chdir(toysim3d / "w")
    E = g.setup("toysim3D_config0_recon", datashuffle=False, scaleinputs=True)
    alone = hm.implausibility([E], [zs[0]], [ve[0]], x, maxno=1)
    T = hm.EmulatorSet([E, M])
    try:
        assert T.fused is True and T.outputs == 3
        both = T._set.implausibility(x, [zs[0], zs[0], zs[1]], [ve[0], ve[0], ve[1]], maxno=3, parts=True)
        with np.errstate(invalid="ignore"):
            row = np.sqrt((both[1][0] - zs[0]) ** 2 / (both[2][0] + ve[0]))
        assert np.array_equal(row, alone[:, 0])
        got = T.implausibility([zs[0], zs[0], zs[1]], [ve[0], ve[0], ve[1]], x, maxno=3)
        assert got.shape == (250, 3) and np.array_equal(got, both[0])
        assert np.allclose(T.implausibility_mv(1, zs, V, x), np.sqrt(I2j), rtol=1e-7, atol=0.0)
        with pytest.raises(ValueError):
            T.implausibility_mv(0, zs, V, x)                                     # item 0 is an Emulator
    finally:
        T.close()
    # a set forced off the fused path: the NumPy route's values
    monkeypatch.setattr(hm.EmulatorSet, "_make_fused", lambda self: False)
    U = hm.EmulatorSet([M])
    try:
        assert U.fused is False
        assert np.array_equal(U.implausibility(zs, ve, x, maxno=2), _imaxes(I2u, 2))
        assert np.array_equal(U.implausibility_mv(0, zs, V, x), np.sqrt(I2j))
    finally:
        U.close()
