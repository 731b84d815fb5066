"""Candidates made and reduced on the GPU (gpe_hm_cells, gpe_hm_cells_mv, gpe_hm_sample;
native.EmulatorSet.cells / cells_mv / sample).

Every expected value is the set's own unchanged route on the explicit candidate rows, reduced by
NumPy, and every bound is an equality: the generators copy values (the mesh) or reproduce an
integer algorithm (PCG64), k_hm_post and the selection arithmetic are untouched, and a minimum
and an integer count do not depend on the order they are combined in.  The sets are the small
ones of test_gpu_implausibility.py (p = 3: n = 60, 130, 300, D = 4, both tile shapes, three
families) and test_gpu_implausibility_multi.py (n = 61, p = 12).  Mesh: g1 = 3, g2 = 2, ns = 70,
so that 64-point chunks cut every cell at another offset.
"""
import numpy as np
import pytest

import implausibility_maps_ref as mapref
import implausibility_multi_ref as mhr
from gp_emu_uqsa_amd import native
from gp_emu_uqsa_amd.history_match import _imaxes
from oracle import gp_oracle as orc
from test_gpu_implausibility import _add, _problem, _resident
from test_gpu_implausibility_multi import _add_multi
from test_gpu_implausibility_multi import _problem as _multi_problem
from test_gpu_implausibility_multi import _resident as _multi_resident

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
ACTIVES = [[0, 1, 2], [3, 0], [2]]
ZS, VE = np.array([2.0, 3.0, 2.5]), np.array([0.01, 0.02, 0.03])
G1, G2, NS = 3, 2, 70


def _three(ctx, hset):
    es = [_problem(60, 3, 4, 11), _problem(130, 2, 3, 12, kind=orc.ALT, family="matern52"),
          _problem(300, 1, 2, 13, family="matern32")]
    for i, (e, a) in enumerate(zip(es, ACTIVES)):
        assert _add(hset, ctx, _resident(ctx, e), a) == i
    return es


@pytest.fixture(scope="module")
def sets(ctx):
    """The p = 3 set twice: at the default chunk and at 64-point chunks."""
    mp = pytest.MonkeyPatch()
    one = native.EmulatorSet(0)
    mp.setenv("GPEMU_HM_CHUNK", "64")
    many = native.EmulatorSet(0)
    mp.undo()
    _three(ctx, one)
    _three(ctx, many)
    yield one, many
    one.close()
    many.close()


def _mesh(ns=NS, D=4, seed=3):
    rs = np.random.RandomState(seed)
    return rs.uniform(size=G1), rs.uniform(size=G2), rs.uniform(size=(ns, D - 2))


def _flags(pair):
    """imp_plot's rule: an emulator is on where it reads both inputs of the pair."""
    return [pair[0] in a and pair[1] in a for a in ACTIVES]


def _median_level(hset, rows):
    """A cut-off that cuts: the median of the largest implausibility over the candidates."""
    return float(np.median(hset.implausibility(rows, ZS, VE, maxno=1)[:, 0]))


def _host_maps(hset, rows, zs, ve, ns, maxno, cm, use=None):
    """The host reduction of hset.implausibility on the explicit rows; a masked output is a zero
    I^2 column.  I^2 is NumPy's expression of the returned parts (k_hm_post stores the variance
    it divides by), which the unmasked case checks against the returned selection."""
    _, mean, var = hset.implausibility(rows, zs, ve, maxno=1, parts=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        I2 = ((mean - np.asarray(zs)[:, None]) ** 2 / (var + np.asarray(ve)[:, None])).T
        if use is None:
            assert np.array_equal(_imaxes(I2, maxno), hset.implausibility(rows, zs, ve, maxno=maxno), equal_nan=True)
        else:
            I2[:, ~np.asarray(use)] = 0.0
        top = _imaxes(I2, maxno).reshape(-1, ns, maxno)
        imp = np.stack([top[:, :, -(l + 1)].min(axis=1) for l in range(maxno)])
        below = np.stack([(top[:, :, -(l + 1)] < cm).sum(axis=1) for l in range(maxno)])
    return imp, below, I2


# ------------------------------------------------------------------ 1. the maps
@pytest.mark.parametrize("pair,masked", [((0, 1), False), ((0, 1), True), ((0, 2), True), ((0, 3), True), ((3, 1), False)])
def test_cells_against_the_explicit_rows(sets, pair, masked):
    hset = sets[0]
    x1, x2, others = _mesh()
    rows = mapref.cell_rows(4, pair[0], pair[1], x1, x2, others)
    use = _flags(pair) if masked else None
    cm = _median_level(hset, rows)
    for maxno in (1, 2, 3):
        want_imp, want_below, I2 = _host_maps(hset, rows, ZS, VE, NS, maxno, cm, use)
        imp, below = hset.cells(4, pair, x1, x2, others, ZS, VE, cm, maxno=maxno, use=use)
        assert imp.shape == below.shape == (maxno, G1, G2) and below.dtype == np.int64
        assert np.array_equal(imp.reshape(maxno, -1), want_imp, equal_nan=True), (pair, masked, maxno)
        assert np.array_equal(below.reshape(maxno, -1), want_below), (pair, masked, maxno)
        ref_imp, ref_below = mapref.maps(I2, G1 * G2, NS, maxno, cm)        # the loops' restatement agrees
        assert np.array_equal(want_imp, ref_imp, equal_nan=True) and np.array_equal(want_below, ref_below)
    assert 0 < want_below[0].sum() < G1 * G2 * NS or masked                   # the cut-off cuts
    if masked:
        assert not all(use) and np.all(I2[:, ~np.asarray(use)] == 0.0)


def test_one_nan(sets):
    """var_extra[0] negative, midway between emulator 0's two smallest variances over the
    candidates: I^2 < 0 at one candidate, whose level 0 is a NaN."""
    hset = sets[0]
    x1, x2, others = _mesh()
    rows = mapref.cell_rows(4, 0, 1, x1, x2, others)
    _, mean, var = hset.implausibility(rows, ZS, VE, maxno=1, parts=True)
    order = np.argsort(var[0])
    assert var[0, order[1]] > var[0, order[0]] > 0.0
    ve = np.array([-0.5 * (var[0, order[0]] + var[0, order[1]]), 0.02, 0.03])
    cell = int(order[0]) // NS
    cm = np.inf                                                   # above every number: only the NaN is out
    for maxno in (1, 3):
        want_imp, want_below, I2 = _host_maps(hset, rows, ZS, ve, NS, maxno, cm)
        assert np.sum(I2 < 0.0) == 1 and I2[order[0], 0] < 0.0
        imp, below = hset.cells(4, (0, 1), x1, x2, others, ZS, ve, cm, maxno=maxno)
        imp, below = imp.reshape(maxno, -1), below.reshape(maxno, -1)
        assert np.array_equal(imp, want_imp, equal_nan=True) and np.array_equal(below, want_below)
        assert np.isnan(imp[0, cell]) and np.all(np.isfinite(np.delete(imp[0], cell)))
        assert below[0, cell] == NS - 1 and np.all(np.delete(below[0], cell) == NS)
        assert np.all(np.isfinite(imp[1:])) and np.all(below[1:] == NS)   # the NaN sorts above: lower levels are numbers


@pytest.mark.parametrize("ns", [1, 70, 150])
def test_chunk_independence(sets, ns):
    one, many = sets
    x1, x2, others = _mesh(ns)
    rows = mapref.cell_rows(4, 2, 0, x1, x2, others)
    cm = _median_level(one, rows)
    a = one.cells(4, (2, 0), x1, x2, others, ZS, VE, cm, maxno=3)
    b = many.cells(4, (2, 0), x1, x2, others, ZS, VE, cm, maxno=3)      # every cell cut at another offset
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)
    for hset in (one, many):
        for u, v in zip(a, hset.cells(4, (2, 0), x1, x2, others, ZS, VE, cm, maxno=3)):
            assert np.array_equal(u, v, equal_nan=True)                  # nor does the call
    want_imp, want_below, _ = _host_maps(one, rows, ZS, VE, ns, 3, cm)
    assert np.array_equal(a[0].reshape(3, -1), want_imp) and np.array_equal(a[1].reshape(3, -1), want_below)
    flags = [True, False, True]
    c = one.cells(4, (2, 0), x1, x2, others, ZS, VE, cm, maxno=2, use=flags)
    d = many.cells(4, (2, 0), x1, x2, others, ZS, VE, cm, maxno=2, use=flags)
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1])


def test_cells_mv_against_the_explicit_rows(ctx, monkeypatch):
    e = _multi_problem(61, 3, 4, 12, orc.ALT, "gaussian", False)
    one = native.EmulatorSet(0)
    monkeypatch.setenv("GPEMU_HM_CHUNK", "64")
    many = native.EmulatorSet(0)
    monkeypatch.delenv("GPEMU_HM_CHUNK")
    try:
        for hset in (one, many):
            B = _multi_resident(ctx, e)
            assert _add_multi(hset, ctx, e, B, e["S_ref"]) == 0
        x1, x2, others = _mesh(D=3)
        z, V = np.linspace(0.5, 1.5, 12), mhr.spd(12, 1e3, seed=61, scale=0.05)
        rows = mapref.cell_rows(3, 2, 1, x1, x2, others)
        I = np.sqrt(one.implausibility_mv(0, rows, z, V)).reshape(G1 * G2, NS)
        cm = float(np.median(I))
        imp, below = one.cells_mv(0, 3, (2, 1), x1, x2, others, z, V, cm)
        assert imp.shape == below.shape == (G1, G2)
        assert np.array_equal(imp.ravel(), I.min(axis=1)) and np.array_equal(below.ravel(), (I < cm).sum(axis=1))
        assert 0 < below.sum() < I.size
        imp2, below2 = many.cells_mv(0, 3, (2, 1), x1, x2, others, z, V, cm)
        assert np.array_equal(imp, imp2) and np.array_equal(below, below2)
        with pytest.raises(native.NotPositiveDefinite):
            one.cells_mv(0, 3, (2, 1), x1, x2, others, z, -np.eye(12), cm)
        assert np.array_equal(one.cells_mv(0, 3, (2, 1), x1, x2, others, z, V, cm)[0], imp)
        # history_match.EmulatorSet.maps(joint=(item, V)) on a fused set: the same maps, one level, ODP = below / ns
        from gp_emu_uqsa_amd import history_match as hm

        class Fused(hm.EmulatorSet):
            def __init__(self, nset):
                self.emuls, self._multi, self.D, self.fused, self._set = [None], [True], 3, True, nset

            def close(self):
                pass
        for S in (Fused(one), Fused(many)):
            for IMP, ODP in (S.maps(z, None, cm, (2, 1), x1, x2, others, maxno=2, joint=(0, V)),
                             hm.imp_maps(S, z, None, cm, (2, 1), x1, x2, others, joint=(0, V))):
                assert IMP.shape == ODP.shape == (1, G1, G2)
                assert np.array_equal(IMP[0], imp) and np.array_equal(ODP[0], below / float(NS))
        # the member's 12 univariate outputs: more levels than the few-level kernels hold (4)
        vd = np.linspace(0.01, 0.02, 12)
        for maxno in (4, 5, 12):
            top = one.implausibility(rows, z, vd, maxno=maxno).reshape(G1 * G2, NS, maxno)
            cmu = float(np.median(top[:, :, -1]))
            for hset in (one, many):
                imp, below = hset.cells(3, (2, 1), x1, x2, others, z, vd, cmu, maxno=maxno)
                for l in range(maxno):
                    assert np.array_equal(imp[l].ravel(), top[:, :, -(l + 1)].min(axis=1)), (maxno, l)
                    assert np.array_equal(below[l].ravel(), (top[:, :, -(l + 1)] < cmu).sum(axis=1)), (maxno, l)
        _check_sample((one, many), 3, np.zeros(3), np.ones(3), z, vd, 4, 5)
    finally:
        one.close()
        many.close()


def test_two_inputs_alone(ctx):
    """D = 2: no other columns, others NULL; ns still counts the (identical) samples of a cell."""
    hset = native.EmulatorSet(0)
    try:
        _add(hset, ctx, _resident(ctx, _problem(60, 2, 3, 61)), [1, 0])
        x1, x2, _ = _mesh()
        others = np.zeros((5, 0))
        rows = mapref.cell_rows(2, 1, 0, x1, x2, others)
        assert rows.shape == (G1 * G2 * 5, 2)
        top = hset.implausibility(rows, [2.0], [0.01], maxno=1).reshape(G1 * G2, 5)
        cm = float(np.median(top))
        imp, below = hset.cells(2, (1, 0), x1, x2, others, [2.0], [0.01], cm)
        assert np.array_equal(imp.ravel(), top.min(axis=1)) and np.array_equal(below.ravel(), (top < cm).sum(axis=1))
        assert set(np.unique(below)) <= {0, 5} and 0 < below.sum() < 30
    finally:
        hset.close()


def test_cells_errors_and_the_other_entries(sets, ctx):
    hset = sets[0]
    x1, x2, others = _mesh()
    rows = mapref.cell_rows(4, 0, 1, x1, x2, others)
    before = hset.implausibility(rows, ZS, VE, maxno=2, parts=True)
    lib, D = hset.lib, native._ptr
    imp, below = np.zeros((3, 6)), np.zeros((3, 6), dtype=np.int64)
    B = below.ctypes.data_as(hset.lib.gpe_hm_cells.argtypes[-1])

    def call(Dn=4, ca=0, cb=1, g1=G1, px1=x1, g2=G2, px2=x2, ns=NS, poth=others, z=ZS, ve=VE, maxno=1, pimp=imp, pb=B):
        return lib.gpe_hm_cells(hset._h, Dn, ca, cb, g1, D(px1), g2, D(px2), ns, D(poth), None, D(z), D(ve), maxno, 1.5,
                                D(pimp), pb)
    assert call() == 0
    for kw in (dict(g1=0), dict(g2=0), dict(ns=0), dict(ca=1), dict(ca=-1), dict(cb=4), dict(Dn=1), dict(Dn=3),
               dict(poth=None), dict(px1=None), dict(px2=None), dict(z=None), dict(ve=None), dict(pimp=None),
               dict(pb=None), dict(maxno=0), dict(maxno=4), dict(g1=1 << 20, g2=1 << 20, ns=1)):
        assert call(**kw) == ERR_ARG, kw
        assert hset.lib.gpe_hm_last_error(hset._h)
    empty = native.EmulatorSet(0)
    try:
        with pytest.raises(RuntimeError) as ei:
            empty.cells(4, (0, 1), x1, x2, others, [], [], 1.5)
        assert getattr(ei.value, "status", None) == ERR_STATE
        with pytest.raises(RuntimeError) as ei:
            empty.sample(np.zeros(4), np.ones(4), 1, 1, 0, 5, [], [], 3.0)
        assert getattr(ei.value, "status", None) == ERR_STATE
    finally:
        empty.close()
    with pytest.raises(RuntimeError) as ei:                       # cells_mv of a single-output member
        hset.cells_mv(0, 4, (0, 1), x1, x2, others, [1.0], np.eye(1), 1.5)
    assert getattr(ei.value, "status", None) == ERR_ARG
    lo, hi = np.zeros(4), np.ones(4)
    for kw in (dict(m=0), dict(first=-1), dict(cap=-1), dict(maxno=0), dict(maxno=4), dict(first=1 << 62, m=1 << 20)):
        args = dict(first=0, m=5, maxno=1, cap=None)
        args.update(kw)
        with pytest.raises(RuntimeError) as ei:
            hset.sample(lo, hi, 12345, 1, args["first"], args["m"], ZS, VE, 3.0, maxno=args["maxno"], cap=args["cap"])
        assert getattr(ei.value, "status", None) == ERR_ARG, kw
    with pytest.raises(RuntimeError) as ei:                       # D smaller than the largest active index + 1
        hset.sample(lo[:3], hi[:3], 12345, 1, 0, 5, ZS, VE, 3.0)
    assert getattr(ei.value, "status", None) == ERR_ARG
    hset.cells(4, (0, 1), x1, x2, others, ZS, VE, 1.5, maxno=3)
    hset.sample(lo, hi, 12345, 1, 0, 200, ZS, VE, 3.0)
    after = hset.implausibility(rows, ZS, VE, maxno=2, parts=True)
    for u, v in zip(before, after):
        assert np.array_equal(u, v)                               # the set's other entries: the bits they returned before


# ------------------------------------------------------------------ 2. the sampler
def _state(seed):
    st = np.random.default_rng(seed).bit_generator.state["state"]
    return st["state"], st["inc"]


def _check_sample(hsets, D, lo, hi, zs, ve, seed, maxno):
    m = 3 * 64 + 5
    state, inc = _state(seed)
    for first in (0, 1000):
        x = (lo + np.random.default_rng(seed).random((first + m, D)) * (hi - lo))[first:]
        imax = hsets[0].implausibility(x, zs, ve, maxno=maxno)
        level = imax[:, -maxno]
        cm = float(np.median(level))
        for hset in hsets:
            # a cut-off that accepts everything: the generator alone
            pts, idx, accepted = hset.sample(lo, hi, state, inc, first, m, zs, ve, np.inf, maxno=maxno)
            assert accepted == m and np.array_equal(pts, x) and np.array_equal(idx, first + np.arange(m))
            mask = level < cm
            assert 0 < mask.sum() < m
            pts, idx, accepted = hset.sample(lo, hi, state, inc, first, m, zs, ve, cm, maxno=maxno)
            assert accepted == mask.sum()
            assert np.array_equal(pts, x[mask]) and np.array_equal(idx, np.flatnonzero(mask) + first)
            assert idx.dtype == np.int64
            cap = int(mask.sum()) // 2                             # storing stops at cap, the count goes on
            p2, i2, a2 = hset.sample(lo, hi, state, inc, first, m, zs, ve, cm, maxno=maxno, cap=cap)
            assert a2 == mask.sum() and np.array_equal(p2, x[mask][:cap]) and np.array_equal(i2, idx[:cap])
            p0, i0, a0 = hset.sample(lo, hi, state, inc, first, m, zs, ve, cm, maxno=maxno, cap=0)
            assert a0 == mask.sum() and p0.shape == (0, D) and i0.shape == (0,)


def test_sample_against_the_host(sets):
    lo = np.array([0.1, -0.2, 0.0, 0.3])
    hi = lo + np.array([0.8, 1.1, 1.0, 0.5])
    for seed, maxno in ((0, 1), (12345, 2)):
        _check_sample(sets, 4, lo, hi, ZS, VE, seed, maxno)


def test_sample_thirteen_inputs(ctx, monkeypatch):
    D = 13
    one = native.EmulatorSet(0)
    monkeypatch.setenv("GPEMU_HM_CHUNK", "64")
    many = native.EmulatorSet(0)
    monkeypatch.delenv("GPEMU_HM_CHUNK")
    try:
        for hset in (one, many):
            _add(hset, ctx, _resident(ctx, _problem(129, 10, 11, 51, family="matern32")), [12, 0, 3, 4, 5, 7, 8, 9, 10, 1])
            _add(hset, ctx, _resident(ctx, _problem(60, 3, 4, 52)), [11, 2, 6])
        lo = np.linspace(-0.25, 0.25, D)
        hi = lo + np.linspace(0.6, 1.2, D)
        _check_sample((one, many), D, lo, hi, [2.0, 3.0], [0.01, 0.02], 4, 1)
    finally:
        one.close()
        many.close()
