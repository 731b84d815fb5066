"""Host checks of the resident emulator set (gpe_hm_*), no GPU:

- tests/implausibility_ref.py, the NumPy reference the GPU tests compare with, against
  oracle.gp_oracle.posterior_ref on synthetic_problem emulators at 1e-8, the bound
  test_gpu_posterior.py uses against the same oracle; its Matern families against
  matern_ref.posterior; its selection against history_match._imaxes;
- csrc/gpemu_hm_plan.hpp (the packed index map of L^-1, the tile list, the chunk and workspace
  sizes) through the stand-alone program tests/host/hm_plan_check.cpp, built with the address
  and undefined-behaviour sanitizers where their runtime links (a stand-alone binary: nothing
  is preloaded), plainly otherwise;
- nonimp_sample's independence of the batch length, on a stand-in set.
"""
import os
import subprocess

import numpy as np
import pytest

import implausibility_ref as iref
import matern_ref as mref
from oracle import gp_oracle as orc
from test_objective_host import SAN, _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "hm_plan_check.cpp")
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")


def _emulator(n, d, q, kind, seed, sigma=0.9):
    X, f, H = orc.synthetic_problem(n, d, seed=seed)
    H = H[:, :q]
    delta, nu = np.linspace(0.5, 1.1, d), 1e-3
    A, _ = orc.kernel_var_ref(X, delta, nu, kind, True)
    beta = orc.optimal_beta_ref(A, H, f)
    return dict(XT=X, fT=f, HT=H, beta=beta, sigma=sigma, delta=delta, nu=nu, kind=kind, A=A)


@pytest.mark.parametrize("n,d,q,kind", [(60, 3, 4, orc.STD), (100, 3, 1, orc.ALT), (129, 10, 11, orc.STD),
                                        (17, 1, 2, orc.ALT)])
def test_reference_against_the_oracle(n, d, q, kind):
    e = _emulator(n, d, q, kind, seed=n)
    xs = np.random.RandomState(n).uniform(size=(40, d))
    xs[3] = e["XT"][5]                        # a point on a training point
    hs = orc.linear_basis(xs)[:, :q]
    mean, var = iref.posterior_diag(e["XT"], e["fT"], e["HT"], xs, hs, e["beta"], e["sigma"], e["delta"], e["nu"],
                                    kind)
    m_ref, v_ref = orc.posterior_ref(e["XT"], e["fT"], e["HT"], e["A"], xs, hs, e["beta"], e["sigma"], e["delta"],
                                     e["nu"], kind)
    assert np.max(np.abs(mean - m_ref)) < 1e-8
    assert np.max(np.abs(var - np.diag(v_ref))) < 1e-8
    # the extended-precision evaluation of the same formulas agrees with both
    mean_l, var_l = iref.posterior_diag(e["XT"], e["fT"], e["HT"], xs, hs, e["beta"], e["sigma"], e["delta"],
                                        e["nu"], kind, dtype=np.longdouble)
    assert mean_l.dtype == np.longdouble
    assert np.max(np.abs((mean_l - mean).astype(float))) < 1e-8
    assert np.max(np.abs((var_l - var).astype(float))) < 1e-8


@pytest.mark.parametrize("family", ["matern32", "matern52"])
def test_reference_matern_and_r(family):
    e = _emulator(60, 3, 4, orc.STD, seed=7)
    r = np.random.RandomState(3).uniform(0.0, 0.02, 60)
    A = mref.kernel_var(e["XT"], e["delta"], e["nu"], orc.STD, family, True)[0]
    A[np.diag_indices_from(A)] += r
    xs = np.random.RandomState(8).uniform(size=(30, 3))
    hs = orc.linear_basis(xs)
    mean, var = iref.posterior_diag(e["XT"], e["fT"], e["HT"], xs, hs, e["beta"], e["sigma"], e["delta"], e["nu"],
                                    orc.STD, family, r_diag=r)
    m_ref, v_ref = mref.posterior(e["XT"], e["fT"], e["HT"], A, xs, hs, e["beta"], e["sigma"], e["delta"], e["nu"],
                                  orc.STD, family)
    assert np.max(np.abs(mean - m_ref)) < 1e-8
    assert np.max(np.abs(var - np.diag(v_ref))) < 1e-8


def test_reference_selection_is_imaxes():
    from gp_emu_uqsa_amd.history_match import _imaxes
    rs = np.random.RandomState(0)
    I2 = rs.uniform(0.0, 9.0, size=(50, 5))
    I2[4, 2] = np.nan
    I2[9, 0] = -1.0                           # a negative denominator: sqrt gives NaN
    I2[11, :] = np.nan
    I2[13, 1] = I2[13, 3]                     # a tie
    I2[17, 4] = np.inf
    for maxno in (1, 2, 5):
        with np.errstate(invalid="ignore"):
            want = _imaxes(I2, maxno)
        assert np.array_equal(iref.imaxes(I2, maxno), want, equal_nan=True)
    assert np.isnan(iref.imaxes(I2, 2)[4, -1]) and np.isfinite(iref.imaxes(I2, 2)[4, 0])
    assert np.isnan(iref.imaxes(I2, 1)[9, 0])


def test_reference_set_semantics():
    """Emulators that read different columns of the candidate rows, in their own order."""
    es = [dict(_emulator(60, 3, 4, orc.STD, 1), active=[0, 1, 2]), dict(_emulator(40, 2, 3, orc.ALT, 2), active=[3, 0]),
          dict(_emulator(30, 1, 2, orc.STD, 3), active=[2])]
    xs = np.random.RandomState(5).uniform(size=(25, 4))
    zs, ve = [2.0, 1.5, 3.0], [0.01, 0.02, 0.03]
    imax, mean, var = iref.implausibility(es, xs, zs, ve, maxno=2)
    assert imax.shape == (25, 2) and mean.shape == var.shape == (3, 25)
    e = es[1]
    x = xs[:, [3, 0]]
    m_ref, v_ref = orc.posterior_ref(e["XT"], e["fT"], e["HT"], e["A"], x, orc.linear_basis(x), e["beta"], e["sigma"],
                                     e["delta"], e["nu"], e["kind"])
    assert np.max(np.abs(mean[1] - m_ref)) < 1e-8 and np.max(np.abs(var[1] - np.diag(v_ref))) < 1e-8
    I = np.abs(mean - np.array(zs)[:, None]) / np.sqrt(var + np.array(ve)[:, None])
    assert np.allclose(imax, np.sort(I, axis=0)[-2:].T, rtol=1e-12)


def test_plan_check_program(tmp_path):
    cxx = _cxx()
    if not cxx:
        pytest.skip("no C++ compiler: the host check of the set's plan cannot be built")
    exe = str(tmp_path / "hm_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-I", CSRC, SRC, "-o", exe]
    built = subprocess.run(base + SAN, capture_output=True, text=True)
    sanitized = built.returncode == 0
    if not sanitized:   # (no sanitizer runtime on this machine)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    print("sanitizers:", sanitized)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "hm_plan_check OK"


def _StandInSet():
    """What nonimp_sample needs of a set: it accepts points inside a ball and counts the calls."""
    from gp_emu_uqsa_amd import history_match as hm

    class StandIn(hm.EmulatorSet):
        def __init__(self):
            self.minmax = {"0": [0.0, 1.0], "2": [0.0, 1.0], "5": [0.0, 1.0]}
            self.D = 3
            self.calls = 0
            self._set = None

        def implausibility(self, zs, var_extra, x, maxno=1):
            self.calls += 1
            d = 10.0 * np.linalg.norm(x - 0.5, axis=1)
            return np.column_stack([0.5 * d, d])

    return StandIn()


def test_nonimp_sample_does_not_depend_on_the_batch():
    from gp_emu_uqsa_amd import history_match as hm
    out = {}
    for batch in (4096, 1000, 37):
        S = _StandInSet()
        out[batch] = hm.nonimp_sample(S, None, 3.0, None, count=50, maxno=1, seed=4, batch=batch)
        assert S.calls >= 1
    pts, tried = out[4096]
    assert pts.shape == (50, 3) and tried >= 50
    assert np.all(10.0 * np.linalg.norm(pts - 0.5, axis=1) < 3.0)
    for batch in (1000, 37):
        assert np.array_equal(out[batch][0], pts) and out[batch][1] == tried
    # the stream itself: the accepted points are the first 50 of one long draw
    x = np.random.default_rng(4).random((tried, 3))
    ok = 10.0 * np.linalg.norm(x - 0.5, axis=1) < 3.0
    assert ok[-1] and ok.sum() == 50 and np.array_equal(x[ok], pts)
    # maxno = 2 reads the second largest; max_tried stops early with what there is
    pts2, tried2 = hm.nonimp_sample(_StandInSet(), None, 3.0, None, count=10 ** 6, maxno=2, seed=4, batch=300,
                                    max_tried=1000)
    x = np.random.default_rng(4).random((1000, 3))
    assert tried2 == 1000 and np.array_equal(pts2, x[5.0 * np.linalg.norm(x - 0.5, axis=1) < 3.0])
