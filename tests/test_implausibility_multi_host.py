"""Host checks of the multi-output member of the resident emulator set (gpe_hm_add_multi,
gpe_hm_implausibility_mv), no GPU:

(a) tests/implausibility_multi_ref.py, the NumPy reference the GPU tests compare with, against
    multi_output_ref.posterior (checked against the oracle in test_multi_output_host.py) at 1e-8,
    the bound of test_implausibility_host.py; its joint measure against the explicit inverse;
(b) csrc/gpemu_hm_mv.hpp (hm_mv_prepare: W^T V W = I, W^T Sigma W = Lambda; the diagonalised I^2
    against a long double solve, 1e-10 relative) through the stand-alone program
    tests/host/hm_mv_check.cpp;
(c) the rows-based functions of csrc/gpemu_hm_plan.hpp through tests/host/hm_plan_rows_check.cpp.
Both programs are built as test_implausibility_host.py builds hm_plan_check.cpp: with the address
and undefined-behaviour sanitizers where their runtime links (stand-alone binaries: nothing is
preloaded), plainly otherwise.

The bound of (b): p eps cond(V) = 31 x 1.1e-16 x 1e3 = 3.4e-12 for the transformation by
C^-T, C C^T = V; 1e-10 leaves a factor 30.  The program prints the worst value it sees.
"""
import os
import subprocess

import numpy as np
import pytest

import implausibility_multi_ref as mref_hm
import multi_output_ref as mo
from oracle import gp_oracle as orc
from test_objective_host import SAN, _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")
NU = 1e-3


@pytest.mark.parametrize("n,d,q,p,kind,family,with_r", [(60, 3, 4, 1, orc.STD, "gaussian", False),
                                                        (61, 3, 4, 12, orc.ALT, "gaussian", False),
                                                        (129, 10, 11, 6, orc.STD, "matern32", False),
                                                        (17, 1, 2, 3, orc.ALT, "gaussian", True)])
def test_reference_against_multi_output_ref(n, d, q, p, kind, family, with_r):
    X, _, H = orc.synthetic_problem(n, d, seed=9)
    H = np.ascontiguousarray(H[:, :q])
    F = mo.outputs(X, p)
    delta = np.linspace(0.5, 1.1, d)
    r = np.random.RandomState(n + 1).uniform(0.0, 0.02, n) if with_r else None
    xs = np.random.RandomState(n).uniform(size=(40, d))
    xs[3] = X[5]                              # a point on a training point
    hs = np.ascontiguousarray(orc.linear_basis(xs)[:, :q])
    B, Sigma = mref_hm.estimates(X, F, H, delta, NU, kind, family, r)
    mean, c = mref_hm.parts(X, F, H, xs, hs, B, delta, NU, kind, family, r)
    m_ref, c_ref, S_ref, B_ref = mo.posterior(X, F, H, xs, hs, delta, NU, kind, family, r=r,
                                              r_scale=1.0 if with_r else 0.0, full=False)
    assert mean.shape == (p, 40) and c.shape == (40,)
    assert np.max(np.abs(B - B_ref)) < 1e-8 and np.max(np.abs(Sigma - S_ref)) < 1e-8
    assert np.max(np.abs(mean.T - m_ref)) < 1e-8
    assert np.max(np.abs(c - c_ref)) < 1e-8
    # the joint measure: the solve against the explicit inverse, and its two special cases
    z = m_ref[7] + 0.3
    V = mref_hm.spd(p, 1e3, seed=p)
    I2 = mref_hm.joint(mean, c, Sigma, z, V)
    for s in (0, 3, 39):
        rr = mean[:, s] - z
        want = rr @ np.linalg.inv(c[s] * Sigma + V) @ rr
        assert abs(I2[s] - want) <= 1e-9 * want
    ve = np.linspace(0.01, 0.02, p)
    uni = mref_hm.univariate(mean, c, Sigma, z, ve)
    assert uni.shape == (p, 40)
    Sd = np.diag(np.diag(Sigma))
    assert np.allclose(mref_hm.joint(mean, c, Sd, z, np.diag(ve)), uni.sum(axis=0), rtol=1e-12, atol=0.0)


def _run_host_program(tmp_path, name):
    cxx = _cxx()
    if not cxx:
        pytest.skip("no C++ compiler: the host check cannot be built")
    exe = str(tmp_path / name)
    base = [cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe]
    built = subprocess.run(base + SAN, capture_output=True, text=True)
    sanitized = built.returncode == 0
    if not sanitized:   # (no sanitizer runtime on this machine)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    print("sanitizers:", sanitized)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == name + " OK"
    return r.stdout


def test_mv_check_program(tmp_path):
    out = _run_host_program(tmp_path, "hm_mv_check")
    assert "worst |W^T V W - I|" in out


def test_plan_rows_check_program(tmp_path):
    _run_host_program(tmp_path, "hm_plan_rows_check")


def test_prototypes_of_the_new_entries():
    """native.SIGNATURES lists the four new entries with the header's argument counts."""
    from gp_emu_uqsa_amd import native
    want = {"gpe_hm_add_multi": 10, "gpe_hm_outputs": 1, "gpe_hm_member_outputs": 2, "gpe_hm_implausibility_mv": 10}
    header = open(os.path.join(ROOT, "include", "gpemu.h")).read()
    for name, nargs in want.items():
        assert name in native.SIGNATURES and len(native.SIGNATURES[name][1]) == nargs
        assert ("int " + name + "(") in header
    assert "#define GPE_ABI_VERSION 10 " in header
