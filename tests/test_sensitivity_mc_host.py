"""CPU checks of the Monte-Carlo sensitivity layer (sensitivity.sobol_points, sobol_estimates)
and of the C-ABI addition it stands on (gpe_posterior_mean declared, exported, in
native.SIGNATURES; ABI still 10).

sobol_estimates on f(x) = x . a + 0.7 x0 x2, a = (1, 2, 0.5, 0), x ~ N(0, I): the variance
decomposes into the linear parts a_i^2 and the interaction 0.49 between inputs 0 and 2, so
V_i = a_i^2, VT_i = a_i^2 + 0.49 [i in {0, 2}] and var = 5.25 + 0.49 = 5.74.  Each estimate
must lie within 4 of its own standard errors (seeds 0 and 1 deviate by at most 1.34, seed 2
by 2.65).  var is the mean of 2 N squared deviations, each of variance E f^4 - var^2 with
E f^4 = 3 * 5.25^2 + 6 * 0.49 * (3 + 4 + 0.75) + 9 * 0.7^4 = 107.6334 (the terms L^4, 6 L^2 P^2
and P^4 of L = x . a and P = 0.7 x0 x2; the odd ones vanish), so it must lie within
4 sqrt((107.6334 - 5.74^2) / (2 N)) of 5.74.
"""
import ctypes
import os
import re

import numpy as np

from gp_emu_uqsa_amd import native
from gp_emu_uqsa_amd import sensitivity as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_COEF = np.array([1.0, 2.0, 0.5, 0.0])


def func(x):
    return x.dot(A_COEF) + 0.7 * x[:, 0] * x[:, 2]


def test_sobol_estimates_on_a_known_function():
    d, N = 4, 65536
    A, B = sa.sobol_points(d, N, seed=0)
    fA, fB = func(A), func(B)
    fAB = np.empty((d, N))
    for i in range(d):
        AB = A.copy()
        AB[:, i] = B[:, i]
        fAB[i] = func(AB)
    est = sa.sobol_estimates(fA, fB, fAB)
    V = A_COEF ** 2
    VT = V + 0.49 * np.array([1.0, 0.0, 1.0, 0.0])
    print("V", est["V"], "se", est["V_se"], "VT", est["VT"], "se", est["VT_se"], "var", est["var"], "mean", est["mean"])
    assert set(est) == {"mean", "var", "V", "VT", "S", "ST", "V_se", "VT_se"}
    assert np.all(est["V_se"][:3] > 0) and np.all(est["VT_se"][:3] > 0)
    assert np.all(np.abs(est["V"] - V) <= 4 * est["V_se"])
    assert np.all(np.abs(est["VT"] - VT) <= 4 * est["VT_se"])
    assert est["V"][3] == 0.0 and est["VT"][3] == 0.0 and est["V_se"][3] == 0.0 and est["VT_se"][3] == 0.0
    assert abs(est["var"] - 5.74) <= 4 * np.sqrt((107.6334 - 5.74 ** 2) / (2 * N))
    assert abs(est["mean"]) <= 4 * np.sqrt(5.74 / (2 * N))
    assert np.array_equal(est["S"], est["V"] / est["var"]) and np.array_equal(est["ST"], est["VT"] / est["var"])


def test_sobol_estimates_formulas():
    """The estimators spelled out on a tiny sample."""
    fA, fB = np.array([1.0, 2.0, 4.0]), np.array([0.0, 3.0, 5.0])
    fAB = np.array([[1.5, 2.0, 3.0], [1.0, 2.0, 4.0]])
    est = sa.sobol_estimates(fA, fB, fAB)
    both = np.concatenate([fA, fB])
    assert est["mean"] == both.mean()
    assert np.isclose(est["var"], np.mean((both - both.mean()) ** 2), rtol=1e-15)
    t = fB * (fAB[0] - fA)
    assert np.isclose(est["V"][0], t.mean(), rtol=1e-15)
    assert np.isclose(est["V_se"][0], t.std(ddof=1) / np.sqrt(3), rtol=1e-15)
    u = 0.5 * (fA - fAB[0]) ** 2
    assert np.isclose(est["VT"][0], u.mean(), rtol=1e-15)
    assert np.isclose(est["VT_se"][0], u.std(ddof=1) / np.sqrt(3), rtol=1e-15)
    assert est["V"][1] == 0.0 and est["VT"][1] == 0.0


def test_sobol_points():
    d, N = 3, 40000
    m, v = [0.5, 0.4, 0.6], [0.02, 0.03, 0.01]
    for dist in ("normal", "uniform"):
        A, B = sa.sobol_points(d, N, 5, dist, m, v)
        A2, B2 = sa.sobol_points(d, N, 5, dist, m, v)
        assert A.shape == B.shape == (N, d)
        assert np.array_equal(A, A2) and np.array_equal(B, B2)
        assert not np.array_equal(A, B)
        assert not np.array_equal(A, sa.sobol_points(d, N, 6, dist, m, v)[0])
        # successive draws of one RandomState
        rs = np.random.RandomState(5)
        if dist == "normal":
            a = np.array(m) + np.sqrt(v) * rs.standard_normal((N, d))
            b = np.array(m) + np.sqrt(v) * rs.standard_normal((N, d))
        else:
            half = np.sqrt(3.0 * np.array(v))
            a = (np.array(m) - half) + 2.0 * half * rs.random_sample((N, d))
            b = (np.array(m) - half) + 2.0 * half * rs.random_sample((N, d))
            for X in (A, B):
                assert np.all(X >= np.array(m) - half) and np.all(X <= np.array(m) + half)
        assert np.array_equal(A, a) and np.array_equal(B, b)
        for X in (A, B):
            # mean m and variance v to 3 / sqrt(N), relative to the standard deviation / variance
            assert np.all(np.abs(X.mean(axis=0) - m) <= 3 / np.sqrt(N) * np.sqrt(v))
            assert np.all(np.abs(X.var(axis=0) - v) <= 3 / np.sqrt(N) * np.array(v) * np.sqrt(2.0))
    sA, _ = sa.sobol_points(2, 10, 0)
    assert np.array_equal(sA, np.random.RandomState(0).standard_normal((10, 2)))
    try:
        sa.sobol_points(2, 10, 0, "cauchy")
    except ValueError as e:
        assert "dist" in str(e)
    else:
        raise AssertionError("an unknown distribution was accepted")


def test_exported_names():
    for name in ("sobol_points", "sobol_estimates", "mc_indices", "mc_main_effect"):
        assert name in sa.__all__ and callable(getattr(sa, name))
    import gp_emu_uqsa_amd as g
    from gp_emu_uqsa_amd import api, model
    assert g.posterior_mean is api.posterior_mean and "posterior_mean" in g.__all__
    assert callable(model.posterior_mean) and callable(native.Context.posterior_mean)


def test_abi_addition():
    """gpe_posterior_mean: declared in include/gpemu.h with the issue's signature, exported by
    the library, in native.SIGNATURES; the ABI version is still 10."""
    text = open(os.path.join(ROOT, "include", "gpemu.h")).read()
    decl = re.search(r"int\s+gpe_posterior_mean\s*\(([^)]*)\)\s*;", text)
    assert decl
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["gpe_ctx* ctx", "int64_t m", "const double* Xs", "const double* Hs", "const double* beta",
                    "double* mean_out"]
    lib = ctypes.CDLL(native.LIB_PATH)
    assert hasattr(lib, "gpe_posterior_mean")
    D = ctypes.POINTER(ctypes.c_double)
    assert native.SIGNATURES["gpe_posterior_mean"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, D, D, D, D])
    assert native.load_library().gpe_abi_version() == 10
    # a NULL context is an argument error, not a crash
    assert native.load_library().gpe_posterior_mean(None, 1, None, None, None, None) == -1
