"""CPU checks of the grouped posterior covariance and of the Monte-Carlo measures that carry the
emulator's uncertainty (sensitivity.sobol_group_estimates), and of the C-ABI addition under
them (gpe_posterior_groups declared, exported, in native.SIGNATURES; ABI still 10).

* tests/posterior_groups_ref.py, the numpy statement of the blocks, against the oracle's
  posterior covariance on one small case.
* sobol_group_estimates against its formulas written out on hand-made f and C.
* sobol_group_estimates against the closed forms of the reference on the two toysim3D
  emulators (tests/golden/sensitivity_toysim3d.npz, Gaussian kernel, nugget 0): numpy means and
  covariances of the groups of sobol_points(3, 4096, seed), seeds 1 and 2; uV, uEV and EV[i]
  within 4 of their own standard errors of o*_uV, o*_uEV and o*_senseindex, and
  0 < uV_se < 0.002.  (Largest deviations found: 1.60 / 1.53 se for emulator 0 at seeds 1 / 2,
  1.77 / 1.20 se for emulator 1; uV_se between 0.0007 and 0.001.)
"""
import ctypes
import os
import re

import numpy as np
import pytest

import matern_ref as mr
import posterior_groups_ref as pgr
from gp_emu_uqsa_amd import native
from gp_emu_uqsa_amd import sensitivity as sa
from oracle import gp_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_reference_blocks_against_the_oracle():
    n, d, m = 60, 3, 24
    X, f, H = orc.synthetic_problem(n, d, seed=4)
    delta, nu, sigma = np.array([0.5, 0.8, 1.1]), 1e-3, 1.3
    A, _ = orc.kernel_var_ref(X, delta, nu, orc.STD, True)
    beta = orc.optimal_beta_ref(A, H, f)
    Xs = np.random.RandomState(3).uniform(size=(m, d))
    Xs[5] = X[7]
    Hs = orc.linear_basis(Xs)
    rmean, rvar = orc.posterior_ref(X, f, H, A, Xs, Hs, beta, sigma, delta, nu, orc.STD)
    mean, cov = pgr.full_cov(X, f, H, A, Xs, Hs, beta, sigma, delta, nu, orc.STD, "gaussian")
    scale = sigma ** 2
    print("full covariance error", np.max(np.abs(cov - rvar)) / scale, "mean", np.max(np.abs(mean - rmean)))
    assert np.max(np.abs(mean - rmean)) <= 1e-10 * max(1.0, np.max(np.abs(rmean)))
    assert np.max(np.abs(cov - rvar)) <= 1e-10 * scale
    # groups of 6 are the diagonal blocks of that matrix; blocks are exactly symmetric
    gm, gc = pgr.group_blocks(X, f, H, A, Xs, Hs, beta, sigma, delta, nu, orc.STD, "gaussian", 6)
    assert gc.shape == (4, 6, 6) and np.array_equal(gm, mean)
    for g in range(4):
        assert np.max(np.abs(gc[g] - cov[6 * g:6 * g + 6, 6 * g:6 * g + 6])) <= 1e-13 * scale
        assert np.array_equal(gc[g], gc[g].T)
    # the alt nugget: cdiag = 1 + nu^2 on the diagonal by index
    A2 = mr.make_A(X, delta, 0.05, orc.ALT, "matern52")[0]
    b2 = orc.optimal_beta_ref(A2, H, f)
    _, rv2 = mr.posterior(X, f, H, A2, Xs, Hs, b2, sigma, delta, 0.05, orc.ALT, "matern52")
    _, c2 = pgr.full_cov(X, f, H, A2, Xs, Hs, b2, sigma, delta, 0.05, orc.ALT, "matern52")
    assert np.max(np.abs(c2 - rv2)) <= 1e-10 * scale


def test_sobol_group_estimates_formulas():
    """Every term spelled out on a tiny sample (N = 4, d = 2: groups [A, B, AB_0, AB_1])."""
    rs = np.random.RandomState(0)
    N, d = 4, 2
    f = rs.standard_normal((N, d + 2))
    R = rs.standard_normal((N, d + 2, d + 2))
    C = np.einsum("nij,nkj->nik", R, R)
    est = sa.sobol_group_estimates(f, C)
    assert set(est) == {k + s for k in ("uE", "uV", "uEV", "EV", "EVT", "V", "VT") for s in ("", "_se")} | {"S", "ST"}

    def ms(t):
        return np.mean(t), np.std(t, ddof=1) / np.sqrt(N)

    fA, fB = f[:, 0], f[:, 1]
    want = {"uE": ms(0.5 * (fA + fB)), "uV": ms(C[:, 0, 1]),
            "uEV": ms(0.5 * (fA - fB) ** 2 + 0.5 * (C[:, 0, 0] + C[:, 1, 1]) - C[:, 0, 1])}
    for k, (val, se) in want.items():
        assert np.isclose(est[k], val, rtol=1e-14, atol=0) and np.isclose(est[k + "_se"], se, rtol=1e-14, atol=0), k
        assert isinstance(est[k], float) and isinstance(est[k + "_se"], float)
    for i in range(d):
        fi = f[:, 2 + i]
        per = {"EV": fB * (fi - fA) + C[:, 1, 2 + i] - C[:, 0, 1],
               "EVT": 0.5 * (fA - fi) ** 2 + 0.5 * (C[:, 0, 0] + C[:, 2 + i, 2 + i]) - C[:, 0, 2 + i],
               "V": fB * (fi - fA), "VT": 0.5 * (fA - fi) ** 2}
        for k, t in per.items():
            val, se = ms(t)
            assert np.isclose(est[k][i], val, rtol=1e-14, atol=0), (k, i)
            assert np.isclose(est[k + "_se"][i], se, rtol=1e-14, atol=0), (k, i)
    assert np.array_equal(est["S"], est["EV"] / est["uEV"]) and np.array_equal(est["ST"], est["EVT"] / est["uEV"])
    # the mean-only terms are sobol_estimates'
    old = sa.sobol_estimates(fA, fB, f[:, 2:].T)
    for k in ("V", "VT", "V_se", "VT_se"):
        assert np.allclose(est[k], old[k], rtol=1e-14, atol=0), k
    # with no covariance the emulator terms reduce to the mean-only ones
    z = sa.sobol_group_estimates(f, np.zeros_like(C))
    assert z["uV"] == 0.0 and np.array_equal(z["EV"], z["V"]) and np.array_equal(z["EVT"], z["VT"])
    with pytest.raises(ValueError):
        sa.sobol_group_estimates(f, C[:, :3, :3])


def saltelli_groups(A, B):
    """N x (d + 2) x d: [A_a, B_a, AB_0_a, ..., AB_d-1_a] for every sample a."""
    N, d = A.shape
    X = np.empty((N, d + 2, d))
    X[:, 0], X[:, 1] = A, B
    for i in range(d):
        X[:, 2 + i] = A
        X[:, 2 + i, i] = B[:, i]
    return X


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("emu", [0, 1])
def test_sobol_group_estimates_against_the_closed_forms(emu, seed):
    z = np.load(os.path.join(GOLD, "sensitivity_toysim3d.npz"))
    p = "o%d_" % emu
    x, f, H = z[p + "x"], z[p + "f"], z[p + "H"]
    delta, sigma, nu = z[p + "delta"], float(z[p + "sigma"]), float(z[p + "nugget"])
    assert nu == 0.0
    A = mr.make_A(x, delta, nu, orc.STD, "gaussian")[0]
    N, d = 4096, 3
    SA, SB = sa.sobol_points(d, N, seed, "normal", z[p + "m"], z[p + "v"])
    Xs = saltelli_groups(SA, SB).reshape(N * (d + 2), d)
    mean, cov = pgr.group_blocks(x, f, H, A, Xs, orc.linear_basis(Xs), z[p + "beta"], sigma, delta, nu,
                                 orc.STD, "gaussian", d + 2)
    est = sa.sobol_group_estimates(mean.reshape(N, d + 2), cov)
    dev = {"uV": abs(est["uV"] - float(z[p + "uV"])) / est["uV_se"],
           "uEV": abs(est["uEV"] - float(z[p + "uEV"])) / est["uEV_se"],
           "EV": np.abs(est["EV"] - z[p + "senseindex"]) / est["EV_se"]}
    print(p, "seed", seed, "deviations in se", dev, "uV_se", est["uV_se"], "uE", est["uE"], float(z[p + "uE"]))
    assert dev["uV"] <= 4 and dev["uEV"] <= 4 and np.all(dev["EV"] <= 4)
    assert 0 < est["uV_se"] < 0.002
    assert abs(est["uE"] - float(z[p + "uE"])) <= 4 * est["uE_se"]


def test_exported_names():
    for name in ("sobol_group_estimates", "mc_emulator_indices"):
        assert name in sa.__all__ and callable(getattr(sa, name))
    import gp_emu_uqsa_amd as g
    from gp_emu_uqsa_amd import api, model
    assert g.posterior_groups is api.posterior_groups and "posterior_groups" in g.__all__
    assert callable(model.posterior_groups) and callable(native.Context.posterior_groups)
    assert "uEV - senseindex" in sa.mc_emulator_indices.__doc__


def test_abi_addition():
    """gpe_posterior_groups: declared in include/gpemu.h with its signature, exported by the
    library, in native.SIGNATURES; the ABI version is still 10."""
    text = open(os.path.join(ROOT, "include", "gpemu.h")).read()
    decl = re.search(r"int\s+gpe_posterior_groups\s*\(([^)]*)\)\s*;", text)
    assert decl
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["gpe_ctx* ctx", "int64_t m", "int32_t G", "const double* Xs", "const double* Hs",
                    "const double* beta", "double sigma", "double* mean_out", "double* cov_out"]
    assert re.search(r"#define GPE_ABI_VERSION 10\b", text) and "gpe_posterior_groups" in text.split("enum gpe_status")[0]
    lib = ctypes.CDLL(native.LIB_PATH)
    assert hasattr(lib, "gpe_posterior_groups")
    D = ctypes.POINTER(ctypes.c_double)
    assert native.SIGNATURES["gpe_posterior_groups"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, D, D, D, ctypes.c_double, D, D])
    assert native.load_library().gpe_abi_version() == 10
    # a NULL context is an argument error, not a crash
    assert native.load_library().gpe_posterior_groups(None, 4, 2, None, None, None, 1.0, None, None) == -1
