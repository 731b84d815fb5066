"""The separable multi-output emulator on the CPU: the dense reference (tests/multi_output_ref.py)
checked against itself, and the library's host algebra (small_multi_from_gram, small_multi_t2,
objective_value_multi) run by a stand-alone program, tests/host/multi_check.cpp: any C++17
compiler, no HIP, no GPU, built with the address and undefined-behaviour sanitizers where their
runtime links (nothing is preloaded), plainly otherwise.

The reference's gradient is held to central differences of its llh (h = 1e-5 in x = 2 log hp)
at 1e-6 of max |grad|, as test_matern_host.py holds the gp4ml one; its p = 1 case to the
oracle's MUCM llh, sigma-hat^2 and gradient / sigma-hat^2 on the recorded problem
tests/golden/objective_n200_d3.npz.

The program gets the Gram of Z = L^-1 [F H], log|A| and the d + 3 contraction sums as k_contract
defines them over M = A^-1 - W W^T, all formed here in NumPy with W from the reference's own
algebra (M = reference M / p), and its llh, Sigma-hat, B and gradient are held to the reference
under the rules of tests/test_gpu_objective.py (its _grad_ok and cond(A) rule, imported); T2 as
test_objective_host.py holds small_t2: entries of Cholesky solves with Q and S, so within a
small multiple of eps cond of the largest."""
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

import matern_ref as mr
import multi_output_ref as mo
from oracle import gp_oracle as orc
from test_gpu_objective import _grad_ok
from test_objective_host import CSRC, ROOT, SAN, _cxx, _fields, _hex, _squareform

SRC = os.path.join(ROOT, "tests", "host", "multi_check.cpp")
GOLD = os.path.join(ROOT, "tests", "golden", "objective_n200_d3.npz")
EPS = np.finfo(float).eps


# ------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("family", mr.FAMILIES)
@pytest.mark.parametrize("kind,fit", [(orc.STD, True), (orc.ALT, True), (orc.STD, False)])
def test_reference_gradient_is_the_derivative(family, kind, fit):
    n, d, p = 60, 3, 3
    X, _, H = orc.synthetic_problem(n, d, seed=9)
    F = mo.outputs(X, p)
    hp = mr.hyperparams(d, orc.MUCM, kind, fit)
    nuf = mr.NU[kind]
    _, grad, _, _ = mo.objective(X, F, H, hp, kind, fit, family, nu_fixed=nuf)
    x = 2.0 * np.log(hp)
    h = 1e-5
    fd = np.empty_like(x)
    for i in range(x.size):
        e = np.zeros_like(x)
        e[i] = h
        up = mo.objective(X, F, H, np.exp(0.5 * (x + e)), kind, fit, family, nu_fixed=nuf, want_grad=False)[0]
        dn = mo.objective(X, F, H, np.exp(0.5 * (x - e)), kind, fit, family, nu_fixed=nuf, want_grad=False)[0]
        fd[i] = (up - dn) / (2.0 * h)
    err = np.max(np.abs(grad - fd)) / np.max(np.abs(grad))
    print(family, kind, fit, "gradient against central differences", err)
    assert err <= 1e-6


@pytest.mark.parametrize("tag,kind,fit", [("std_mucm_fitnug", orc.STD, True), ("std_mucm_fixnug", orc.STD, False)])
@pytest.mark.parametrize("point", [0, 1])
def test_reference_with_one_output_is_the_oracles_mucm(tag, kind, fit, point):
    z = np.load(GOLD)
    X, f = z["X"], z["f"]
    H = orc.linear_basis(X)
    key = f"{tag}_p{point}"
    hp, nuf = z[key + "_hp"], float(z[key + "_nufixed"])
    llh, grad, Sigma, B = mo.objective(X, f[:, None], H, hp, kind, fit, nu_fixed=nuf)
    rl, rg, rs2 = float(z[key + "_llh"]), z[key + "_grad"], float(z[key + "_sig2"])
    ol, og, os2 = orc.objective_ref(X, f, H, hp, orc.MUCM, kind, fit, nu_fixed=nuf)
    assert abs(ol - rl) <= 1e-10 * abs(rl)      # (the oracle is the recorded result)
    delta = hp[:X.shape[1]]
    cond = np.linalg.cond(orc.kernel_var_ref(X, delta, hp[X.shape[1]] if fit else nuf, kind, True)[0])
    rtol = max(1e-10, 4 * EPS * cond)
    print(key, "llh", abs(llh - rl) / abs(rl), "sigma2", abs(Sigma[0, 0] - rs2) / rs2,
          "grad", _grad_ok(grad, rg / rs2)[1])
    assert abs(llh - rl) <= rtol * max(1.0, abs(rl))
    assert Sigma.shape == (1, 1) and abs(Sigma[0, 0] - rs2) <= 1e-10 * rs2
    assert _grad_ok(grad, rg / rs2)[0]
    assert np.max(np.abs(B[:, 0] - orc.optimal_beta_ref(
        orc.kernel_var_ref(X, delta, hp[X.shape[1]] if fit else nuf, kind, True)[0], H, f))) <= 1e-8 * np.max(np.abs(B))


# ------------------------------------------------------------------ the library's host algebra
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(text) -> the program's output lines for the commands in text."""
    cxx = _cxx()
    if not cxx:
        pytest.skip("no C++ compiler: the host check of the multi-output algebra cannot be built")
    exe = str(tmp_path_factory.mktemp("multi") / "multi_check")
    base = [cxx, "-std=c++17", "-O1", "-I", CSRC, SRC, "-o", exe]
    built = subprocess.run(base + SAN, capture_output=True, text=True)
    sanitized = built.returncode == 0
    if not sanitized:   # (no sanitizer runtime on this machine)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    print("sanitizers:", sanitized)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.strip().splitlines()
        assert lines[-1] == "multi_check OK"
        return lines[:-1]
    return run


def _record(X, F, H, hp, kind, fit, family, nuf):
    """One `multi` command from NumPy's own algebra, and what the program must print."""
    n, d = X.shape
    q, p = H.shape[1], F.shape[1]
    delta = hp[:d]
    nu = float(hp[d]) if fit else nuf
    A, rho, g = mr.make_A(X, delta, nu, kind, family, None, 1.0)
    L = np.linalg.cholesky(A)
    Linv = sla.solve_triangular(L, np.eye(n), lower=True)
    Z = Linv @ np.column_stack([F, H])
    G = Z.T @ Z
    logdetA = 2.0 * np.sum(np.log(np.diag(L)))
    cmd_head = f"multi {p} {q} {d} {int(kind) | mr.FAMILY_CODE[family]} {float(nu).hex()} {int(fit)} {n} {hp.size} "
    ref = mo.objective(X, F, H, hp, kind, fit, family, nu_fixed=nuf)
    if ref is None:
        return cmd_head + f"{float(logdetA).hex()} {_hex(G)} {_hex(np.zeros(d + 3))}", None
    llh, grad, Sigma, B = ref
    _, _, Gm, Q, _, PF, S = mo.algebra(A, F, H)
    # M = A^-1 - W W^T = reference M / p, and k_contract's sums over it (g for the length
    # scales, rho for the nugget's off-diagonal sum)
    M = Linv.T @ Linv - Gm @ sla.solve(Q, Gm.T) - ((n - q) / p) * PF @ sla.solve(S, PF.T)
    Mg = np.tril(M * _squareform(g, n), -1)
    red = [np.sum(Mg * (X[:, k, None] - X[None, :, k]) ** 2 / delta[k] ** 2) for k in range(d)]
    red += [np.sum(np.tril(M * _squareform(rho, n), -1)), np.trace(M), 0.0]
    Kq, C = np.linalg.cholesky(Q), np.linalg.cholesky(S)
    sc = np.sqrt((n - q) / p)
    T2 = np.zeros((p + q, p + q))
    Cit = sla.solve_triangular(C, np.eye(p), lower=True).T
    T2[:p, :p] = sc * Cit
    T2[p:, :p] = -sc * B @ Cit
    T2[p:, p:] = sla.solve_triangular(Kq, np.eye(q), lower=True).T
    want = dict(llh=llh, grad=grad, Sigma=Sigma, B=B, T2=T2.ravel(order="F"),
                rtol=max(1e-10, 4 * EPS * np.linalg.cond(A)),
                condT=max(np.linalg.cond(Q), np.linalg.cond(S)), cfac=(n - q) / p)
    return cmd_head + f"{float(logdetA).hex()} {_hex(G)} {_hex(red)}", want


@pytest.mark.parametrize("p", [1, 3, 17])
@pytest.mark.parametrize("family,kind,fit", [("gaussian", orc.STD, True), ("gaussian", orc.ALT, True),
                                             ("matern52", orc.STD, False), ("matern32", orc.ALT, True)])
def test_host_algebra_against_the_reference(check, p, family, kind, fit):
    n, d = 120, 3
    X, _, H = orc.synthetic_problem(n, d, seed=9)
    F = mo.outputs(X, p)
    hp = mr.hyperparams(d, orc.MUCM, kind, fit)
    cmd, w = _record(X, F, H, hp, kind, fit, family, mr.NU[kind])
    (line,) = check(cmd + "\n")
    assert line.startswith("multi ok"), line
    llh, cfac, gscale, Sigma, B, T2, grad = _fields(line, "llh", "cfac", "gscale", "Sigma", "B", "T2", "grad")
    q = H.shape[1]
    serr = np.max(np.abs(Sigma.reshape(p, p) - w["Sigma"])) / np.max(np.abs(w["Sigma"]))
    berr = np.max(np.abs(B.reshape(q, p) - w["B"])) / np.max(np.abs(w["B"]))
    print(p, family, kind, fit, "llh err", abs(llh[0] - w["llh"]) / max(1.0, abs(w["llh"])), "rtol", w["rtol"],
          "grad err", _grad_ok(grad, w["grad"])[1], "Sigma err", serr, "B err", berr)
    assert abs(llh[0] - w["llh"]) <= w["rtol"] * max(1.0, abs(w["llh"]))
    assert _grad_ok(grad, w["grad"])[0], (grad, w["grad"])
    assert serr <= 1e-10
    assert berr <= 1e-8      # (a GLS solve: the posterior tolerance)
    assert np.array_equal(Sigma.reshape(p, p), Sigma.reshape(p, p).T)
    tol = 64 * EPS * w["condT"] * np.max(np.abs(w["T2"]))
    assert np.max(np.abs(T2 - w["T2"])) <= tol, (np.max(np.abs(T2 - w["T2"])), tol)
    assert abs(cfac[0] - w["cfac"]) <= 1e-12 * w["cfac"] and gscale[0] == p


def test_host_algebra_refusals(check):
    n, d, p = 80, 3, 3
    X, _, H = orc.synthetic_problem(n, d, seed=9)
    F = mo.outputs(X, p)
    hp = mr.hyperparams(d, orc.MUCM, orc.STD, True)
    Fdup = F.copy()
    Fdup[:, 2] = Fdup[:, 0]                     # a duplicated output column: S is singular
    Hdef = np.column_stack([H, H[:, 1]])        # a repeated basis column: Q is singular
    out = check("\n".join(_record(X, Fx, Hx, hp, orc.STD, True, "gaussian", 0.0)[0]
                          for Fx, Hx in ((Fdup, H), (F, Hdef), (Fdup, Hdef))) + "\n")
    assert out[0] == "multi notpd F^T P F not positive definite"
    assert out[1] == "multi notpd H^T A^-1 H not positive definite"
    assert out[2] == "multi notpd H^T A^-1 H not positive definite"      # (Q is met first)
