"""Extended-precision reference for the objective at ill-conditioned hyperparameters
(tests/golden/ozaki_hard.npz; used by tests/test_ozaki_hard_ref.py and the GPU test
tests/test_gpu_ozaki_tri.py).

At nuggets of 1e-4 .. 1e-6 two correct float64 evaluations of the gradient differ by 1e-11 ..
1e-9 of scale, so float64 cannot judge the int8 products there.  objective_ld evaluates the
formulae of oracle.gp_oracle.objective_fast (K-build, blocked Cholesky, recursive triangular
inverse, A^-1 = L^-T L^-1, the Frobenius contraction) entirely in np.longdouble (x87 80-bit,
eps 1.1e-19) from the same float64 inputs.  Own code: numpy and oracle.gp_oracle only.

Run from the repository root:  python tests/golden/make_ozaki_hard.py
(about 20 s per n = 1100 case, 1 min at n = 1600).  Per case the file holds the recipe
(X, f, H, r are rebuilt from it by problem()), llh_ref and grad_ref rounded to float64, the
float64 objective_fast's errors E_cpu against them, and (max diag L / min diag L)^2.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import gp_oracle as orc  # noqa: E402

LD = np.longdouble
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ozaki_hard.npz")

# name, n, d, variant, kernel, delta, nugget (fitted) or None, nu_fixed, per-point r, hard
CASES = [
    ("gp4ml_std_d2_nu1e-4", 1100, 2, orc.GP4ML, orc.STD, [1.0, 1.0], 1e-4, 0.0, False, True),
    ("gp4ml_std_d2_nu1e-6", 1100, 2, orc.GP4ML, orc.STD, [1.0, 1.0], 1e-6, 0.0, False, True),
    ("gp4ml_std_d1_nu1e-4", 1100, 1, orc.GP4ML, orc.STD, [0.5], 1e-4, 0.0, False, True),
    ("gp4ml_alt_d2_nu1e-3_r", 1100, 2, orc.GP4ML, orc.ALT, [1.0, 1.0], 1e-3, 0.0, True, True),
    ("mucm_std_d2_nu1e-4", 1100, 2, orc.MUCM, orc.STD, [1.0, 1.0], 1e-4, 0.0, False, True),
    ("mucm_std_d3_fixed1e-4", 1100, 3, orc.MUCM, orc.STD, [1.0, 0.7, 1.0], None, 1e-4, False, True),
    ("gp4ml_std_d10_benign", 1100, 10, orc.GP4ML, orc.STD, [0.05, 1.0] * 5, 1e-3, 0.0, False, False),
    ("gp4ml_std_d2_nu1e-4_n1600", 1600, 2, orc.GP4ML, orc.STD, [1.0, 1.0], 1e-4, 0.0, False, True),
]
SIGMA = 1.0


def recipe(case, n=None):
    """The case as a dict of plain values (what the .npz stores); n overrides the size."""
    name, n0, d, variant, kind, delta, nu, nu_fixed, use_r, hard = case
    n = n0 if n is None else n
    hp = list(delta)
    if nu is not None:
        hp.append(nu)
    if variant == orc.GP4ML:
        hp.append(SIGMA)
    return dict(name=name, n=n, d=d, seed=n0 + d, hp=np.array(hp, dtype=np.float64), variant=variant,
                kernel=kind, fit_nugget=nu is not None, r_seed=n0 if use_r else -1, nu_fixed=nu_fixed,
                hard=hard)


def problem(rc):
    """X, f, H, r of a recipe (r None without per-point variances)."""
    X, f, H = orc.synthetic_problem(int(rc["n"]), int(rc["d"]), seed=int(rc["seed"]))
    r = None
    if int(rc["r_seed"]) >= 0:
        r = np.random.RandomState(int(rc["r_seed"])).uniform(1e-4, 1e-3, size=int(rc["n"]))
    return X, f, H, r


# ---------------------------------------------------------------- long-double linear algebra
def _chol_unblocked(A):
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j:, j] = v / np.sqrt(v[0])
    return L


def tri_inv(L):
    """Inverse of a lower-triangular matrix, recursively by halves:
    [[X11, 0], [-X22 L21 X11, X22]]; blocks of at most 16 rows by forward substitution."""
    n = L.shape[0]
    if n <= 16:
        X = np.zeros_like(L)
        for j in range(n):
            X[j, j] = LD(1) / L[j, j]
            for i in range(j + 1, n):
                X[i, j] = -(L[i, j:i] @ X[j:i, j]) / L[i, i]
        return X
    h = n // 2
    X = np.zeros_like(L)
    X[:h, :h] = tri_inv(L[:h, :h])
    X[h:, h:] = tri_inv(L[h:, h:])
    X[h:, :h] = -(X[h:, h:] @ (L[h:, :h] @ X[:h, :h]))
    return X


def chol_blocked(A, nb=64):
    """Right-looking blocked Cholesky (lower): diagonal block, panel L21 = A21 L11^-T through
    the block's inverse, trailing update."""
    A = A.copy()
    n = A.shape[0]
    for k in range(0, n, nb):
        e = min(k + nb, n)
        L11 = _chol_unblocked(A[k:e, k:e])
        A[k:e, k:e] = L11
        if e < n:
            L21 = A[e:, k:e] @ tri_inv(L11).T
            A[e:, k:e] = L21
            A[e:, e:] -= L21 @ L21.T
    return np.tril(A)


def objective_ld(X, f, H, hp, variant, kind, fit_nugget, r=None, nu_fixed=0.0):
    """objective_fast's formulae in np.longdouble -> (llh, grad, sig2, diag_ratio2), the first
    three still long double.  Raises LinAlgError when the matrix is not positive definite."""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an extended-precision type here"
    X = np.asarray(X, np.float64).astype(LD)
    f = np.asarray(f, np.float64).astype(LD)
    H = np.asarray(H, np.float64).astype(LD)
    hp = np.asarray(hp, np.float64).astype(LD)
    n, d = X.shape
    q = H.shape[1]
    delta = hp[:d]
    nu = hp[d] if fit_nugget else LD(np.float64(nu_fixed))
    s2 = hp[-1] ** 2 if variant == orc.GP4ML else LD(1)
    one = LD(1)
    # K-build
    Dk = [((X[:, k, None] - X[None, :, k]) / delta[k]) ** 2 for k in range(d)]
    E = np.exp(-sum(Dk))
    np.fill_diagonal(E, LD(0))          # off-diagonal exp(-r^2), as squareform(e)
    if kind == orc.ALT:
        C = E + (one + nu ** 2) * np.eye(n, dtype=LD)
    else:
        C = (one - nu) * E + np.eye(n, dtype=LD)
    A = s2 * C
    if variant == orc.GP4ML and kind == orc.ALT and r is not None:
        A[np.diag_indices(n)] += np.asarray(r, np.float64).astype(LD)
    L = chol_blocked(A)
    dg = np.diag(L)
    ratio2 = float((dg.max() / dg.min()) ** 2)
    Linv = tri_inv(L)
    z = Linv @ f
    w = Linv @ H
    Q = w.T @ w
    Kq = _chol_unblocked(Q)
    Kqi = tri_inv(Kq)
    B = Kqi.T @ (Kqi @ (w.T @ z))
    u = z - w @ B
    quad = u @ u
    logdetA = 2 * np.sum(np.log(dg))
    logdetQ = 2 * np.sum(np.log(np.diag(Kq)))
    if variant == orc.GP4ML:
        pi = 4 * np.arctan(one)
        llh = (quad + logdetA + logdetQ + (n - q) * np.log(2 * pi)) / 2
        sig2, c, gscale = s2, one, one
    else:
        sig2 = quad / (n - q - 2)
        llh = ((n - q) * np.log(sig2) + logdetA + logdetQ) / 2
        c = (n - q) / (sig2 * (n - q - 2))
        gscale = sig2
    Ainv = Linv.T @ Linv
    alpha = Linv.T @ u
    W = (Linv.T @ w) @ Kqi.T
    M = Ainv - W @ W.T - c * np.outer(alpha, alpha)
    grad = np.empty(hp.size, dtype=LD)
    pre = s2 if kind == orc.ALT else (one - nu) * s2
    ME = M * E
    for i in range(d):
        grad[i] = gscale * pre * np.sum(ME * Dk[i]) / 2
    if fit_nugget:
        if kind == orc.ALT:
            grad[d] = gscale * s2 * nu ** 2 * np.trace(M) / 2
        else:
            grad[d] = gscale * (-nu * s2 / 2) * np.sum(ME) / 2
    if variant == orc.GP4ML:
        grad[-1] = np.sum(M * (s2 * C)) / 2
        if kind == orc.STD and r is not None:
            grad[-1] -= (np.diag(M) @ np.asarray(r, np.float64).astype(LD)) / 2
    return llh, grad, sig2, ratio2


def grad_err(g, g_ref):
    """E(g) = max |g - g_ref| / (|g_ref| + max |g_ref|)."""
    g_ref = np.asarray(g_ref, np.float64)
    return float(np.max(np.abs(np.asarray(g, np.float64) - g_ref) / (np.abs(g_ref) + np.max(np.abs(g_ref)))))


def llh_err(llh, llh_ref):
    return float(abs(llh - llh_ref) / max(1.0, abs(llh_ref)))


def main():
    import time
    out = {"names": np.array([c[0] for c in CASES])}
    for case in CASES:
        rc = recipe(case)
        X, f, H, r = problem(rc)
        t0 = time.time()
        fast = orc.objective_fast(X, f, H, rc["hp"], rc["variant"], rc["kernel"], rc["fit_nugget"], r=r,
                                  nu_fixed=rc["nu_fixed"])
        if fast is None:
            raise SystemExit(f"{rc['name']}: the float64 Cholesky fails; not a usable case")
        llh, grad, _, ratio2 = objective_ld(X, f, H, rc["hp"], rc["variant"], rc["kernel"], rc["fit_nugget"],
                                            r=r, nu_fixed=rc["nu_fixed"])
        if rc["hard"] and ratio2 < 1e3:
            raise SystemExit(f"{rc['name']}: diag(L) ratio^2 {ratio2:.3g} < 1e3; not a hard case")
        llh_ref, grad_ref = float(llh), np.asarray(grad, np.float64)
        e_g, e_l = grad_err(fast[1], grad_ref), llh_err(fast[0], llh_ref)
        print(f"{rc['name']:28s} n={rc['n']} llh={llh_ref:.12g} ratio2={ratio2:.3g} "
              f"E_cpu grad={e_g:.2e} llh={e_l:.2e}  ({time.time() - t0:.0f} s)", flush=True)
        for k, v in rc.items():
            if k != "name":
                out[f"{rc['name']}/{k}"] = np.asarray(v)
        out[f"{rc['name']}/llh_ref"] = np.float64(llh_ref)
        out[f"{rc['name']}/grad_ref"] = grad_ref
        out[f"{rc['name']}/E_cpu_grad"] = np.float64(e_g)
        out[f"{rc['name']}/E_cpu_llh"] = np.float64(e_l)
        out[f"{rc['name']}/diag_ratio2"] = np.float64(ratio2)
    np.savez(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
