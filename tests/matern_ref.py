"""Dense NumPy reference for the Matern correlation families (test infrastructure, NumPy /
SciPy only).

With s = sum_k ((x_k - x'_k) / delta_k)^2 and r = sqrt(s):

  gaussian   rho = exp(-s)                                   g = exp(-s)
  matern32   rho = (1 + sqrt3 r) exp(-sqrt3 r)               g = (3/2) exp(-sqrt3 r)
  matern52   rho = (1 + sqrt5 r + (5/3) s) exp(-sqrt5 r)     g = (5/6)(1 + sqrt5 r) exp(-sqrt5 r)

g is defined by d rho / d(2 log delta_k) = g(s) u_k^2, u_k = (x_k - x'_k) / delta_k: the
part ``exp_save`` plays in the reference's grad_delta_A.  Nothing divides by r.

``objective`` is oracle.gp_oracle.objective_ref op for op with exp(-s) replaced by rho in the
matrix and in the nugget derivative and by g in the delta derivatives; for the gaussian
family it runs the oracle's own operations.  ``FAMILY_CODE`` are the C-ABI family bits.
"""
import numpy as np
from scipy import linalg as sla
from scipy.spatial import distance as dist

from oracle import gp_oracle as orc

FAMILIES = ("gaussian", "matern32", "matern52")
FAMILY_CODE = {"gaussian": 0x00, "matern32": 0x10, "matern52": 0x20}
SQRT3 = np.sqrt(3.0)
SQRT5 = np.sqrt(5.0)


def rho_g(s, family):
    """(rho(s), g(s)) elementwise."""
    s = np.asarray(s, dtype=np.float64)
    if family == "gaussian":
        e = np.exp(-s)
        return e, e
    if family == "matern32":
        t = SQRT3 * np.sqrt(s)
        e = np.exp(-t)
        return (1.0 + t) * e, 1.5 * e
    if family == "matern52":
        t = SQRT5 * np.sqrt(s)
        e = np.exp(-t)
        return (1.0 + t + (5.0 / 3.0) * s) * e, (5.0 / 6.0) * (1.0 + t) * e
    raise ValueError(family)


def kernel_var(X, delta, nu, kind, family, predict=True):
    """K.var(X, predict) -> (A, rho, g); rho and g condensed (pdist order), as the oracle's
    exp_save."""
    X = np.asarray(X, dtype=np.float64)
    inv_len = 1.0 / np.asarray(delta, dtype=np.float64)
    rho, g = rho_g(dist.pdist(X * inv_len, "sqeuclidean"), family)
    if kind == orc.ALT:
        A = dist.squareform(rho)
        np.fill_diagonal(A, 1.0 + nu ** 2 if predict else 1.0)
    else:
        A = dist.squareform((1.0 - nu) * rho)
        np.fill_diagonal(A, 1.0 if predict else 1.0 - nu)
    return A, rho, g


def kernel_covar(XT, XV, delta, nu, kind, family):
    """K.covar(XT, XV) -> n x m."""
    inv_len = 1.0 / np.asarray(delta, dtype=np.float64)
    c = rho_g(dist.cdist(np.asarray(XT) * inv_len, np.asarray(XV) * inv_len, "sqeuclidean"), family)[0]
    return c if kind == orc.ALT else (1.0 - nu) * c


def kernel_grad(X, delta, col, col_scale, pre, family):
    """What gpe_kernel_grad_k writes: pre ((col_k - col_l) col_scale)^2 g with a column,
    pre rho without; zero diagonal."""
    X = np.asarray(X, dtype=np.float64)
    rho, g = rho_g(dist.pdist(X / np.asarray(delta, dtype=np.float64), "sqeuclidean"), family)
    if col is None:
        return dist.squareform(pre * rho)
    p = dist.pdist((np.asarray(col, dtype=np.float64) * col_scale).reshape(-1, 1), "sqeuclidean")
    return dist.squareform(pre * p * g)


def make_A(X, delta, nu, kind, family, r=None, s2=1.0, predict=True):
    """Data.make_A(s2, predict): r / s2 on the diagonal for the alt-nugget kernel only."""
    A, rho, g = kernel_var(X, delta, nu, kind, family, predict)
    if kind == orc.ALT and r is not None:
        A[np.diag_indices_from(A)] += np.asarray(r, dtype=np.float64) / s2
    return A, rho, g


def objective(X, f, H, hp, variant, kind, fit_nugget, family, r=None, nu_fixed=0.0, want_grad=True):
    """(LLH, grad, sig2), or None when a Cholesky fails: oracle.gp_oracle.objective_ref with
    the family's rho and g."""
    X = np.asarray(X, np.float64)
    f = np.asarray(f, np.float64)
    H = np.asarray(H, np.float64)
    n, d = X.shape
    q = H.shape[1]
    delta, nu, sigma = orc.split_hp(hp, d, variant, fit_nugget)
    nu_eff = nu if nu is not None else float(nu_fixed)
    if variant == orc.GP4ML:
        s2 = sigma ** 2
        A, rho, g = make_A(X, delta, nu_eff, kind, family, r, s2)
        A = s2 * A
    else:
        s2 = 1.0
        A, rho, g = make_A(X, delta, nu_eff, kind, family, None, 1.0)
    try:
        L, Q, Kq, invA_f, invA_H, sKH, B = orc._common_solves_ref(A, H, f)
    except np.linalg.LinAlgError:
        return None
    logdetA = 2.0 * np.sum(np.log(np.diag(L)))
    invA_H_B = invA_H.dot(B)
    quad = f.T.dot(invA_f - invA_H_B)
    if variant == orc.GP4ML:
        llh = -0.5 * (-quad - logdetA - np.log(sla.det(Q)) - (n - q) * np.log(2.0 * np.pi))
        sig2 = s2
        factor = 1.0
        gs2 = s2
    else:
        sig2 = quad / (n - q - 2.0)
        llh = -0.5 * (-(n - q) * np.log(sig2) - logdetA - np.log(np.linalg.det(Q)))
        factor = (n - q) / (sig2 * (n - q - 2))
        gs2 = sig2
    if not want_grad:
        return llh, None, sig2
    H_B = H.dot(B).T
    grad = np.empty(np.asarray(hp).size)
    for i in range(d):
        dA = orc.grad_delta_ref(X[:, i], delta[i], nu_eff, g, gs2, kind)
        grad[i] = orc._grad_term_ref(L, dA, f, invA_f, invA_H_B, H_B, Kq, sKH, invA_H, factor)
    if fit_nugget:
        dA = orc.grad_nugget_ref(n, nu_eff, rho, gs2, kind)
        grad[d] = orc._grad_term_ref(L, dA, f, invA_f, invA_H_B, H_B, Kq, sKH, invA_H, factor)
    if variant == orc.GP4ML:
        dA = A.copy()
        if r is not None:
            dA[np.diag_indices_from(dA)] -= r
        grad[-1] = orc._grad_term_ref(L, dA, f, invA_f, invA_H_B, H_B, Kq, sKH, invA_H, factor)
    return llh, grad, sig2


def posterior(XT, fT, HT, A, Xs, Hs, beta, sigma, delta, nu, kind, family):
    """Posterior mean / full variance, after oracle.gp_oracle.posterior_ref."""
    covar = kernel_covar(XT, Xs, delta, nu, kind, family)
    mean = Hs.dot(beta) + covar.T.dot(sla.solve(A, fT - HT.dot(beta)))
    invA_H = sla.solve(A, HT)
    t1 = Hs - covar.T.dot(invA_H)
    t2 = HT.T.dot(invA_H)
    Ass = kernel_var(Xs, delta, nu, kind, family, True)[0]
    t3 = Ass - covar.T.dot(sla.solve(A, covar))
    var = sigma ** 2 * (t3 + t1.dot(sla.solve(t2, t1.T)))
    return mean, var


# ---- the problems of tests/test_gpu_matern.py ------------------------------------------
SHAPES = [(129, 2), (200, 10), (300, 5), (260, 40), (520, 3)]
SIGMA = 1.3
NU = {orc.STD: 1e-3, orc.ALT: 0.05}


def deltas(d):
    """The length scales of a shape (at d = 40 longer ones: with the others every
    correlation there is ~ 0 and a test shows nothing)."""
    return np.linspace(2.5, 4.0, d) if d == 40 else np.linspace(0.5, 1.1, d)


def hyperparams(d, variant, kind, fit_nugget):
    """Untransformed hp = [delta, nu (if fitted), sigma (gp4ml)]."""
    hp = list(deltas(d))
    if fit_nugget:
        hp.append(NU[kind])
    if variant == orc.GP4ML:
        hp.append(SIGMA)
    return np.array(hp)
