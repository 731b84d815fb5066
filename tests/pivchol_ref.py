"""Pivoted-Cholesky reference for gpe_posterior_pivchol (test infrastructure, NumPy only).

``pivchol`` is the greedy algorithm of include/gpemu.h; ``CASES`` are the problems both test
files use: the training side is ``loo_ref.problem(name)`` (SIGMA and the GLS beta of
``orc.optimal_beta_ref``), the m test points an oLHC design with its toy-simulator outputs.
m was chosen for the tile and panel edges of the device code (tiles of 128 rows, panels of
128 pivots): one padded tile, one row in a second tile, ragged tiles, five panels.
"""
import functools

import numpy as np

import loo_ref
from oracle import gp_oracle as orc

SIGMA = loo_ref.SIGMA

# name (of loo_ref.CASES) -> (m, seed)
CASES = {
    "n60_std": (100, 11),       # one padded tile, one panel
    "n60_alt_r": (129, 12),     # one row in a second tile, one step into a second panel
    "n300_alt_r": (300, 13),    # ragged tiles, three panels
    "n129_std": (257, 15),      # one row in a third tile
    "n1000_std": (700, 14),     # six tiles, five full panels and a ragged one
}
# the stop rule: (case, tol) -> rank of the reference
STOP_CASES = {("n60_std", 0.25): 3, ("n300_alt_r", 0.5): 88, ("n1000_std", 0.2): 86}
# the design problem: candidates for the n60_std emulator, picks
DESIGN = ("n60_std", 40, 21, 8)


def pivchol(S, k=None, tol=0.0):
    """(piv, pivvar, L, rank) of the greedy pivoted Cholesky of S, untrimmed (k entries /
    columns; -1 / 0 / zero columns from rank on).  At step t the pivot is the unchosen point
    with the largest remaining variance d (lowest index on ties, a NaN never wins); stop
    before the step if t = k or d_p <= tol max(d^0)."""
    S = np.asarray(S, dtype=float)
    m = S.shape[0]
    k = m if k is None else k
    d = np.diag(S).copy()
    thr = tol * np.max(np.where(np.isnan(d), -np.inf, d))
    chosen = np.zeros(m, dtype=bool)
    piv = np.full(k, -1, dtype=np.int64)
    pivvar = np.zeros(k)
    L = np.zeros((m, k))
    rank = 0
    for t in range(k):
        cand = np.where(chosen | np.isnan(d), -np.inf, d)
        p = int(np.argmax(cand))            # first occurrence: the lowest index on ties
        if chosen[p] or np.isnan(d[p]) or not d[p] > thr:
            break
        dp = d[p]
        root = np.sqrt(dp)
        c = S[:, p] - L[:, :t].dot(L[p, :t])
        col = np.where(chosen, 0.0, c / root)
        col[p] = root
        L[:, t] = col
        chosen[p] = True
        live = ~chosen
        d[live] -= col[live] ** 2
        piv[t] = p
        pivvar[t] = dp
        rank = t + 1
    return piv, pivvar, L, rank


def gaps(S, k=None):
    """Per step of the reference, (largest - second largest remaining variance) / max diag S
    (inf at the last step): a pivot is only determined where this exceeds the error of S."""
    S = np.asarray(S, dtype=float)
    m = S.shape[0]
    k = m if k is None else k
    piv, _, L, rank = pivchol(S, k)
    d = np.diag(S).copy()
    scale = np.max(d)
    out = np.full(rank, np.inf)
    chosen = np.zeros(m, dtype=bool)
    for t in range(rank):
        live = np.where(~chosen)[0]
        if live.size > 1:
            top = np.sort(d[live])[-2:]
            out[t] = (top[1] - top[0]) / scale
        chosen[piv[t]] = True
        d -= L[:, t] ** 2
    return out


def safe_prefix(g, bound):
    """Number of leading steps whose gap is >= bound."""
    bad = np.where(g < bound)[0]
    return int(bad[0]) if bad.size else int(g.size)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict of a case: the training side (X, f, H, r, kind, delta, nu, A, beta), the test
    points (Xs, Hs, y) and the oracle's posterior (mean, S).  Where the training side has an
    r, the test points have one too (r_new, r_scale = 1; else None, 0), and S_r is S with
    sigma^2 r_scale r_new on its diagonal: the covariance of a call that passes r_new.
    Computed once and shared; callers must not modify it."""
    m, seed = CASES[name]
    X, f, H, r, kind, delta, nu, A = loo_ref.problem(name)
    beta = orc.optimal_beta_ref(A, H, f)
    Xs = orc.olhc_design(m, X.shape[1], seed)
    Hs = orc.linear_basis(Xs)
    y = orc.toysim_outputs(Xs, seed)
    r_new = None if r is None else np.random.RandomState(seed + 5).uniform(0, 0.02, m)
    r_scale = 0.0 if r is None else 1.0
    mean, S = orc.posterior_ref(X, f, H, A, Xs, Hs, beta, SIGMA, delta, nu, kind)
    S_r = None if r is None else S + np.diag(SIGMA ** 2 * r_scale * r_new)
    out = dict(X=X, f=f, H=H, r=r, kind=kind, delta=delta, nu=nu, A=A, beta=beta, Xs=Xs, Hs=Hs, y=y,
               r_new=r_new, r_scale=r_scale, mean=mean, S=S, S_r=S_r)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# every case without r_new (S, what the issue's figures and the stop rule refer to), and the
# cases that have an r also with it (S_r)
VARIANTS = [(name, False) for name in CASES] + [(name, True) for name in CASES if name.endswith("_r")]


def covariance(name, with_r):
    c = case(name)
    return c["S_r"] if with_r else c["S"]


@functools.lru_cache(maxsize=None)
def reference(name, with_r=False):
    """(piv, pivvar, L, rank, gaps) of the full factorisation of a case's covariance (shared,
    read-only)."""
    S = covariance(name, with_r)
    out = pivchol(S) + (gaps(S),)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def design_problem():
    """The greedy-design check: (case dict of n60_std, candidates, their basis, picks)."""
    name, ncand, seed, picks = DESIGN
    c = case(name)
    cand = orc.olhc_design(ncand, c["X"].shape[1], seed)
    cand.setflags(write=False)
    return c, cand, orc.linear_basis(cand), picks


def brute_force_design(c, cand, picks):
    """The greedy maximum-variance batch by refitting: after each pick the candidate joins the
    training set (any output: the variance does not depend on it; beta = 0) and the posterior
    variance of every candidate is recomputed with orc.make_A_ref / orc.posterior_ref.
    Returns (indices, variances at the time of each pick, smallest top-two gap / first variance)."""
    X, H = np.array(c["X"]), np.array(c["H"])
    f = np.zeros(X.shape[0])
    beta = np.zeros(H.shape[1])
    Hc = orc.linear_basis(cand)
    idx, var, gap = [], [], np.inf
    for _ in range(picks):
        A, _ = orc.make_A_ref(X, c["delta"], c["nu"], c["kind"], r=None, s2=1.0, predict=True)
        _, V = orc.posterior_ref(X, f, H, A, cand, Hc, beta, SIGMA, c["delta"], c["nu"], c["kind"])
        v = np.diag(V).copy()
        v[idx] = -np.inf
        p = int(np.argmax(v))
        top = np.sort(v)[-2:]
        idx.append(p)
        var.append(v[p])
        gap = min(gap, (top[1] - top[0]) / var[0])
        X = np.vstack([X, cand[p:p + 1]])
        H = np.vstack([H, Hc[p:p + 1]])
        f = np.append(f, 0.0)
    return np.array(idx), np.array(var), gap
