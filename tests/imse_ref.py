"""Integrated-variance (IMSE) design reference for gpe_posterior_imse (test infrastructure,
NumPy only).

``imse`` is the greedy algorithm of include/gpemu.h with an eager C (the cross-covariance of
the reference rows with the candidates, downdated after every pick).  The problems are
``pivchol_ref.case(name)``; its m points are split as the first m_c candidates and the rest
the reference sample.  The splits were chosen for the edges of the device code (columns of L
in 64-row slabs and 128-row tiles, panels of 128 picks, 8 columns of C per workgroup).
"""
import functools

import numpy as np

import pivchol_ref as pr

SIGMA = pr.SIGMA

# name (of pivchol_ref.CASES) -> (m_c, k)
CASES = {
    "n60_std": (64, 40),         # one padded tile, ragged m_r = 36
    "n60_alt_r": (100, 29),      # the reference rows straddle the 128-row tile edge
    "n300_alt_r": (200, 140),    # one trailing update, 12 steps into the second panel
    "n129_std": (129, 129),      # every candidate picked, one candidate in a second tile, m_r = 128
    "n1000_std": (500, 160),     # ragged tiles, second panel
}
# (case, with r_new, weighted, tol): uniform weights with and without r_new, the weighted
# variants, the stop rule
VARIANTS = ([(name, False, False, 0.0) for name in CASES] +
            [(name, True, False, 0.0) for name in CASES if name.endswith("_r")] +
            [("n300_alt_r", False, True, 0.0), ("n1000_std", False, True, 0.0)])
STOP_VARIANTS = [("n300_alt_r", False, False, 0.5), ("n1000_std", False, False, 0.5),
                 ("n1000_std", False, False, 0.3)]
GAP = 1e-6   # a pick is compared only where the top two scores differ by this much of the best


def weights(name, weighted):
    """None (uniform), or RandomState(31).uniform(0, 1, m_r) with every 7th weight zero,
    normalised."""
    if not weighted:
        return None
    mr = pr.CASES[name][0] - CASES[name][0]
    w = np.random.RandomState(31).uniform(0.0, 1.0, mr)
    w[::7] = 0.0
    return w / w.sum()


def imse(S, mc, k, w=None, tol=0.0):
    """(piv, gain, pivvar, imse0, rank, gaps, margin) of the greedy integrated-variance design
    on S: candidates the first mc rows, reference rows the rest, untrimmed (k entries; -1 / 0 / 0
    from rank on).  gaps[t] = (best - second best eligible score) / best (inf with one eligible
    candidate); margin = min over steps and unchosen c of |d_c - thr| / max d^0."""
    S = np.asarray(S, dtype=float)
    m = S.shape[0]
    mr = m - mc
    w = np.full(mr, 1.0 / mr) if w is None else np.asarray(w, dtype=float)
    d = np.diag(S)[:mc].copy()
    C = S[mc:, :mc].copy()
    scale = np.max(np.where(np.isnan(d), -np.inf, d))
    thr = tol * scale
    imse0 = 0.0
    for r in range(mr):
        imse0 += w[r] * S[mc + r, mc + r]
    chosen = np.zeros(mc, dtype=bool)
    piv = np.full(k, -1, dtype=np.int64)
    gain = np.zeros(k)
    pivvar = np.zeros(k)
    gaps = np.full(k, np.inf)
    L = np.zeros((mc, k))
    rank, margin = 0, np.inf
    for t in range(k):
        q = (w[:, None] * C * C).sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            score = q / d
        live = ~chosen
        margin = min(margin, np.min(np.abs(d[live] - thr)) / scale)
        elig = live & (d > thr) & ~np.isnan(score)
        if not elig.any():
            break
        s = np.where(elig, score, -np.inf)
        p = int(np.argmax(s))               # first occurrence: the lowest index on ties
        if elig.sum() > 1:
            top = np.sort(s[elig])[-2:]
            gaps[t] = (top[1] - top[0]) / top[1]
        dp = d[p]
        root = np.sqrt(dp)
        col = (S[:mc, p] - L[:, :t].dot(L[p, :t])) / root
        col[chosen] = 0.0
        col[p] = root
        L[:, t] = col
        lam = C[:, p] / root
        chosen[p] = True
        live = ~chosen
        C[:, live] -= np.outer(lam, col[live])
        d[live] -= col[live] ** 2
        piv[t], gain[t], pivvar[t] = p, score[p], dp
        rank = t + 1
    return piv, gain, pivvar, imse0, rank, gaps[:rank], margin


def covariance(name, with_r):
    return pr.covariance(name, with_r)


@functools.lru_cache(maxsize=None)
def reference(name, with_r=False, weighted=False, tol=0.0):
    """imse() of a variant on the oracle's covariance (shared, read-only)."""
    mc, k = CASES[name]
    out = imse(covariance(name, with_r), mc, k, weights(name, weighted), tol)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def conditioned_imse(S, mc, picks, w=None):
    """sum_r w_r of diag(S_rr - S_rP S_PP^-1 S_Pr): the reference block conditioned directly
    on the picks."""
    S = np.asarray(S, dtype=float)
    mr = S.shape[0] - mc
    w = np.full(mr, 1.0 / mr) if w is None else np.asarray(w, dtype=float)
    P = np.asarray(picks, dtype=int)
    Srp = S[mc:, P]
    X = np.linalg.solve(S[np.ix_(P, P)], Srp.T)
    return float(w.dot(np.diag(S)[mc:] - np.einsum("rp,pr->r", Srp, X)))
