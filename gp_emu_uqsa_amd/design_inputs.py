"""Optimised Latin hypercube designs (reference: design_inputs/design_inputs.py:13-77).

Behaviour kept for drop-in parity with the reference:
- the same np.random consumption: per design k and dimension i, uniform(0, 1, n) then
  shuffle(arange(n));
- the same selection rule. The reference records `argmin(pdist(...))`, the INDEX of the closest
  pair, as "maximin", and keeps the design whose index is largest (:62-67). It is not the design
  with the largest minimum distance, but it is what reference runs produce, so it is reproduced;
- the same unscaling to `minmax` and the same '%.8f' text file.

Only the removed `np.int` alias (:54) is replaced by `int`.

The selection statistic, argmin(pdist([x_k; fextra])) over every candidate design, is
computed on the GPU (gpe_lhc_maximin: all N designs batched, the fextra-fextra pairs once)
with distances bit-identical to pdist's.  The designs are drawn on the host first, in the
reference's RNG order, in batches of at most _BATCH doubles.

``max_variance_design`` (no counterpart in the reference) asks a trained emulator where the
next simulator runs would teach it most: the greedy maximum-variance batch among candidate
points, the first pivots of a pivoted Cholesky of their posterior covariance on the GPU
(gpe_posterior_pivchol).  ``imse_design`` answers the same question with the integrated-variance
rule: the batch that most reduces the posterior variance averaged over a reference sample of
the inputs the emulator will be used on (gpe_posterior_imse).
"""
from __future__ import annotations

import numpy as _np

from . import native as _native

_BATCH = 1 << 25


def optLatinHyperCube(dim=None, n=None, N=None, minmax=None, filename="inputs", fextra=None):
    """Design n points in `dim` dimensions, pick one of N oLHC designs, save to `filename`."""
    print('dim:', dim)
    print('n:', n)
    print('N:', N)
    print('minmax:', minmax)
    print('filename:', filename)
    if dim is None or n is None or N is None or minmax is None:
        print("Please supply values for function arguments (default for filename is \"inputs\")")
    if len(minmax) != dim:
        print("WARNING: length of 'minmax' (list of lists) must equal 'dim'")
        raise SystemExit
    what = "combining with supplied extra data, " if fextra is not None else ""
    print("\nGenerating", N, "oLHC samples of", n, "points,", what +
          "and checking maximin criterion (pick design with maximum minimum distance between design points)...")
    xe = None if fextra is None else _np.asarray(fextra, dtype=float).reshape(-1, dim)
    if n + (0 if xe is None else xe.shape[0]) < 2:
        raise ValueError("attempt to get argmin of an empty sequence")
    u = _np.zeros((n, dim))
    b = _np.zeros((n, dim), dtype=int)
    best_D, best_k, best_maximin = None, 0, None
    per = max(1, _BATCH // (n * dim))
    ctx = _native.default_context()
    for k0 in range(0, N, per):
        kb = min(per, N - k0)
        xs = _np.empty((kb, n, dim))
        for k in range(kb):
            for i in range(dim):
                u[:, i] = _np.random.uniform(0.0, 1.0, n)
                b[:, i] = _np.arange(0, n, 1)
                _np.random.shuffle(b[:, i])
                xs[k, :, i] = (b[:, i] + u[:, i]) / float(n)
        maximin = ctx.lhc_maximin(xs, xe)
        for k in range(kb):
            if k0 + k == 0 or maximin[k] > best_maximin:
                best_D = _np.copy(xs[k])
                best_k = k0 + k
                best_maximin = maximin[k]
    D = best_D
    print("Optimal LHC design was no.", best_k)
    print("Saving inputs to file...")
    lim = _np.array(minmax, dtype=float)
    for i in range(dim):
        D[:, i] = D[:, i] * (lim[i, 1] - lim[i, 0]) + lim[i, 0]
    _np.savetxt(filename, D, delimiter=" ", fmt='%.8f')
    print("DONE!")
    return None


MAX_CANDIDATES = 16384


def max_variance_design(E, candidates, k, tol=0.0):
    """The greedy maximum-variance batch of k points among `candidates` for emulator E.

    Each pick is the candidate with the largest posterior variance given E.training and the
    candidates picked before it, with E's current hyperparameters (the outputs at the picks
    are not needed: the variance does not depend on them).  `candidates` are points in the
    emulator's scaled input space, one row each, with as many columns as E's training inputs.
    Returns (indices into candidates, their conditional variances at the time of each pick);
    fewer than k if the largest remaining variance falls to tol * the largest initial one.
    At most 16384 candidates (one chunk of the posterior): ValueError beyond."""
    x = _np.asarray(candidates, dtype=float)
    if x[0].size == 1:
        x = _np.array([x]).T
    if x[0, :].size != E.training.inputs[0, :].size:
        print("ERROR: test points have different number of columns to data in emulator. Exiting.")
        raise SystemExit(1)
    if x.shape[0] > MAX_CANDIDATES:
        raise ValueError(f"max_variance_design takes at most {MAX_CANDIDATES} candidates, got {x.shape[0]}")
    from . import model as _model
    xs = _model.Data(x, None, E.basis, E.par, E.beliefs, E.K)
    ctx = _model.upload_training(E.training)
    ctx.ensure_factor(E.K.kind, E.K.d, float(E.K.n), 1.0, E.training.r_scale())
    _, piv, pivvar, _, _ = ctx.posterior_pivchol(xs.inputs, xs.H, E.par.beta, float(E.par.sigma), k=int(k),
                                                 tol=tol, want_L=False)
    return piv, pivvar


def _scaled_points(E, points):
    x = _np.asarray(points, dtype=float)
    if x[0].size == 1:
        x = _np.array([x]).T
    if x[0, :].size != E.training.inputs[0, :].size:
        print("ERROR: test points have different number of columns to data in emulator. Exiting.")
        raise SystemExit(1)
    return x


def imse_design(E, candidates, reference, k, weights=None, tol=1e-8):
    """The greedy integrated-variance (IMSE, Cohn's ALC) batch of k points among `candidates`.

    Each pick is the candidate whose run most reduces the posterior variance of emulator E
    averaged over `reference`, a sample of the input distribution the emulator will be used on
    (`weights`: one value >= 0 per reference point, default equal), given E.training and the
    candidates picked before it, with E's current hyperparameters (the outputs at the picks are
    not needed).  Where ``max_variance_design`` goes to the boundary of the input box, this rule
    goes where the reference sample is.  Both arrays are points in the emulator's scaled input
    space, one row each, with as many columns as E's training inputs.
    Returns (indices into candidates, the reduction of the averaged variance each pick bought,
    the averaged variance before any pick): after t picks imse0 - sum(gains[:t]) is left.
    Fewer than k picks if no candidate is eligible any more: a candidate whose remaining
    variance has fallen to tol * the largest initial one is dropped.  The default 1e-8 is the
    accuracy of the posterior covariance itself: such a variance carries fewer than three
    correct digits, and the score, a ratio with it as the denominator, is noise.
    At most 16384 candidates and reference points together (one chunk of the posterior), and
    k at most the number of candidates: ValueError beyond."""
    x = _scaled_points(E, candidates)
    xr = _scaled_points(E, reference)
    if x.shape[0] + xr.shape[0] > MAX_CANDIDATES:
        raise ValueError(f"imse_design takes at most {MAX_CANDIDATES} candidates and reference points together, "
                         f"got {x.shape[0]} + {xr.shape[0]}")
    k = int(k)
    if not 1 <= k <= x.shape[0]:
        raise ValueError(f"imse_design picks 1 <= k <= {x.shape[0]} (the candidates), got k = {k}")
    w = None
    if weights is not None:
        w = _np.asarray(weights, dtype=float).ravel()
        if w.size != xr.shape[0] or not _np.all(w >= 0.0):
            raise ValueError("imse_design takes one weight >= 0 per reference point")
    from . import model as _model
    xs = _model.Data(_np.vstack([x, xr]), None, E.basis, E.par, E.beliefs, E.K)
    ctx = _model.upload_training(E.training)
    ctx.ensure_factor(E.K.kind, E.K.d, float(E.K.n), 1.0, E.training.r_scale())
    _, piv, gain, _, imse0, _ = ctx.posterior_imse(xs.inputs, xs.H, E.par.beta, float(E.par.sigma), x.shape[0], k,
                                                   w=w, tol=tol)
    return piv, gain, imse0
