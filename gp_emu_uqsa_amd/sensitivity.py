"""Uncertainty and sensitivity analysis, MUCM case2 (reference:
gp_emu_uqsa/sensitivity/sensitivityfunctions.py and _sensitivityclasses.py).

Same entry points, messages, attributes and output file as the reference:
``setup(emul, m, v)``, ``Sensitivity.uncertainty / sensitivity / main_effect /
interaction_effect / totaleffectvariance / to_file`` and ``sense_table``.

Where the work goes:
* The O(n^2) part runs on the GPU with the emulator's resident factor of
  training.A (the same one Posterior uses).
  - `gpe_sense_pairs` gives tr(A^-1 K) and [e G]^T K [e G] for the n x n
    Gaussian-integral matrices Rtt (:90-102) and, for every input P, Pw
    (:599-626). The reference builds these, and the n x n x d arrays behind
    Pw, with Python loops; here they are never formed.
  - `gpe_solve` gives e, G, A^-1 Rt and A^-1 T (:40-44, :187, :451).
  - `gpe_gauss_transform` gives the Tw . e sums of the main and interaction
    effects (:277-285, :353-373).
* The host keeps the O(n d) per-point factors. They are in closed form: B and C
  are diagonal, so every per-point (2C+B) / (4C+B) solve of the reference is
  elementwise. The host also keeps the small (d+1)-sized algebra.

Every pair matrix has the form K(k,l) = u_k u_l exp(-sum_i w_i (x_ki - x_li)^2):
  Rtt: w_i = 2 c_i^2 / (4 c_i + b_i),
       u_k = (1-nu) (prod b/(4c+b))^(1/4) exp(-sum_i c_i b_i (x_ki-m_i)^2 / (4c_i+b_i))
  Pw (w = [P]): w_P = 2 c_P^2 / (b_P + 4 c_P), w_i = 0 otherwise,
       u_k = (1-nu) sqrt(prod_{i!=P} P1_i . P4_P)
             exp(-sum_{i!=P} P2_i (x_ki-m_i)^2 - c_P b_P (x_kP-m_P)^2 / (b_P+4c_P))
with b = 1/v, c = 1/delta^2, P1 = b/(b+2c), P2 = c b/(b+2c), P4 = sqrt(b/(b+4c)).
(Minimising the quadratic of the reference's per-pair solve gives these exponents.)

The reference's totaleffectvariance (:405-463) forms Qw/Sw/Pw/Uw for w = [P]
before swapping w and wb, so its E(V) is senseindex[P] and EVTw[P] = uEV -
senseindex[P]. This is reproduced as is.

Without closed forms (any correlation family, normal or uniform inputs), by Monte Carlo on a
Sobol' design: ``mc_indices`` / ``mc_main_effect`` for the posterior mean as a function (one
gpe_posterior_mean call), and ``mc_emulator_indices`` for the measures that carry the
emulator's own uncertainty (var*[E f], E*[Var f], E*[V_i] and the true E*[V_Ti]), from the
posterior covariance inside the design's groups of d + 2 points (one gpe_posterior_groups call).
"""
from __future__ import annotations

import numpy as np

from .model import Data, posterior_gradient, posterior_groups, posterior_mean, upload_training

__all__ = ["setup", "sense_table", "Sensitivity", "NonGaussianKernel", "derivative_measures",
           "sobol_points", "sobol_estimates", "mc_indices", "mc_main_effect",
           "sobol_group_estimates", "mc_emulator_indices"]


class NonGaussianKernel(ValueError):
    """The emulator's correlation family has no closed-form sensitivity integrals here."""


def derivative_measures(emul, x):
    """Derivative-based global sensitivity measures of the emulator's posterior mean over the
    points x (m x d, in the coordinates ``posterior`` takes, drawn from the inputs'
    distribution): (nu, nu / sum(nu)) with nu_k = mean over the points of (d mean / d x_k)^2.

    No closed form is involved, so this works for every correlation family, and it is a
    route for Matern emulators, on which ``setup`` raises ``NonGaussianKernel`` (the
    variance-based one is ``mc_indices`` / ``mc_main_effect``).  One
    gpe_posterior_grad call without the variance gradient (``posterior_gradient`` with
    want_var=False)."""
    x = np.asarray(x, dtype=float)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    xs = Data(x, None, emul.basis, emul.par, emul.beliefs, emul.K)
    dmean, _ = posterior_gradient(xs, emul.training, emul.par, emul.K, want_var=False)
    nu = np.mean(dmean ** 2, axis=0)
    tot = float(np.sum(nu))
    return nu, (nu / tot if tot > 0.0 else np.zeros_like(nu))


def sobol_points(d, N, seed=0, dist="normal", m=0.0, v=1.0):
    """The two independent sample matrices (A, B), each N x d, of a Sobol' design, in the
    coordinates ``posterior`` takes; m and v are the inputs' means and variances (scalars or d
    values).  Both come from one ``np.random.RandomState(seed)``, A from its first draw and B
    from the next: dist="normal" gives m + sqrt(v) * standard_normal((N, d)), dist="uniform"
    random_sample((N, d)) scaled to [m - sqrt(3 v), m + sqrt(3 v)] (mean m, variance v)."""
    d, N = int(d), int(N)
    m = np.broadcast_to(np.asarray(m, dtype=float), (d,))
    v = np.broadcast_to(np.asarray(v, dtype=float), (d,))
    rs = np.random.RandomState(seed)
    if dist == "normal":
        draw = lambda: m + np.sqrt(v) * rs.standard_normal((N, d))
    elif dist == "uniform":
        half = np.sqrt(3.0 * v)
        draw = lambda: (m - half) + 2.0 * half * rs.random_sample((N, d))
    else:
        raise ValueError("dist must be 'normal' or 'uniform', not " + repr(dist))
    A = draw()
    B = draw()
    return A, B


def sobol_estimates(fA, fB, fAB):
    """Monte-Carlo variance-based indices from a function's values at a Sobol' design (host
    only): fA, fB (N) at the rows of A and B, fAB (d x N) with fAB[i] at A with column i taken
    from B.  Returns a dict:
      mean, var   mean and mean squared deviation of [fA; fB]
      V, V_se     V_i = mean(fB (fAB_i - fA)) (Saltelli et al. 2010), the main-effect variance
      VT, VT_se   VT_i = 1/2 mean((fA - fAB_i)^2) (Jansen 1999), the total-effect variance
      S, ST       V / var, VT / var
    The standard errors are the standard deviation (ddof = 1) of the N per-sample terms over
    sqrt(N)."""
    fA = np.asarray(fA, dtype=float).ravel()
    fB = np.asarray(fB, dtype=float).ravel()
    fAB = np.asarray(fAB, dtype=float).reshape(-1, fA.size)
    N = fA.size
    both = np.concatenate([fA, fB])
    f0 = float(np.mean(both))
    var = float(np.mean((both - f0) ** 2))
    tV = fB[None, :] * (fAB - fA[None, :])
    tT = 0.5 * (fA[None, :] - fAB) ** 2
    V, VT = tV.mean(axis=1), tT.mean(axis=1)
    out = {"mean": f0, "var": var, "V": V, "VT": VT,
           "V_se": tV.std(axis=1, ddof=1) / np.sqrt(N), "VT_se": tT.std(axis=1, ddof=1) / np.sqrt(N)}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["S"], out["ST"] = V / var, VT / var
    return out


def _mean_at(emul, x):
    """The emulator's posterior mean at the rows of x: one gpe_posterior_mean call."""
    xs = Data(np.ascontiguousarray(x, dtype=float), None, emul.basis, emul.par, emul.beliefs, emul.K)
    return posterior_mean(xs, emul.training, emul.par, emul.K)


def mc_indices(emul, m, v, samples, seed=0, dist="normal"):
    """Main-effect and total-effect indices of the emulator's posterior mean by Monte Carlo, for
    inputs with means m and variances v (``sobol_points``): ``sobol_estimates``' dict from the
    (d + 2) * samples points [A; B; AB_0; ...; AB_d-1], evaluated in ONE posterior-mean call.

    No closed form is involved, so this works for every correlation family and both input
    distributions; it is the variance-based route for Matern emulators, on which ``setup``
    raises ``NonGaussianKernel``.  The indices are those of the posterior mean as a function:
    the emulator's own uncertainty about them (the reference's E*[V_i] terms) is not included."""
    d = emul.training.inputs.shape[1]
    N = int(samples)
    A, B = sobol_points(d, N, seed, dist, m, v)
    X = np.empty(((d + 2) * N, d))
    X[:N], X[N:2 * N] = A, B
    for i in range(d):
        blk = X[(2 + i) * N:(3 + i) * N]
        blk[:] = A
        blk[:, i] = B[:, i]
    f = _mean_at(emul, X)
    return sobol_estimates(f[:N], f[N:2 * N], f[2 * N:].reshape(d, N))


def mc_main_effect(emul, m, v, points=100, samples=10000, seed=0, w=None, dist="normal", grid_index=None):
    """Main effects of the posterior mean by Monte Carlo: for each input P in w (None: all)
    and each of ``points`` values across input_range[P] (the grid of
    ``Sensitivity.main_effect``), the mean of the posterior mean with input P held at the
    value and the other inputs drawn from their distribution -- matrix A of ``sobol_points``,
    drawn once and used for every value and every input.  One posterior-mean call per input.

    Returns a dict: ``mean_effect`` and its standard error ``se`` (d x points; rows of inputs
    outside w are 0), and ``uE`` and ``uE_se``, the mean of the posterior mean over A itself.
    grid_index (a slice or an index array) evaluates only those of the ``points`` grid values;
    the other entries are NaN.
    For a Gaussian kernel, normal inputs and a linear mean these estimate
    ``Sensitivity.mean_effect`` and ``uE``; they work for every family and both distributions
    and, like ``mc_indices``, describe the posterior mean only."""
    d = emul.training.inputs.shape[1]
    N, points = int(samples), int(points)
    A, _ = sobol_points(d, N, seed, dist, m, v)
    fA = _mean_at(emul, A)
    out = {"mean_effect": np.zeros((d, points)), "se": np.zeros((d, points)),
           "uE": float(np.mean(fA)), "uE_se": float(np.std(fA, ddof=1) / np.sqrt(N))}
    at = np.arange(points) if grid_index is None else np.arange(points)[grid_index]
    for P in (range(d) if w is None else w):
        grid = np.linspace(emul.all_data.input_range[P][0], emul.all_data.input_range[P][1], points)
        X = np.tile(A, (at.size, 1))
        X[:, P] = np.repeat(grid[at], N)
        f = _mean_at(emul, X).reshape(at.size, N)
        for key, val in (("mean_effect", f.mean(axis=1)), ("se", f.std(axis=1, ddof=1) / np.sqrt(N))):
            out[key][P] = np.nan
            out[key][P, at] = val
    return out


def sobol_group_estimates(f, C):
    """Uncertainty and sensitivity measures WITH the emulator's own uncertainty, by Monte Carlo
    from the posterior mean and the posterior covariance inside the groups of a Sobol' design
    (host only).  f is N x (d + 2) and C is N x (d + 2) x (d + 2): the mean and covariance at
    the points [A_a, B_a, AB_0_a, ..., AB_d-1_a] of sample a, AB_i being A with column i taken
    from B.  Two points of a group are independent draws (A, B), share one coordinate (B, AB_i)
    or share all but one (A, AB_i), which is every pair the integrals below range over.

    Every term is the mean of its N per-sample values, with ``*_se`` = std(ddof = 1) / sqrt(N):
      uE      E*[E f]       1/2 (fA + fB)
      uV      var*[E f]     c(A, B)
      uEV     E*[Var f]     1/2 (fA - fB)^2 + 1/2 (c(A, A) + c(B, B)) - c(A, B)
      EV[i]   E*[V_i]       fB (fAB_i - fA) + c(B, AB_i) - c(A, B)
      EVT[i]  E*[V_Ti]      1/2 (fA - fAB_i)^2 + 1/2 (c(A, A) + c(AB_i, AB_i)) - c(A, AB_i)
      S, ST                 EV / uEV, EVT / uEV
      V, VT (and _se)       the mean-only terms of ``sobol_estimates``: the above without c
    EVT is the true total-effect variance E*[E[Var(f | x_-i)]], not the reference's
    ``uEV - senseindex[P]`` (see the module docstring)."""
    f = np.asarray(f, dtype=float)
    C = np.asarray(C, dtype=float)
    if f.ndim != 2 or f.shape[1] < 3 or C.shape != (f.shape[0], f.shape[1], f.shape[1]):
        raise ValueError("f must be N x (d + 2) and C N x (d + 2) x (d + 2)")
    N = f.shape[0]
    fA, fB, fAB = f[:, 0], f[:, 1], f[:, 2:].T                 # (N), (N), (d x N)
    cAA, cBB, cAB = C[:, 0, 0], C[:, 1, 1], C[:, 0, 1]
    cii = np.diagonal(C, axis1=1, axis2=2)[:, 2:].T            # c(AB_i, AB_i)
    cBi, cAi = C[:, 1, 2:].T, C[:, 0, 2:].T                    # c(B, AB_i), c(A, AB_i)
    tV = fB[None, :] * (fAB - fA[None, :])
    tT = 0.5 * (fA[None, :] - fAB) ** 2
    terms = {"uE": 0.5 * (fA + fB), "uV": cAB,
             "uEV": 0.5 * (fA - fB) ** 2 + 0.5 * (cAA + cBB) - cAB,
             "EV": tV + cBi - cAB[None, :],
             "EVT": tT + 0.5 * (cAA[None, :] + cii) - cAi,
             "V": tV, "VT": tT}
    out = {}
    for key, t in terms.items():
        val, se = t.mean(axis=-1), t.std(axis=-1, ddof=1) / np.sqrt(N)
        out[key], out[key + "_se"] = (float(val), float(se)) if t.ndim == 1 else (val, se)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["S"], out["ST"] = out["EV"] / out["uEV"], out["EVT"] / out["uEV"]
    return out


def mc_emulator_indices(emul, m, v, samples, seed=0, dist="normal"):
    """The uncertainty and sensitivity measures that carry the emulator's own uncertainty --
    var*[E f], E*[Var f], E*[V_i], E*[V_Ti] -- by Monte Carlo, for inputs with means m and
    variances v: ``sobol_group_estimates``' dict on the design of ``sobol_points`` (the one
    ``mc_indices`` uses at the same seed), interleaved sample by sample into groups
    [A_a, B_a, AB_0_a, ..., AB_d-1_a] of d + 2 points and evaluated in ONE posterior-groups call
    (gpe_posterior_groups: the covariance inside each group and nothing else).

    No closed form is involved, so this works for every correlation family and both input
    distributions: it gives a Matern emulator, on which ``setup`` raises ``NonGaussianKernel``,
    what ``uncertainty()``, ``sensitivity()`` and ``totaleffectvariance()`` report for the
    Gaussian kernel.  EVT is the true total-effect variance, not the reference's
    ``uEV - senseindex[P]``.  d + 2 <= 64, else ValueError."""
    d = emul.training.inputs.shape[1]
    if d + 2 > 64:
        raise ValueError("mc_emulator_indices takes at most 62 inputs (groups of d + 2 <= 64 points), not %d" % d)
    N = int(samples)
    A, B = sobol_points(d, N, seed, dist, m, v)
    X = np.empty((N, d + 2, d))
    X[:, 0], X[:, 1] = A, B
    for i in range(d):
        X[:, 2 + i] = A
        X[:, 2 + i, i] = B[:, i]
    xs = Data(X.reshape(N * (d + 2), d), None, emul.basis, emul.par, emul.beliefs, emul.K)
    f, C = posterior_groups(xs, emul.training, emul.par, emul.K, d + 2)
    return sobol_group_estimates(f.reshape(N, d + 2), C)


def setup(emul, m, v, case="case2"):
    """Sensitivity instance for emulator `emul`, input means m and variances v
    (reference sensitivityfunctions.py:7-54).

    The closed forms are those of the Gaussian kernel: any other family raises
    ``NonGaussianKernel``.  The variance-based route for such an emulator is Monte Carlo on its
    posterior mean, ``mc_indices`` and ``mc_main_effect``; ``derivative_measures`` is the
    derivative-based one."""
    print("\n*** Initialising Sensitivity class ***")
    family = getattr(emul.K, "family", "gaussian")
    if family != "gaussian":
        raise NonGaussianKernel(
            "sensitivity analysis needs a gaussian kernel: its integrals are closed forms of "
            "exp(-((x-x')/delta)^2), and this emulator's kernel is " + family
            + " (mc_indices and mc_main_effect estimate the variance-based measures for any kernel)")
    if not isinstance(m, list) or not isinstance(v, list):
        print("ERROR: 2nd and 3rd arguments must be lists of floats. "
              "Return None.")
        return None
    if case == "case2":
        if len(emul.par.beta) != emul.training.inputs[0].size + 1 \
                or False in [i == 'x' for i in emul.beliefs.basis_str[1:]]:
            print("The case2 sensitivity routines only work for emulators "
                  "with a gaussian kernel and linear mean. "
                  "This mean function will not work. Return None.")
            return None
        if len(m) != len(emul.par.beta) - 1 or len(v) != len(emul.par.beta) - 1:
            print("Mean and Variance lists must both contain as many items "
                  "as there are input dimensions. Return None.")
            return None
    else:
        print("Only case2 of MUCM's U & S analysis is implemented. Return None.")
        return None
    return Sensitivity(emul, np.array(m), np.array(v))


class Sensitivity:
    """Reference _sensitivityclasses.py:7-662 (case2)."""

    def __init__(self, emul, m, v):
        self.v = v
        self.m = m
        self.x = emul.training.inputs
        self.input_range = emul.all_data.input_range
        self.minmax = emul.all_data.minmax
        self.B = np.linalg.inv(np.diag(self.v))
        self.C = np.diag(1.0 / (np.array(emul.par.delta) ** 2))
        self.f = emul.training.outputs
        self.H = emul.training.H
        self.beta = emul.par.beta
        self.sigma = emul.par.sigma
        self.nugget = emul.par.nugget
        self._training = emul.training
        self._K = emul.K
        self._b = np.diag(self.B).copy()
        self._c = np.diag(self.C).copy()
        self.UPSQRT_const()
        Z = self._gpu().solve(np.column_stack([self.f - self.H.dot(self.beta), self.H]))
        self.e = Z[:, 0].copy()
        self.G = Z[:, 1:].copy()
        self.W = np.linalg.inv(self.H.T.dot(self.G))
        self._Z = Z                           # [e G] = A^-1 [f - H beta, H]
        self._AinvT = self._gpu().solve(self.T)
        self._evint_cache = None
        self.done_uncertainty = False
        self.done_sensitivity = False
        self.done_main_effect = False
        self.done_interaction = False
        self.done_totaleffectvar = False

    def _gpu(self):
        """The context with this emulator's training set and factor of training.A resident
        (as Posterior holds it); another emulator's analysis may have replaced them."""
        ctx = upload_training(self._training)
        K = self._K
        ctx.ensure_factor(K.kind, K.d, float(K.n), 1.0, self._training.r_scale())
        return ctx

    @property
    def A(self):
        """training.A as the reference holds it (formed on request only)."""
        return self._training.A

    # ------------------------------------------------------------ constants
    def UPSQRT_const(self):
        """T, R, Q, S, U and the per-point factors (:519-552), elementwise."""
        b, c, nu = self._b, self._c, self.nugget
        self.T1 = np.sqrt(self.B.dot(np.linalg.inv(self.B + 2.0 * self.C)))
        self.T2 = 0.5 * 2.0 * self.C.dot(self.B).dot(np.linalg.inv(self.B + 2.0 * self.C))
        self.T3 = (self.x - self.m) ** 2
        self.Tk_b4_prod = np.sqrt(b / (b + 2.0 * c))[None, :] * np.exp(-self.T3 * (c * b / (b + 2.0 * c))[None, :])
        self.T = (1.0 - nu) * np.prod(self.Tk_b4_prod, axis=1)
        self.R = np.append([1.0], self.m)
        self.Q = np.outer(self.R.T, self.R)
        self.S = np.outer(self.R.T, self.T)
        self.U = (1.0 - nu) * np.prod(np.diag(np.sqrt(self.B.dot(np.linalg.inv(self.B + 4.0 * self.C)))))
        self.Sw_b4_prod = self.Tk_b4_prod
        self.P1 = self.B.dot(np.linalg.inv(self.B + 2.0 * self.C))
        self.P2 = 0.5 * 2.0 * self.C.dot(self.B).dot(np.linalg.inv(self.B + 2.0 * self.C))
        self.P3 = self.T3
        self.P4 = np.sqrt(self.B.dot(np.linalg.inv(self.B + 4.0 * self.C)))
        self.P5 = 0.5 * np.linalg.inv(self.B + 4.0 * self.C)

    # ------------------------------------------------------------ uncertainty
    def uncertainty(self):
        """E*[E[f(X)]], var*[E[f(X)]], E*[var[f(X)]] (:54-203)."""
        print("\n*** Uncertainty measures ***")
        self.done_uncertainty = True
        m, b, c, nu = self.m, self._b, self._c, self.nugget
        d = m.size
        self.w = list(range(d))
        self.Rh = np.append([1.0], np.array(m[self.w]))
        self.Rhh = np.zeros([1 + d, 1 + d])
        self.Rhh[0, 0] = 1.0
        self.Rhh[0, 1:] = m
        self.Rhh[1:, 0] = m
        self.Rhh[1:, 1:] = np.outer(m, m) + np.linalg.inv(np.diag(b))
        # R integrals: the per-point (2C+B) solve is elementwise (:79-88)
        mpk = (2.0 * c * self.x + b * m) / (2.0 * c + b)
        Qk = (2.0 * ((mpk - self.x) ** 2).dot(c) + ((mpk - m) ** 2).dot(b))
        self.Rt = (1.0 - nu) * np.sqrt(np.linalg.det(self.B) / np.linalg.det(2.0 * self.C + self.B)) \
            * np.exp(-0.5 * Qk)
        self.Rht = self.Rt[None, :] * np.vstack([np.ones(self.x.shape[0]), mpk.T])
        # U integrals (:105-160)
        Bbold = np.block([[2.0 * self.C + self.B, -2.0 * self.C], [-2.0 * self.C, 2.0 * self.C + self.B]])
        self.U2 = (1.0 - nu) * np.linalg.det(self.B) / np.sqrt(np.linalg.det(Bbold))
        self.Uh = self.U2 * self.Rh
        self.Uhh = self.U2 * self.Rhh
        Bboldk = np.block([[2.0 * self.C + self.B, -2.0 * self.C], [-2.0 * self.C, 4.0 * self.C + self.B]])
        Ufact = ((1.0 - nu) ** 2) * np.linalg.det(self.B) / np.sqrt(np.linalg.det(Bboldk))
        n = self.x.shape[0]
        rhs = np.vstack([np.repeat(self.B.dot(m)[:, None], n, axis=1),
                         2.0 * self.C.dot(self.x.T) + self.B.dot(m)[:, None]])
        mp = np.linalg.solve(Bboldk, rhs)
        mp1, mp2 = mp[:d], mp[d:]
        Qku = (2.0 * ((mp2 - self.x.T) ** 2).T.dot(c) + 2.0 * ((mp1 - mp2) ** 2).T.dot(c)
               + ((mp1 - m[:, None]) ** 2).T.dot(b) + ((mp2 - m[:, None]) ** 2).T.dot(b))
        self.Ut = Ufact * np.exp(-0.5 * Qku)
        self.Uht = self.Ut[None, :] * np.vstack([np.ones(n), mp1, mp2])
        Bboldkl = np.block([[4.0 * self.C + self.B, -2.0 * self.C], [-2.0 * self.C, 4.0 * self.C + self.B]])
        self._Ufact2 = ((1.0 - nu) ** 3) * np.linalg.det(self.B) / np.sqrt(np.linalg.det(Bboldkl))
        self._hk = np.exp(-0.5 * Qk)
        self.Utild = 1
        # S integrals (:163-181)
        Smat = np.zeros([3 * d, 3 * d])
        Smat[:d, :d] = 4.0 * self.C + self.B
        Smat[d:2 * d, d:2 * d] = 2.0 * self.C + self.B
        Smat[2 * d:, 2 * d:] = 2.0 * self.C + self.B
        Smat[:d, d:2 * d] = -2.0 * self.C
        Smat[:d, 2 * d:] = -2.0 * self.C
        Smat[d:2 * d, :d] = -2.0 * self.C
        Smat[2 * d:, :d] = -2.0 * self.C
        Smat2 = np.block([[4.0 * self.C + self.B, -4.0 * self.C], [-4.0 * self.C, 4.0 * self.C + self.B]])
        self.S = ((1.0 - nu) ** 2) * ((np.sqrt(np.linalg.det(self.B))) ** 3) / np.sqrt(np.linalg.det(Smat))
        self.Stild = (1.0 - nu) * np.linalg.det(self.B) / np.sqrt(np.linalg.det(Smat2))
        # Rtt on the GPU: tr(A^-1 Rtt) and [e G]^T Rtt [e G]
        w0 = 2.0 * c * c / (4.0 * c + b)
        u0 = (1.0 - nu) * np.prod(b / (4.0 * c + b)) ** 0.25 \
            * np.exp(-((self.x - m) ** 2).dot(c * b / (4.0 * c + b)))
        tr, quad = self._gpu().sense_pairs(w0[None, :], u0[None, :], self._Z)
        trRtt, eRe, GRG = tr[0], quad[0, 0, 0], quad[0, 1:, 1:]
        AinvRt = self._gpu().solve(self.Rt)
        s2 = self.sigma ** 2
        G, W, e, beta = self.G, self.W, self.e, self.beta
        self.uE = self.Rh.T.dot(beta) + self.Rt.T.dot(e)
        self.uV = s2 * (self.U2 - self.Rt.T.dot(AinvRt)
                        + (self.Rh - G.T.dot(self.Rt)).T.dot(W).dot(self.Rh - G.T.dot(self.Rt)))
        self.I1 = s2 * (self.Utild - trRtt + np.trace(W.dot(self.Rhh - 2.0 * self.Rht.dot(G) + GRG)))
        self.I2 = beta.T.dot(self.Rhh).dot(beta) + 2.0 * beta.T.dot(self.Rht).dot(e) + eRe
        self.uEV = (self.I1 - self.uV) + (self.I2 - self.uE ** 2)
        print("E*[ E[f(X)] ]  :", self.uE)
        print("var*[ E[f(X)] ]:", self.uV)
        print("E*[ var[f(X)] ]:", self.uEV)

    @property
    def Utt(self):
        """Ufact2 exp(-(Qk + Ql)/2) (:146-159): rank one, formed on request."""
        return self._Ufact2 * np.outer(self._hk, self._hk)

    # ------------------------------------------------------------ w / wb terms
    def setup_w_wb(self, P):
        self.w = [P]
        self.wb = [k for k in range(len(self.m)) if k not in self.w]

    def _qw(self, w):
        """Qw (:554-582): R R^T with v_w added on the w diagonal."""
        Qw = np.outer(self.R, self.R)
        for i in w:
            Qw[1 + i, 1 + i] += self.v[i]
        return Qw

    def _estar(self, w):
        """Estar (:584-596)."""
        b, c = self._b, self._c
        E = np.repeat(self.R[:, None], self.x.shape[0], axis=1)
        for kn in w:
            E[1 + kn] = (2 * c[kn] * self.x[:, kn] + b[kn] * self.m[kn]) / (2 * c[kn] + b[kn])
        return E

    def _uw(self, wb):
        return (1.0 - self.nugget) * np.prod(np.diag(np.sqrt(self.B.dot(np.linalg.inv(self.B + 4.0 * self.C))))[wb])

    def _pw_factors(self):
        """(w, u) of Pw for w = [P], every P (see the module docstring)."""
        b, c, nu, m = self._b, self._c, self.nugget, self.m
        d = m.size
        P1, P2, P4 = b / (b + 2.0 * c), c * b / (b + 2.0 * c), np.sqrt(b / (b + 4.0 * c))
        dm2 = (self.x - m) ** 2
        W = np.zeros((d, d))
        Uf = np.zeros((d, self.x.shape[0]))
        for P in range(d):
            wb = [i for i in range(d) if i != P]
            W[P, P] = 2.0 * c[P] ** 2 / (b[P] + 4.0 * c[P])
            const = (1.0 - nu) * np.sqrt(np.prod(P1[wb]) * P4[P])
            Uf[P] = const * np.exp(-dm2[:, wb].dot(P2[wb]) - dm2[:, P] * c[P] * b[P] / (b[P] + 4.0 * c[P]))
        return W, Uf

    def _evint_all(self):
        """EEE - EE2 for w = [P], every P (:481-506); one pair-kernel call for all P."""
        if self._evint_cache is not None:
            return self._evint_cache
        d = self.m.size
        W, Uf = self._pw_factors()
        trPw, quad = self._gpu().sense_pairs(W, Uf, self._Z)
        s2 = self.sigma ** 2
        G, Wm, e, beta, T, R = self.G, self.W, self.e, self.beta, self.T, self.R
        TG = T.dot(G)
        EE2 = s2 * (self.U - T.dot(self._AinvT) + (R - TG).dot(Wm).dot(R - TG)) + (R.dot(beta) + T.dot(e)) ** 2
        out = np.zeros(d)
        for P in range(d):
            w = [P]
            wb = [k for k in range(d) if k not in w]
            Qw = self._qw(w)
            Sw = self._estar(w) * T[None, :]      # (1-nu) Estar prod(Sw_b4_prod) (:615-619)
            SwG = Sw.dot(G)
            EEE = s2 * (self._uw(wb) - trPw[P]
                        + np.trace(Wm.dot(Qw - SwG - SwG.T + quad[P, 1:, 1:]))) \
                + quad[P, 0, 0] + 2.0 * beta.T.dot(Sw).dot(e) + beta.T.dot(Qw).dot(beta)
            out[P] = EEE - EE2
        self._evint_cache = out
        return out

    # ------------------------------------------------------------ public measures
    def sensitivity(self):
        """Sensitivity indices E(V_w) for each input (:466-516)."""
        print("\n*** Calculate sensitivity indices ***")
        self.done_sensitivity = True
        ev = self._evint_all()
        self.senseindex = np.zeros([self.m.size])
        for P in range(self.m.size):
            self.setup_w_wb(P)
            self.EVint = ev[P]
            if self.done_uncertainty:
                print("E(V" + str(self.w) + ")/EV:", self.EVint / self.uEV)
            else:
                print("E(V" + str(self.w) + "):", self.EVint)
            self.senseindex[P] = self.EVint
        if self.done_uncertainty:
            print("Sum of Sensitivities:", np.sum(self.senseindex / self.uEV))

    def totaleffectvariance(self):
        """Total effect variances as the reference computes them (:405-463)."""
        self.done_totaleffectvar = True
        print("\n*** Calculate total effect variance ***")
        self.senseindexwb = np.zeros([self.m.size])
        self.EVTw = np.zeros([self.m.size])
        self.EVf = self.uEV
        print("E*[ var[f(X)] ]:", self.EVf)
        ev = self._evint_all()
        for P in range(self.m.size):
            self.EVaaa = ev[P]
            self.senseindexwb[P] = self.EVaaa
            self.EVTw[P] = self.EVf - self.EVaaa
            print("E(V[T" + str(P) + "]):", self.EVTw[P])

    def _line_sums(self, w, Y):
        """Tw . e for index set w at the rows of Y (len(w) columns)."""
        wb = [k for k in range(self.m.size) if k not in w]
        a = (1.0 - self.nugget) * np.prod(self.Tk_b4_prod[:, wb], axis=1) * self.e
        return self._gpu().gauss_transform(w, self._c[w], Y, a)

    def main_effect(self, plot=False, points=100, customKey=[], customLabels=[], plotShrink=0.9, w=[],
                    black_white=False):
        """Main effects of each input over its range (:238-324)."""
        print("\n*** Main effect measures ***")
        self.done_main_effect = True
        self.effect = np.zeros([self.m.size, points])
        self.mean_effect = np.zeros([self.m.size, points])
        if w == []:
            w = range(0, len(self.m))
        if plot:
            import matplotlib.pyplot as plt
            from cycler import cycler
            fig = plt.figure()
            ax = plt.subplot(111)
            if black_white:
                ax.set_prop_cycle(cycler('linestyle', ['-', '--', '-.', ':']))
                colors = plt.get_cmap('plasma')(np.linspace(0, 1.0, len(w)))
            else:
                colors = plt.get_cmap('jet')(np.linspace(0, 1.0, len(w)))
        base = self.R.dot(self.beta) + self.T.dot(self.e)
        cn = 0
        for P in w:
            print("Main effect measures for input", P, "range", self.input_range[P])
            self.setup_w_wb(P)
            xs = np.linspace(self.input_range[P][0], self.input_range[P][1], points)
            Twe = self._line_sums([P], xs[:, None])
            Rwb = self.R.dot(self.beta) + self.beta[1 + P] * (xs - self.m[P])
            self.mean_effect[P] = Rwb + Twe
            self.effect[P] = self.mean_effect[P] - base
            if plot:
                label = 'x' + str(P)
                if customKey != []:
                    try:
                        label = str(customKey[P])
                    except IndexError:
                        pass
                ax.plot(np.linspace(0.0, 1.0, points), self.effect[P], linewidth=2.0, label=label,
                        color=colors[cn])
            cn = cn + 1
        if plot:
            box = ax.get_position()
            ax.set_position([box.x0, box.y0, box.width * plotShrink, box.height])
            ax.legend(loc='center left', bbox_to_anchor=(1, 0.5))
            xl, yl = "xw", "Main Effect"
            if customLabels != []:
                xl = customLabels[0] if len(customLabels) > 0 else xl
                yl = customLabels[1] if len(customLabels) > 1 else yl
            plt.xlabel(xl)
            plt.ylabel(yl)
            print("Plotting main effects...")
            plt.show()

    def interaction_effect(self, i, j, points=25, customLabels=[]):
        """Interaction effect of inputs i and j on a points x points grid (:327-401)."""
        print("\n*** Interaction effects ***")
        self.done_interaction = True
        self.interaction = np.zeros([points, points])
        print("Recalculating main effect with", points, "points...")
        self.main_effect(plot=False, points=points, w=[i, j])
        self.w = [i, j]
        self.wb = [k for k in range(len(self.m)) if k not in self.w]
        ra_i = self.input_range[i]
        ra_j = self.input_range[j]
        print("\nCalculating", points * points, "interaction effects...")
        xi = np.linspace(ra_i[0], ra_i[1], points)
        xj = np.linspace(ra_j[0], ra_j[1], points)
        Y = np.column_stack([np.repeat(xi, points), np.tile(xj, points)])
        Twe = self._line_sums([i, j], Y).reshape(points, points)
        Rwb = (self.R.dot(self.beta) + self.beta[1 + i] * (xi - self.m[i])[:, None]
               + self.beta[1 + j] * (xj - self.m[j])[None, :])
        self.interaction = (Rwb + self.R.dot(self.beta)) + (Twe + self.T.dot(self.e)) \
            - self.mean_effect[i][:, None] - self.mean_effect[j][None, :]
        import matplotlib.pyplot as plt
        plt.figure()
        ax = plt.gca()
        im = ax.imshow(self.interaction, origin='lower', cmap=plt.get_cmap('hot'),
                       extent=(ra_i[0], ra_i[1], ra_j[0], ra_j[1]))
        plt.colorbar(im)
        xl, yl = "input " + str(self.w[0]), "input " + str(self.w[1])
        if customLabels != []:
            xl = customLabels[0] if len(customLabels) > 0 else xl
            yl = customLabels[1] if len(customLabels) > 1 else yl
        plt.xlabel(xl)
        plt.ylabel(yl)
        extent = ax.get_images()[0].get_extent()
        ax.set_aspect(abs((extent[1] - extent[0]) / (extent[3] - extent[2])) / 1.0)
        plt.show()

    def to_file(self, filename):
        """Results file in the reference's format (:641-662)."""
        print("Sensitivity & Uncertainty results to file...")
        with open(filename, 'w') as f:
            if self.done_uncertainty:
                f.write("EE " + str(self.uE) + "\n")
                f.write("VE " + str(self.uV) + "\n")
                f.write("EV " + str(self.uEV) + "\n")
            if self.done_sensitivity:
                f.write("EVw " + ' '.join(map(str, self.senseindex)) + "\n")
            if self.done_totaleffectvar:
                f.write("EVTw " + ' '.join(map(str, self.EVTw)) + "\n")
            if self.done_main_effect:
                f.write("xw " + ' '.join(map(str, [i for i in np.linspace(0.0, 1.0, self.effect[0].size)])) + "\n")
                for i in range(0, len(self.m)):
                    f.write("ME" + str(i) + " " + ' '.join(map(str, self.effect[i])) + "\n")


def sense_table(sense_list, inputNames=[], outputNames=[], rowHeight=6):
    """Table plot of sensitivity indices, one row per Sensitivity instance
    (reference sensitivityfunctions.py:57-148)."""
    import matplotlib.pyplot as plt
    print("\n*** Creating sensitivity table ***")
    if not isinstance(sense_list, list):
        print("ERROR: first argument must be list e.g. [s] or [s,] or [s1, s2]. "
              "Return None.")
        return None
    rows = len(sense_list)
    cols = len(sense_list[0].m) + 1
    for s in sense_list:
        if len(s.m) != cols - 1:
            print("Each emulator must be built with the same number of inputs.")
            return None
    for s in sense_list:
        if not s.done_uncertainty:
            s.uncertainty()
        if not s.done_sensitivity:
            s.sensitivity()
    if inputNames == []:
        inputNames = ["input " + str(i) for i in range(cols - 1)]
    inputNames.append("Sum")
    if outputNames == []:
        outputNames = ["output " + str(i) for i in range(rows)]
    cells = np.zeros([rows, cols])
    for si, s in enumerate(sense_list):
        cells[si, 0:cols - 1] = s.senseindex / s.uEV
        cells[si, cols - 1] = np.sum(s.senseindex / s.uEV)
    tab_2 = [['%.3f' % j for j in i] for i in cells]
    fig = plt.figure(figsize=(16, 8))
    fig.add_subplot(111, frameon=False, xticks=[], yticks=[])
    img = plt.imshow(cells, cmap="hot", vmin=0.0, vmax=1.0)
    img.set_visible(False)
    tb = plt.table(cellText=tab_2, colLabels=inputNames, rowLabels=outputNames, loc='center',
                   cellColours=img.to_rgba(cells))
    tb.scale(1, rowHeight)
    for i in range(1, rows + 1):
        for j in range(0, cols):
            tb._cells[(i, j)]._text.set_color('green')
    plt.show()
    return None
