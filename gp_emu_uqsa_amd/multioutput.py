"""The separable multi-output emulator (MUCM's ProcBuildMultiOutputGPSep; Conti & O'Hagan
2010): p outputs of one simulator share the correlation function, so one Cholesky per
objective evaluation, one variance product and one pass over the kernel values serve them all,
where p separate emulators (the reference's ``examples/sensitivity_multi_outputs``,
``history_match``'s ``emuls``) pay p times.  The p x p between-output covariance Sigma is
estimated in closed form, as the ``mucm`` objective estimates sigma^2.

    M = setup("config", outputs=[0, 1])      # same config and beliefs files as api.setup
    train(M)                                 # sets M.par (delta, nugget), M.Sigma, M.B
    mean = posterior_mean(M, x)              # m x p
    mean, c, Sigma = posterior(M, x)         # cov(output a at x, b at x') = Sigma[a, b] c(x, x')
    E0 = M.single(0)                         # an ordinary Emulator for output 0

Output j alone is a single-output emulator with the shared delta and nugget,
sigma = sqrt(Sigma[j, j]) and beta = B[:, j]; ``M.single(j)`` builds it, and ``history_match``,
``sensitivity``, ``loo`` and the design tools take it unchanged.
"""
from __future__ import annotations

import copy as _copy

import numpy as _np

from . import distributed as _distributed
from . import files as _files
from . import kernels as _kernels
from . import model as _model
from . import native as _native
from . import optimize as _optimize


class _MultiOptimize(_optimize.Optimize):
    """Optimize's multistart L-BFGS-B (its guesses, bounds, transform and constraint
    handling) on gpe_objective_multi: data is the training set with output 0 as its
    ``outputs``, F all p outputs."""

    def __init__(self, data, F, basis, par, beliefs, config):
        self.F = _np.ascontiguousarray(F, dtype=float)
        self.Sigma = None
        self.B = None
        super().__init__(data, basis, par, beliefs, config)

    def context(self):
        """The context with data's training set and F resident."""
        if _distributed.active_objective() is not None:
            raise RuntimeError("the multi-output objective runs on one GPU (no row-block distribution)")
        ctx = _model.upload_training(self.data)
        ctx.ensure_outputs(self.F)
        return ctx

    def _concurrency(self, ntries):
        return 1      # (one context holds the outputs)

    def _call_multi(self, x, want_grad=True):
        return self.context().objective_multi(self.data.K.kind, x, nu_fixed=float(self.data.K.n),
                                              want_grad=want_grad)

    def _keep(self, Sigma, B):
        self.Sigma, self.B = Sigma, B
        self.par.sigma = float(_np.sqrt(Sigma[0, 0]))      # (par describes output 0)

    def loglikelihood_mucm(self, x):
        x = self.data.K.untransform(x)
        self.data.K.set_params(x)
        self.data.make_A()
        try:
            llh, grad, Sigma, B = self._call_multi(x)
        except _native.NotPositiveDefinite:
            print("  Matrix not PSD for", x, ", try adjusting nugget.")
            return None
        self._keep(Sigma, B)
        return llh, grad

    def sigma_analytic_mucm(self, x):
        self.data.K.set_params(x)
        self.data.make_A()
        try:
            _, _, Sigma, B = self._call_multi(_np.asarray(x, dtype=float), want_grad=False)
        except _native.NotPositiveDefinite:
            print("  In sigma_analytic_mucm(): Matrix not PSD for", x, ", try adjusting nugget.")
            raise SystemExit(1)
        self._keep(Sigma, B)

    def optimalbeta(self):
        ctx = self.context()
        ctx.ensure_factor(self.data.K.kind, self.data.K.d, float(self.data.K.n), 1.0, self.data.r_scale())
        self.B = ctx.beta_multi()
        self.par.beta = self.B[:, 0].copy()


class MultiEmulator:
    """What ``setup`` returns: the shared pieces of an ``Emulator`` (config, beliefs, par, basis,
    tv_conf, all_data, K), the training set (``training``: a ``Data`` whose ``outputs`` is output
    0; ``F``: all p outputs, n x p) and the validation set (``x_V``, ``Y_V``), and after ``train``
    ``Sigma`` (p x p) and ``B`` (q x p)."""

    def __init__(self, config, beliefs, par, basis, tv_conf, all_data, Y_full, outputs, training, F,
                 x_V, Y_V, opt, K):
        self.config, self.beliefs, self.par, self.basis = config, beliefs, par, basis
        self.tv_conf, self.all_data, self.Y_full, self.outputs = tv_conf, all_data, Y_full, list(outputs)
        self.training, self.F, self.x_V, self.Y_V, self.opt, self.K = training, F, x_V, Y_V, opt, K
        self.Sigma = None
        self.B = None

    @property
    def p(self):
        return self.F.shape[1]

    def single(self, j):
        """An ordinary ``Emulator`` for output j: the shared delta and nugget,
        sigma = sqrt(Sigma[j, j]), beta = B[:, j]."""
        if self.Sigma is None:
            raise RuntimeError("train() the MultiEmulator first")
        par = _copy.copy(self.par)
        par.delta = _np.array(self.K.d, dtype=float)
        par.nugget = self.K.n
        par.sigma = float(_np.sqrt(self.Sigma[j, j]))
        par.beta = _np.array(self.B[:, j], dtype=float)
        beliefs = _copy.copy(self.beliefs)
        beliefs.output = self.outputs[j]
        all_data = _copy.copy(self.all_data)
        all_data.y_full = self.Y_full[:, j].copy()
        training = _model.Data(self.training.inputs, self.F[:, j].copy(), self.basis, par, beliefs, self.K)
        if not _np.isscalar(self.training.r):
            training.set_r(self.training.r, message=False)
        validation = _model.Data(self.x_V, self.Y_V[:, j].copy(), self.basis, par, beliefs, self.K)
        post = _model.Posterior(validation, training, par, beliefs, self.K)
        opt_T = _optimize.Optimize(training, self.basis, par, beliefs, _copy.copy(self.config))
        return _model.Emulator(self.config, beliefs, par, self.basis, self.tv_conf, all_data, training,
                               validation, post, opt_T, self.K)


def _rows_T(all_data):
    tv, V = all_data.tv, all_data.V
    return list(range(0, tv.c * V)) + list(range((tv.c + tv.noV) * V, tv.k * V + all_data.remainder))


def _rows_V(all_data):
    tv, V = all_data.tv, all_data.V
    return list(range(tv.c * V, (tv.c + 1) * V))


def setup(config_file, outputs, datashuffle=True, scaleinputs=True):
    """Read config + beliefs as ``api.setup`` does and return a ``MultiEmulator`` for the columns
    ``outputs`` of the outputs file (they replace the beliefs' ``output``).  The input scaling and
    the T / V split are All_Data's; the rows are shuffled once (np.random.shuffle) with every
    output column beside its inputs.  Sigma is analytic, so the beliefs' ``mucm`` is read as T."""
    outputs = [int(o) for o in outputs]
    if not 1 <= len(outputs) <= 64:
        raise ValueError("outputs: 1 to 64 columns of the outputs file")
    config = _files.Config(config_file)
    beliefs = _files.Beliefs(config.beliefs)
    beliefs.output = outputs[0]
    beliefs.mucm = "T"
    par = _model.Hyperparams(beliefs)
    basis = _model.Basis(beliefs)
    tv_conf = _model.TV_config(*config.tv_config)
    all_data = _model.All_Data(config.inputs, config.outputs, tv_conf, beliefs, par, False, scaleinputs)
    try:
        Y = _np.loadtxt(config.outputs, usecols=outputs, ndmin=2)
    except (IndexError, ValueError):
        print("ERROR: an output (column) of", outputs, "is not in the outputs file")
        raise SystemExit(1)
    if datashuffle:
        print("Shuffling", all_data.numpoints, "data points (all", len(outputs), "outputs)")
        perm = _np.arange(all_data.numpoints)
        _np.random.shuffle(perm)
        all_data.x_full = all_data.x_full[perm]
        Y = Y[perm]
        all_data.y_full = Y[:, 0].copy()
    alt = beliefs.alt_nugget == "T"
    K = _kernels.for_beliefs(beliefs.kernel, alt)(all_data.x_full.shape[1], par)
    rT, rV = _rows_T(all_data), _rows_V(all_data)
    x_T, F = all_data.x_full[rT, :], _np.ascontiguousarray(Y[rT, :])
    training = _model.Data(x_T, F[:, 0].copy(), basis, par, beliefs, K)
    opt = _MultiOptimize(training, F, basis, par, beliefs, config)
    return MultiEmulator(config, beliefs, par, basis, tv_conf, all_data, Y, outputs, training, F,
                         all_data.x_full[rV, :], Y[rV, :], opt, K)


def train(M, message=False):
    """One training round on T (no files are written): the multistart L-BFGS-B of ``Optimize`` on
    the multi-output objective.  Sets M.par (delta, nugget; sigma and beta of output 0), M.Sigma
    and M.B."""
    print("\n*** Training", M.p, "outputs on", M.training.inputs.shape[0], "points ***")
    M.opt.llh_optimize(message)
    M.training.remake()
    M.Sigma = _np.array(M.opt.Sigma, dtype=float)
    M.B = _np.array(M.opt.B, dtype=float)
    return None


def _points(M, x):
    x = _np.asarray(x, dtype=float)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    if x.shape[1] != M.training.inputs.shape[1]:
        raise ValueError("test points have a different number of columns than the emulator's inputs")
    return x


def _resident(M):
    if M.Sigma is None:
        raise RuntimeError("train() the MultiEmulator first")
    ctx = M.opt.context()
    ctx.ensure_factor(M.K.kind, M.K.d, float(M.K.n), 1.0, M.training.r_scale())
    return ctx


def posterior_mean(M, x):
    """The posterior means of the p outputs at x (m x p): one fused kernel in which every kernel
    value is formed once and used p times (gpe_posterior_mean_multi); any m."""
    x = _points(M, x)
    return _resident(M).posterior_mean_multi(x, M.basis.design_matrix(x), M.B)


def posterior(M, x, full=False):
    """(mean m x p, c, Sigma): cov(output a at x_s, output b at x_t) = Sigma[a, b] c[s, t]; c is
    the single-output posterior covariance at sigma = 1, m x m with ``full``, else its diagonal."""
    x = _points(M, x)
    ctx = _resident(M)
    H = M.basis.design_matrix(x)
    mean = ctx.posterior_mean_multi(x, H, M.B)
    _, c = ctx.posterior(x, H, M.B[:, 0], 1.0, full_var=bool(full))
    return mean, c, M.Sigma.copy()
