"""Public API with the reference's signatures (emulatorfunctions.py:13-286):
setup, train, plot, posterior, posterior_sample; and loo, posterior_gradient and
posterior_mean, which the reference lacks."""
from __future__ import annotations

import numpy as _np

from . import files as _files
from . import kernels as _kernels
from . import model as _model
from . import native as _native
from . import optimize as _optimize
from . import plotting as _plotting


def setup(config_file, datashuffle=True, scaleinputs=True):
    """Read config + beliefs, load and split the data, build kernel, data sets,
    validation posterior and optimiser; return an Emulator (reference :13-57)."""
    config = _files.Config(config_file)
    beliefs = _files.Beliefs(config.beliefs)
    par = _model.Hyperparams(beliefs)
    basis = _model.Basis(beliefs)
    tv_conf = _model.TV_config(*config.tv_config)
    all_data = _model.All_Data(config.inputs, config.outputs, tv_conf, beliefs, par,
                               datashuffle, scaleinputs)
    alt = beliefs.alt_nugget == "T"
    if alt:
        print("\n*** Using alternative nugget ***")
    if beliefs.kernel != "gaussian":
        print("\n*** Using kernel", beliefs.kernel, "***")
    K = _kernels.for_beliefs(beliefs.kernel, alt)(all_data.x_full.shape[1], par)
    x_T, y_T = all_data.choose_T()
    x_V, y_V = all_data.choose_V()
    training = _model.Data(x_T, y_T, basis, par, beliefs, K)
    validation = _model.Data(x_V, y_V, basis, par, beliefs, K)
    post = _model.Posterior(validation, training, par, beliefs, K)
    opt_T = _optimize.Optimize(training, basis, par, beliefs, config)
    return _model.Emulator(config, beliefs, par, basis, tv_conf, all_data, training,
                           validation, post, opt_T, K)


def train(E, auto=True, message=False, no_retrain=False):
    """Train on T, validate on V, optionally fold V into T and repeat; write the
    updated beliefs and T-data files (reference :61-124)."""
    E.tv_conf.auto_train(auto, no_retrain)
    while E.tv_conf.doing_training():
        print("\n*** Training round", E.tv_conf.no_of_trains, "***")
        print("Training points:", E.training.inputs.shape[0])
        E.opt_T.llh_optimize(message)
        E.training.remake()
        E.validation.remake()
        E.post.remake()
        E.post.mahalanobis_distance()
        E.post.indiv_standard_error(ise=2.0)
        E.beliefs.final_beliefs(E, False)
        E.post.final_design_points(E, False)
        if E.tv_conf.check_still_training():
            print("Preparing for next round of training...")
            E.post.incVinT()
            E.tv_conf.next_Vset()
            E.all_data.choose_new_V(E.validation)
            E.training.remake()
            E.validation.remake()
            E.post.remake()
    if E.tv_conf.do_final_build():
        print("\n*** Doing final build ***")
        if E.tv_conf.noV != 0 and E.training.inputs.shape[0] < E.all_data.numpoints:
            E.post.incVinT()
        E.training.remake()
        E.opt_T.llh_optimize(message)
        E.training.remake()
        E.beliefs.final_beliefs(E, True)
        E.post.final_design_points(E, True)
    return None


def _as_points(E, x):
    x = _np.asarray(x, dtype=float)
    if x[0].size == 1:
        x = _np.array([x]).T
    if x[0, :].size != E.training.inputs[0, :].size:
        print("ERROR: test points have different number of columns to data in emulator. Exiting.")
        raise SystemExit(1)
    return x


def posterior(E, x, predict=True):
    """(mean, full covariance) at x (reference :226-252)."""
    x = _as_points(E, x)
    xs = _model.Data(x, None, E.basis, E.par, E.beliefs, E.K)
    p = _model.Posterior(xs, E.training, E.par, E.beliefs, E.K, predict=predict)
    return p.mean, p.var


def posterior_gradient(E, x, want_var=True):
    """(dmean, dvar), m x d each: the gradients of ``posterior``'s mean and of the diagonal of
    its covariance with respect to x, as ``posterior`` takes it (no counterpart in the
    reference).  Analytic and for every kernel family; dvar is None without want_var."""
    x = _as_points(E, x)
    xs = _model.Data(x, None, E.basis, E.par, E.beliefs, E.K)
    return _model.posterior_gradient(xs, E.training, E.par, E.K, want_var=want_var)


def posterior_mean(E, x):
    """The posterior mean alone at x, as ``posterior`` takes it (m values; no counterpart in
    the reference): no covariance is formed, so millions of points cost what their kernel
    evaluations cost.  For every kernel family; equal to ``posterior``'s mean to rounding."""
    x = _as_points(E, x)
    xs = _model.Data(x, None, E.basis, E.par, E.beliefs, E.K)
    return _model.posterior_mean(xs, E.training, E.par, E.K)


def posterior_groups(E, x, group):
    """(mean (m), cov (m // group, group, group)) at x, as ``posterior`` takes it: the posterior
    covariance inside groups of ``group`` consecutive points, i.e. the block diagonal of
    ``posterior``'s covariance without its other entries (no counterpart in the reference; the
    points' own r is not added).  For every kernel family and any number of points;
    1 <= group <= 64 and the number of points a multiple of it, else ValueError."""
    x = _as_points(E, x)
    if isinstance(group, bool) or int(group) != group or not 1 <= group <= 64:
        raise ValueError("group must be an integer in 1..64")
    if x.shape[0] % int(group) != 0:
        raise ValueError("the number of points (%d) is not a multiple of group (%d)" % (x.shape[0], group))
    xs = _model.Data(x, None, E.basis, E.par, E.beliefs, E.K)
    return _model.posterior_groups(xs, E.training, E.par, E.K, int(group))


def loo(E):
    """Leave-one-out validation of E on its own training set with its current
    hyperparameters: a ``LeaveOneOut`` with mean, var, var_obs, error, score and
    indiv_standard_error (no counterpart in the reference; one pass over L^-1 on the GPU
    where the reference would need one refit per training point)."""
    return _model.LeaveOneOut(E.training, E.par, E.beliefs, E.K)


def posterior_sample(E, x, predict=True):
    """mean + chol(var) u, u ~ N(0, I) from np.random (reference :255-286); the
    Cholesky of the posterior covariance runs on the GPU (gpe_cholesky)."""
    x = _as_points(E, x)
    xs = _model.Data(x, None, E.basis, E.par, E.beliefs, E.K)
    p = _model.Posterior(xs, E.training, E.par, E.beliefs, E.K, predict=predict)
    L = _native.default_context().cholesky(p.var, want=("L",))["L"]
    u = _np.random.randn(x.shape[0])
    return p.mean + L.dot(u)


def plot(E, plot_dims, fixed_dims=[], fixed_vals=[], mean_or_var="mean", customLabels=[],
         points=False, predict=True):
    """1-D or 2-D plot of the posterior mean or variance on a 30 x 30 grid
    (reference :128-223); the variance uses the diagonal-only posterior path."""
    return _plotting.plot(E, plot_dims, fixed_dims, fixed_vals, mean_or_var, customLabels,
                          points, predict)
