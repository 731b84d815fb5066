"""posterior_gradient and sensitivity.derivative_measures end to end: an emulator trained on
the toy-sim example (as test_gpu_matern.test_train_toy_sim_with_matern52 trains it), with the
Gaussian kernel and with `kernel matern52`.

The analytic gradients are compared with central differences (step h = 1e-5) of
g.posterior's mean and diagonal variance.  Those carry the GPU posterior's own error, up to
1e-8, divided by 2 h: hence 1e-6 max(1, max |d|) here, against 1e-8 where the comparison is
with the dense reference (test_gpu_posterior_grad.py).
"""
import os
import shutil

import numpy as np
import pytest

import gp_emu_uqsa_amd as g
from gp_emu_uqsa_amd import api, kernels, model, sensitivity

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(__file__), "golden", "examples")
STEP = 1e-5


@pytest.fixture(scope="module", params=["gaussian", "matern52"])
def emulator(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("grad") / "toy-sim"
    shutil.copytree(os.path.join(EX, "toy-sim"), d)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        if request.param != "gaussian":
            with open("toy-sim_beliefs", "a") as fh:
                fh.write("kernel " + request.param + "\n")
        np.random.seed(0)
        E = g.setup("toy-sim_config")
        g.train(E, auto=True)
    finally:
        os.chdir(cwd)
    assert type(E.K) is kernels.for_beliefs(request.param, False)
    return E


def points(E, m, seed):
    return np.random.RandomState(seed).uniform(0.05, 0.95, (m, E.training.inputs.shape[1]))


def test_posterior_gradient_against_central_differences(emulator):
    E = emulator
    x = points(E, 50, 4)
    d = x.shape[1]
    dmean, dvar = api.posterior_gradient(E, x)
    assert dmean.shape == dvar.shape == (50, d)
    fm, fv = np.empty((50, d)), np.empty((50, d))
    for k in range(d):
        out = []
        for sgn in (1.0, -1.0):
            xp = x.copy()
            xp[:, k] += sgn * STEP
            mean, var = g.posterior(E, xp)
            out.append((mean, np.diag(var)))
        fm[:, k] = (out[0][0] - out[1][0]) / (2.0 * STEP)
        fv[:, k] = (out[0][1] - out[1][1]) / (2.0 * STEP)
    em = np.max(np.abs(dmean - fm)) / max(1.0, np.max(np.abs(fm)))
    ev = np.max(np.abs(dvar - fv)) / max(1.0, np.max(np.abs(fv)))
    print(E.K.family if hasattr(E.K, "family") else "gaussian", "d mean against central differences", em,
          "d var", ev, "max |d mean|", np.max(np.abs(fm)), "max |d var|", np.max(np.abs(fv)))
    assert np.max(np.abs(fm)) > 1e-2   # (no comparison of zeros)
    assert em <= 1e-6 and ev <= 1e-6
    only_mean, none = api.posterior_gradient(E, x, want_var=False)
    assert none is None and np.array_equal(only_mean, dmean)
    assert g.posterior_gradient is api.posterior_gradient
    # the same through a Posterior object
    xs = model.Data(x, None, E.basis, E.par, E.beliefs, E.K)
    pm, pv = model.Posterior(xs, E.training, E.par, E.beliefs, E.K, full_var=False).gradient()
    assert np.array_equal(pm, dmean) and np.array_equal(pv, dvar)


def test_derivative_measures(emulator):
    E = emulator
    x = points(E, 400, 6)
    d = x.shape[1]
    nu, share = sensitivity.derivative_measures(E, x)
    assert nu.shape == share.shape == (d,)
    assert np.all(nu >= 0.0) and np.all(share >= 0.0)
    assert abs(np.sum(share) - 1.0) <= 1e-14
    dmean, _ = api.posterior_gradient(E, x)
    want = np.mean(dmean ** 2, axis=0)
    np.testing.assert_allclose(nu, want, rtol=1e-13, atol=0.0)
    np.testing.assert_allclose(share, want / np.sum(want), rtol=1e-13, atol=0.0)
    if getattr(E.K, "family", "gaussian") != "gaussian":
        # the closed forms still refuse the emulator: derivative_measures is its route
        with pytest.raises(sensitivity.NonGaussianKernel, match="gaussian kernel"):
            sensitivity.setup(E, [0.5] * d, [0.02] * d)
