"""gpe_loo on the GPU against the NumPy closed form (tests/loo_ref.py, itself checked
against n brute-force refits in test_loo_host.py).

Mean (max |d mean| / max |f|) and variance (max relative error) are held to 1e-8, the
tolerance the posterior is held to elsewhere in the suite; the two host routes agree to
1e-11 or better on these cases, so 1e-8 sits 1000x above the reference's own error.
"""
import os
import shutil

import numpy as np
import pytest

import gp_emu_uqsa_amd as g
import loo_ref
from gp_emu_uqsa_amd import native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-8
EX = os.path.join(os.path.dirname(__file__), "golden", "examples")


def _factor(ctx, name):
    X, f, H, r, kind, delta, nu, _ = loo_ref.problem(name)
    ctx.set_data(X, f, H, r)
    ctx.factor(kind, delta, nu, 1.0, 0.0 if r is None else 1.0)
    return f


def _check(name, f, mean, var):
    rm, rv, _ = loo_ref.reference(name)
    em, ev = loo_ref.errors(mean, var, rm, rv, f)
    print(name, "mean error", em, "variance error", ev)
    assert em < TOL
    assert ev < TOL


@pytest.mark.parametrize("name", sorted(loo_ref.CASES))
def test_loo_matches_closed_form(ctx, name):
    f = _factor(ctx, name)
    mean, var, _ = ctx.loo(loo_ref.SIGMA)
    _check(name, f, mean, var)


def test_two_calls_are_bit_identical(ctx):
    _factor(ctx, "n1000_std")
    a = ctx.loo(loo_ref.SIGMA)
    b = ctx.loo(loo_ref.SIGMA)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_beta_out_is_the_gls_beta(ctx):
    """Both come from the Gram matrix of L^-1 [f H] of the same factor; when that is formed by
    another route (forward substitution before the inverse exists) they differ by its
    rounding, cond(A) eps = 3e5 x 1e-16."""
    _factor(ctx, "n300_alt_r")
    before = ctx.beta()
    beta = ctx.loo(loo_ref.SIGMA)[2]
    after = ctx.beta()
    scale = np.max(np.abs(after))
    assert np.max(np.abs(beta - after)) <= 1e-9 * scale
    assert np.max(np.abs(beta - before)) <= 1e-9 * scale


def test_after_a_gradient_objective_and_a_new_factor(ctx):
    """The objective's gradient leaves its own L^-1 and A^-1 in the workspace; the factor
    that follows must invalidate them, and gpe_loo must invert the new one."""
    name = "n1000_std"
    X, f, H, r, kind, delta, nu, _ = loo_ref.problem(name)
    ctx.set_data(X, f, H, r)
    hp = np.concatenate([1.3 * delta, [5e-3, 0.9]])   # other hyperparameters than the factor's
    ctx.objective(native.GP4ML, kind, hp, want_grad=True)
    ctx.factor(kind, delta, nu, 1.0, 0.0)
    mean, var, _ = ctx.loo(loo_ref.SIGMA)
    _check(name, f, mean, var)


def test_without_a_factor_is_a_state_error():
    c = native.Context(0)
    try:
        X, f, H = orc.synthetic_problem(60, 3, seed=0)
        c.set_data(X, f, H)
        with pytest.raises(RuntimeError, match=r"gpe_loo failed \(-4\): no resident factor \(call gpe_factor\)"):
            c.loo(loo_ref.SIGMA)
    finally:
        c.close()


def test_too_few_points_is_an_argument_error(ctx):
    X, f, H = orc.synthetic_problem(4, 2, seed=0)   # n = 4, q = 3 < n - 1: no residual degree of freedom
    ctx.set_data(X, f, H)
    ctx.factor(native.KERNEL_STD, [1.0, 1.0], 1e-3, 1.0, 0.0)
    with pytest.raises(RuntimeError, match=r"gpe_loo failed \(-1\)"):
        ctx.loo(loo_ref.SIGMA)


def test_api_loo_on_the_toy_sim_example(tmp_path, monkeypatch, capsys):
    d = tmp_path / "toy-sim"
    shutil.copytree(os.path.join(EX, "toy-sim"), d)
    monkeypatch.chdir(d)
    np.random.seed(0)
    E = g.setup("toy-sim_config")
    lo = g.loo(E)
    sigma = float(E.par.sigma)
    mean, var, beta = native.default_context().loo(sigma)   # the factor g.loo left resident
    assert lo.mean.tobytes() == mean.tobytes()
    assert lo.var.tobytes() == var.tobytes()
    assert lo.beta.tobytes() == beta.tobytes()
    n = E.training.outputs.size
    assert lo.mean.shape == lo.var.shape == (n,)
    assert np.all(lo.var > 0.0)
    rs = E.training.r_scale()
    var_obs = var + sigma ** 2 * rs * np.asarray(E.training.r, dtype=float) if rs != 0.0 else var
    np.testing.assert_array_equal(lo.var_obs, var_obs)
    err = (E.training.outputs - mean) / np.sqrt(var_obs)
    np.testing.assert_array_equal(lo.error, err)
    assert lo.score == pytest.approx(np.mean(0.5 * np.log(2.0 * np.pi * var_obs) + 0.5 * err ** 2), rel=1e-14)
    capsys.readouterr()
    assert lo.indiv_standard_error(ise=0) is True
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("  Bad predictions:")]
    assert len(lines) == n
    assert lines[0] == "  Bad predictions: " + str(E.training.inputs[0, :]) + " ise: " + str(np.round(err[0], decimals=4))
    assert lo.indiv_standard_error(ise=np.max(np.abs(err)) * 2.0) is False
