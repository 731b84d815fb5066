"""CPU checks of the Matern reference (tests/matern_ref.py) that the GPU tests lean on, and of
the host-side surface of the families: the beliefs key and the kernel class setup() picks.

The gp4ml gradient is held to central differences of the LLH (h = 1e-5 in 2 log hp) at 1e-6
of max |grad|: the two agree to about 1e-8 on these cases, which leaves two decades for the
step size.  The MUCM gradient is not the derivative of the MUCM LLH (the reference scales it
by sigma-hat^2, for the Gaussian kernel too), so it has no such check.
"""
import os
import shutil
import types

import numpy as np
import pytest

import matern_ref as mr
from gp_emu_uqsa_amd import api, files, kernels, native
from oracle import gp_oracle as orc

EX = os.path.join(os.path.dirname(__file__), "golden", "examples")


@pytest.mark.parametrize("variant", [orc.GP4ML, orc.MUCM])
@pytest.mark.parametrize("kind", [orc.STD, orc.ALT])
def test_gaussian_family_is_the_oracle(kind, variant):
    X, f, H = orc.synthetic_problem(200, 10, seed=9)
    hp = mr.hyperparams(10, variant, kind, True)
    ref = orc.objective_ref(X, f, H, hp, variant, kind, True)
    got = mr.objective(X, f, H, hp, variant, kind, True, "gaussian")
    assert abs(got[0] - ref[0]) <= 1e-8 * abs(ref[0])
    assert np.max(np.abs(got[1] - ref[1])) <= 1e-8 * np.max(np.abs(ref[1]))
    assert abs(got[2] - ref[2]) <= 1e-8 * abs(ref[2])


@pytest.mark.parametrize("family", ["matern32", "matern52"])
def test_rho_and_g_at_and_near_zero(family):
    """rho(0) = 1, g(0) = 3/2 or 5/6, no NaN; g is the derivative of rho: with every
    delta_k scaled alike, d rho / d(2 log delta) = sum_k g u_k^2 = g s = -s d rho / ds."""
    rho, g = mr.rho_g(np.array([0.0]), family)
    assert rho[0] == 1.0 and g[0] == (1.5 if family == "matern32" else 5.0 / 6.0)
    s = np.linspace(0.01, 30.0, 400)
    h = 1e-6
    drho = (mr.rho_g(s * (1 + h), family)[0] - mr.rho_g(s * (1 - h), family)[0]) / (2 * h)
    assert np.max(np.abs(-drho - mr.rho_g(s, family)[1] * s)) <= 1e-9


@pytest.mark.parametrize("n,d", [(129, 2), (300, 5)])
@pytest.mark.parametrize("kind", [orc.STD, orc.ALT])
@pytest.mark.parametrize("family", ["matern32", "matern52"])
def test_gp4ml_gradient_is_the_derivative(family, kind, n, d):
    X, f, H = orc.synthetic_problem(n, d, seed=9)
    hp = mr.hyperparams(d, orc.GP4ML, kind, True)
    _, grad, _ = mr.objective(X, f, H, hp, orc.GP4ML, kind, True, family)
    x = 2.0 * np.log(hp)
    h = 1e-5
    fd = np.empty_like(x)
    for i in range(x.size):
        e = np.zeros_like(x)
        e[i] = h
        up = mr.objective(X, f, H, np.exp((x + e) / 2.0), orc.GP4ML, kind, True, family, want_grad=False)[0]
        dn = mr.objective(X, f, H, np.exp((x - e) / 2.0), orc.GP4ML, kind, True, family, want_grad=False)[0]
        fd[i] = (up - dn) / (2.0 * h)
    err = np.max(np.abs(grad - fd)) / np.max(np.abs(grad))
    print(family, kind, n, d, "gradient against central differences", err)
    assert err <= 1e-6


@pytest.mark.parametrize("n,d", mr.SHAPES)
@pytest.mark.parametrize("family", ["matern32", "matern52"])
def test_gpu_cases_are_well_conditioned(family, n, d):
    """What the GPU tests assert of their inputs before they apply their tolerances."""
    X, _, _ = orc.synthetic_problem(n, d, seed=9)
    for kind in (orc.STD, orc.ALT):
        A, rho, _ = mr.kernel_var(X, mr.deltas(d), mr.NU[kind], kind, family)
        cond, med = np.linalg.cond(A), np.median(rho)
        print(family, n, d, kind, "cond", cond, "median rho", med)
        assert cond <= 1e6 and med >= 0.05


@pytest.fixture()
def toysim_dir(tmp_path, monkeypatch):
    d = tmp_path / "toy-sim"
    shutil.copytree(os.path.join(EX, "toy-sim"), d)
    monkeypatch.chdir(d)
    return d


def _fake_emulator(config):
    return types.SimpleNamespace(config=config, tv_conf=types.SimpleNamespace(no_of_trains=2),
                                 par=types.SimpleNamespace(beta=np.array([0.5, 2.8]), delta=np.array([0.2, 0.16]),
                                                           sigma=0.61, nugget=0.03),
                                 all_data=types.SimpleNamespace(input_minmax=[[0.01, 0.98], [0.013, 0.99]]))


def test_beliefs_kernel_key(toysim_dir):
    c = files.Config("toy-sim_config")
    b = files.Beliefs(c.beliefs)
    assert b.kernel == "gaussian"                       # absent: the reference's kernel
    b.final_beliefs(_fake_emulator(c), final=True)
    text = open("toy-sim_beliefs-2f").read()
    assert "kernel" not in text                         # files of gaussian emulators unchanged
    assert text.splitlines()[-1].startswith("input_minmax ")
    for fam in ("gaussian", "matern32", "matern52"):
        shutil.copy("toy-sim_beliefs", "b_" + fam)
        with open("b_" + fam, "a") as fh:
            fh.write("kernel " + fam + "\n")
        assert files.Beliefs("b_" + fam).kernel == fam
    b52 = files.Beliefs("b_matern52")
    b52.final_beliefs(_fake_emulator(c), final=True)
    lines = open("toy-sim_beliefs-2f").read().splitlines()
    assert lines[-1] == "kernel matern52"
    assert lines[:-1] == text.splitlines()              # nothing else moved
    assert files.Beliefs("toy-sim_beliefs-2f").kernel == "matern52"


def test_beliefs_bad_kernel_exits(toysim_dir, capsys):
    with open("toy-sim_beliefs", "a") as fh:
        fh.write("kernel matern72\n")
    with pytest.raises(SystemExit):
        files.Beliefs("toy-sim_beliefs")
    assert "kernel should be one of gaussian, matern32, matern52" in capsys.readouterr().out


def test_kernel_codes_compose():
    assert (kernels.kernel.kind, kernels.kernel_alt_nug.kind) == (0, 1)
    assert kernels.kernel_matern32.kind == native.KERNEL_MATERN32 == mr.FAMILY_CODE["matern32"]
    assert kernels.kernel_matern32_alt_nug.kind == native.KERNEL_MATERN32 | native.KERNEL_ALT_NUG
    assert kernels.kernel_matern52.kind == native.KERNEL_MATERN52 == mr.FAMILY_CODE["matern52"]
    assert kernels.kernel_matern52_alt_nug.kind == native.KERNEL_MATERN52 | native.KERNEL_ALT_NUG


@pytest.mark.parametrize("family,alt,cls", [
    (None, "F", kernels.kernel), (None, "T", kernels.kernel_alt_nug),
    ("gaussian", "F", kernels.kernel), ("gaussian", "T", kernels.kernel_alt_nug),
    ("matern32", "F", kernels.kernel_matern32), ("matern32", "T", kernels.kernel_matern32_alt_nug),
    ("matern52", "F", kernels.kernel_matern52), ("matern52", "T", kernels.kernel_matern52_alt_nug)])
def test_setup_picks_the_kernel_class(toysim_dir, monkeypatch, family, alt, cls):
    """setup() up to the kernel object: the posterior (the first GPU call) is stubbed out."""
    text = open("toy-sim_beliefs").read().replace("mucm T", "mucm F")
    text += "alt_nugget " + alt + "\n" + ("" if family is None else "kernel " + family + "\n")
    open("toy-sim_beliefs", "w").write(text)
    monkeypatch.setattr(api._model, "Posterior", lambda *a, **k: None)
    np.random.seed(0)
    E = api.setup("toy-sim_config")
    assert type(E.K) is cls
    assert E.K.family == (family or "gaussian")
    assert E.training.K is E.K and E.validation.K is E.K
