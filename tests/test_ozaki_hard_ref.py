"""The extended-precision reference of the hard hyperparameter points
(tests/golden/make_ozaki_hard.py, tests/golden/ozaki_hard.npz) tied to the oracle: its
long-double objective, run on every recipe shrunk to n = 256, against objective_ref (the
op-for-op restatement of the reference project) and objective_fast, to the suite's 1e-7 of
scale (the float64 evaluations' own error at these points is <= 1.1e-9: a margin of ~100),
and the committed fixture holds every case with finite values."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import gp_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ozaki_hard", os.path.join(GOLDEN, "make_ozaki_hard.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

needs_ld = pytest.mark.skipif(np.finfo(np.longdouble).eps >= 1e-18,
                              reason="np.longdouble is 64-bit here: no extended-precision reference")


@needs_ld
@pytest.mark.parametrize("case", gen.CASES, ids=[c[0] for c in gen.CASES])
def test_longdouble_objective_matches_oracles(case):
    rc = gen.recipe(case, n=256)
    X, f, H, r = gen.problem(rc)
    args = (X, f, H, rc["hp"], rc["variant"], rc["kernel"], rc["fit_nugget"])
    llh, grad, sig2, _ = gen.objective_ld(*args, r=r, nu_fixed=rc["nu_fixed"])
    llh, grad, sig2 = float(llh), np.asarray(grad, np.float64), float(sig2)
    for name, fn in (("objective_ref", orc.objective_ref), ("objective_fast", orc.objective_fast)):
        ref = fn(*args, r=r, nu_fixed=rc["nu_fixed"])
        assert ref is not None, name
        e_l, e_g = gen.llh_err(ref[0], llh), gen.grad_err(ref[1], grad)
        print(f"{rc['name']} n=256 {name}: E llh {e_l:.2e} grad {e_g:.2e}")
        assert e_l <= 1e-7, (name, ref[0], llh)
        assert e_g <= 1e-7, (name, ref[1], grad)
        assert abs(ref[2] - sig2) <= 1e-7 * abs(sig2), (name, ref[2], sig2)


def test_fixture_holds_every_case():
    z = np.load(os.path.join(GOLDEN, "ozaki_hard.npz"))
    assert list(z["names"]) == [c[0] for c in gen.CASES]
    for case in gen.CASES:
        rc = gen.recipe(case)
        name = rc["name"]
        for k, v in rc.items():
            if k != "name":
                assert np.array_equal(z[f"{name}/{k}"], np.asarray(v)), (name, k)
        g = z[f"{name}/grad_ref"]
        assert g.shape == rc["hp"].shape and g.dtype == np.float64 and np.all(np.isfinite(g))
        for k in ("llh_ref", "E_cpu_grad", "E_cpu_llh", "diag_ratio2"):
            assert np.isfinite(z[f"{name}/{k}"]), (name, k)
        if rc["hard"]:
            assert z[f"{name}/diag_ratio2"] >= 1e3
        assert z[f"{name}/E_cpu_grad"] < 1e-7 and z[f"{name}/E_cpu_llh"] < 1e-7
