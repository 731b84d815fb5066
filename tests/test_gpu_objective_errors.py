"""The objective's error paths as native.py raises them, on each of the four routes to a
result: k_tiny (n = 100), k_snb (n = 300), the general single-GPU path (n = 600) and the
row-block loopback (P = 2, n = 300); d = 3, linear basis.  Per route: the exception type and
message of a zero and a NaN length scale, an n_hp off by one in each direction, a bad variant
and a matrix that is not positive definite (the golden files' nonpd_hp recipe: length scales
200, no nugget), and after each failure a correct evaluation that returns the bytes of the one
made before it, so the context is left usable."""
import numpy as np
import pytest

from gp_emu_uqsa_amd import native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

D = 3
GOOD = np.array([0.6, 0.8, 1.1, 1e-2, 0.9])       # delta (3), nu, sigma: gp4ml, fitted nugget
ROUTES = [("tiny", 100), ("snb", 300), ("general", 600), ("rowblock", 300)]


def _with(k, v):
    hp = GOOD.copy()
    hp[k] = v
    return hp


# (id, variant, hp, exception, text the message contains)
FAILURES = [
    ("zero_delta1", native.GP4ML, _with(1, 0.0), native.NotPositiveDefinite, "delta[1] is zero or NaN"),
    ("nan_delta2", native.GP4ML, _with(2, np.nan), native.NotPositiveDefinite, "delta[2] is zero or NaN"),
    ("n_hp_short", native.GP4ML, GOOD[:3], RuntimeError, "n_hp inconsistent with d"),
    ("n_hp_long", native.GP4ML, np.append(GOOD, 1.0), RuntimeError, "n_hp inconsistent with d"),
    ("bad_variant", 7, GOOD, RuntimeError, "bad variant"),
    ("not_pd", native.GP4ML, np.array([200.0, 200.0, 200.0, 1.0]), native.NotPositiveDefinite, "pivot"),
]


@pytest.fixture(scope="module")
def rowblock():
    X, f, H = orc.synthetic_problem(300, D, seed=1)
    dc = native.DistContext(0, 2)
    dc.set_data(X, f, H)
    yield dc
    dc.close()


@pytest.mark.parametrize("route,n", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("failure", FAILURES, ids=[f[0] for f in FAILURES])
def test_failure_message_and_context_usable(ctx, rowblock, route, n, failure):
    _, variant, hp, exc, text = failure
    if route == "rowblock":
        c = rowblock
    else:
        c = ctx
        c.set_data(*orc.synthetic_problem(n, D, seed=1))
    before = c.objective(native.GP4ML, native.KERNEL_STD, GOOD, want_grad=True)
    with pytest.raises(exc) as info:
        c.objective(variant, native.KERNEL_STD, hp, nu_fixed=0.0, want_grad=True)
    assert text in str(info.value), str(info.value)
    if exc is RuntimeError:   # (NotPositiveDefinite is an ArithmeticError: not one of these)
        assert not isinstance(info.value, native.NotPositiveDefinite)
    after = c.objective(native.GP4ML, native.KERNEL_STD, GOOD, want_grad=True)
    assert after[0] == before[0] and after[2] == before[2], (before, after)
    assert np.array_equal(after[1], before[1]), (before[1], after[1])
    assert np.all(np.isfinite(after[1])) and np.isfinite(after[0])
