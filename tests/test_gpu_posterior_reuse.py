"""One context taken through posterior calls of growing, shrinking and growing sizes, and
through every entry point that owns an ad-hoc GEMM descriptor slot, gives the bits of the
same single call on a fresh context: no workspace capacity goes stale and no descriptor slot
of one entry point is read by another.

n = 200, d = 3, linear basis, KERNEL_ALT_NUG with r.  Every comparison is np.array_equal:
each call's sums run in a fixed order that depends on its own sizes only."""
import numpy as np
import pytest

from gp_emu_uqsa_amd import native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

N, D = 200, 3
DELTA, NU, SIGMA = np.array([0.6, 0.8, 1.1]), 1e-2, 0.9
PC_PANEL = 128   # gpemu_pivchol.hpp: k = PC_PANEL + 8 crosses one panel boundary


def _fresh():
    X, f, H = orc.synthetic_problem(N, D, seed=11)
    r = np.random.RandomState(5).uniform(0.0, 0.02, N)
    ctx = native.Context(0)
    ctx.set_data(X, f, H, r)
    ctx.factor(native.KERNEL_ALT_NUG, DELTA, NU, 1.0, 1.0)
    return ctx


def _calls(beta):
    rs = np.random.RandomState(7)
    pts = {m: rs.uniform(size=(m, D)) for m in (130, 700, 300)}
    Hs = {m: orc.linear_basis(x) for m, x in pts.items()}
    r_new = rs.uniform(0.0, 0.02, 300)
    t, U = rs.normal(size=300), rs.normal(size=(4, 300))

    def full(m):
        return lambda c: c.posterior(pts[m], Hs[m], beta, SIGMA, full_var=True)

    def diag(m, precision):
        return lambda c: c.posterior(pts[m], Hs[m], beta, SIGMA, full_var=False, precision=precision)

    return [
        ("full m=130", full(130)),
        ("full m=700", full(700)),
        ("diag m=700 precision 64", diag(700, 64)),
        ("diag m=700 precision 32", diag(700, 32)),
        ("noise_sample m=300", lambda c: c.noise_sample(pts[300], Hs[300], beta, SIGMA, t, U, r_new, 1.0)),
        ("pivchol m=300", lambda c: c.posterior_pivchol(pts[300], Hs[300], beta, SIGMA, k=PC_PANEL + 8,
                                                        r_new=r_new, r_scale=1.0)[:4]),
        ("full m=130 again", full(130)),
    ]


def test_one_context_through_all_sizes_matches_fresh_contexts():
    shared = _fresh()
    try:
        calls = _calls(shared.beta())
        for name, call in calls:
            got = call(shared)
            fresh = _fresh()
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want)
            for i, (a, b) in enumerate(zip(got, want)):
                assert np.all(np.isfinite(a)), (name, i)
                assert np.array_equal(a, b), (name, i, float(np.max(np.abs(a - b))))
    finally:
        shared.close()
