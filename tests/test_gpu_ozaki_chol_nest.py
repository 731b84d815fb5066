"""The split Cholesky's first phase split once more at q = h / 2: the trapezoid {rows [q, NB),
columns [q, h), column <= row} takes the update by the columns [0, q) as a second int8 product
(build_plan's nested split, chol_schur at q, OzCholNest).

Contexts: tests/test_gpu_ozaki_chol.py's floors plus GPEMU_OZAKI_CHOL_NEST_MIN=256 (the floor
gpe_create allows), beside the switch-off context (GPEMU_OZAKI_CHOL_NEST=0: the two-phase
sweep), a GPEMU_OZAKI=0 context (the fp64 sweep) and the oracle's objective_fast.  Shapes (tile
columns of 128; nti x cap the product's 256-tile rows and columns):

  n     NB  h   q   nti x cap
  1024   8   4   2  3 x 1   the smallest trapezoid
  1400  11   8   4  4 x 2   the last tile ragged, padding past n_pad
  2900  23  16   8  8 x 4
  1100   9   8   -  not split, so not nested: bit-equal to the switch-off context
  1600  13   8   4  5 x 2   the hard point that nests

Tolerances, cases and recipes are test_gpu_ozaki_chol.py's (imported, not restated): LLH within
1e-10 max(1, |LLH|) of the oracle, gradient within 1e-10 of scale of the fp64 context's and
1e-7 of the oracle's, sigma^2 within 1e-10 relative.  That the nesting ran is read off
gpe_ozaki_stats: one k_oz_gemm launch more than the split sweep's count.
"""
import threading

import numpy as np
import pytest

import test_gpu_ozaki_chol as tc
from gp_emu_uqsa_amd import native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

NEST = dict(tc.FLOORS, GPEMU_OZAKI_CHOL_NEST_MIN="256")

nest = tc._fixture(**NEST)                                   # gradient evaluations nest
off = tc._fixture(**NEST, GPEMU_OZAKI_CHOL_NEST="0")         # the switch: the two-phase sweep
parent = tc._fixture(**tc.FLOORS)                            # no variable: the default threshold, far above
fp64 = tc._fixture(GPEMU_OZAKI="0")
nestf = tc._fixture(**NEST, GPEMU_OZAKI_CHOL="3")            # and gpe_factor's sweep (L itself)


def _count(n, nested=True):
    """k_oz_gemm launches of one gradient objective: the LAUUM, the TRTRI pairs from 512 rows,
    S when the sweep splits, the trapezoid's product when it nests."""
    NB = (n + 127) // 128
    h = 1
    while 2 * h < NB:
        h *= 2
    splits = 128 * (NB - h) >= 256
    nests = splits and nested and h >= 4 and (h // 2) % 2 == 0
    return 1 + 2 * tc._pairs(NB, 4) + (1 if splits else 0) + (1 if nests else 0)


def _bytes(res):
    return (np.float64(res[0]).tobytes(), np.asarray(res[1], dtype=np.float64).tobytes(), np.float64(res[2]).tobytes())


@pytest.mark.parametrize("n,case", tc.SHAPES, ids=[f"{n}-{k}" for n, k in tc.SHAPES])
def test_nested_objective(nest, fp64, n, case):
    res = tc._grad(nest, n, case, count=_count(n))
    tc._against(n, case, res, tc._grad(fp64, n, case), "nested")


@pytest.mark.parametrize("n,case", [(1024, "gp4ml_fit"), (1400, "alt_r"), (2900, "mucm_fix")])
def test_switch_off_is_the_two_phase_sweep(off, parent, n, case):
    """GPEMU_OZAKI_CHOL_NEST=0 at the floors against a context without either variable (the
    default threshold leaves every size here un-nested): the same launches, the same bytes."""
    a = tc._grad(off, n, case, count=_count(n, nested=False))
    b = tc._grad(parent, n, case, count=_count(n, nested=False))
    assert _bytes(a) == _bytes(b), (a, b)


@pytest.mark.parametrize("case", ["gp4ml_fit", "mucm_fix"])
def test_unsplit_size_is_not_nested(nest, off, fp64, case):
    """n = 1100: S would have 128 rows, the sweep stays whole and so un-nested."""
    n = 1100
    a = tc._grad(nest, n, case, count=_count(n))
    b = tc._grad(off, n, case, count=_count(n))
    assert _count(n) == 1 + 2 * tc._pairs(9, 4)
    assert _bytes(a) == _bytes(b), (a, b)
    tc._against(n, case, a, tc._grad(fp64, n, case), "not nested")


def test_value_only_does_not_nest():
    """GPEMU_OZAKI_CHOL=2 splits the value-only evaluations too; they do not nest (one launch: S)
    and give the switch-off context's bytes, before and after a nested gradient evaluation."""
    n, case = 1400, "mucm_fix"
    variant, kind, _, _ = tc.CASES[case]
    X, f, H, r, hp, nu_fixed, _ = tc._problem(n, case)
    out = []
    for env in (dict(NEST, GPEMU_OZAKI_CHOL="2"), dict(NEST, GPEMU_OZAKI_CHOL="2", GPEMU_OZAKI_CHOL_NEST="0")):
        c = tc._context(**env)
        try:
            c.set_data(X, f, H, r)
            c.set_profiling(True)
            v1 = c.objective(variant, kind, hp, nu_fixed=nu_fixed, want_grad=False)
            assert c.ozaki_stats()["launches"] == 1
            c.set_profiling(False)
            tc._grad(c, n, case, count=_count(n, nested="GPEMU_OZAKI_CHOL_NEST" not in env))
            v2 = c.objective(variant, kind, hp, nu_fixed=nu_fixed, want_grad=False)
            assert v1[0] == v2[0] and v1[2] == v2[2]
            out.append((v1[0], v1[2]))
        finally:
            c.close()
    assert out[0] == out[1], out


def test_int8_ops_are_the_closed_forms(nest, off):
    """n = 2900 (NB 23, h 16, q 8, 16 moduli): the nested evaluation's int8 operations are the
    switch-off evaluation's (whose closed forms tests/test_gpu_ozaki_chol.py writes out) plus
    the trapezoid's: K = 128 q = 1024 over the 256-tiles of 8 tile rows capped at 4 columns,
    1 + 2 + 3 + 4 + 4 x 4 = 26 tiles.  Integers far below 2^53: the equality is exact."""
    n, N, T = 2900, 16, 256
    variant, kind, _, _ = tc.CASES["gp4ml_fit"]
    X, f, H, r, hp, nu_fixed, _ = tc._problem(n, "gp4ml_fit")
    stats = []
    for c in (off, nest):
        c.set_data(X, f, H, r)
        c.set_profiling(True)
        try:
            c.objective(variant, kind, hp, nu_fixed=nu_fixed)
            stats.append(c.ozaki_stats())
        finally:
            c.set_profiling(False)
    want = 2 * T * T * 1024 * 26 * N
    print(f"int8 ops off {stats[0]['int8_ops']:.0f} nested {stats[1]['int8_ops']:.0f} trapezoid {want}")
    assert stats[1]["launches"] == stats[0]["launches"] + 1 == _count(n)
    assert stats[1]["int8_ops"] - stats[0]["int8_ops"] == float(want)


@pytest.mark.parametrize("n", [1024, 1400])
def test_factor_of_nested_sweep(nestf, fp64, n):
    """L itself (test_gpu_ozaki_chol.py's docstring): gpe_factor through the nested sweep
    (GPEMU_OZAKI_CHOL=3), A^-1 B through gpe_solve, the residual no larger than 4 x the fp64
    context's own."""
    X, f, H, _, hp, _, _ = tc._problem(n, "gp4ml_fit")
    d = X.shape[1]
    delta, nu = hp[:d], hp[d]
    A, _ = orc.kernel_var_ref(X, delta, nu, orc.STD, True)
    B = np.random.RandomState(n).standard_normal((n, 4))

    def defect(c):
        c.set_data(X, f, H)
        c.factor(native.KERNEL_STD, delta, nu, 1.0, 0.0)
        Xs = c.solve(B)
        return float(np.max(np.abs(A @ Xs - B)) / (np.max(np.abs(A)) * np.max(np.abs(Xs)))), c.beta()

    e8, b8 = defect(nestf)
    e64, b64 = defect(fp64)
    print(f"factor n={n}: solve residual nested {e8:.3e} fp64 {e64:.3e}; beta diff {np.max(np.abs(b8 - b64)):.2e}")
    assert e8 <= 4.0 * e64, (e8, e64)
    assert np.max(np.abs(b8 - b64)) <= 1e-10 * (1.0 + np.max(np.abs(b64))), (b8, b64)


@pytest.mark.parametrize("name", tc._hard_names())
def test_hard_points_nested(nest, fp64, name):
    """tests/golden/ozaki_hard.npz at n = 1100 (not nested) and n = 1600 (NB 13, h 8, q 4), the
    rule of test_gpu_ozaki_tri.py::test_hard_points:
    E(int8, nested) <= 4 max(E(fp64 GPU), E(float64 CPU), n 2^-53)."""
    z = np.load(tc.GOLDEN)
    rc = {k: z[f"{name}/{k}"] for k in ("n", "d", "seed", "hp", "variant", "kernel", "fit_nugget", "r_seed",
                                        "nu_fixed")}
    n, d, variant, kind = int(rc["n"]), int(rc["d"]), int(rc["variant"]), int(rc["kernel"])
    hp, fitn, nu_fixed = rc["hp"], bool(rc["fit_nugget"]), float(rc["nu_fixed"])
    X, f, H = orc.synthetic_problem(n, d, seed=int(rc["seed"]))
    r = np.random.RandomState(int(rc["r_seed"])).uniform(1e-4, 1e-3, size=n) if int(rc["r_seed"]) >= 0 else None
    llh_ref, g_ref = float(z[f"{name}/llh_ref"]), z[f"{name}/grad_ref"]

    def E(res):
        return (float(np.max(np.abs(res[1] - g_ref) / tc._scale(g_ref))),
                abs(res[0] - llh_ref) / max(1.0, abs(llh_ref)))

    nest.set_data(X, f, H, r)
    fp64.set_data(X, f, H, r)
    nest.set_profiling(True)
    try:
        e8 = E(nest.objective(variant, kind, hp, nu_fixed=nu_fixed))
        assert nest.ozaki_stats()["launches"] == _count(n)
    finally:
        nest.set_profiling(False)
    e64 = E(fp64.objective(variant, kind, hp, nu_fixed=nu_fixed))
    ecpu = E(orc.objective_fast(X, f, H, hp, variant, kind, fitn, r=r, nu_fixed=nu_fixed))
    floor = n * 2.0 ** -53
    print(f"HARD {name} n={n} launches={_count(n)} grad E: int8 {e8[0]:.2e} fp64 {e64[0]:.2e} cpu {ecpu[0]:.2e} | "
          f"llh E: int8 {e8[1]:.2e} fp64 {e64[1]:.2e} cpu {ecpu[1]:.2e} | floor {floor:.2e}")
    assert e8[0] <= 4.0 * max(e64[0], ecpu[0], floor), (e8, e64, ecpu)
    assert e8[1] <= 4.0 * max(e64[1], ecpu[1], floor), (e8, e64, ecpu)


@pytest.mark.parametrize("bad", [100, 300, 800], ids=["first", "middle", "schur"])
def test_not_positive_definite(nest, off, fp64, bad):
    """test_gpu_ozaki_chol.py's construction at n = 1024 (q 128 = 256, h 128 = 512) with the
    failing pivot in the first sweep's columns, in the middle sweep's and in S: the switch-off
    context's decision each time, for gradient and value-only calls, twice in a row; a good
    matrix on the same context then gives the oracle's result."""
    X, f, H, r, hp = tc._non_pd_problem(bad)
    assert orc.objective_fast(X, f, H, hp, orc.GP4ML, orc.ALT, True, r=r) is None
    for c in (off, nest, nest):
        c.set_data(X, f, H, r)
        with pytest.raises(native.NotPositiveDefinite):
            c.objective(orc.GP4ML, orc.ALT, hp)
        with pytest.raises(native.NotPositiveDefinite):
            c.objective(orc.GP4ML, orc.ALT, hp, want_grad=False)
    tc._against(1024, "gp4ml_fit", tc._grad(nest, 1024, "gp4ml_fit", count=_count(1024)),
                tc._grad(fp64, 1024, "gp4ml_fit"), "after non-PD")


@pytest.mark.parametrize("n", [1024, 1400, 2900])
def test_same_bytes_every_time(nest, n):
    first = _bytes(tc._grad(nest, n, "gp4ml_fit"))
    for _ in range(4):
        assert _bytes(tc._grad(nest, n, "gp4ml_fit")) == first


def test_two_in_flight_give_their_solo_bytes():
    """Two nesting contexts, each on its own thread, evaluating at once at n = 1400 (each then
    takes the per-step launches of the three sweeps)."""
    n, cases = 1400, ("gp4ml_fit", "alt_r")
    ctxs = [tc._context(**NEST) for _ in cases]
    try:
        solo = [_bytes(tc._grad(c, n, case, count=_count(n))) for c, case in zip(ctxs, cases)]
        out, err = [None, None], []
        gate = threading.Barrier(2)

        def work(k):
            try:
                gate.wait()
                out[k] = [_bytes(tc._grad(ctxs[k], n, cases[k])) for _ in range(3)]
            except Exception as e:   # noqa: BLE001
                err.append(e)

        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not err, err
        for k in range(2):
            assert all(b == solo[k] for b in out[k])
    finally:
        for c in ctxs:
            c.close()
