"""The single-GPU TRTRI on the int8 matrix cores (trtri_pair_ozaki, oz_l21_ahead, the plan
cache of oz_prepare) at small ragged shapes, and the int8 products at ill-conditioned
hyperparameters against an extended-precision reference.

Contexts: GPEMU_OZAKI_MIN_NP=512 and GPEMU_OZAKI_TRI_MIN=512 (the floors gpe_create allows),
so every TRTRI level whose blocks have at least 4 tile rows of 128 runs its two products on
the int8 path, beside a GPEMU_OZAKI=0 context (fp64 products) on the same data.

Which LLH assertion (z_from_factor, gpemu.hip): an objective with the gradient factors with
invert = true, so the augmented row is not carried (zaug_valid = false) and z = L^-1 [f H]
comes from the skinny product WITH X = L^-1 (linv_valid).  The LLH therefore reads X, and
with the TRTRI on the int8 path it need not be bit-equal to the fp64 context's: the ragged
tests assert the suite's 1e-10 max(1, |llh|) against the oracle, not ==.

test_hard_points: E = error against tests/golden/ozaki_hard.npz (long double, eps 1.1e-19),
gradient E(g) = max |g - g_ref| / (|g_ref| + max |g_ref|), LLH relative to max(1, |llh_ref|).
Asserted: E(int8) <= 4 max(E(fp64 GPU), E(float64 CPU objective_fast), n 2^-53); the floor is
the summation-order noise of a length-n float64 sum, the factor 4 the spread of float64-accurate
evaluations of the same rounded inputs (lost low bits would show as orders of magnitude).
Default-threshold sizes (n >= 6144) are out of this check's reach: one long-double case there
is about an hour of arithmetic.  Measured on an MI355X (floor 1.2e-13, 1.8e-13 at n = 1600);
every case meets the factor 4, the largest E(int8) / bound being 1.04 (gradient, nu = 1e-6):

  case                        gradient E: int8  fp64 GPU  CPU f64 | LLH E: int8  fp64 GPU  CPU f64
  gp4ml_std_d2_nu1e-4                  1.65e-12  1.65e-12  3.91e-12 |  1.10e-12  1.11e-12  4.95e-12
  gp4ml_std_d2_nu1e-6                  4.24e-10  2.23e-10  4.06e-10 |  2.33e-10  2.34e-10  3.18e-10
  gp4ml_std_d1_nu1e-4                  2.35e-11  1.58e-10  4.05e-10 |  7.74e-14  7.84e-14  6.17e-13
  gp4ml_alt_d2_nu1e-3_r                2.52e-12  6.69e-13  2.92e-12 |  3.57e-13  3.56e-13  2.41e-12
  mucm_std_d2_nu1e-4                   7.41e-13  1.09e-12  3.10e-12 |  4.74e-13  4.76e-13  1.89e-12
  mucm_std_d3_fixed1e-4                3.64e-12  2.94e-12  9.17e-12 |  6.06e-13  6.07e-13  1.10e-12
  gp4ml_std_d10_benign                 5.49e-16  1.37e-16  4.80e-16 |  1.80e-15  1.80e-15  0
  gp4ml_std_d2_nu1e-4_n1600            1.89e-12  1.76e-12  6.98e-12 |  1.30e-12  1.29e-12  4.40e-12
"""
import functools
import os

import numpy as np
import pytest

from gp_emu_uqsa_amd import native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ozaki_hard.npz")


def _context(**env):
    mp = pytest.MonkeyPatch()
    for k, v in env.items():
        mp.setenv(k, v)
    try:
        return native.Context(0)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def oz():
    c = _context(GPEMU_OZAKI_MIN_NP="512", GPEMU_OZAKI_TRI_MIN="512")
    yield c
    c.close()


@pytest.fixture(scope="module")
def fp64():
    c = _context(GPEMU_OZAKI="0")
    yield c
    c.close()


def _scale(g):
    return np.abs(g) + np.max(np.abs(g))


CASES = {   # (variant, kernel, fit nugget, r): those of test_gpu_ozaki.py
    "gp4ml_fit": (orc.GP4ML, orc.STD, True, False),
    "mucm_fix": (orc.MUCM, orc.STD, False, False),
    "alt_r": (orc.GP4ML, orc.ALT, True, True),
    "std_r": (orc.GP4ML, orc.STD, True, True),
}


@functools.lru_cache(maxsize=None)
def _problem(n, d, case):
    """Data, hyperparameters (test_gpu_ozaki.py's recipe) and the oracle's result, computed
    once per (n, d, case) and shared; nothing modifies them."""
    variant, kind, fitn, use_r = CASES[case]
    X, f, H = orc.synthetic_problem(n, d, seed=n + d)
    r = np.random.RandomState(n).uniform(1e-4, 1e-3, size=n) if use_r else None
    hp = list(np.linspace(0.5, 1.1, d))
    if fitn:
        hp.append(3e-2 if kind == orc.ALT else 1e-3)
    if variant == orc.GP4ML:
        hp.append(1.1)
    hp = np.array(hp)
    nu_fixed = 5e-3 if not fitn else 0.0
    ref = orc.objective_fast(X, f, H, hp, variant, kind, fitn, r=r, nu_fixed=nu_fixed)
    return X, f, H, r, hp, nu_fixed, ref


def _check(n, d, case, oz, fp64):
    """One gradient objective on both contexts: the int8 result within 1e-10 of scale of the
    fp64 path's and 1e-7 of the oracle's, the LLH within 1e-10 of the oracle's."""
    variant, kind, _, _ = CASES[case]
    X, f, H, r, hp, nu_fixed, ref = _problem(n, d, case)
    oz.set_data(X, f, H, r)
    fp64.set_data(X, f, H, r)
    llh, g, s2 = oz.objective(variant, kind, hp, nu_fixed=nu_fixed)
    llh64, g64, _ = fp64.objective(variant, kind, hp, nu_fixed=nu_fixed)
    err64 = np.max(np.abs(g - g64) / _scale(g64))
    err = np.max(np.abs(g - ref[1]) / _scale(ref[1]))
    print(f"n={n} d={d} {case}: grad vs fp64 {err64:.2e}, vs oracle {err:.2e}, "
          f"llh vs fp64 {abs(llh - llh64):.2e}, vs oracle {abs(llh - ref[0]):.2e}")
    assert err64 <= 1e-10, (err64, g, g64)
    assert err <= 1e-7, (err, g, ref[1])
    assert abs(llh - ref[0]) <= 1e-10 * max(1.0, abs(ref[0])), (llh, ref[0])
    assert abs(llh64 - ref[0]) <= 1e-10 * max(1.0, abs(ref[0])), (llh64, ref[0])
    assert abs(s2 - ref[2]) <= 1e-10 * abs(ref[2]), (s2, ref[2])
    return llh, g


def test_plan_follows_n_pad(fp64):
    """One context through n = 1100 -> 1200 -> 1600 -> 1100 (n_pad 1152, 1280, 1664, 1152: the
    first two share np2 = 1280, n_pad rounded to the 256-tiles).  The int8 plan cached for
    n_pad 1152 holds the top TRTRI pair (0, 8, 9); at n_pad 1280 the pair is (0, 8, 10): a
    cache keyed on np2 alone fails the second step with GPE_ERR_STATE ("TRTRI pair without an
    int8 plan").  Every step against the fp64 context and the oracle; the two n = 1100
    results agree with each other."""
    c = _context(GPEMU_OZAKI_MIN_NP="512", GPEMU_OZAKI_TRI_MIN="512")
    try:
        out = [_check(n, 3, "gp4ml_fit", c, fp64) for n in (1100, 1200, 1600, 1100)]
    finally:
        c.close()
    (llh_a, g_a), (llh_b, g_b) = out[0], out[3]
    assert np.max(np.abs(g_a - g_b) / _scale(g_a)) <= 1e-10, (g_a, g_b)
    assert abs(llh_a - llh_b) <= 1e-10 * max(1.0, abs(llh_a)), (llh_a, llh_b)


# n, d -> NB: the int8 pairs (t0, h, t1) by level
#   1100, 3 -> 9:  (0,4,8); (0,8,9)            Rb = 128 padded to Pb = 256 on the top level
#   1600, 5 -> 13: (0,4,8), (8,12,13); (0,8,13)   two pairs sharing the buffers, the second
#                                                 ragged; Rb = 640 -> Pb = 768
#   2900, 20 -> 23: (0,4,8), (8,12,16), (16,20,23); (0,8,16); (0,16,23)   three int8 levels,
#                   the first of them (whose first L21 is converted ahead on the second stream)
#                   not the top one
RAGGED = ([(1100, 3, k) for k in CASES] + [(1600, 5, k) for k in CASES] +
          [(2900, 20, "gp4ml_fit"), (2900, 20, "alt_r")])


@pytest.mark.parametrize("n,d,case", RAGGED, ids=[f"{n}-{d}-{k}" for n, d, k in RAGGED])
def test_ragged_int8_trtri(oz, fp64, n, d, case):
    _check(n, d, case, oz, fp64)


def _int8_pairs(NB, min_tiles=4):
    """Pairs of the TRTRI levels of span s (blocks of s / 2 tile rows) from min_tiles up."""
    pairs, s = 0, 2
    while s // 2 < NB:
        if s // 2 >= min_tiles:
            pairs += sum(1 for t0 in range(0, NB, s) if t0 + s // 2 < NB)
        s *= 2
    return pairs


@pytest.mark.parametrize("n,d,pairs", [(1100, 3, 2), (1600, 5, 3), (2900, 20, 5)])
def test_int8_trtri_launch_count(oz, n, d, pairs):
    """The shapes above do run their TRTRI pairs on the int8 path: one k_oz_gemm for the
    LAUUM and two per pair (gpe_ozaki_stats counts them with profiling on)."""
    assert _int8_pairs((n + 127) // 128) == pairs
    variant, kind, _, _ = CASES["gp4ml_fit"]
    X, f, H, r, hp, nu_fixed, ref = _problem(n, d, "gp4ml_fit")
    oz.set_data(X, f, H, r)
    oz.set_profiling(True)
    try:
        _, g, _ = oz.objective(variant, kind, hp, nu_fixed=nu_fixed)
        assert oz.ozaki_stats()["launches"] == 1 + 2 * pairs
    finally:
        oz.set_profiling(False)
    assert np.max(np.abs(g - ref[1]) / _scale(ref[1])) <= 1e-7


# ---------------------------------------------------------------- hard hyperparameter points
def _hard_names():
    return [str(s) for s in np.load(GOLDEN)["names"]]


@pytest.mark.parametrize("name", _hard_names())
def test_hard_points(oz, fp64, name):
    """See the module docstring: the bound and the measured table."""
    z = np.load(GOLDEN)
    rc = {k: z[f"{name}/{k}"] for k in ("n", "d", "seed", "hp", "variant", "kernel", "fit_nugget", "r_seed",
                                        "nu_fixed")}
    n, d, variant, kind = int(rc["n"]), int(rc["d"]), int(rc["variant"]), int(rc["kernel"])
    hp, fitn, nu_fixed = rc["hp"], bool(rc["fit_nugget"]), float(rc["nu_fixed"])
    X, f, H = orc.synthetic_problem(n, d, seed=int(rc["seed"]))
    r = np.random.RandomState(int(rc["r_seed"])).uniform(1e-4, 1e-3, size=n) if int(rc["r_seed"]) >= 0 else None
    llh_ref, g_ref = float(z[f"{name}/llh_ref"]), z[f"{name}/grad_ref"]

    def E(res):
        return (float(np.max(np.abs(res[1] - g_ref) / _scale(g_ref))),
                abs(res[0] - llh_ref) / max(1.0, abs(llh_ref)))

    oz.set_data(X, f, H, r)
    fp64.set_data(X, f, H, r)
    e8 = E(oz.objective(variant, kind, hp, nu_fixed=nu_fixed))
    e64 = E(fp64.objective(variant, kind, hp, nu_fixed=nu_fixed))
    ecpu = E(orc.objective_fast(X, f, H, hp, variant, kind, fitn, r=r, nu_fixed=nu_fixed))
    floor = n * 2.0 ** -53
    print(f"HARD {name} n={n} grad E: int8 {e8[0]:.2e} fp64 {e64[0]:.2e} cpu {ecpu[0]:.2e} | "
          f"llh E: int8 {e8[1]:.2e} fp64 {e64[1]:.2e} cpu {ecpu[1]:.2e} | floor {floor:.2e} "
          f"(fixture E_cpu {float(z[f'{name}/E_cpu_grad']):.2e} / {float(z[f'{name}/E_cpu_llh']):.2e})")
    assert e8[0] <= 4.0 * max(e64[0], ecpu[0], floor), (e8, e64, ecpu)
    assert e8[1] <= 4.0 * max(e64[1], ecpu[1], floor), (e8, e64, ecpu)
