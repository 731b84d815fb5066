"""CPU checks of the exact reference of the int8 products (tests/oz_product_ref.py): the limb
product against Fraction arithmetic, the restated constants against what oz_consts gives
(tests/host/oz_plan_check.cpp prints them), and that the comparator of the GPU tests
(tests/test_gpu_oz_product.py) does reject the two smallest errors it is there to catch."""
import re
from fractions import Fraction

import numpy as np

import oz_product_ref as ozr
from test_ozaki_host import plan_check   # noqa: F401  (fixture: the program's one run)


def _operand(rng, R, K, spread=60, scale=0):
    x = rng.standard_normal((R, K)) * np.exp2(rng.integers(-spread, 1, size=(R, K)).astype(float))
    return np.ldexp(x, scale)


def test_limb_product_equals_fraction_arithmetic():
    rng = np.random.default_rng(1)
    for (Ra, Rb, K, nmod) in ((3, 4, 5, 16), (2, 2, 64, 8), (5, 3, 7, 12)):
        ref = ozr.Ref(_operand(rng, Ra, K), _operand(rng, Rb, K, scale=37), K=64, nmod=nmod)
        assert np.max(np.abs(ref.Ai)) <= 2.0 ** ref.beta and np.max(np.abs(ref.Ai)) >= 2.0 ** (ref.beta - 1)
        for i in range(Ra):
            for j in range(Rb):
                want = sum(Fraction(float(ref.Ai[i, k])) * Fraction(float(ref.Bi[j, k])) for k in range(K))
                assert want.denominator == 1 and int(ref.Cint[i, j]) == want.numerator
    # operands at the limit |X'| = 2^53 and the int64 route
    A = np.array([[2.0 ** 53, -(2.0 ** 53), 2.0 ** 53 - 1.0], [1.0, -3.0, 2.0 ** 52 + 1.0]])
    for use_int64 in (False, True):
        C = ozr.exact_product(A, A, use_int64=use_int64)
        for i in range(2):
            for j in range(2):
                assert int(C[i, j]) == sum(int(A[i, k]) * int(A[j, k]) for k in range(3))
    B = np.rint(np.ldexp(rng.standard_normal((40, 300)), 52))
    assert (ozr.exact_product(B, B) == ozr.exact_product(B, B, use_int64=True)).all()


def test_exponents_and_markers():
    a = np.array([[0.0, 0.0, 0.0], [1.0, -3.0, 0.5], [np.nan, 1.0, 0.0], [np.inf, 0.0, 0.0], [5e-324, 0.0, 0.0]])
    ex = ozr.exponents(a, 53)
    assert ex.tolist() == [0, 52 - 1, ozr.EX_NAN, ozr.EX_NAN, 52 + 1074]
    Xi = ozr.int_operand(a, ex)
    assert Xi[1].tolist() == [2.0 ** 51, -3 * 2.0 ** 51, 2.0 ** 50] and not Xi[2].any() and Xi[4, 0] == 2.0 ** 52
    assert ozr.centred(np.array([126, 127, -127, 253 * 7 - 126], dtype=object), 253).tolist() == [126, -126, 126, -126]
    assert ozr.centred(np.array([128, -128, 127, 300], dtype=object), 256).tolist() == [-128, -128, 127, 44]


def test_constants_match_oz_consts(plan_check):   # noqa: F811
    out = plan_check.stdout
    assert tuple(int(v) for v in re.search(r"^mods=([\d,]+)$", out, flags=re.M).group(1).split(",")) == ozr.MODS
    betas = re.findall(r"^beta (\d+) (\d+) (\d+)$", out, flags=re.M)
    assert len(betas) == 11 * 15
    for nmod, K, beta in betas:
        assert ozr.consts(int(nmod), int(K))[0] == int(beta), (nmod, K)
    mds = re.findall(r"^Md (\d+) (\S+)$", out, flags=re.M)
    assert len(mds) == 11
    for nmod, md in mds:
        M = ozr.consts(int(nmod), 64)[1]
        assert abs(Fraction(float.fromhex(md)) / M - 1) == ozr.md_rel_error(int(nmod))
        # the share of the bound's 4 2^-53 that the derivation gives Md (oz_product_ref's docstring)
        assert ozr.md_rel_error(int(nmod)) <= Fraction(1, 1 << 52), nmod
    assert ozr.OZ_MAX_K == 131072 - 128 and 130560 <= ozr.OZ_MAX_K


def test_comparator_rejects_8_ulp_and_one_wrong_residue():
    rng = np.random.default_rng(2)
    for nmod in (16, 8):
        # (full-size entries: where |C'| is far below K 2^(2 beta) the bound's absolute term,
        # the accuracy an exact product of beta-bit operands has, is the larger one)
        a, b = _operand(rng, 6, 64, spread=0, scale=200), _operand(rng, 5, 64, spread=0, scale=-200)
        ref = ozr.Ref(a, b, K=64, nmod=nmod)
        good = ozr.expected(ref)
        bad, worst = ozr.compare(good, ref)
        assert not bad.any() and worst <= 0.25
        for ulps in (1, -1):              # (inside the bound: the kernel rounds three times)
            bad, _ = ozr.compare(good + ulps * np.spacing(good), ref)
            assert not bad.any()
        C = good.copy()
        i8, j8 = np.unravel_index(np.argmax(np.abs(good)), good.shape)
        C[i8, j8] += 8 * np.spacing(C[i8, j8])
        bad, worst = ozr.compare(C, ref)
        assert bad[i8, j8] and bad.sum() == 1 and worst > 1.0
        # one residue of modulus l off by one moves C' by a multiple of M / m_l (mod M)
        for l in (0, nmod - 1):
            C = good.copy()
            C[1, 2] += np.ldexp(float(ref.M // ozr.MODS[l]), -int(ref.ea[1] + ref.eb[2]))
            bad, _ = ozr.compare(C, ref)
            assert bad[1, 2] and bad.sum() == 1
        # the accumulate form: exact rational of product + old C, one more rounding allowed
        Cold = rng.standard_normal(good.shape) * np.abs(good).max()
        acc = np.array([[float(Fraction(float(-good[i, j])) + Fraction(float(Cold[i, j]))) for j in range(5)]
                        for i in range(6)])
        bad, _ = ozr.compare(acc, ref, alpha=-1.0, Cold=Cold)
        assert not bad.any()
        acc[0, 0] += 8 * np.spacing(max(abs(acc[0, 0]), abs(good[0, 0])))
        bad, _ = ozr.compare(acc, ref, alpha=-1.0, Cold=Cold)
        assert bad[0, 0] and bad.sum() == 1
        # a NaN where a number is due, and a number where a NaN is due
        C = good.copy()
        C[0, 0] = np.nan
        assert ozr.compare(C, ref)[0][0, 0]
    a[1, 5] = np.inf
    ref = ozr.Ref(a, b, K=64)
    good = ozr.expected(ref)
    assert np.isnan(good[1]).all() and not ozr.compare(good, ref)[0].any()
    good[1, 0] = 0.0
    assert ozr.compare(good, ref)[0][1, 0]
