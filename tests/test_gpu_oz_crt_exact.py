"""k_oz_crt (gpemu_ozaki.hpp) bit for bit: the reconstruction's arithmetic is stated -- per entry,
with c_l the centred residue of the exact C' modulo m_l (the low byte for 256),

    shi = fma(c_l, rhi_l, shi),  slo = fma(c_l, rlo_l, slo)    for l = 0 .. N - 1 in that order,
    v   = (shi - rint(shi)) + slo,
    s   = ldexp(alpha Md, -(e_i + e_j)),
    C   = v s,  or  fma(v, s, C)  in accumulate mode;  NaN where e_i or e_j is EX_NAN

-- so a model of it in exact rationals, each operation rounded once to fp64, says which fp64
number every entry is.  One product per case through gpe_test_oz_product; at least 2048
entries of it (the edges and corners of the written region, the rest drawn at random) must
equal the model's bit for bit, and every other entry stays within the bound of
tests/oz_product_ref.py's compare.  The bound alone cannot tell a reordered slo chain or a
contracted final sum from the stated one; the model can.

An exact zero is compared as a value: the model's rationals carry no sign of zero.
"""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import oz_product_ref as ozr

pytestmark = pytest.mark.gpu

SENT = -1.2345678e300   # what C holds where nothing may be written
NSAMPLE = 2048


@functools.lru_cache(maxsize=None)
def crt_consts(nmod):
    """oz_consts' (rhi, rlo, Md): y / m = rhi + rlo with rhi on the 2^-41 grid, and the fp64
    product of the moduli in order."""
    mods = ozr.MODS[:nmod]
    rhi, rlo, Md = [], [], 1.0
    for m in mods:
        Md *= float(m)
    for l, m in enumerate(mods):
        Mm = 1
        for j, mj in enumerate(mods):
            if j != l:
                Mm = (Mm * (mj % m)) % m
        y = pow(Mm, -1, m)
        Q, R = divmod(y << 41, m)
        rhi.append(math.ldexp(float(Q), -41))
        rlo.append(math.ldexp(float(R) / float(m), -41))
    return rhi, rlo, Md


def rnd(fr):
    """A rational rounded to the nearest fp64, ties to even (CPython's integer true division)."""
    return fr.numerator / fr.denominator


def model(Cint, ei, ej, alpha, nmod, cold=None):
    """The fp64 number k_oz_crt's stated arithmetic gives for one entry."""
    if ei == ozr.EX_NAN or ej == ozr.EX_NAN:
        return math.nan
    rhi, rlo, Md = crt_consts(nmod)
    shi = slo = 0.0
    for l in range(nmod):
        m = ozr.MODS[l]
        c = int(Cint) % m
        c = c - m if c >= (m + 1) // 2 else c
        shi = rnd(Fraction(c) * Fraction(rhi[l]) + Fraction(shi))
        slo = rnd(Fraction(c) * Fraction(rlo[l]) + Fraction(slo))
    frac = rnd(Fraction(shi) - Fraction(float(np.rint(shi))))
    v = rnd(Fraction(frac) + Fraction(slo))
    s = math.ldexp(alpha * Md, -(int(ei) + int(ej)))
    assert math.isfinite(s) and s != 0.0
    return rnd(Fraction(v) * Fraction(s) + (Fraction(cold) if cold is not None else 0))


def rough(rng, R, Kv, spread=70):
    """Mixed signs, rows scaled by 2^+-200, entries spread over 2^-spread inside a row."""
    x = rng.standard_normal((R, Kv)) * np.exp2(-rng.integers(0, spread + 1, size=(R, Kv)).astype(float))
    x[rng.random((R, Kv)) < 0.05] = 0.0
    return np.ldexp(x, rng.integers(-200, 201, size=(R, 1)).astype(np.int32))


def desc(op):
    """op (R x Kv) stored row by row (trans 0)."""
    return dict(src=np.ascontiguousarray(op).ravel(), ld=op.shape[1], R=op.shape[0], Kv=op.shape[1])


def written(rows, cols, ti0, tri, lower128):
    gi, j = (np.arange(rows - 256 * ti0) + 256 * ti0)[:, None], np.arange(cols)[None, :]
    ok = np.ones((rows - 256 * ti0, cols), bool)
    if tri:
        ok &= (j >> 8) <= (gi >> 8)
    if lower128:
        ok &= (j >> 7) <= (gi >> 7)
    return ok


def sample(rng, w):
    """At least NSAMPLE written entries: the first and last written entry of every 37th row and
    column and of the first and last ones (edges, corners, the tile and lower128 borders), the
    rest at random."""
    pick = np.zeros(w.shape, bool)
    lr, cols = w.shape
    for i in sorted(set(range(0, lr, 37)) | {0, lr - 1, min(127, lr - 1), min(128, lr - 1), min(255, lr - 1), min(256, lr - 1)}):
        js = np.nonzero(w[i])[0]
        if js.size:
            pick[i, [js[0], js[-1]]] = True
    for j in sorted(set(range(0, cols, 37)) | {0, cols - 1, min(127, cols - 1), min(128, cols - 1), min(255, cols - 1)}):
        rs = np.nonzero(w[:, j])[0]
        if rs.size:
            pick[[rs[0], rs[-1]], j] = True
    rest = np.flatnonzero(w & ~pick)
    need = max(0, NSAMPLE - int(pick.sum()))
    assert rest.size >= need
    pick.ravel()[rng.choice(rest, size=need, replace=False)] = True
    return pick


def run_case(ctx, what, a, b, *, rows, cols, K, nmod=16, ti0=0, tri=False, lower128=False, alpha=1.0, acc=False, seed=0):
    rng = np.random.default_rng(seed)
    ref = ozr.Ref(a, b, K=K, nmod=nmod).rows_from(256 * ti0)
    lr = rows - 256 * ti0
    w = written(rows, cols, ti0, tri, lower128)
    ldc, cc = lr + 5, cols + 3
    C0 = np.full((cc, ldc), SENT)
    cold = None
    if acc:
        exp = ozr.expected(ref, alpha)[:lr, :cols]
        cold = np.where(np.isfinite(exp), exp, 1.0) * rng.standard_normal((lr, cols)) * np.exp2(rng.integers(-5, 6, size=(lr, cols)))
        cold[rng.random((lr, cols)) < 0.1] = 0.0
        C0[:cols, :lr] = cold.T
    out = ctx.test_oz_product(desc(a), None if b is None else desc(b), C=C0.ravel(), ldc=ldc, rows=rows, cols=cols, ti0=ti0,
                              K=K, tri=tri, lower128=lower128, alpha=alpha, acc=acc, nmod=nmod)
    C = out["C"].reshape(cc, ldc).T
    keep = C0.T
    full = np.zeros(C.shape, bool)
    full[:lr, :cols] = w
    assert np.array_equal(C[~full].view(np.uint64), keep[~full].view(np.uint64)), what + ": written outside the product"
    pick = sample(rng, w)
    assert pick.sum() >= NSAMPLE
    wrong = []
    for i, j in zip(*np.nonzero(pick)):
        want = model(ref.Cint[i, j], ref.ea[i], ref.eb[j], alpha, nmod, None if cold is None else float(cold[i, j]))
        got = float(C[i, j])
        same = math.isnan(got) if math.isnan(want) else (got == 0.0 if want == 0.0 else
                                                           np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64))
        if not same:
            wrong.append((int(i), int(j), got.hex(), want.hex()))
    print("%s: %d entries bit for bit, %d differ" % (what, int(pick.sum()), len(wrong)))
    assert not wrong, "%s: %d of %d sampled entries are not the model's, first (i, j, got, model) %s" % (
        what, len(wrong), int(pick.sum()), wrong[:4])
    bad, worst = ozr.compare(C[:lr, :cols], ref, alpha=alpha, Cold=cold, where=w & ~pick)
    assert not bad.any(), what + ": " + ozr.describe(bad, C[:lr, :cols], ref, alpha)


@pytest.mark.parametrize("nmod", [16, 12, 8])
@pytest.mark.parametrize("acc", [0, 1])
def test_one_tile(ctx, nmod, acc):
    """One 256 x 256 tile, K = 128: the compile-time instance (16 moduli) and the generic one."""
    rng = np.random.default_rng(200 + nmod)
    a, b = rough(rng, 256, 128), rough(rng, 256, 128)
    run_case(ctx, "one tile nmod %d acc %d" % (nmod, acc), a, b, rows=256, cols=256, K=128, nmod=nmod, acc=bool(acc), seed=nmod)


@pytest.mark.parametrize("nmod,acc", [(16, 0), (16, 1), (12, 0)])
def test_ragged_rectangle_with_nan_rows(ctx, nmod, acc):
    """300 x 260 of 2 x 2 tiles: threads past rows / cols, the exponent loads at the ragged column
    edge, and a non-finite row of each operand (NaN rows and columns of C)."""
    rng = np.random.default_rng(210 + nmod)
    a, b = rough(rng, 300, 128), rough(rng, 260, 120)
    a[17, 5] = np.nan
    b[258, 0] = np.inf
    run_case(ctx, "300 x 260 nmod %d acc %d" % (nmod, acc), a, b, rows=300, cols=260, K=128, nmod=nmod, acc=bool(acc), seed=3)


@pytest.mark.parametrize("acc,alpha", [(0, 1.0), (1, -1.0)])
def test_triangle_lower128(ctx, acc, alpha):
    """tri and lower128 over 2 tile rows of A A^T (the Schur update's call with acc and alpha -1)."""
    a = rough(np.random.default_rng(220), 500, 128)
    run_case(ctx, "tri lower128 acc %d" % acc, a, None, rows=500, cols=500, K=128, tri=True, lower128=True, alpha=alpha,
             acc=bool(acc), seed=4)


@pytest.mark.parametrize("nmod", [16, 8])
def test_triangle_from_tile_row_1(ctx, nmod):
    """ti0 = 1: the tile decoding counts from tile (1, 0) and C's row 0 is product row 256."""
    a = rough(np.random.default_rng(230), 700, 64)
    run_case(ctx, "tri ti0 1 nmod %d" % nmod, a, None, rows=700, cols=700, K=64, nmod=nmod, ti0=1, tri=True, seed=5)
