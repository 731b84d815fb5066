"""The operand conversion of the int8 products (gpemu_ozaki.hpp: k_oz_rowexp / k_oz_colexp, then
k_oz_split_rect<false>, k_oz_split_rect<true> or k_oz_split) against exact integers, one operand
at a time through gpe_test_oz_planes: the production oz_operand / oz_operand_packed on buffers
of the hook's own, which returns the exponents and the int8 planes of every modulus.

What the planes must be (the results contract of the conversion): every byte the int8 value of
a representative of rint(x 2^e) modulo m_l -- for odd m_l the centred one, |r| <= (m_l - 1) / 2,
which oz_residues promises -- and exactly 0 where the entry is masked, padded (rows past R, k
past Kv) or in a row whose exponent is EX_NAN.  The hook fills the planes with 0x55 first, so a
byte no thread wrote fails the congruence.  The reference is tests/oz_product_ref.py's
exponents / int_operand / masked in exact Python integers (int64: |x 2^e| <= 2^53).

Shapes: the smallest that reach every path of the three kernels -- threads of
k_oz_split_rect<false> whose 8 k are all kept, all dropped and astride the mask's diagonal;
64 x 64 blocks of k_oz_split_rect<true> wholly dropped, ragged in rows and in k; a source off
the 16-byte grid (the scalar loads), which must give the aligned run's bytes; the packed form
with np < np2.  Every operand has a NaN row, an infinite row, a zero row and a row whose
largest entries are +-(2^53 - 1) 2^-e beside entries that round to 0.  Everything the contract
says is never read is NaN in the source.
"""
import numpy as np
import pytest

import oz_product_ref as ozr

pytestmark = pytest.mark.gpu

ROW_NAN, ROW_INF, ROW_ZERO, ROW_FULL = 3, 5, 6, 9


def operand(rng, R, Kv):
    """R x Kv with rows scaled by 2^+-200, entries spread over 2^-70 inside a row, and the four
    special rows; their special entries sit on and beside the diagonal, where either mask keeps
    at least one."""
    x = rng.standard_normal((R, Kv)) * np.exp2(-rng.integers(0, 71, size=(R, Kv)).astype(float))
    x[rng.random((R, Kv)) < 0.05] = 0.0
    x = np.ldexp(x, rng.integers(-200, 201, size=(R, 1)).astype(np.int32))
    x[ROW_NAN, ROW_NAN] = np.nan
    x[ROW_INF, ROW_INF] = -np.inf
    x[ROW_ZERO] = 0.0
    big = (2.0 ** 53 - 1.0) * 2.0 ** -17
    x[ROW_FULL] = np.where(rng.random(Kv) < 0.5, 1.0, -1.0) * 2.0 ** -19   # (2^-19 2^17 = 1/4: rounds to 0)
    x[ROW_FULL, ROW_FULL - 1:ROW_FULL + 2] = [-big, big, -big]
    return x


def store(op, trans, mask, offset=0, pad=2):
    """The source holding the kept entries of op: op(r, k) at offset + k + r ld (trans 0) or
    offset + r + k ld (trans 1), ld the inner extent + pad; NaN wherever the contract says the
    kernels do not read (dropped entries, the gap between columns, before offset)."""
    R, Kv = op.shape
    r, k = np.arange(R)[:, None], np.arange(Kv)[None, :]
    keep = k >= r if mask == 1 else (k <= r if mask == 2 else np.ones((R, Kv), bool))
    vis = np.where(keep, op, np.nan)
    inner, outer = (R, Kv) if trans else (Kv, R)
    ld = inner + pad
    src = np.full(offset + outer * ld + 3, np.nan)
    src[offset:offset + outer * ld].reshape(outer, ld)[:, :inner] = vis.T if trans else vis
    return dict(src=src, ld=ld, offset=offset, trans=int(trans), R=R, Kv=Kv, mask=mask)


def check(what, out, op, mask, K, nmod):
    """Exponents and planes of one run against the exact integers of the masked operand."""
    R, Kv = op.shape
    P = ozr.pad(R)
    beta = ozr.consts(nmod, K)[0]
    dense = ozr.masked(op, mask)
    ex = ozr.exponents(dense, beta)
    want_ex = np.zeros(P, dtype=np.int64)
    want_ex[:R] = ex
    assert out["ex"].shape == (P,) and np.array_equal(out["ex"], want_ex), "%s: exponents differ at rows %s" % (
        what, np.nonzero(out["ex"] != want_ex)[0][:8])
    assert ex[ROW_NAN] == ozr.EX_NAN and ex[ROW_INF] == ozr.EX_NAN and ex[ROW_ZERO] == 0
    Xi = np.zeros((P, K), dtype=np.int64)
    Xi[:R, :Kv] = ozr.int_operand(np.where(np.isfinite(dense), dense, 0.0), ex).astype(np.int64)
    # (16 moduli: beta = 53, the row's largest is 2^53 - 1 itself; fewer bits round it to 2^beta)
    assert np.abs(Xi[ROW_FULL]).max() == (2 ** 53 - 1 if beta == 53 else 2 ** beta)
    assert 1 <= (np.abs(Xi[ROW_FULL]) > 0).sum() <= 3
    r, k = np.arange(P)[:, None], np.arange(K)[None, :]
    zero = (r >= R) | (k >= Kv) | (want_ex == ozr.EX_NAN)[:, None]
    zero |= (k < r) if mask == 1 else ((k > r) if mask == 2 else False)
    planes = out["planes"]
    assert planes.shape == (nmod, P, K) and planes.dtype == np.int8
    for l in range(nmod):
        m = ozr.MODS[l]
        got = planes[l].astype(np.int64)
        wrong = (got - Xi) % m != 0
        assert not wrong.any(), "%s: modulus %d (%d): %d bytes not congruent, first (row, k, got, x) %s" % (
            what, l, m, wrong.sum(), [(int(i), int(j), int(got[i, j]), int(Xi[i, j])) for i, j in
                                      list(zip(*np.nonzero(wrong)))[:5]])
        assert not got[zero].any(), "%s: modulus %d (%d): nonzero where masked, padded or non-finite at %s" % (
            what, l, m, list(zip(*np.nonzero(zero & (got != 0))))[:5])
        if m & 1:
            assert np.abs(got).max() <= (m - 1) // 2, "%s: modulus %d (%d): |r| up to %d" % (what, l, m, np.abs(got).max())


# R = 70, Kv = 100 in P = 256 rows of Kp = 128: row r's threads of 8 k are kept, dropped or astride
# the diagonal k = r; rows past R and the threads past Kv write zeros
@pytest.mark.parametrize("mask,nmod", [(0, 16), (1, 16), (2, 16), (1, 8), (2, 12)])
def test_rows_along_k(ctx, mask, nmod):
    op = operand(np.random.default_rng(10 + mask), 70, 100)
    out = ctx.test_oz_planes(store(op, 0, mask), K=128, nmod=nmod)
    check("trans 0 mask %d nmod %d" % (mask, nmod), out, op, mask, 128, nmod)


# R = 130, Kv = 72 in P = 256, Kp = 128: blocks of 64 rows x 64 k; block (2, .) ragged in rows,
# (., 1) ragged in k, (3, .) past R, and under mask 2 block (0, 1) wholly dropped (k >= 64 > r)
@pytest.mark.parametrize("mask,nmod", [(0, 16), (2, 16), (2, 8), (0, 12)])
def test_rows_across_k(ctx, mask, nmod):
    op = operand(np.random.default_rng(20 + mask), 130, 72)
    out = ctx.test_oz_planes(store(op, 1, mask), K=128, nmod=nmod)
    check("trans 1 mask %d nmod %d" % (mask, nmod), out, op, mask, 128, nmod)


# mask 1 across k (the TRTRI's other side): blocks below the diagonal wholly dropped
def test_rows_across_k_upper(ctx):
    op = operand(np.random.default_rng(23), 130, 72)
    out = ctx.test_oz_planes(store(op, 1, 1), K=128, nmod=16)
    check("trans 1 mask 1", out, op, 1, 128, 16)


@pytest.mark.parametrize("trans,mask", [(0, 1), (1, 2)])
def test_source_off_the_16_byte_grid(ctx, trans, mask):
    """An odd element offset and an odd ld: the scalar load paths.  The bytes are the aligned run's."""
    R, Kv = (70, 100) if not trans else (130, 72)
    op = operand(np.random.default_rng(30 + trans), R, Kv)
    even = ctx.test_oz_planes(store(op, trans, mask), K=128, nmod=16)
    odd = ctx.test_oz_planes(store(op, trans, mask, offset=1, pad=3), K=128, nmod=16)
    check("offset 1, trans %d" % trans, odd, op, mask, 128, 16)
    assert np.array_equal(odd["ex"], even["ex"]) and np.array_equal(odd["planes"], even["planes"])


@pytest.mark.parametrize("nmod", [16, 12, 8])
def test_packed(ctx, nmod):
    """X 384 x 384 lower-triangular in np2 = 512 through k_oz_colexp / k_oz_split: operand row j is
    column j of X (k >= j kept); columns and rows past 384 are padding."""
    R = 384
    op = operand(np.random.default_rng(40), R, R)   # op(j, k) = X[k, j]
    out = ctx.test_oz_planes(store(op, 0, 1), packed=True, nmod=nmod)
    check("packed nmod %d" % nmod, out, op, 1, 512, nmod)
