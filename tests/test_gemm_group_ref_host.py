"""CPU checks of tests/gemm_group_ref.py: the module, not the kernel.  Its exactness claims,
its K-range rule against a brute-force mask, and that its comparator rejects planted errors."""
from fractions import Fraction

import numpy as np
import pytest

import gemm_group_ref as gr

T = gr.TILE


def test_sums_of_grid_products_are_exact_in_any_order():
    rng = np.random.default_rng(1)
    K = gr.K_MAX
    top = (1 << gr.GRID_BITS) - 1
    ja = rng.integers(-top, top + 1, size=(6, K))
    jb = rng.integers(-top, top + 1, size=(6, K))
    ja[0], jb[0] = top, top                       # the largest sum there is
    ja[1], jb[1] = top, -top
    ja[2, ::2], jb[2] = -top, top                 # cancelling halves
    for a, b in zip(ja, jb):
        exact = [int(x) * int(y) for x, y in zip(a, b)]
        assert abs(sum(exact)) < 1 << 51 and K * (1 << 40) < 1 << 63
        prod = (a * gr.UNIT) * (b * gr.UNIT)
        assert all(Fraction(float(p)) == Fraction(e, 1 << 40) for p, e in zip(prod[:64], exact[:64]))
        for seed in range(4):
            perm = np.random.default_rng(seed).permutation(K)
            run = np.cumsum(prod[perm])           # one addition after another, in this order
            want = np.cumsum(np.array(exact, dtype=np.int64)[perm])
            assert np.array_equal(run * 2.0 ** 40, want.astype(np.float64))
        # split K: shares summed apart, then the partials in index order
        for ks in (2, 3, 5, 8):
            ns = K // gr.GK
            cuts = [gr.GK * (q * ns // ks) for q in range(ks + 1)]
            parts = [np.cumsum(prod[c0:c1])[-1] if c1 > c0 else 0.0 for c0, c1 in zip(cuts, cuts[1:])]
            assert np.cumsum(parts)[-1] * 2.0 ** 40 == float(sum(exact))
    # the reference's own product
    S = (ja @ jb.T).astype(np.float64) * gr.UNIT * gr.UNIT
    assert np.array_equal(S, (ja * gr.UNIT) @ (jb.T * gr.UNIT))


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 0.0), (1.0, 0.5), (-1.0, 1.0), (2.0, -0.5), (-0.5, 0.25)])
def test_power_of_two_scaling_is_exact(alpha, beta):
    K = gr.K_MAX
    assert gr.exact_scaling(alpha, beta, K)
    rng = np.random.default_rng(2)
    s = rng.integers(-K * ((1 << 20) - 1) ** 2, K * ((1 << 20) - 1) ** 2, size=200, endpoint=True)
    c = rng.integers(-(1 << 30) + 1, 1 << 30, size=200)
    s[:2] = K * ((1 << 20) - 1) ** 2
    c[:2] = [(1 << 30) - 1, -(1 << 30) + 1]
    for sj, cj in zip(s, c):
        S, C0 = float(sj) * 2.0 ** -40, float(cj) * gr.UNIT
        want = Fraction(alpha) * Fraction(int(sj), 1 << 40) + Fraction(beta) * Fraction(int(cj), 1 << 20)
        assert Fraction(alpha * S + beta * C0) == want                    # the reference's order
        assert Fraction(alpha * ((beta / alpha) * C0 + S)) == want        # the kernel's order


def test_general_scaling_is_not_called_exact():
    assert not gr.exact_scaling(-0.7, 0.3, 512)
    assert not gr.exact_scaling(1.0, 0.3, 512)
    with pytest.raises(AssertionError):
        gr.exact_scaling(2.0 ** -30, 1.0, 512)     # the two grids are 2^50 apart


@pytest.mark.parametrize("flags", range(8))
@pytest.mark.parametrize("mul,off", [(1, 0), (2, 0), (2, 1), (3, 2)])
@pytest.mark.parametrize("mt,K", [(1, 16), (1, 128), (3, 384), (3, 272), (5, 640), (5, 400), (4, 1024)])
def test_k_range_against_a_mask(flags, mul, off, mt, K):
    """Element by element: k is in row m's range iff it is inside K, not before the diagonal
    tile of m's own row (G_KBEG_TI: the operand is zero left of it) and not past the diagonal
    tile of global row ti mul + off (G_KEND_TI: the triangle ends there)."""
    p = dict(mt=mt, nt=mt, K=K, flags=flags, kti_mul=mul, kti_off=off)
    k = np.arange(K + 300)
    for ti in range(mt):
        mask = k < K
        if flags & gr.G_KBEG_TI:
            mask &= k // T >= ti
        if flags & gr.G_KEND_TI:
            mask &= k // T <= ti * mul + off
        k0, k1 = gr.k_range(p, ti)
        inside = (k >= k0) & (k < k1)
        assert np.array_equal(mask, inside), (ti, k0, k1)
    covered = gr.tiles(p)
    assert len(set(covered)) == len(covered)
    assert set(covered) == {(i, j) for i in range(mt) for j in range(mt) if not (flags & gr.G_CLOWER) or j <= i}


def _group(kind, rng):
    lay = gr.Layout()
    probs = [gr.problem(lay, kind, 2, 2, 160, pad=2, gap=4, alpha=1.0, beta=0.5),
             gr.problem(lay, kind, 3, 3, 384, pad=6, gap=2, flags=gr.G_CLOWER | gr.G_KBEG_TI, alpha=-1.0),
             gr.problem(lay, kind, 2, 1, 256, flags=gr.G_KEND_TI, alpha=-0.7, beta=0.3)]
    return lay.lens, probs, gr.fill(lay.lens, probs, kind, rng)


@pytest.mark.parametrize("kind", range(4))
def test_comparator_accepts_the_reference_and_rejects_planted_errors(kind):
    lens, probs, bufs = _group(kind, np.random.default_rng(kind))
    ref = gr.expected(bufs, probs, kind)
    want, written, bound = ref
    assert gr.compare(want, bufs, probs, kind, ref) == 0.0
    # the result of fp64 arithmetic in another order is inside the bound, and not at zero
    p = probs[2]
    ic = gr.c_index(p, 1, 0)
    k0, k1 = gr.k_range(p, 1)
    A = bufs[p["a"][0]][gr.a_index(p, kind, 1, k0, k1)]
    B = bufs[p["b"][0]][gr.b_index(p, kind, 0, k0, k1)]
    acc = (p["beta"] / p["alpha"]) * bufs[p["c"][0]][ic]
    for k in range(k1 - k0):
        acc = acc + A[:, k:k + 1] * B[k:k + 1, :]
    got = [w.copy() for w in want]
    got[p["c"][0]][ic] = p["alpha"] * acc
    assert 0.0 < gr.compare(got, bufs, probs, kind, ref) < 1.0
    # one K stage dropped in one tile: every form of problem
    for drop in [(0, 1, 1), (1, 2, 1), (2, 1, 0), (2, 0, 0)]:
        wrong = gr.expected(bufs, probs, kind, drop_stage=drop)[0]
        with pytest.raises(AssertionError, match="problem %d tile \\(%d, %d\\)" % drop):
            gr.compare(wrong, bufs, probs, kind, ref)
    # one element changed outside the written set: a gap, an operand, an upper tile under G_CLOWER
    upper = gr.c_index(dict(probs[1], flags=0), 0, 2)[5, 7]
    assert not written[probs[1]["c"][0]][upper]
    for buf, idx in [(0, 1), (probs[0]["a"][0], probs[0]["a"][1] + 9), (probs[1]["c"][0], upper),
                     (2, lens[2] - 1)]:
        got = [w.copy() for w in want]
        got[buf][idx] = 0.0 if got[buf][idx] != 0.0 else 1.0
        with pytest.raises(AssertionError, match="buffer %d element %d changed" % (buf, idx)):
            gr.compare(got, bufs, probs, kind, ref)
    # a sentinel replaced by a NaN of another payload is a change too
    got = [w.copy() for w in want]
    got[0][0] = np.nan
    with pytest.raises(AssertionError, match="changed"):
        gr.compare(got, bufs, probs, kind, ref)
    # ti and tj swapped: tiles (0, 1) and (1, 0) of the square problem trade places
    got = [w.copy() for w in want]
    i01, i10 = gr.c_index(probs[0], 0, 1), gr.c_index(probs[0], 1, 0)
    got[2][i01], got[2][i10] = want[2][i10], want[2][i01]
    with pytest.raises(AssertionError, match="problem 0 tile"):
        gr.compare(got, bufs, probs, kind, ref)
    # a NaN or an infinity in a written tile
    got = [w.copy() for w in want]
    got[2][gr.c_index(probs[2], 0, 0)[3, 3]] = np.nan
    with pytest.raises(AssertionError, match="problem 2 tile \\(0, 0\\) entry \\(3, 3\\)"):
        gr.compare(got, bufs, probs, kind, ref)


def test_fill_and_footprint():
    lens, probs, bufs = _group(2, np.random.default_rng(7))
    opnd, cin, wr = gr.footprint(lens, probs, 2)
    for i, b in enumerate(bufs):
        rest = ~(opnd[i] | wr[i])
        assert np.all(b[rest] == gr.sentinel(i)) and rest.any()
        assert np.all(np.isnan(b[wr[i] & ~cin[i]]))
        assert np.all(np.abs(b[opnd[i]]) < 1.0) and np.all(np.abs(b[cin[i]]) < 2.0 ** 10)
    # under G_KBEG_TI the operand left of the diagonal tile is never read; upper C tiles stay
    p = probs[1]
    assert not opnd[p["a"][0]][gr.a_index(p, 2, 2, 0, 2 * T)].any()
    assert opnd[p["a"][0]][gr.a_index(p, 2, 2, 2 * T, 3 * T)].all()
    assert not wr[p["c"][0]][gr.c_index(p, 0, 1)].any()
    poisoned = gr.fill(lens, probs, 2, np.random.default_rng(7), poison=True)
    assert all(np.all(np.isnan(b[~(o | c)])) for b, o, c in zip(poisoned, opnd, cin))
    gr.expected(poisoned, probs, 2)               # reads nothing that is NaN
    # what the hook leaves to the test
    twice = [probs[0], dict(probs[0])]
    with pytest.raises(AssertionError, match="written twice"):
        gr.footprint(lens, twice, 2)
    alias = [dict(probs[0], c=probs[0]["a"])]
    with pytest.raises(AssertionError):
        gr.footprint(lens, alias, 2)
    with pytest.raises(AssertionError, match="leaves its buffer"):
        gr.footprint([n - 4 for n in lens], probs, 2)
