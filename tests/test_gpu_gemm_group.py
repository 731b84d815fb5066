"""The grouped fp64 GEMM (k_gemm, csrc/gpemu_kernels.hpp) launch by launch against exact sums:
one launch at a time through gpe_test_gemm_group -- mkprob, split_k, add_launch (push_prob,
order_tiles, the CDEF choice) and launch_gemm_range (launch_k_gemm), the launch layer of
csrc/gpemu_gemm_sched.hpp that the row-block path shares, on buffers of the hook's own -- compared with
tests/gemm_group_ref.py.  Operands lie on a grid where every partial sum is exact in fp64, so
the comparison is bit for bit (np.array_equal) unless a case says `bound`; everything outside
the covered C tiles must come back unchanged, bit for bit.  Every C tile written with
beta == 0 starts as NaN.  Every case asserts the path it took: the split each problem got,
whether the launch had a tile list, whether the CDEF instance ran.

Every group runs twice, in the implicit tile order (the kernel's own decodes) and with the tile
list of order_tiles: same bits, and the list is a permutation of exactly the tiles the problems
cover.  The split-K groups run twice more under split_k.
"""
import numpy as np
import pytest

import gemm_group_ref as gr
from gemm_group_ref import G_CLOWER, G_KBEG_TI, G_KEND_TI, TILE, Layout, problem

pytestmark = pytest.mark.gpu

GPE_ERR_ARG = -1


# ---------------------------------------------------------------- running and checking
def want_cdef(probs):
    """The host's rule (gemm_cdef): the launch takes the CDEF instance when some problem has
    beta != 0 and at least 10 K stages."""
    return any(p.get("beta", 0.0) != 0.0 and p["K"] >= 160 for p in probs)


def want_ksplit(probs):
    """split_k's rule: only beta == 0 groups of fewer than 256 tiles, shares of at least 64
    of the longest K, at most 8 and at most 512 partial tiles."""
    T = sum(len(gr.tiles(p)) for p in probs)
    if any(p.get("beta", 0.0) != 0.0 for p in probs) or T >= 256:
        return 1
    ks = min(8, 512 // T, max(p["K"] for p in probs) // 64)
    return ks if ks >= 2 else 1


def codes(probs):
    return sorted(ip << 24 | ti << 12 | tj for ip, p in enumerate(probs) for ti, tj in gr.tiles(p))


def same_bits(x, y):
    return all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(x, y))


def check(ctx, lens, probs, kind, *, seed=0, poison=False, split=False, ksplit=None, cdef=None):
    """Fill, run, compare: in the implicit order and listed; with split also under split_k, as
    one launch and as the same launch twice in a row (the second needs the counters back at
    zero).  All runs must give the same bits.  Returns the largest fraction of the rounding
    bound seen (0.0 for exact cases)."""
    bufs = gr.fill(lens, probs, kind, np.random.default_rng(seed), poison)
    ref = gr.expected(bufs, probs, kind)
    cdef = want_cdef(probs) if cdef is None else cdef
    ntiles = sum(len(gr.tiles(p)) for p in probs)
    outs, worst = [], 0.0
    runs = [dict(listed=False), dict(listed=True)]
    if split:
        runs += [dict(split=True, reps=1), dict(split=True, reps=2)]
    for kw in runs:
        o = ctx.test_gemm_group(bufs, probs, kind=kind, **kw)
        worst = max(worst, gr.compare(o["bufs"], bufs, probs, kind, ref))
        ks = (want_ksplit(probs) if ksplit is None else ksplit) if kw.get("split") else 1
        assert list(o["ksplit"]) == [ks] * len(probs), (kw, o["ksplit"])
        assert o["workgroups"] == ntiles * ks
        assert o["cdef"] == cdef, kw
        assert o["listed"] == bool(kw.get("listed")), kw
        if o["listed"]:
            assert sorted(o["tiles"].tolist()) == codes(probs)
        outs.append(o["bufs"])
    assert all(same_bits(outs[0], o) for o in outs[1:]), "runs of one group, different results"
    return worst


def single(kind, mt, nt, K, **kw):
    lay = Layout()
    return lay.lens, [problem(lay, kind, mt, nt, K, **kw)]


# ---------------------------------------------------------------- short and boundary pipelines
# stages nk = K / 16: 1 (no further stage), 2 and 3 (even / odd tail of the stage-pair loop),
# 9 | 10 (C preloaded | C added inside the K loop), 11 and 12 (the straight-line prologue, then
# an odd / even tail)
@pytest.mark.parametrize("K", [16, 32, 48, 144, 160, 176, 192])
@pytest.mark.parametrize("kind", range(4))
def test_one_tile_pipelines(ctx, kind, K):
    for alpha, beta in [(1.0, 0.0), (-1.0, 0.5)]:
        lens, probs = single(kind, 1, 1, K, alpha=alpha, beta=beta)
        check(ctx, lens, probs, kind, seed=K + kind, cdef=(beta != 0.0 and K >= 160))


@pytest.mark.parametrize("kind", range(4))
def test_256_by_384(ctx, kind):
    lens, probs = single(kind, 2, 3, 208, alpha=-1.0, beta=0.5)     # 13 stages
    check(ctx, lens, probs, kind, seed=kind, cdef=True)
    lens, probs = single(kind, 2, 3, 144, alpha=-1.0, beta=0.5)
    check(ctx, lens, probs, kind, seed=kind, cdef=False)


@pytest.mark.parametrize("K", [144, 160, 512])
@pytest.mark.parametrize("kind", range(4))
def test_general_scaling_within_the_rounding_bound(ctx, kind, K):
    """bound: alpha = -0.7, beta = 0.3 (gemm_group_ref: (K + 6) 2^-53 (|alpha| |A||B| + |beta| |C0|))."""
    lens, probs = single(kind, 2, 1, K, alpha=-0.7, beta=0.3, pad=2)
    frac = check(ctx, lens, probs, kind, seed=K, cdef=K >= 160)
    print("rounding bound fraction kind %d K %d: %.4f" % (kind, K, frac))
    assert 0.0 < frac <= 1.0


# ---------------------------------------------------------------- windows
@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("kind", range(4))
def test_leading_dimensions_and_offsets(ctx, kind, poison):
    """ld larger than the extent, non-zero even offsets, and all three windows in ONE buffer;
    the gaps hold the sentinel, or NaN (poison)."""
    lay = Layout(1)
    probs = [problem(lay, kind, 2, 2, 176, bufs=(0, 0, 0), pad=6, gap=10, alpha=-1.0, beta=0.5),
             problem(lay, kind, 1, 2, 48, bufs=(0, 0, 0), pad=130, gap=2)]
    check(ctx, lay.lens, probs, kind, seed=3, poison=poison)


def lauum(mt, ld_pad=0, off=0, **kw):
    """A^-1 = X^T X as build_plan has it: X lower-triangular column-major, both operands the
    same window (K-contiguous: opA(m, k) = X(k, m)), lower C tiles only, K from the row's
    own diagonal tile on.  X's strictly upper tiles are never read."""
    n = TILE * mt
    ld = n + ld_pad
    lens = [off + ld * n + 2, n * n]
    x = (0, off, ld)
    return lens, [dict(a=x, b=x, c=(1, 0, n), mt=mt, nt=mt, K=n, flags=G_CLOWER | G_KBEG_TI, **kw)]


def trtri_level(NB, pairs, ld_pad=0):
    """The two launches of one TRTRI level as build_plan has them (trtri_level_pairs' block
    pairs {t0, h, t1}, written out by the caller): buffer 0 is B (X = L^-1 on and below the
    diagonal blocks already inverted, scratch above), buffer 1 is A (L).
      first  <1, 0>: T^T = X11^T L21^T into B's upper block (t0:h, h:t1), G_KBEG_TI
      second <0, 0>: X21 = -X22 T into B's lower block (h:t1, t0:h), G_KEND_TI
    Operands and C are windows of the same matrix, on disjoint tiles."""
    n = TILE * NB
    ld = n + ld_pad
    lens = [ld * n, ld * n]
    tile = lambda buf, i, j: (buf, TILE * i + TILE * j * ld, ld)
    first, second = [], []
    for t0, h, t1 in pairs:
        a, b = h - t0, t1 - h
        first.append(dict(a=tile(0, t0, t0), b=tile(1, h, t0), c=tile(0, t0, h), mt=a, nt=b, K=a * TILE,
                          flags=G_KBEG_TI, alpha=1.0, beta=0.0))
        second.append(dict(a=tile(0, h, h), b=tile(0, t0, h), c=tile(0, h, t0), mt=b, nt=a, K=b * TILE,
                           flags=G_KEND_TI, alpha=-1.0, beta=0.0))
    return lens, (1, first), (0, second)


TRTRI_LEVELS = [(3, [(0, 2, 3)]), (5, [(0, 1, 2), (2, 3, 4)]), (5, [(0, 4, 5)])]


@pytest.mark.parametrize("NB,pairs", TRTRI_LEVELS)
def test_trtri_windows_of_one_matrix(ctx, NB, pairs):
    lens, first, second = trtri_level(NB, pairs, ld_pad=4)
    for kind, probs in (first, second):
        check(ctx, lens, probs, kind, seed=NB, poison=True)


# ---------------------------------------------------------------- G_CLOWER and the K ranges
@pytest.mark.parametrize("mt", [1, 2, 3, 5])
@pytest.mark.parametrize("kind", [0, 2])
def test_clower(ctx, kind, mt):
    """The Cholesky's trailing update form (beta = 1, CDEF); upper tiles hold the sentinel."""
    lens, probs = single(kind, mt, mt, 160, flags=G_CLOWER, alpha=-1.0, beta=1.0)
    check(ctx, lens, probs, kind, seed=mt, cdef=True)
    lens, probs = single(kind, mt, mt, 48, flags=G_CLOWER)
    check(ctx, lens, probs, kind, seed=mt, poison=True)


@pytest.mark.parametrize("mt", [2, 3, 5])
@pytest.mark.parametrize("kind", [1, 2])
def test_kbeg_ti(ctx, kind, mt):
    lens, probs = single(kind, mt, 2, TILE * mt, flags=G_KBEG_TI)
    check(ctx, lens, probs, kind, seed=mt, poison=True)


@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_kbeg_ti_rows_with_an_empty_range(ctx, beta):
    """K = 272 < 3 x 128: row 2 has one stage, row 3 none (kbeg = 384 > K): C = beta C0."""
    lens, probs = single(1, 4, 2, 272, flags=G_KBEG_TI, alpha=-1.0, beta=beta)
    assert gr.k_range(probs[0], 2) == (256, 272) and gr.k_range(probs[0], 3)[0] > 272
    check(ctx, lens, probs, 1, seed=5, poison=True, cdef=beta != 0.0)


# single problem: mt % 8 == 0 takes the XCD decode, other mt the longest-first decode; as the
# second of two problems the same rows take the generic decode (ti = local % mt)
@pytest.mark.parametrize("mt,nt", [(8, 1), (8, 3), (3, 2), (5, 2)])
@pytest.mark.parametrize("kind", [0, 3])
def test_kend_ti(ctx, kind, mt, nt):
    lens, probs = single(kind, mt, nt, TILE * mt, flags=G_KEND_TI, alpha=-1.0)
    check(ctx, lens, probs, kind, seed=mt + nt, poison=True)
    lay = Layout()
    probs = [problem(lay, kind, 1, 2, 32), problem(lay, kind, mt, nt, TILE * mt, flags=G_KEND_TI, alpha=-1.0)]
    check(ctx, lay.lens, probs, kind, seed=mt + nt, poison=True)


@pytest.mark.parametrize("mul", [2, 3])
@pytest.mark.parametrize("off", [0, 1, 2])
def test_kend_ti_cyclic_rows(ctx, mul, off):
    """The row-block TRTRI's form: row ti ends at (ti mul + off + 1) x 128, capped by K; K is
    chosen so that the last row is capped, at no multiple of 128."""
    mt = 3
    K = TILE * ((mt - 1) * mul + off) + 48
    lens, probs = single(0, mt, 2, K, flags=G_KEND_TI, kti_mul=mul, kti_off=off, alpha=-1.0)
    p = probs[0]
    assert [gr.k_range(p, ti)[1] for ti in range(mt)] == [TILE * (off + 1), TILE * (mul + off + 1), K]
    check(ctx, lens, probs, 0, seed=mul + off, poison=True)
    lay = Layout()     # and as one of two problems, with beta != 0
    probs = [problem(lay, 0, 2, 1, 64),
             problem(lay, 0, mt, 1, K, flags=G_KEND_TI, kti_mul=mul, kti_off=off, alpha=-1.0, beta=0.5)]
    check(ctx, lay.lens, probs, 0, seed=mul + off, poison=True)


@pytest.mark.parametrize("mt", [2, 4])
def test_lauum_form(ctx, mt):
    lens, probs = lauum(mt, ld_pad=2, off=6)
    check(ctx, lens, probs, 2, seed=mt, poison=True)
    # both range flags at once (rows end at their diagonal tile too: one tile of K per row)
    lens, probs = lauum(mt)
    probs[0]["flags"] |= G_KEND_TI
    assert all(gr.k_range(probs[0], ti) == (TILE * ti, TILE * ti + TILE) for ti in range(mt))
    check(ctx, lens, probs, 2, seed=mt, poison=True)


# ---------------------------------------------------------------- split K
@pytest.mark.parametrize("K,ks", [(128, 2), (192, 3), (320, 5), (1024, 8)])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_split_k(ctx, kind, K, ks):
    lens, probs = single(kind, 1, 2, K, alpha=-1.0)
    check(ctx, lens, probs, kind, seed=K, split=True, ksplit=ks, poison=True)


def test_split_k_uneven_and_empty_shares(ctx):
    """ksplit = 5 on rows of 20, 12 and 4 stages: 12 is no multiple of 5, and a row of 4
    stages leaves one share empty.  Two problems: the counters and partial slots of the second
    follow the first's."""
    lay = Layout()
    probs = [problem(lay, 1, 3, 1, 320, flags=G_KBEG_TI), problem(lay, 1, 3, 2, 320, flags=G_KBEG_TI, alpha=-1.0)]
    assert [(k1 - k0) // 16 for k0, k1 in (gr.k_range(probs[0], ti) for ti in range(3))] == [20, 12, 4]
    check(ctx, lay.lens, probs, 1, seed=1, split=True, ksplit=5, poison=True)


def test_split_k_lauum(ctx):
    lens, probs = lauum(3)     # 6 tiles of 24, 16 and 8 stages in 6 shares
    check(ctx, lens, probs, 2, seed=2, split=True, ksplit=6, poison=True)


@pytest.mark.parametrize("NB,pairs", TRTRI_LEVELS)
def test_split_k_trtri_level(ctx, NB, pairs):
    lens, first, second = trtri_level(NB, pairs)
    for kind, probs in (first, second):
        assert want_ksplit(probs) >= 2
        check(ctx, lens, probs, kind, seed=NB, split=True, poison=True)


def test_split_k_declines(ctx):
    lens, probs = single(0, 1, 2, 320, alpha=-1.0, beta=0.5)      # beta != 0
    check(ctx, lens, probs, 0, split=True, ksplit=1, cdef=True)
    lay = Layout()                                                # one beta != 0 problem in the group
    probs = [problem(lay, 0, 1, 1, 128), problem(lay, 0, 1, 1, 128, beta=1.0)]
    check(ctx, lay.lens, probs, 0, split=True, ksplit=1)
    lens, probs = single(0, 16, 16, 128)                          # 256 tiles
    check(ctx, lens, probs, 0, split=True, ksplit=1)
    lens, probs = single(0, 1, 1, 112)                            # no two shares of 64
    check(ctx, lens, probs, 0, split=True, ksplit=1)


# ---------------------------------------------------------------- groups
@pytest.mark.parametrize("kind", range(4))
def test_three_problems(ctx, kind):
    lay = Layout()
    probs = [problem(lay, kind, 3, 3, 384, flags=G_CLOWER | G_KBEG_TI, alpha=2.0, pad=2),
             problem(lay, kind, 2, 3, 96, alpha=-1.0, beta=0.5, gap=4),
             problem(lay, kind, 4, 1, 400, flags=G_KEND_TI, alpha=-0.5, beta=0.25, pad=4)]
    check(ctx, lay.lens, probs, kind, seed=kind, poison=True, cdef=True)


def test_300_one_tile_problems(ctx):
    """Past the 255 problems a tile list can name: the implicit order, and the kernel's binary
    search over tile_begin."""
    lay = Layout()
    probs = [problem(lay, 3, 1, 1, 16, alpha=(-1.0) ** i * 2.0 ** (i % 3), gap=2 * (i % 5)) for i in range(300)]
    bufs = gr.fill(lay.lens, probs, 3, np.random.default_rng(300))
    o = ctx.test_gemm_group(bufs, probs, kind=3)
    gr.compare(o["bufs"], bufs, probs, 3)
    assert not o["listed"] and not o["cdef"] and o["workgroups"] == 300 and o["tiles"] is None
    assert list(o["ksplit"]) == [1] * 300


@pytest.mark.parametrize("kind", range(4))
def test_mixed_cdef_launch(ctx, kind):
    """One CDEF launch holding a problem that qualifies (K = 512, beta != 0); a G_KEND_TI
    problem with beta != 0 whose first row has 8 stages (C preloaded inside the CDEF instance)
    and later rows 16 and 24 (C deferred); and a beta == 0 problem over NaN with 16 stages,
    whose C chunks are loaded and must be discarded."""
    lay = Layout()
    probs = [problem(lay, kind, 1, 2, 512, alpha=-1.0, beta=1.0),
             problem(lay, kind, 3, 1, 384, flags=G_KEND_TI, alpha=-1.0, beta=0.5, pad=2),
             problem(lay, kind, 2, 1, 256, alpha=1.0, beta=0.0, gap=6)]
    check(ctx, lay.lens, probs, kind, seed=kind, poison=True, cdef=True)


# ---------------------------------------------------------------- argument checks
def test_argument_checks(ctx):
    """Each refused form answers GPE_ERR_ARG with text; nothing is launched, and the buffers
    are not touched."""
    lay = Layout()
    good = problem(lay, 0, 2, 2, 64, pad=2)
    lens = lay.lens
    bufs = [np.zeros(n) for n in lens]

    def refused(p, word, nprob=1, **kw):
        with pytest.raises(RuntimeError, match=r"gpe_test_gemm_group failed \(%d\).*%s" % (GPE_ERR_ARG, word)):
            ctx.test_gemm_group(bufs, [p] * nprob, **dict(dict(kind=0), **kw))

    ctx.test_gemm_group(bufs, [good], kind=0)                       # the form the others vary
    for fused in (8, 16, 32, 64, 128, 16 | 64):
        refused(dict(good, flags=fused), "fused")
    refused(dict(good, K=72), "multiple of 16")
    refused(dict(good, K=0), "multiple of 16")
    refused(dict(good, alpha=0.0), "alpha")
    refused(dict(good, alpha=float("nan")), "alpha")
    for key in "abc":
        buf, off, ld = good[key]
        refused(dict(good, **{key: (buf, off, ld + 1)}), "odd leading")
        refused(dict(good, **{key: (buf, off + 1, ld)}), "offset")
        refused(dict(good, **{key: (buf, -2, ld)}), "offset")
        refused(dict(good, **{key: (buf, off + 6, ld)}), "leaves its buffer")   # (4 spare: pad and tail)
        refused(dict(good, **{key: (3, off, ld)}), "buffer index")
    refused(dict(good, c=(2, 0, (1 << 21) + 2)), "2\\^21")
    refused(dict(good, mt=4097), "4096")
    refused(dict(good, nt=0), "4096")
    refused(dict(good, kti_mul=-1), "kti")
    refused(dict(good, mt=3), "A leaves its buffer at tile row 2")
    # the window test is over the tile's own K range: K = 256 fits while rows end at 128 ...
    lay2 = Layout()
    tri = problem(lay2, 0, 1, 1, 128)
    bufs2 = [np.zeros(n) for n in lay2.lens]
    with pytest.raises(RuntimeError, match="leaves its buffer"):
        ctx.test_gemm_group(bufs2, [dict(tri, K=256)], kind=0)
    o = ctx.test_gemm_group(bufs2, [dict(tri, K=256, flags=G_KEND_TI)], kind=0)
    assert o["workgroups"] == 1
    # ... and reaches past the buffer with a row offset
    with pytest.raises(RuntimeError, match="leaves its buffer"):
        ctx.test_gemm_group(bufs2, [dict(tri, K=256, flags=G_KEND_TI, kti_off=1)], kind=0)
    refused(good, "255 problems", nprob=256, listed=True)
    for kw in (dict(kind=4), dict(kind=-1), dict(reps=0), dict(reps=17), dict(split=2), dict(listed=2)):
        refused(good, "kind 0..3", **kw)
    assert all(np.all(b == 0.0) for b in bufs)
