"""k_oz_gemm's stage pipeline (gpemu_ozaki.hpp) at the smallest shapes where its schedule can
go wrong: the ring's prologue, steady state and drain around the ring depth, and launches whose
tiles run different stage counts.  Every case is one product through gpe_test_oz_product,
judged by tests/oz_product_ref.py (exponents exactly, residues congruent and in range, C within
its derived bound), and then run ten times in a row: C and the returned residues must be
byte-identical across the ten (a ring hazard -- a stage read before it landed, a buffer
overwritten before its last read -- shows first as a run that differs).

The loop's stages, for a tile of ns stages and a ring of NBUF = 4 buffers: a tile shorter than
the ring loads whole in the prologue; otherwise the prologue leaves half of stage NBUF - 1 to
the first step, steps 0 .. ns - NBUF - 1 are the steady state (loads under both k-steps), step
ns - NBUF carries the last half stage, the next NBUF - 2 steps only wait, the last step has no
barrier.  ns = NBUF - 1, NBUF, NBUF + 1, 2 NBUF, 2 NBUF + 1 take every one of these paths with
the fewest stages; 31 and 32 wrap the ring index several times at both parities.
"""
import numpy as np
import pytest

import oz_product_ref as ozr
from test_gpu_oz_product import check, dense, dropped, integers, nan_dropped, run, store

pytestmark = pytest.mark.gpu

NBUF = 4
REPS = 10


def run_checked_and_repeated(ctx, what, a, b, ref, *, rows, cols, ti0=0, tri=False, lower128=False, alpha=1.0,
                             **kw):
    """One product against the reference (residues of moduli 0 and 1), then the same call until
    it has run REPS times with the residues of modulus 1: the same bytes every time."""
    got = run(ctx, a, b, rows=rows, cols=cols, ti0=ti0, tri=tri, lower128=lower128, alpha=alpha, **kw)
    check(what, got, ref, rows=rows, cols=cols, ti0=ti0, tri=tri, lower128=lower128, alpha=alpha)
    C0, res0 = np.ascontiguousarray(got[0].T), got[3][1]
    lr = rows - 256 * ti0
    ldc, cc = lr + 5, cols + 3   # (run()'s default frame around C)
    for rep in range(1, REPS):
        o = ctx.test_oz_product(a, b, C=np.full(cc * ldc, -1.2345678e300), ldc=ldc, rows=rows, cols=cols, ti0=ti0,
                                tri=tri, lower128=lower128, alpha=alpha, res_mod=1, **kw)
        assert np.array_equal(o["C"].view(np.uint64), C0.ravel().view(np.uint64)), "%s: C of run %d differs" % (what, rep)
        assert np.array_equal(o["res"], res0), "%s: residues of run %d differ at %s" % (
            what, rep, list(zip(*np.nonzero(o["res"] != res0)))[:5])
    return got


# ---------------------------------------------------------------- one tile, K = 64 ns
NS = [NBUF - 1, NBUF, NBUF + 1, 2 * NBUF, 2 * NBUF + 1, 31, 32]


@pytest.mark.parametrize("ns", NS)
def test_one_tile_integers(ctx, ns):
    """Random 53-bit integer operands (e = 0, X' = X): every stage carries full-size terms."""
    rng = np.random.default_rng(500 + ns)
    K = 64 * ns
    a, b = integers(rng, 256, K), integers(rng, 256, K)
    ref = ozr.Ref(a, b, K=K)
    assert not ref.ea.any() and not ref.eb.any() and (ref.Ai == a).all() and (ref.Bi == b).all()
    run_checked_and_repeated(ctx, "integers ns=%d" % ns, store(a, 0), store(b, 0), ref, rows=256, cols=256, K=K)


@pytest.mark.parametrize("ns", NS)
def test_one_tile_onehot(ctx, ns):
    """Row i of A is 2^52 at k_i alone and B(j, k) = +-(2^52 + j K + k), all distinct:
    C(i, j) = 2^52 B(j, k_i), so a stale, early-overwritten or skipped stage names the k whose
    value came out instead.  The k_i visit every stage and every 16-byte slot of a stage."""
    K = 64 * ns
    ki = (59 * np.arange(256)) % K
    assert len(set((ki // 64).tolist())) == ns and len(set((ki % 64 // 16).tolist())) == 4
    a = np.zeros((256, K))
    a[np.arange(256), ki] = 2.0 ** 52
    j, k = np.arange(256)[:, None], np.arange(K)[None, :]
    b = np.where((j + k) % 2 == 0, 1.0, -1.0) * (2.0 ** 52 + j * K + k)
    ref = ozr.Ref(a, b, K=K)
    assert not ref.ea.any() and not ref.eb.any() and (ref.Bi == b).all()
    got = run_checked_and_repeated(ctx, "one-hot ns=%d" % ns, store(a, 0), store(b, 0), ref, rows=256, cols=256, K=K)
    C = got[0][:256, :256]
    want = 2.0 ** 52 * b[:, ki].T
    if not (np.abs(C - want) <= 4 * np.spacing(np.abs(want))).all():
        msg = []
        for i, jj in list(zip(*np.nonzero(np.abs(C - want) > 4 * np.spacing(np.abs(want)))))[:6]:
            kk = np.nonzero(np.abs(b[jj]) == np.abs(C[i, jj]) / 2.0 ** 52)[0]
            msg.append("C(%d, %d): wanted k = %d (stage %d), got %s" % (
                i, jj, ki[i], ki[i] // 64, ("k = %d (stage %d)" % (kk[0], kk[0] // 64)) if kk.size else "no B(j, .)"))
        raise AssertionError("; ".join(msg))


# ---------------------------------------------------------------- mixed stage counts in one launch
def test_rectangular_3x2_kbeg2(ctx):
    """3 x 2 tiles, kbeg 2: tile column tj starts at k = 256 tj, so with K = 512 the launch
    holds tiles of 8 stages (tj = 0) and of 4 (tj = 1).  B's rows are zero before their own
    index (mask 1), as the contract demands of the k a range skips; garbage lies there in the
    source."""
    rng = np.random.default_rng(520)
    Ra, Rb, K = 768, 512, 512
    a = integers(rng, Ra, K)
    bm = integers(rng, Rb, K, mask=1)
    sb = nan_dropped(store(bm, 0, ld=K + 2, garbage=dropped(rng, Rb, K, 1)), Rb, K, 1)
    sb["mask"] = 1
    ref = ozr.Ref(a, dense(bm, 1), K=K)
    run_checked_and_repeated(ctx, "3x2 kbeg 2", store(a, 0, ld=K), sb, ref, rows=Ra, cols=Rb, K=K, kbeg=2)


def test_rectangular_3x2_kend1(ctx):
    """3 x 2 tiles, kend 1: tile row ti ends at k = 256 (ti + 1): 4, 8 and 12 stages with
    K = 768.  A's rows are zero past their own index (mask 2)."""
    rng = np.random.default_rng(521)
    Ra, Rb, K = 768, 512, 768
    am = integers(rng, Ra, K, mask=2)
    b = integers(rng, Rb, K)
    sa = nan_dropped(store(am, 0, ld=K + 4, garbage=dropped(rng, Ra, K, 2)), Ra, K, 2)
    sa["mask"] = 2
    ref = ozr.Ref(dense(am, 2), b, K=K)
    run_checked_and_repeated(ctx, "3x2 kend 1", sa, store(b, 0, ld=K), ref, rows=Ra, cols=Rb, K=K, kend=1)


def test_packed_768(ctx):
    """The packed (LAUUM) form at R = 768: six tiles, tile row ti from k = 256 ti: 12, 8 and 4
    stages in one launch."""
    rng = np.random.default_rng(522)
    n = 768
    op = dense(integers(rng, n, n, mask=1), 1)
    src = nan_dropped(store(op, 0, ld=n + 2, garbage=dropped(rng, n, n, 1)), n, n, 1, every=7)
    ref = ozr.Ref(op, K=n)
    assert not ref.ea.any() and (ref.Ai == op).all()
    run_checked_and_repeated(ctx, "packed 768", src, None, ref, rows=n, cols=n, tri=True, lower128=True, packed=True)


def test_triangular_from_tile_row_1(ctx):
    """The triangular form from ti0 = 1 (tile rows 1 and 2 of 3, five tiles of 5 stages): the
    residues and k_oz_crt's tile decoding count from tile (1, 0)."""
    rng = np.random.default_rng(523)
    R, K = 768, 64 * (NBUF + 1)
    a = integers(rng, R, K)
    ref = ozr.Ref(a, K=K)
    run_checked_and_repeated(ctx, "tri ti0=1", store(a, 0, ld=K + 2), None, ref, rows=R, cols=R, ti0=1, tri=True,
                             lower128=True, K=K)
