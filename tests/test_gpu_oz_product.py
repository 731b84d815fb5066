"""The int8 products (gpemu_ozaki.hpp) kernel by kernel against exact integers: one product at
a time through gpe_test_oz_product -- the production sequence k_oz_colexp / k_oz_rowexp<T>
(+ k_oz_il_to_ex), k_oz_split / k_oz_split_rect<T>, k_oz_gemm, k_oz_crt on buffers of the
hook's own.  The hook does not repeat that sequence: it calls the launch layer every
production product calls (gpemu_ozaki.hpp: oz_operand / oz_operand_packed for the operands,
OzShape for the tile list and its k ranges, oz_product_launch for the two kernels), so the
launch lines, grids and the k-range rule checked here are the ones production runs.  The
results are compared entry by entry with tests/oz_product_ref.py: the row exponents
exactly, the residues of two moduli (congruent to the exact C', within the epilogue's stated
range), and C within the bound derived there from k_oz_crt's arithmetic.
A failure names the operand form, the entry (so the tile, row and column) and, for the
residues, the modulus; the one-hot group also names the k the wrong value came from.

Sources are written as the call sites hold them (column-major blocks with a leading
dimension); everything a form's contract says is never read -- the masked-out triangle, the
gap between the columns, the part of a scratch block past its rows -- is NaN in the source.
"""
import numpy as np
import pytest

import oz_product_ref as ozr

pytestmark = pytest.mark.gpu

SENT = -1.2345678e300   # what C holds where nothing may be written


# ---------------------------------------------------------------- operands and sources
def rough(rng, R, Kv, spread=70):
    """Mixed signs, every row scaled by 2^+-200, entries spread over 2^-spread inside a row
    (more than beta: the small ones lose bits or vanish in X')."""
    x = rng.standard_normal((R, Kv)) * np.exp2(-rng.integers(0, spread + 1, size=(R, Kv)).astype(float))
    x[rng.random((R, Kv)) < 0.05] = 0.0
    return np.ldexp(x, rng.integers(-200, 201, size=(R, 1)).astype(np.int32))


def integers(rng, R, Kv, beta=53, mask=0):
    """Integer operands with every row's maximum in [2^(beta-1), 2^beta): e = 0 and X' = X, so
    the reference is the plain exact product of the inputs.  The maximum sits where the mask
    keeps it (the diagonal)."""
    x = np.rint(rng.standard_normal((R, Kv)) * np.exp2(beta - 3 - rng.integers(0, 41, size=(R, Kv)).astype(float)))
    x = np.clip(x, -(2.0 ** (beta - 1)), 2.0 ** (beta - 1))
    r = np.arange(R)
    k = np.minimum(r, Kv - 1) if mask else rng.integers(0, Kv, size=R)
    x[r, k] = np.where(rng.random(R) < 0.5, -1.0, 1.0) * (2.0 ** (beta - 1) + rng.integers(0, 1 << 20, size=R))
    return x


def store(op, trans, ld=None, offset=0, garbage=None):
    """The source array holding op: op(r, k) at offset + k + r ld (trans 0) or offset + r + k ld
    (trans 1); NaN everywhere else, and garbage (same shape as op, NaN = keep op) over op."""
    R, Kv = op.shape
    if garbage is not None:
        op = np.where(np.isnan(garbage), op, garbage)
    inner, outer = (R, Kv) if trans else (Kv, R)
    ld = ld or inner
    assert ld >= inner
    src = np.full(offset + outer * ld + 3, np.nan)
    block = src[offset:offset + outer * ld].reshape(outer, ld)
    block[:, :inner] = op.T if trans else op
    return dict(src=src, ld=ld, offset=offset, trans=int(trans), R=R, Kv=Kv)


def dropped(rng, R, Kv, mask):
    """Garbage for the part of an R x Kv operand that the mask drops (NaN = keep)."""
    r, k = np.arange(R)[:, None], np.arange(Kv)[None, :]
    drop = k < r if mask == 1 else k > r
    g = np.where(rng.random((R, Kv)) < 0.5, np.inf, 1e300 * rng.standard_normal((R, Kv)))
    g[rng.random((R, Kv)) < 0.3] = -0.0
    g[(r + k) % 7 == 0] = 7.0
    out = np.full((R, Kv), np.nan)
    out[drop] = g[drop]
    # (NaN stands for 'keep' here: the NaNs of the garbage are nan_dropped's)
    return out


def nan_dropped(src_desc, R, Kv, mask, every=5):
    """Put NaN into every `every`-th dropped entry of a stored operand (store() keeps NaN for
    'no garbage', so the NaNs go in afterwards)."""
    d = src_desc
    for r in range(R):
        ks = range(0, r, every) if mask == 1 else range(r + 1, Kv, every)
        for k in ks:
            d["src"][d["offset"] + (r + k * d["ld"] if d["trans"] else k + r * d["ld"])] = np.nan
    return d


# ---------------------------------------------------------------- running and checking
def run(ctx, a, b, *, rows, cols, ti0=0, Cold=None, extra=(5, 3), res_mods=(0, 1), **kw):
    """One product; C is (rows - 256 ti0 + extra[0]) x (cols + extra[1]) column-major, filled
    with SENT (or Cold in its top-left corner).  Returns (C 2-d, exa, exb, {l: residues})."""
    lr = rows - 256 * ti0
    ldc, cc = lr + extra[0], cols + extra[1]
    C0 = np.full((cc, ldc), SENT)
    if Cold is not None:
        C0[:cols, :lr] = Cold.T
    res = {}
    out = None
    for l in res_mods or (None,):
        o = ctx.test_oz_product(a, b, C=C0.ravel(), ldc=ldc, rows=rows, cols=cols, ti0=ti0, res_mod=l, **kw)
        if out is not None:
            assert np.array_equal(o["C"].view(np.uint64), out["C"].view(np.uint64)), "two runs, two results"
        out = o
        if l is not None:
            res[l] = o["res"]
    return out["C"].reshape(cc, ldc).T, out["exa"], out["exb"], res


def region(rows, cols, ti0=0, tri=False, lower128=False, shape=None):
    """Boolean map of the entries of the local C (row 0 = product row 256 ti0) that the product
    writes."""
    lr = rows - 256 * ti0
    w = np.zeros(shape or (lr, cols), bool)
    gi, j = (np.arange(lr) + 256 * ti0)[:, None], np.arange(cols)[None, :]
    ok = np.ones((lr, cols), bool)
    if tri:
        ok &= (j >> 8) <= (gi >> 8)
    if lower128:
        ok &= (j >> 7) <= (gi >> 7)
    w[:lr, :cols] = ok
    return w


def check(what, got, ref, *, rows, cols, ti0=0, tri=False, lower128=False, alpha=1.0, Cold=None):
    """Exponents, residues, C and the untouched rest of C of one run against ref (the exact
    product of the whole operands; the run covers its rows from 256 ti0)."""
    C, exa, exb, res = got
    assert np.array_equal(exa, ref.padded_ex("a")), "%s: exponents of A differ at rows %s" % (
        what, np.nonzero(exa != ref.padded_ex("a"))[0][:8])
    assert np.array_equal(exb, ref.padded_ex("b")), "%s: exponents of B differ at rows %s" % (
        what, np.nonzero(exb != ref.padded_ex("b"))[0][:8])
    sub = ref.rows_from(256 * ti0)
    Ra, Rb = sub.Cint.shape
    for l, r in res.items():
        m = ozr.MODS[l]
        cov = region(r.shape[0] + 256 * ti0, r.shape[1], ti0, tri=tri)   # whole 256-tiles
        want = np.zeros(r.shape, dtype=np.int64)
        want[:Ra, :Rb] = sub.residues(l)                                 # (padding rows: C' = 0)
        got_r = r.astype(np.int64)
        wrong = cov & ((got_r - want) % m != 0)
        assert not wrong.any(), "%s: residues mod %d (modulus %d) wrong at %d entries, first (i, j, got, want) %s" % (
            what, m, l, wrong.sum(), [(int(i), int(j), int(got_r[i, j]), int(want[i, j])) for i, j in
                                      list(zip(*np.nonzero(wrong)))[:5]])
        # k_oz_gemm's epilogue: the low byte (m = 256), else within one of the centred range
        assert (got_r == want)[cov].all() if m == 256 else (np.abs(got_r) <= m // 2 + 1).all(), (what, m)
    w = region(rows, cols, ti0, tri, lower128, shape=C.shape)
    keep = np.full(C.shape, SENT)
    if Cold is not None:
        keep[:rows - 256 * ti0, :cols] = Cold
    assert np.array_equal(C[~w].view(np.uint64), keep[~w].view(np.uint64)), "%s: written outside the product at %s" % (
        what, list(zip(*np.nonzero(~w & (C.view(np.uint64) != keep.view(np.uint64)))))[:5])
    lr = rows - 256 * ti0
    bad, worst = ozr.compare(C[:lr, :cols], sub, alpha=alpha, Cold=Cold, where=w[:lr, :cols])
    print("%s: largest error / bound %.3g over %d entries" % (what, worst, int(w.sum())))
    assert not bad.any(), what + ": " + ozr.describe(bad, C[:lr, :cols], sub, alpha)
    return worst


def dense(desc_op, mask=0):
    return ozr.masked(desc_op, mask)


# ---------------------------------------------------------------- 1. one tile, K = 64 ns
@pytest.mark.parametrize("ns", [1, 2, 3, 4, 5, 7, 8, 9])
def test_one_tile_stage_ring(ctx, ns):
    """Prologue (ns < 3: fewer stages than the ring is deep, wait_stage's own vmcnt), steady
    state and drain of k_oz_gemm's stage ring."""
    rng = np.random.default_rng(100 + ns)
    K = 64 * ns
    a, b = rough(rng, 256, K), rough(rng, 256, K)
    got = run(ctx, store(a, 0), store(b, 0), rows=256, cols=256, K=K)
    check("ns=%d" % ns, got, ozr.Ref(a, b, K=K), rows=256, cols=256)


def test_one_tile_empty_k_range(ctx):
    """ns = 0: the one tile of the launch, (1, 0) with kbeg 3 and kdiv 1, starts at k = 256 = K.
    Whatever the operands hold, the product over an empty range is exactly 0."""
    rng = np.random.default_rng(100)
    a, b = rough(rng, 512, 256), rough(rng, 256, 256)
    C, exa, exb, res = run(ctx, store(a, 0), store(b, 0), rows=512, cols=256, ti0=1, K=256, kbeg=3, kdiv=1)
    assert not res[0].any() and not res[1].any()
    assert (C[:256, :256] == 0.0).all() and (C[256:] == SENT).all() and (C[:, 256:] == SENT).all()
    beta = ozr.consts(16, 256)[0]
    assert np.array_equal(exa, ozr.exponents(a, beta)) and np.array_equal(exb, ozr.exponents(b, beta))


def test_one_tile_cancelling_rows(ctx):
    """Integer rows whose products cancel exactly: C' = 0, +1, -1 from terms of 2^104, the terms
    in three different stages.  The residues are those of 0 and +-1; C within the bound (its
    absolute term: an exact product of 53-bit operands resolves 2^-78 M, not 1)."""
    rng = np.random.default_rng(7)
    K = 256
    a, b = integers(rng, 256, K), integers(rng, 256, K)
    p, q = 2.0 ** 52, 2.0 ** 52 + 1.0
    a[0] = 0.0
    a[0, [5, 100, 200]] = [p, q, 1.0]
    for j, last in ((0, 0.0), (1, 1.0), (2, -1.0)):
        b[j] = 0.0
        b[j, [5, 100, 200]] = [q, -p, last]
    ref = ozr.Ref(a, b, K=K)
    assert [int(ref.Cint[0, j]) for j in range(3)] == [0, 1, -1] and not ref.ea.any() and (ref.Ai == a).all()
    got = run(ctx, store(a, 0), store(b, 0), rows=256, cols=256, K=K)
    assert got[3][0][0, :3].tolist() == [0, 1, -1] and got[3][1][0, :3].tolist() == [0, 1, -1]
    check("cancelling", got, ref, rows=256, cols=256)


# ---------------------------------------------------------------- 2. one-hot operands
ONEHOT_K = 320   # five stages; 59 k mod 320 puts the 256 rows on 256 different k, every slot of a stage


def _onehot_msg(C, B, ki):
    """For the first wrong entries: the k whose B value came out instead of B(j, k_i)."""
    got = np.abs(C) / 2.0 ** 52
    out = []
    for i, j in list(zip(*np.nonzero(C != 2.0 ** 52 * B[:, ki].T)))[:6]:
        k = np.nonzero(np.abs(B[j]) == got[i, j])[0]
        out.append("C(%d, %d): wanted k = %d, got %s" % (i, j, ki[i], ("k = %d" % k[0]) if k.size else "no B(j, .)"))
    return "; ".join(out)


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_onehot_rectangular(ctx, ta, tb):
    """Row i of A is 2^52 at k_i alone, B holds distinct integers: C(i, j) = 2^52 B(j, k_i), so a
    wrong swizzle slot, row pitch or stage offset shows which k it read."""
    K = ONEHOT_K
    ki = (59 * np.arange(256)) % K
    assert len(set(ki.tolist())) == 256 and len(set((ki % 64).tolist())) == 64
    a = np.zeros((256, K))
    a[np.arange(256), ki] = 2.0 ** 52
    j, k = np.arange(256)[:, None], np.arange(K)[None, :]
    b = np.where((j + k) % 2 == 0, 1.0, -1.0) * (2.0 ** 52 + j * K + k)
    ref = ozr.Ref(a, b, K=K)
    assert not ref.ea.any() and not ref.eb.any() and (ref.Bi == b).all()
    got = run(ctx, store(a, ta, ld=330), store(b, tb, ld=332), rows=256, cols=256, K=K)
    C = got[0][:256, :256]
    check("one-hot trans %d %d" % (ta, tb), got, ref, rows=256, cols=256)
    # (2^52 B is an fp64 number and the bound is below one ulp of it only where it must be:
    # name the k of an entry that is not that number)
    assert (np.abs(C - 2.0 ** 52 * b[:, ki].T) <= 4 * np.spacing(np.abs(C))).all(), _onehot_msg(C, b, ki)


def test_onehot_packed(ctx):
    """The same through k_oz_colexp / k_oz_split and the packed panels: X (768 x 768 lower),
    columns 256..511 one-hot at rows 512 + (59 i mod 256), columns 0..255 distinct integers."""
    n = 768
    X = np.zeros((n, n))   # X[k, j]
    kk, jj = np.arange(n)[:, None], np.arange(256)[None, :]
    X[:, :256] = np.where(kk >= jj, np.where((jj + kk) % 2 == 0, 1.0, -1.0) * (2.0 ** 52 + jj * n + kk), 0.0)
    ki = 512 + (59 * np.arange(256)) % 256
    X[ki, 256 + np.arange(256)] = 2.0 ** 52
    X[512:, 512:] = np.tril(integers(np.random.default_rng(3), 256, 256, mask=1).T)
    op = X.T.copy()
    ref = ozr.Ref(op, K=n)
    assert not ref.ea.any() and (ref.Ai == op).all()
    src = store(op, 0, ld=n + 2, garbage=dropped(np.random.default_rng(4), n, n, 1))
    got = run(ctx, nan_dropped(src, n, n, 1, every=11), None, rows=n, cols=n, packed=True)
    check("one-hot packed", got, ref, rows=n, cols=n, tri=True, lower128=True)
    C = got[0][256:512, :256]
    want = 2.0 ** 52 * X[ki, :256]
    assert (np.abs(C - want) <= 4 * np.spacing(np.abs(want))).all(), _onehot_msg(C, X[:, :256].T, ki)


# ---------------------------------------------------------------- 3. several tiles
def test_tiles_rectangular_ragged(ctx):
    """2 x 3 tiles (oz_res_tile's ti ntj + tj, k_oz_crt's t / ntj and t % ntj, the list's
    padding to 8 entries), 300 x 700 of them wanted: the rest of C keeps its sentinel."""
    rng = np.random.default_rng(30)
    a, b = rough(rng, 300, 128), rough(rng, 700, 120)
    got = run(ctx, store(a, 1, ld=301), store(b, 0, ld=128), rows=300, cols=700, K=128)
    check("2x3 tiles", got, ozr.Ref(a, b, K=128), rows=300, cols=700)


@pytest.mark.parametrize("lower128", [0, 1])
def test_tiles_triangular_from_tile_row_1(ctx, lower128):
    """tri with tile rows 1..3 of 4 (ti0 = 1: the residues and k_oz_crt's tile decoding count
    from tile (1, 0), C's row 0 is product row 256); lower128: the upper 128-tiles of the
    diagonal 256-tiles stay untouched."""
    rng = np.random.default_rng(31)
    a = rough(rng, 1000, 128)
    got = run(ctx, store(a, 0, ld=130), None, rows=1000, cols=1000, ti0=1, K=128, tri=1, lower128=lower128)
    check("tri ti0=1 lower128=%d" % lower128, got, ozr.Ref(a, K=128), rows=1000, cols=1000, ti0=1, tri=True,
          lower128=bool(lower128))


# ---------------------------------------------------------------- 4. the production forms
def _gen(rng, R, Kv, integer, mask=0, beta=53):
    return integers(rng, R, Kv, beta, mask) if integer else rough(rng, R, Kv)


@pytest.mark.parametrize("integer", [0, 1])
def test_form_lauum_packed(ctx, integer):
    """lauum_ozaki at np = 384: np2 = 512, the last 256-tiles run past np; k_oz_colexp, k_oz_split
    (vector and scalar paths), kbeg 1.  Above the diagonal the source holds garbage."""
    rng = np.random.default_rng(40 + integer)
    n = 384
    op = dense(_gen(rng, n, n, integer, mask=1), 1)          # op(r = column, k = row), k >= r
    src = nan_dropped(store(op, 0, ld=n + 6, garbage=dropped(rng, n, n, 1)), n, n, 1)
    ref = ozr.Ref(op, K=512)
    assert not integer or (not ref.ea.any() and (ref.Ai[:, :n] == op).all())
    got = run(ctx, src, None, rows=n, cols=n, packed=True)
    check("packed int=%d" % integer, got, ref, rows=n, cols=n, tri=True, lower128=True)


@pytest.mark.parametrize("integer", [0, 1])
def test_form_trtri_pair(ctx, integer):
    """The two products of oz_tri_pair_launches at Ra = 384, Rb = 128 (Pa = 512, Pb = 256 > Rb).
    T = L21 X11: A = L21's rows (transposed split), B = X11's columns with mask 1, kbeg 2.
    X21 = -X22 T: A = X22's rows with mask 2 (transposed), B = T's columns (ld Pb: the rows of
    the scratch block past Rb are never read), kend 1, alpha -1."""
    rng = np.random.default_rng(42 + integer)
    Ra, Rb, Pa, Pb = 384, 128, 512, 256
    l21 = _gen(rng, Rb, Ra, integer)
    x11 = _gen(rng, Ra, Ra, integer, mask=1)
    sb = nan_dropped(store(x11, 0, ld=Ra + 2, garbage=dropped(rng, Ra, Ra, 1)), Ra, Ra, 1)
    sb["mask"] = 1
    ref = ozr.Ref(l21, dense(x11, 1), K=Pa)
    assert not integer or (not ref.ea.any() and not ref.eb.any())
    got = run(ctx, store(l21, 1, ld=Rb + 4), sb, rows=Rb, cols=Ra, K=Pa, kbeg=2, extra=(Pb - Rb, 0))
    check("T = L21 X11 int=%d" % integer, got, ref, rows=Rb, cols=Ra)
    x22 = _gen(rng, Rb, Rb, integer, mask=2)
    t = _gen(rng, Ra, Rb, integer)                            # op(r = column of T, k = row of T)
    sa = nan_dropped(store(x22, 1, ld=Rb + 2, garbage=dropped(rng, Rb, Rb, 2)), Rb, Rb, 2)
    sa["mask"] = 2
    ref = ozr.Ref(dense(x22, 2), t, K=Pb)
    got = run(ctx, sa, store(t, 0, ld=Pb), rows=Rb, cols=Ra, K=Pb, kend=1, alpha=-1.0)
    check("X21 = -X22 T int=%d" % integer, got, ref, rows=Rb, cols=Ra, alpha=-1.0)


@pytest.mark.parametrize("integer", [0, 1])
def test_form_chol_schur(ctx, integer):
    """chol_schur at Rb = 384, Ra = 256: S = A22 - L21 L21^T, B is A (one set of planes, one
    exponent array), tri, lower128, k_oz_crt's accumulate mode into a non-zero A22."""
    rng = np.random.default_rng(44 + integer)
    Ra, Rb = 256, 384
    l21 = _gen(rng, Rb, Ra, integer)
    ref = ozr.Ref(l21, K=Ra)
    scale = np.ldexp(1.0, -(ref.ea[:, None] + ref.ea[None, :]).astype(np.int32)) * 2.0 ** 106
    a22 = rng.standard_normal((Rb, Rb)) * scale * np.exp2(-rng.integers(0, 60, size=(Rb, Rb)).astype(float))
    got = run(ctx, store(l21, 1, ld=Rb + 128), None, rows=Rb, cols=Rb, Cold=a22, K=Ra, tri=1, lower128=1, acc=1,
              alpha=-1.0)
    check("Schur int=%d" % integer, got, ref, rows=Rb, cols=Rb, tri=True, lower128=True, alpha=-1.0, Cold=a22)


@pytest.mark.parametrize("nmod", [8, 16])
@pytest.mark.parametrize("m", [1, 130, 257])
def test_form_posterior(ctx, m, nmod):
    """posterior_oz at np = 384 (np2 = 512): A = the rows of L^-1 (transposed split, mask 2,
    kend 1), B = m points (ragged R, Kv = np < Kp), 8 moduli (precision 32) and 16."""
    rng = np.random.default_rng(46 + m + nmod)
    n, K = 384, 512
    beta = ozr.consts(nmod, K)[0]
    integer = m == 130
    linv = _gen(rng, n, n, integer, mask=2, beta=beta)
    ks = _gen(rng, m, n, integer, beta=beta)
    sa = nan_dropped(store(linv, 1, ld=n, garbage=dropped(rng, n, n, 2)), n, n, 2)
    sa["mask"] = 2
    ref = ozr.Ref(dense(linv, 2), ks, K=K, nmod=nmod)
    assert not integer or (not ref.ea.any() and not ref.eb.any())
    got = run(ctx, sa, store(ks, 0, ld=n), rows=n, cols=m, K=K, kend=1, nmod=nmod, extra=(0, 2))
    check("posterior m=%d nmod=%d" % (m, nmod), got, ref, rows=n, cols=m)


@pytest.mark.parametrize("integer", [0, 1])
def test_form_dist_slab(ctx, integer):
    """oz_slab's product at P = 3, Kp = 384: op = X_r^T (rows = the columns of L^-1, k = the
    rank's local rows), kbeg 3: tile row ti starts at k = 128 floor(2 ti / 3).  The operand is
    zero exactly where that range skips and full elsewhere (the real X_r has more zeros, never
    fewer), so a range that started later or earlier than the zeros would show.  Tile rows
    1..5 of 6: 3 stages from k = 0 (ti = 1), 4 from 128 (ti = 2), 2 from 256 (ti = 3, 4: the
    short prologue) and none (ti = 5: K = 384 is where it starts)."""
    rng = np.random.default_rng(48 + integer)
    R, K, P = 1408, 384, 3
    x = _gen(rng, R, K, integer)
    kb = 128 * ((2 * (np.arange(R) // 256)) // P)
    x[np.arange(K)[None, :] < kb[:, None]] = 0.0
    if integer:   # (the row maximum back where the zeros took it; rows from 1280 on are zero)
        live = kb < K
        x[live, kb[live]] = 2.0 ** 52 + 5.0
    ref = ozr.Ref(x[256:], x, K=K)
    full = ozr.Ref.from_ints(np.concatenate([np.zeros((256, R), dtype=object), ref.Cint]),
                             np.concatenate([ozr.exponents(x[:256], ref.beta), ref.ea]), ref.eb, K=K)
    assert not integer or not full.ea.any()
    got = run(ctx, store(x, 0, ld=K + 128), None, rows=R, cols=R, ti0=1, K=K, kbeg=3, kdiv=P, tri=1, lower128=1)
    check("slab int=%d" % integer, got, full, rows=R, cols=R, ti0=1, tri=True, lower128=True)


# ---------------------------------------------------------------- 5. the split's scalar paths
def test_split_fallbacks_same_bits(ctx):
    """k_oz_split_rect's scalar paths: a source off the 16-byte grid (offset 1), an odd ld, the
    last row of an odd R in the transposed form, Kv no multiple of 8 -- the bits of the aligned
    run, which itself meets the reference."""
    rng = np.random.default_rng(50)
    K = 256
    a, b = rough(rng, 255, 250), rough(rng, 253, 251)
    ref = ozr.Ref(a, b, K=K)
    base = None
    for (ta, tb) in ((1, 0), (0, 1)):
        for (off, odd) in ((0, 0), (1, 0), (0, 1), (1, 1)):
            lda = (256 if ta else 250) + odd
            ldb = (254 if tb else 252) + odd
            got = run(ctx, store(a, ta, ld=lda, offset=off), store(b, tb, ld=ldb, offset=off), rows=255, cols=253, K=K)
            if base is None:
                check("aligned", got, ref, rows=255, cols=253)
                base = got
            what = "trans %d %d offset %d odd ld %d" % (ta, tb, off, odd)
            assert np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2]), what
            for l in (0, 1):
                assert np.array_equal(got[3][l], base[3][l]), what + ": residues of modulus %d" % l
            assert np.array_equal(got[0].view(np.uint64), base[0].view(np.uint64)), what


# ---------------------------------------------------------------- 6. NaN and Inf
@pytest.mark.parametrize("form", ["colexp", "rowexp", "rowexp_atomic"])
def test_nan_and_inf_rows(ctx, form):
    """A NaN in one row of A and an infinity in one row of B through k_oz_colexp, the wave
    reduction k_oz_rowexp<false> and the atomic max k_oz_rowexp<true> (the bad entry in the
    second of its two k blocks): those rows and columns of C are NaN, the exponents carry the
    marker, every other entry is as exact as without them."""
    rng = np.random.default_rng(60)
    if form == "colexp":
        n = 256
        op = dense(rough(rng, n, n), 1)
        op[7, 200] = np.nan
        op[130, 255] = -np.inf
        ref = ozr.Ref(op, K=n)
        got = run(ctx, store(op, 0, ld=n), None, rows=n, cols=n, packed=True)
        check(form, got, ref, rows=n, cols=n, tri=True, lower128=True)
        C = got[0]
        assert np.isnan(C[7, :8]).all() and np.isnan(C[130, :131]).all() and np.isnan(C[131:256, 130]).all()
    else:
        t = int(form == "rowexp_atomic")
        K = 320
        a, b = rough(rng, 256, K), rough(rng, 256, K)
        a[7, 300] = np.nan
        a[9, 3] = np.inf
        b[11, 290] = np.inf
        b[250, 0] = np.nan
        ref = ozr.Ref(a, b, K=K)
        got = run(ctx, store(a, t), store(b, t), rows=256, cols=256, K=K)
        check(form, got, ref, rows=256, cols=256)
        C = got[0][:256, :256]
        assert np.isnan(C[[7, 9]]).all() and np.isnan(C[:, [11, 250]]).all() and np.isnan(C).sum() == 4 * 256 - 4
    assert (ref.ea == ozr.EX_NAN).sum() == 2 and (got[1] == ozr.EX_NAN).sum() == 2


# ---------------------------------------------------------------- 7. the bound on K
K_MAX = 255 * 512   # 130560 <= OZ_MAX_K


def test_longest_sum_extreme_residues(ctx):
    """K = 130560, rows +-x constant along k, x in [2^52, 2^53) with residue -128 mod 256 and
    (m - 1) / 2 modulo the five largest odd moduli: |acc| = K 2^14 (m = 256) and K ((m - 1) / 2)^2
    with both signs, the largest |t| the fp32 reduction of k_oz_gemm's epilogue meets.
    C' = +-K x^2 in closed form."""
    M6 = 1
    for m in ozr.MODS[:6]:
        M6 *= m
    x = 0
    for m in ozr.MODS[:6]:
        want = -128 if m == 256 else (m - 1) // 2
        x += want * (M6 // m) * pow(M6 // m, -1, m)
    x %= M6
    x += ((2 ** 52 - x) // M6 + 1) * M6
    assert 2 ** 52 <= x < 2 ** 53 and M6 < 2 ** 48
    assert [ozr.centred(np.array([x], dtype=object), m)[0] for m in ozr.MODS[:6]] == [-128, 126, 125, 123, 120, 119]
    s = np.where(np.arange(256) % 3 == 0, -1, 1)
    a = np.empty((256, K_MAX))
    a[:] = (s * float(x))[:, None]
    Cint = np.array([[int(si) * int(sj) * K_MAX * x * x for sj in s] for si in s], dtype=object)
    ref = ozr.Ref.from_ints(Cint, np.zeros(256, int), np.zeros(256, int), K=K_MAX)
    assert ref.beta == 53 and 2 * K_MAX * x * x < ref.M
    got = run(ctx, store(a, 0), None, rows=256, cols=256, K=K_MAX, res_mods=(0, 1, 5))
    check("K = 130560, extreme residues", got, ref, rows=256, cols=256)


def test_longest_sum_random_rows(ctx):
    """K = 130560, random integer rows of period 512 along k: the exact product is 255 times the
    512-long one; tens of thousands of different t / m at large |t| through the epilogue's
    rintf(t / m)."""
    rng = np.random.default_rng(71)
    a0, b0 = integers(rng, 256, 512), integers(rng, 256, 512)
    ref0 = ozr.Ref(a0, b0, K=K_MAX)
    assert not ref0.ea.any() and not ref0.eb.any() and ref0.beta == 53
    ref = ozr.Ref.from_ints(ref0.Cint * 255, ref0.ea, ref0.eb, K=K_MAX)
    got = run(ctx, store(np.tile(a0, (1, 255)), 0), store(np.tile(b0, (1, 255)), 0), rows=256, cols=256, K=K_MAX,
              res_mods=(1, 15))
    check("K = 130560, random rows", got, ref, rows=256, cols=256)


# ---------------------------------------------------------------- 8. fewer moduli
@pytest.mark.parametrize("nmod", [8, 12])
def test_fewer_moduli(ctx, nmod):
    """beta follows oz_consts(nmod, K): the operands are truncated to it and the product of the
    truncated X' is exact."""
    rng = np.random.default_rng(80 + nmod)
    K = 256
    a, b = rough(rng, 256, K), rough(rng, 256, K)
    ref = ozr.Ref(a, b, K=K, nmod=nmod)
    got = run(ctx, store(a, 0), store(b, 1), rows=256, cols=256, K=K, nmod=nmod, res_mods=(0, nmod - 1))
    check("nmod=%d" % nmod, got, ref, rows=256, cols=256)


def test_bad_arguments_are_refused(ctx):
    """K that is no multiple of 64 (the kernel would drop the remainder), K past OZ_MAX_K, a
    window outside its source, C too small: GPE_ERR_ARG, nothing launched."""
    a = store(np.ones((256, 64)), 0)
    C = np.zeros(256 * 256)
    for kw in (dict(K=96), dict(K=ozr.OZ_MAX_K + 64), dict(K=64, nmod=5), dict(K=64, nmod=17), dict(K=64, kbeg=4),
               dict(K=64, ti0=1), dict(K=64, rows=257), dict(K=64, kdiv=0, kbeg=3)):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.test_oz_product(a, None, C=C, ldc=256, **dict(dict(rows=256, cols=256), **kw))
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.test_oz_product(dict(a, Kv=70), None, C=C, ldc=256, rows=256, cols=256, K=128)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.test_oz_product(a, None, C=C[:-1], ldc=256, rows=256, cols=256, K=64)
