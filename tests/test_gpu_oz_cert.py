"""The 15-moduli certificate of the int8 products (gpemu_ozaki.hpp: the row sums of the split
kernels, k_oz_cert, k_oz_gemm's early return for the sixteenth modulus, k_oz_crt_cert) through
gpe_test_oz_product_cert -- the production launch layer with a certificate, as the objective's
products run -- against tests/oz_product_ref.py: exact Python integers, and its bound with
M = M15 (the first 15 moduli) where 15 moduli were used, M16 where the certificate was refused.
The operands keep 53 bits either way.  Operand makers, sources and the entrywise check are those
of tests/test_gpu_oz_product.py.

Every product runs ten times: C byte for byte the same and nmod_used the same every time (the
sums are integer additions, so the flag cannot depend on the order of the atomics).

The objective case: n = 1100, d = 3 with the int8 thresholds at their floors (the context of
test_gpu_ozaki_tri.py::test_hard_points) and the certificates' own threshold at its floor
(GPEMU_OZAKI_CERT_MIN_NP=512; by default they start at n_pad 4096), beside
GPEMU_OZAKI_CERT=0 and GPEMU_OZAKI=0 contexts and one with the int8 floors alone.
"""
import threading

import numpy as np
import pytest

import oz_product_ref as ozr
import test_gpu_oz_product as base
import test_gpu_ozaki_chol as tc
import test_gpu_ozaki_tri as tri

pytestmark = pytest.mark.gpu

RUNS = 10
M15 = ozr.consts(15, 64)[1]


def run(ctx, a, b, *, rows, cols, ti0=0, Cold=None, extra=(5, 3), **kw):
    """base.run with a certificate, RUNS times (the residues of moduli 0 and 1 from the first
    two): ((C 2-d, exa, exb, {l: residues}), nmod_used)."""
    lr = rows - 256 * ti0
    ldc, cc = lr + extra[0], cols + extra[1]
    C0 = np.full((cc, ldc), base.SENT)
    if Cold is not None:
        C0[:cols, :lr] = Cold.T
    res, out = {}, None
    for rep in range(RUNS):
        l = rep if rep < 2 else None
        o = ctx.test_oz_product(a, b, C=C0.ravel(), ldc=ldc, rows=rows, cols=cols, ti0=ti0, res_mod=l, cert=True, **kw)
        if out is not None:
            assert np.array_equal(o["C"].view(np.uint64), out["C"].view(np.uint64)), "run %d: another C" % rep
            assert o["nmod_used"] == out["nmod_used"], "run %d: nmod_used %d after %d" % (rep, o["nmod_used"], out["nmod_used"])
        out = o
        if l is not None:
            res[l] = o["res"]
    assert out["nmod_used"] in (15, 16)
    return (out["C"].reshape(cc, ldc).T, out["exa"], out["exb"], res), out["nmod_used"]


def ref_for(ref, used):
    """ref (built with 16 moduli: 53-bit operands) with the modulus product of the moduli used."""
    if used == 15:
        ref.nmod, ref.M = 15, M15   # (rows_from keeps them; the operands' bits are already in Cint)
    return ref


def check(what, got, used, want_used, ref, **kw):
    assert used == want_used, "%s: nmod_used %d, expected %d" % (what, used, want_used)
    return base.check(what, got, ref_for(ref, used), **kw)


# ---------------------------------------------------------------- flat operands: next to wrap-around
def _flat(K):
    return np.full((256, K), 2.0 ** 53 - 1.0)


def _flat_ref(K):
    x = (1 << 53) - 1
    C = np.full((256, 256), K * x * x, dtype=object)
    return ozr.Ref.from_ints(C, np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64), K=K)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_flat_certified(ctx, sign):
    """Every entry of both operands (2^53 - 1) of one sign, K = 1280: y = 2^21 for every entry,
    s = 1280 2^42, s^2 = 2^104.64 < T15 = 2^104.76: certified, and |C'| = 1280 (2^53 - 1)^2 =
    2^116.32 sits just under M15 / 2 = 2^116.38 -- the case closest to wrap-around."""
    K = 1280
    assert 2 * K * ((1 << 53) - 1) ** 2 < M15 and (K << 42) ** 2 < 34409203667017820043519436844158
    got, used = run(ctx, base.store(sign * _flat(K), 0), base.store(_flat(K), 0), rows=256, cols=256, K=K)
    ref = _flat_ref(K)
    if sign < 0:
        ref.Cint = -ref.Cint
    check("flat K=1280 sign %+d" % sign, got, used, 15, ref, rows=256, cols=256)


def test_flat_refused(ctx):
    """The same with K = 1344: s^2 = 2^104.78 >= T15, and on 15 moduli the true C' (2^116.39 >
    M15 / 2) would wrap.  Refused: 16 moduli, the entries within the 16-moduli bound."""
    K = 1344
    assert 2 * K * ((1 << 53) - 1) ** 2 > M15 and (K << 42) ** 2 >= 34409203667017820043519436844158
    got, used = run(ctx, base.store(_flat(K), 0), base.store(_flat(K), 0), rows=256, cols=256, K=K)
    check("flat K=1344", got, used, 16, _flat_ref(K), rows=256, cols=256)


def _decaying(rng, R, K):
    """Benign rows: the maximum (53 bits after scaling) at one k, the rest falling off fast."""
    x = rng.standard_normal((R, K)) * np.exp2(-np.abs(np.arange(K)[None, :] - rng.integers(0, K, size=(R, 1))) / 2.0)
    return np.ldexp(x, rng.integers(-30, 31, size=(R, 1)).astype(np.int32))


@pytest.mark.parametrize("trans", [0, 1])
def test_one_bad_pair_refuses_the_product(ctx, trans):
    """Decaying operands except one flat row in A and one in B (K = 1344: that one entry of C'
    would wrap on 15 moduli).  The maxima over the rows decide: the whole product is refused."""
    rng = np.random.default_rng(70 + trans)
    K = 1344
    a, b = _decaying(rng, 256, K), _decaying(rng, 256, K)
    a[37] = 2.0 ** 53 - 1.0
    b[201] = -(2.0 ** 53 - 1.0)
    ref = ozr.Ref(a, b, K=K)
    assert 2 * abs(int(ref.Cint[37, 201])) > M15
    got, used = run(ctx, base.store(a, trans), base.store(b, trans), rows=256, cols=256, K=K)
    check("one bad pair trans %d" % trans, got, used, 16, ref, rows=256, cols=256)
    # without the two rows the same operands are certified
    a[37], b[201] = a[36], b[200]
    got, used = run(ctx, base.store(a, trans), base.store(b, trans), rows=256, cols=256, K=K)
    check("no bad pair trans %d" % trans, got, used, 15, ozr.Ref(a, b, K=K), rows=256, cols=256)


# ---------------------------------------------------------------- benign operands: 15 moduli
@pytest.mark.parametrize("ns", [1, 2, 4, 5, 9])
def test_one_tile_stage_counts(ctx, ns):
    rng = np.random.default_rng(200 + ns)
    K = 64 * ns
    a, b = base.rough(rng, 256, K), base.rough(rng, 256, K)
    got, used = run(ctx, base.store(a, 0), base.store(b, 1), rows=256, cols=256, K=K)
    check("ns=%d" % ns, got, used, 15, ozr.Ref(a, b, K=K), rows=256, cols=256)


def test_tiles_ragged_with_sentinel(ctx):
    """2 x 3 tiles, 300 x 700 wanted, integer operands at 53 bits: the rest of C keeps its sentinel."""
    rng = np.random.default_rng(210)
    a, b = base.integers(rng, 300, 128), base.integers(rng, 700, 120)
    got, used = run(ctx, base.store(a, 1, ld=301), base.store(b, 0, ld=128), rows=300, cols=700, K=128)
    check("2x3 tiles", got, used, 15, ozr.Ref(a, b, K=128), rows=300, cols=700)


@pytest.mark.parametrize("integer", [0, 1])
def test_form_chol_schur_accumulate(ctx, integer):
    """chol_schur's form (B is A, tri, lower128, accumulate into a non-zero A22, alpha -1)."""
    rng = np.random.default_rng(220 + integer)
    Ra, Rb = 256, 384
    l21 = base._gen(rng, Rb, Ra, integer)
    ref = ozr.Ref(l21, K=Ra)
    scale = np.ldexp(1.0, -(ref.ea[:, None] + ref.ea[None, :]).astype(np.int32)) * 2.0 ** 106
    a22 = rng.standard_normal((Rb, Rb)) * scale * np.exp2(-rng.integers(0, 60, size=(Rb, Rb)).astype(float))
    got, used = run(ctx, base.store(l21, 1, ld=Rb + 128), None, rows=Rb, cols=Rb, Cold=a22, K=Ra, tri=1, lower128=1,
                    acc=1, alpha=-1.0)
    check("Schur int=%d" % integer, got, used, 15, ref, rows=Rb, cols=Rb, tri=True, lower128=True, alpha=-1.0, Cold=a22)


def test_form_chol_nest_capped(ctx):
    """The nested split's trapezoid: the triangle capped at B's tile columns (B = A's first rows)."""
    rng = np.random.default_rng(230)
    Rb, K, cols = 640, 256, 256
    l = base.rough(rng, Rb, K)
    ref = ozr.Ref(l, l[:cols], K=K)
    a22 = rng.standard_normal((Rb, cols)) * np.ldexp(1.0, -(ref.ea[:, None] + ref.eb[None, :]).astype(np.int32)) * 2.0 ** 100
    src = base.store(l, 1, ld=Rb + 2)
    got, used = run(ctx, src, dict(src, R=cols), rows=Rb, cols=cols, Cold=a22, K=K, tri=1, lower128=1, acc=1, alpha=-1.0)
    check("trapezoid", got, used, 15, ref, rows=Rb, cols=cols, tri=True, lower128=True, alpha=-1.0, Cold=a22)


def test_form_lauum_packed(ctx):
    """lauum_ozaki at np = 384 (np2 = 512): k_oz_colexp and k_oz_split with the column sums."""
    rng = np.random.default_rng(240)
    n = 384
    op = base.dense(base.rough(rng, n, n), 1)
    src = base.nan_dropped(base.store(op, 0, ld=n + 6, garbage=base.dropped(rng, n, n, 1)), n, n, 1)
    got, used = run(ctx, src, None, rows=n, cols=n, packed=True)
    check("packed", got, used, 15, ozr.Ref(op, K=512), rows=n, cols=n, tri=True, lower128=True)


@pytest.mark.parametrize("integer", [0, 1])
def test_form_trtri_pair(ctx, integer):
    """The two products of oz_tri_pair_launches at Ra = 384, Rb = 128 (Pa = 512, Pb = 256 > Rb)."""
    rng = np.random.default_rng(250 + integer)
    Ra, Rb, Pa, Pb = 384, 128, 512, 256
    l21 = base._gen(rng, Rb, Ra, integer)
    x11 = base._gen(rng, Ra, Ra, integer, mask=1)
    sb = base.nan_dropped(base.store(x11, 0, ld=Ra + 2, garbage=base.dropped(rng, Ra, Ra, 1)), Ra, Ra, 1)
    sb["mask"] = 1
    got, used = run(ctx, base.store(l21, 1, ld=Rb + 4), sb, rows=Rb, cols=Ra, K=Pa, kbeg=2, extra=(Pb - Rb, 0))
    check("T = L21 X11 int=%d" % integer, got, used, 15, ozr.Ref(l21, base.dense(x11, 1), K=Pa), rows=Rb, cols=Ra)
    x22 = base._gen(rng, Rb, Rb, integer, mask=2)
    t = base._gen(rng, Ra, Rb, integer)
    sa = base.nan_dropped(base.store(x22, 1, ld=Rb + 2, garbage=base.dropped(rng, Rb, Rb, 2)), Rb, Rb, 2)
    sa["mask"] = 2
    got, used = run(ctx, sa, base.store(t, 0, ld=Pb), rows=Rb, cols=Ra, K=Pb, kend=1, alpha=-1.0)
    check("X21 = -X22 T int=%d" % integer, got, used, 15, ozr.Ref(base.dense(x22, 2), t, K=Pb), rows=Rb, cols=Ra,
          alpha=-1.0)


@pytest.mark.parametrize("m", [1, 130])
def test_form_posterior(ctx, m):
    """posterior_oz's form at np = 384 (np2 = 512), 16 moduli: transposed split with mask 2, kend 1."""
    rng = np.random.default_rng(260 + m)
    n, K = 384, 512
    integer = m == 130
    linv = base._gen(rng, n, n, integer, mask=2)
    ks = base._gen(rng, m, n, integer)
    sa = base.nan_dropped(base.store(linv, 1, ld=n, garbage=base.dropped(rng, n, n, 2)), n, n, 2)
    sa["mask"] = 2
    got, used = run(ctx, sa, base.store(ks, 0, ld=n), rows=n, cols=m, K=K, kend=1, extra=(0, 2))
    check("posterior m=%d" % m, got, used, 15, ozr.Ref(base.dense(linv, 2), ks, K=K), rows=n, cols=m)


def test_form_dist_slab(ctx):
    """oz_slab's form at P = 3, Kp = 384, tile rows 1..5 of 6 (kbeg 3, ti0 = 1)."""
    rng = np.random.default_rng(270)
    R, K, P = 1408, 384, 3
    x = base.rough(rng, R, K)
    kb = 128 * ((2 * (np.arange(R) // 256)) // P)
    x[np.arange(K)[None, :] < kb[:, None]] = 0.0
    ref = ozr.Ref(x[256:], x, K=K)
    full = ozr.Ref.from_ints(np.concatenate([np.zeros((256, R), dtype=object), ref.Cint]),
                             np.concatenate([ozr.exponents(x[:256], ref.beta), ref.ea]), ref.eb, K=K)
    got, used = run(ctx, base.store(x, 0, ld=K + 128), None, rows=R, cols=R, ti0=1, K=K, kbeg=3, kdiv=P, tri=1, lower128=1)
    check("slab", got, used, 15, full, rows=R, cols=R, ti0=1, tri=True, lower128=True)


# ---------------------------------------------------------------- NaN
@pytest.mark.parametrize("trans", [0, 1])
def test_nan_row(ctx, trans):
    """A NaN in one row of A: that row of C is NaN, every other entry has the bits of the run
    without it (the row's planes are zero and it adds at most its y = 1 terms to its own sum)."""
    rng = np.random.default_rng(280 + trans)
    K = 320
    a, b = base.rough(rng, 256, K), base.rough(rng, 256, K)
    clean, used0 = run(ctx, base.store(a, trans), base.store(b, trans), rows=256, cols=256, K=K)
    check("without NaN", clean, used0, 15, ozr.Ref(a, b, K=K), rows=256, cols=256)
    a[77, 300] = np.nan
    got, used = run(ctx, base.store(a, trans), base.store(b, trans), rows=256, cols=256, K=K)
    check("NaN row trans %d" % trans, got, used, 15, ozr.Ref(a, b, K=K), rows=256, cols=256)
    C, C0 = got[0], clean[0]
    assert np.isnan(C[77, :256]).all() and np.isnan(C).sum() == 256
    keep = np.ones(C.shape, bool)
    keep[77, :256] = False
    assert np.array_equal(C[keep].view(np.uint64), C0[keep].view(np.uint64))


def test_nan_column_packed(ctx):
    rng = np.random.default_rng(290)
    n = 256
    op = base.dense(base.rough(rng, n, n), 1)
    clean, used0 = run(ctx, base.store(op, 0, ld=n), None, rows=n, cols=n, packed=True)
    op[7, 200] = np.nan
    got, used = run(ctx, base.store(op, 0, ld=n), None, rows=n, cols=n, packed=True)
    check("packed NaN", got, used, 15, ozr.Ref(op, K=n), rows=n, cols=n, tri=True, lower128=True)
    assert used0 == 15
    C, C0 = got[0], clean[0]
    nan = np.isnan(C)
    w = base.region(n, n, tri=True, lower128=True, shape=C.shape)   # (the diagonal 128-tiles are written whole)
    i, j = np.arange(C.shape[0])[:, None], np.arange(C.shape[1])[None, :]
    assert np.array_equal(nan, w & ((i == 7) | (j == 7)))
    assert np.array_equal(C[~nan].view(np.uint64), C0[~nan].view(np.uint64))


def test_needs_16_moduli(ctx):
    a = base.store(np.ones((256, 64)), 0)
    with pytest.raises(RuntimeError, match="a certificate needs nmod = 16"):
        ctx.test_oz_product(a, None, C=np.zeros(256 * 256), ldc=256, rows=256, cols=256, K=64, nmod=15, cert=True)


# ---------------------------------------------------------------- the objective
N_OBJ, D_OBJ, CASE = 1100, 3, "gp4ml_fit"
FLOORS = dict(GPEMU_OZAKI_MIN_NP="512", GPEMU_OZAKI_TRI_MIN="512", GPEMU_OZAKI_CERT_MIN_NP="512")


def _objective(c):
    variant, kind, _, _ = tri.CASES[CASE]
    X, f, H, r, hp, nu_fixed, _ = tri._problem(N_OBJ, D_OBJ, CASE)
    c.set_data(X, f, H, r)
    return c.objective(variant, kind, hp, nu_fixed=nu_fixed)


def _dist(a, b, ref):
    """(gradient in units of scale, LLH relative) between two results, both in the oracle's units
    (ref: one scale for every distance that is compared with another)."""
    return (float(np.max(np.abs(a[1] - b[1]) / tri._scale(ref[1]))), abs(a[0] - b[0]) / max(1.0, abs(ref[0])))


def test_objective_certified():
    """n = 1100, d = 3 at the floors: the LAUUM and the two products of each of the two int8
    TRTRI pairs carry a certificate and all are certified; the result meets the oracle at the
    suite's tolerance; default and GPEMU_OZAKI_CERT=0 are no further apart than
    GPEMU_OZAKI_CERT=0 and the fp64 path; with the switch off no product carries a certificate."""
    ref = tri._problem(N_OBJ, D_OBJ, CASE)[6]
    on, off, fp64 = tri._context(**FLOORS), tri._context(**FLOORS, GPEMU_OZAKI_CERT="0"), tri._context(GPEMU_OZAKI="0")
    below = tri._context(GPEMU_OZAKI_MIN_NP="512", GPEMU_OZAKI_TRI_MIN="512")   # n_pad under the certificates' default start
    try:
        r_below, st_below = _objective(below), below.oz_cert_stats()
        below.close()
        r_on, r_off, r_64 = _objective(on), _objective(off), _objective(fp64)
        st_on, st_off, st_64 = on.oz_cert_stats(), off.oz_cert_stats(), fp64.oz_cert_stats()
        # truthful operation counts: with every product certified, 15 / 16 of the switch-off count
        ops = []
        for c in (on, off):
            c.set_profiling(True)
            try:
                again = _objective(c)
                ops.append(c.ozaki_stats())
            finally:
                c.set_profiling(False)
            assert again[0] == (r_on if c is on else r_off)[0] and np.array_equal(again[1], (r_on if c is on else r_off)[1])
    finally:
        for c in (on, off, fp64):
            c.close()
    print("cert stats: default %s, CERT=0 %s, fp64 %s" % (st_on, st_off, st_64))
    assert st_on["products"] == 5 and st_on["certified"] == st_on["products"], st_on
    assert st_off == dict(products=0, certified=0) and st_64 == dict(products=0, certified=0)
    # below the certificates' threshold: none, and the switch-off result bit for bit
    assert st_below == dict(products=0, certified=0), st_below
    assert r_below[0] == r_off[0] and r_below[2] == r_off[2] and np.array_equal(r_below[1], r_off[1])
    assert ops[0]["launches"] == ops[1]["launches"] == 5
    assert ops[0]["int8_ops"] * 16 == ops[1]["int8_ops"] * 15, ops
    for what, res in (("default", r_on), ("CERT=0", r_off)):
        err = np.max(np.abs(res[1] - ref[1]) / tri._scale(ref[1]))
        print(f"{what}: grad vs oracle {err:.2e}, llh vs oracle {abs(res[0] - ref[0]):.2e}")
        assert err <= 1e-7, (err, res[1], ref[1])
        assert abs(res[0] - ref[0]) <= 1e-10 * max(1.0, abs(ref[0])), (res[0], ref[0])
        assert abs(res[2] - ref[2]) <= 1e-10 * abs(ref[2]), (res[2], ref[2])
    d_cert, d_int8 = _dist(r_on, r_off, ref), _dist(r_off, r_64, ref)
    print(f"default vs CERT=0: grad {d_cert[0]:.2e} llh {d_cert[1]:.2e}; CERT=0 vs fp64: grad {d_int8[0]:.2e} llh {d_int8[1]:.2e}")
    assert d_cert[0] <= d_int8[0] and d_cert[1] <= d_int8[1], (d_cert, d_int8)


def test_two_contexts_in_flight_repeat():
    """Two default contexts evaluating at once, three times each: byte-identical repeats and the
    same certificates."""
    cs = [tri._context(**FLOORS) for _ in range(2)]
    tri._problem(N_OBJ, D_OBJ, CASE)
    out = [[], []]
    err = []

    def work(i):
        try:
            for _ in range(3):
                res = _objective(cs[i])
                out[i].append((res, cs[i].oz_cert_stats()))
        except Exception as e:   # (reported below: an exception in a thread is otherwise lost)
            err.append(e)

    try:
        ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        for c in cs:
            c.close()
    assert not err, err
    first = out[0][0]
    for runs in out:
        assert len(runs) == 3
        for res, st in runs:
            assert st == first[1] and st["certified"] == st["products"] == 5, st
            assert res[0] == first[0][0] and res[2] == first[0][2]
            assert np.array_equal(res[1].view(np.uint64), first[0][1].view(np.uint64))


# ---------------------------------------------------------------- the split and nested Cholesky
T15 = 34409203667017820043519436844158
NEST = dict(tc.FLOORS, GPEMU_OZAKI_CHOL_NEST_MIN="256", GPEMU_OZAKI_CERT_MIN_NP="512")


def test_objective_split_nested_certified():
    """n = 2900, d = 20 (NB 23, h 16, q 8) with every int8 threshold at its floor: the trapezoid and
    S of the split sweep (chol_schur at q and at h, accumulate mode), two products for each of the
    five int8 TRTRI pairs and the LAUUM, 13 products, all with a certificate and all certified.  The
    top pair's T = L21 X11 takes L21's planes and sums from S (the l21_done path): its A is S's A,
    the same integers; no product's maxima are zero (a sum array left unwritten would certify
    everything).  LLH, gradient and sigma^2 against the oracle at the suite's tolerances; default
    against GPEMU_OZAKI_CERT=0 no further than GPEMU_OZAKI_CERT=0 against the fp64 path; the
    operation count 15 / 16 of the switch-off context's."""
    n, case = 2900, "gp4ml_fit"
    ref = tc._problem(n, case)[6]
    on, off, fp64 = tc._context(**NEST), tc._context(**NEST, GPEMU_OZAKI_CERT="0"), tc._context(GPEMU_OZAKI="0")
    try:
        r_on = tc._grad(on, n, case)
        st, sums = on.oz_cert_stats(), on.oz_cert_sums()
        r_off, r_64 = tc._grad(off, n, case), tc._grad(fp64, n, case)
        ops = []
        for c in (on, off):
            c.set_profiling(True)
            try:
                again = tc._grad(c, n, case)
                ops.append(c.ozaki_stats())
            finally:
                c.set_profiling(False)
            first = r_on if c is on else r_off
            assert again[0] == first[0] and np.array_equal(again[1], first[1])
    finally:
        for c in (on, off, fp64):
            c.close()
    print("cert stats", st, "log2(A B):", ["%.1f" % np.log2(float(a) * float(b)) for a, b in sums])
    assert st == dict(products=13, certified=13), st
    assert len(sums) == 13 and all(a > 0 and b > 0 and a * b < T15 for a, b in sums), sums
    # the trapezoid, S and the LAUUM multiply an operand by itself (A = B); the ten TRTRI products do
    # not, and the top pair's T has S's A
    own = [a for a, b in sums if a == b]
    assert len(own) >= 3, sums
    assert any(a != b and a in own for a, b in sums), ("no T product with S's L21 sums", sums)
    assert ops[0]["launches"] == ops[1]["launches"] == 13
    assert ops[0]["int8_ops"] * 16 == ops[1]["int8_ops"] * 15, ops
    for what, res in (("default", r_on), ("CERT=0", r_off)):
        tc._against(n, case, res, r_64, what)
    d_cert, d_int8 = _dist(r_on, r_off, ref), _dist(r_off, r_64, ref)
    print(f"default vs CERT=0: grad {d_cert[0]:.2e} llh {d_cert[1]:.2e}; CERT=0 vs fp64: grad {d_int8[0]:.2e} llh {d_int8[1]:.2e}")
    assert d_cert[0] <= d_int8[0] and d_cert[1] <= d_int8[1], (d_cert, d_int8)
