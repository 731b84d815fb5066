"""Reference for one launch of the grouped fp64 GEMM (k_gemm, csrc/gpemu_kernels.hpp) as the
test hook gpe_test_gemm_group runs it: plain NumPy, no GPU, no longdouble.  Checked on the
CPU by tests/test_gemm_group_ref_host.py; used on the GPU by tests/test_gpu_gemm_group.py.

A problem is the dict Context.test_gemm_group takes: a, b, c = (buffer, element offset, leading
dimension), mt, nt, K, flags, kti_mul, kti_off, alpha, beta.  With kind 0..3 (1, 2: opA is
K-contiguous; 2, 3: opB is) and 128 x 128 tiles (ti, tj):

    opA(m, k) = A[off + k + m lda]  (K-contiguous)   or  A[off + m + k lda]
    opB(k, n) = B[off + k + n ldb]  (K-contiguous)   or  B[off + n + k ldb]
    C(m, n)   = C[off + m + n ldc]
    C = alpha sum_{k in [kbeg, kend)} opA(m, k) opB(k, n) + beta C0      (tile by tile)

Exactness.  Operand entries are j 2^-20 with integer |j| < 2^20 (GRID_BITS), so a product
lies on the 2^-40 grid and is below 1 in magnitude; a sum of K <= 2048 (K_MAX) of them, in
any order and over any subset, is below 2^11 and a multiple of 2^-40: at most 51 significant
bits, exact in fp64.  That covers the MFMA's accumulation order, the split-K partials and
their final sum.  The reference sum is an int64 matrix product of the j (K 2^40 < 2^63: no
overflow).  C0 lies on the same 2^-20 grid with |C0| < 2^10, and alpha, beta are signed
powers of two such that alpha S + beta C0 -- and (beta / alpha) C0 + S, what the kernel
accumulates before it scales by alpha -- fit 53 bits (exact_scaling asserts it).  Such cases
are compared bit for bit.

Rounding bound (general alpha, beta; operands still on the grid, S exact):

    |C - (alpha S + beta C0)| <= (K_tile + 6) 2^-53 (|alpha| (|A| |B|) + |beta| |C0|)

entrywise, K_tile the tile's own K range: one rounding per accumulation step once
(beta / alpha) C0 is in the accumulator, two for that scaling (the quotient, the product),
one for the scaling by alpha, and the reference's own three (two products, one sum).  Every
intermediate is bounded by the bracket (divided by |alpha| inside the kernel), so each
rounding is at most 2^-53 of it, to first order.  Derived, not measured.
"""
import numpy as np

TILE = 128
GK = 16
G_CLOWER, G_KBEG_TI, G_KEND_TI = 1, 2, 4
GRID_BITS = 20          # operand entries: j 2^-20, |j| < 2^20
C_BITS = 30             # C0 entries: j 2^-20, |j| < 2^30 (|C0| < 2^10)
K_MAX = 2048
UNIT = 2.0 ** -GRID_BITS


def sentinel(buf):
    """What buffer `buf` holds where nothing belongs: a large value on the grid, one per buffer."""
    return 4099.0 + 2.0 * buf + 3 * UNIT


# ---------------------------------------------------------------- the documented rules
def k_range(p, ti):
    """[kbeg, kend) of tile row ti; kend <= kbeg: empty (C = beta C0)."""
    flags = p.get("flags", 0)
    kbeg = TILE * ti if flags & G_KBEG_TI else 0
    kend = p["K"]
    if flags & G_KEND_TI:
        kend = min(kend, TILE * (ti * p.get("kti_mul", 1) + p.get("kti_off", 0) + 1))
    return kbeg, kend


def tiles(p):
    """The (ti, tj) a problem covers: all mt x nt, or tj <= ti under G_CLOWER (nt is not read)."""
    if p.get("flags", 0) & G_CLOWER:
        return [(ti, tj) for ti in range(p["mt"]) for tj in range(ti + 1)]
    return [(ti, tj) for ti in range(p["mt"]) for tj in range(p["nt"])]


def a_index(p, kind, ti, k0, k1):
    """Buffer indices of opA(m, k), m in tile row ti, k in [k0, k1): shape (128, k1 - k0)."""
    _, off, ld = p["a"]
    m = (TILE * ti + np.arange(TILE, dtype=np.int64))[:, None]
    k = np.arange(k0, k1, dtype=np.int64)[None, :]
    return off + k + m * ld if kind in (1, 2) else off + m + k * ld


def b_index(p, kind, tj, k0, k1):
    """Buffer indices of opB(k, n), n in tile column tj: shape (k1 - k0, 128)."""
    _, off, ld = p["b"]
    n = (TILE * tj + np.arange(TILE, dtype=np.int64))[None, :]
    k = np.arange(k0, k1, dtype=np.int64)[:, None]
    return off + k + n * ld if kind in (2, 3) else off + n + k * ld


def c_index(p, ti, tj):
    _, off, ld = p["c"]
    m = (TILE * ti + np.arange(TILE, dtype=np.int64))[:, None]
    n = (TILE * tj + np.arange(TILE, dtype=np.int64))[None, :]
    return off + m + n * ld


def footprint(lens, probs, kind):
    """Per buffer, boolean maps of what the launch reads as an operand, reads as C (beta != 0)
    and may write: exactly the C tiles the problems cover.  Asserts what the hook leaves to
    the test: every window inside its buffer, no element written twice, none both written
    and read as an operand."""
    opnd = [np.zeros(n, bool) for n in lens]
    cin = [np.zeros(n, bool) for n in lens]
    wr = [np.zeros(n, bool) for n in lens]
    for p in probs:
        for ti, tj in tiles(p):
            k0, k1 = k_range(p, ti)
            if k1 > k0:
                ia, ib = a_index(p, kind, ti, k0, k1), b_index(p, kind, tj, k0, k1)
                assert ia.max() < lens[p["a"][0]] and ib.max() < lens[p["b"][0]], "operand window leaves its buffer"
                opnd[p["a"][0]][ia] = True
                opnd[p["b"][0]][ib] = True
            ic = c_index(p, ti, tj)
            assert ic.max() < lens[p["c"][0]], "C window leaves its buffer"
            assert not wr[p["c"][0]][ic].any(), "a C element is written twice"
            wr[p["c"][0]][ic] = True
            if p.get("beta", 0.0) != 0.0:
                cin[p["c"][0]][ic] = True
    for o, w in zip(opnd, wr):
        assert not (o & w).any(), "an element is both an operand and written"
    return opnd, cin, wr


# ---------------------------------------------------------------- inputs
def fill(lens, probs, kind, rng, poison=False):
    """Input buffers for a launch: operands read get grid values below 1, C read (beta != 0)
    grid values below 2^10, C only written (beta == 0) NaN, everything else the buffer's
    sentinel -- or, with poison, NaN: operand entries outside every tile's K range, the gaps
    between windows and the padding of a leading dimension then all hold NaN."""
    opnd, cin, wr = footprint(lens, probs, kind)
    bufs = []
    for i, n in enumerate(lens):
        b = np.full(n, np.nan if poison else sentinel(i))
        b[opnd[i]] = rng.integers(-(1 << GRID_BITS) + 1, 1 << GRID_BITS, size=int(opnd[i].sum())) * UNIT
        b[cin[i]] = rng.integers(-(1 << C_BITS) + 1, 1 << C_BITS, size=int(cin[i].sum())) * UNIT
        b[wr[i] & ~cin[i]] = np.nan
        bufs.append(b)
    return bufs


def to_grid_int(x, bits):
    """The integers j of x = j 2^-20; asserts the module's premise on what it reads."""
    j = x * float(1 << GRID_BITS)
    assert np.all(np.isfinite(j)) and np.all(j == np.rint(j)), "a value that is read is off the 2^-20 grid"
    assert np.all(np.abs(j) < float(1 << bits)), "a value that is read is too large"
    return j.astype(np.int64)


def is_pow2(x):
    return x != 0.0 and np.isfinite(x) and abs(np.frexp(x)[0]) == 0.5


def exact_scaling(alpha, beta, K):
    """True when alpha S + beta C0 is exact for every S, C0 of the module's ranges, in the
    reference's order and in the kernel's ((beta / alpha) C0 + S, then times alpha)."""
    if not is_pow2(alpha) or (beta != 0.0 and not is_pow2(beta)):
        return False
    assert K <= K_MAX
    grid = abs(alpha) * 2.0 ** (-2 * GRID_BITS)
    top = abs(alpha) * K
    if beta != 0.0:
        grid = min(grid, abs(beta) * UNIT)
        top += abs(beta) * 2.0 ** (C_BITS - GRID_BITS)
    assert top / grid <= 2.0 ** 53, "alpha, beta leave the exact range"
    assert 2.0 ** -500 < grid and top < 2.0 ** 500
    return True


# ---------------------------------------------------------------- the reference
def expected(bufs, probs, kind, drop_stage=None):
    """(want, written, bound): the buffers after the launch, the map of elements that may
    have changed, and per element the rounding bound (0 where the result is exact; NaN
    outside written).  drop_stage = (p, ti, tj): that tile loses its last K stage (a planted
    error for the comparator's own test)."""
    lens = [b.size for b in bufs]
    _, _, written = footprint(lens, probs, kind)
    want = [b.copy() for b in bufs]
    bound = [np.full(n, np.nan) for n in lens]
    for ip, p in enumerate(probs):
        alpha, beta, K = p.get("alpha", 1.0), p.get("beta", 0.0), p["K"]
        assert K % GK == 0 and 0 < K <= K_MAX and alpha != 0.0
        exact = exact_scaling(alpha, beta, K)
        A, B, C = bufs[p["a"][0]], bufs[p["b"][0]], bufs[p["c"][0]]
        for ti, tj in tiles(p):
            k0, k1 = k_range(p, ti)
            if drop_stage == (ip, ti, tj):
                k1 -= GK
            ic = c_index(p, ti, tj)
            S = np.zeros((TILE, TILE))
            Sabs = np.zeros((TILE, TILE))
            if k1 > k0:
                ja = to_grid_int(A[a_index(p, kind, ti, k0, k1)], GRID_BITS)
                jb = to_grid_int(B[b_index(p, kind, tj, k0, k1)], GRID_BITS)
                S = (ja @ jb).astype(np.float64) * UNIT * UNIT          # |sum| < 2^51: exact
                if not exact:
                    Sabs = (np.abs(ja) @ np.abs(jb)).astype(np.float64) * UNIT * UNIT
            if beta != 0.0:
                c0 = C[ic]
                to_grid_int(c0, C_BITS)
                want[p["c"][0]][ic] = alpha * S + beta * c0
            else:
                c0 = np.zeros((TILE, TILE))
                want[p["c"][0]][ic] = alpha * S
            bound[p["c"][0]][ic] = 0.0 if exact else \
                (max(k1 - k0, 0) + 6) * 2.0 ** -53 * (abs(alpha) * Sabs + abs(beta) * np.abs(c0))
    return want, written, bound


def locate(probs, buf, idx):
    """(problem, ti, tj, m, n) of element idx of buffer buf, if a covered C tile holds it."""
    for ip, p in enumerate(probs):
        if p["c"][0] != buf:
            continue
        for ti, tj in tiles(p):
            hit = np.argwhere(c_index(p, ti, tj) == idx)
            if hit.size:
                return "problem %d tile (%d, %d) entry (%d, %d)" % (ip, ti, tj, hit[0][0], hit[0][1])
    return "outside every C tile"


def compare(got, bufs, probs, kind, ref=None):
    """Assert that `got` is what the launch may leave of the inputs `bufs`: every element
    outside the covered C tiles bit for bit as it was, the exact ones equal, the others within
    their bound.  Returns the largest |error| / bound seen (0.0 if every case was exact)."""
    want, written, bound = ref if ref is not None else expected(bufs, probs, kind)
    worst = 0.0
    for i, (g, b0, w, wr, bd) in enumerate(zip(got, bufs, want, written, bound)):
        assert g.shape == b0.shape
        same = g.view(np.uint64) == b0.view(np.uint64)
        bad = np.flatnonzero(~wr & ~same)
        assert bad.size == 0, "buffer %d element %d changed (%r -> %r): %s; %d such" % (
            i, bad[0], b0[bad[0]], g[bad[0]], locate(probs, i, bad[0]), bad.size)
        gw, ww, bw = g[wr], w[wr], bd[wr]
        err = np.abs(gw - ww)
        ok = np.isfinite(gw) & (err <= bw)          # bound 0: equality
        if not ok.all():
            k = np.flatnonzero(wr)[np.flatnonzero(~ok)[0]]
            raise AssertionError("buffer %d element %d: got %r, want %r (bound %.3g): %s; %d such" % (
                i, k, g[k], w[k], bd[k], locate(probs, i, k), int((~ok).sum())))
        nz = bw > 0
        if nz.any():
            worst = max(worst, float(np.max(err[nz] / bw[nz])))
    return worst


# ---------------------------------------------------------------- layout helpers
class Layout:
    """Buffers as lists of column-major blocks: block() reserves `outer` columns of `inner`
    contiguous elements with a leading dimension inner + pad, after a gap; all even."""

    def __init__(self, nbuf=3):
        self.lens = [0] * nbuf

    def block(self, buf, inner, outer, pad=0, gap=0):
        assert pad % 2 == 0 and gap % 2 == 0 and inner % 2 == 0
        off, ld = self.lens[buf] + gap, inner + pad
        self.lens[buf] = off + ld * outer + 2
        return (buf, off, ld)


def problem(lay, kind, mt, nt, K, *, bufs=(0, 1, 2), pad=0, gap=0, **kw):
    """One problem with windows of its own: A in buffer bufs[0], B in bufs[1], C in bufs[2],
    each with `pad` extra leading dimension and `gap` elements in front."""
    M, N = TILE * mt, TILE * nt
    a = lay.block(bufs[0], K, M, pad, gap) if kind in (1, 2) else lay.block(bufs[0], M, K, pad, gap)
    b = lay.block(bufs[1], K, N, pad, gap) if kind in (2, 3) else lay.block(bufs[1], N, K, pad, gap)
    c = lay.block(bufs[2], M, N, pad, gap)
    return dict(a=a, b=b, c=c, mt=mt, nt=nt, K=K, **kw)
