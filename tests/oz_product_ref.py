"""Exact reference of one int8 product (gpemu_ozaki.hpp) in numpy and Python integers, and the
entrywise comparison with what the kernels return (tests/test_gpu_oz_product.py; checked on
the CPU by tests/test_oz_product_ref_host.py).

The product, as the kernels define it: per row r of an operand op (R x K, zero where masked),
    e_r = beta - 1 - ilogb(max_k |op(r, k)|)   (0 for a zero row, EX_NAN for a non-finite one)
    X'  = rint(ldexp(op, e_r))                  (both exact in fp64; |X'| <= 2^beta)
    C'  = A' B'^T                               (exact integers)
    C   = alpha C' 2^-(e_i + e_j) (+ C_old)     (one rounding would be the ideal)

The bound of compare(), from k_oz_crt's arithmetic, with
P = alpha C' 2^-(e_i + e_j) the exact product entry:

    |C - P| <= 4 2^-53 |P| + 2^-78 M |alpha| 2^-(e_i + e_j)        (+ 2^-53 |C| with acc)

  - k_oz_crt forms the centred fraction v of sum_l c_l y_l / m_l = C' / M (mod 1) as
    (shi - rint(shi)) + slo.  shi = sum c_l rhi_l is exact (multiples of 2^-41 below 2^11) and
    so is its centred fractional part.  slo = sum c_l rlo_l: each rlo_l < 2^-41 is stored
    rounded (relative 2^-53, absolute <= 2^-94; times |c_l| <= 128, 16 of them: 2^-83) and
    each of the 16 fma roundings is at most half an ulp of |slo| < 16 128 2^-41 = 2^-30, i.e.
    2^-84, together 2^-80: |slo - exact| < 2^-79.8.  The sum frac + slo rounds once:
    v = (C' / M)(1 + d1) + a, |d1| <= 2^-53, |a| < 2^-79.8 (1 + 2^-53).
  - C = v s, s = alpha Md 2^-(e_i + e_j) with Md the fp64 product of the moduli: one rounding
    of the product (d2), and Md's own error |Md / M - 1| <= 2^-52 (md_rel_error() gives the
    actual figure for every nmod; the host test asserts it), exact for alpha a power of two.
    So C = P (1 + d1)(1 + d2)(1 + dM) + a M alpha 2^-(..) (1 + ..): the relative part is
    below (1 + 1 + 2) 2^-53 + O(2^-106) -- the 4 -- and the absolute part below
    2^-79.8 (1 + 2^-50) M |alpha| 2^-(..) < 2^-78 M |alpha| 2^-(..) with a factor 3 to spare.
  - acc: C = fma(v, s, C_old) rounds v s + C_old once instead of v s: the product's rounding
    d2 is replaced by one of the result, 2^-53 |C| (the bound keeps both).
alpha is a power of two (+-1 in every production call), so P is a dyadic rational: the
reference side rounds nothing.
"""
import math
from fractions import Fraction

import numpy as np

MODS = (256, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193, 191)
EX_NAN = -(1 << 20)
OZ_MAX_K = (1 << 17) - 128
T = 256


def consts(nmod, K):
    """(beta, M): oz_consts' operand bits for sums of length K and the exact modulus product."""
    log2M = 0.0
    M = 1
    for m in MODS[:nmod]:
        log2M += math.log2(float(m))
        M *= m
    beta = min(53, int(math.floor((log2M - 1.0 - math.log2(float(K)) - 1e-9) / 2.0)))
    return beta, M


def md_rel_error(nmod):
    """|Md / M - 1| of oz_consts' Md (the moduli multiplied in fp64 in order), exactly."""
    Md = 1.0
    for m in MODS[:nmod]:
        Md *= float(m)
    M = consts(nmod, 64)[1]
    return abs(Fraction(Md) / M - 1)


def pad(n):
    return (n + T - 1) // T * T


def masked(op, mask):
    """op (R x Kv) with the entries the mask drops set to zero: k < r (1), k > r (2)."""
    R, Kv = op.shape
    r, k = np.arange(R)[:, None], np.arange(Kv)[None, :]
    keep = k >= r if mask == 1 else (k <= r if mask == 2 else np.ones((R, Kv), bool))
    return np.where(keep, op, 0.0)


def exponents(op, beta):
    """e_r of every row of op (R x K), int64; EX_NAN for a row holding a NaN or an infinity."""
    op = np.asarray(op, dtype=np.float64)
    ex = np.zeros(op.shape[0], dtype=np.int64)
    if op.shape[1] == 0:
        return ex
    bad = ~np.isfinite(op).all(axis=1)
    mx = np.max(np.abs(np.where(np.isfinite(op), op, 0.0)), axis=1)
    nz = mx > 0.0
    ilogb = np.frexp(mx)[1].astype(np.int64) - 1   # mx = f 2^e, f in [0.5, 1)
    ex[nz] = beta - 1 - ilogb[nz]
    ex[bad] = EX_NAN
    return ex


def int_operand(op, ex):
    """X' = rint(ldexp(op, e)) as integer-valued fp64 (zero rows where e is EX_NAN)."""
    op = np.asarray(op, dtype=np.float64)
    ok = ex != EX_NAN
    out = np.zeros_like(op)
    out[ok] = np.rint(np.ldexp(op[ok], ex[ok][:, None].astype(np.int32)))
    return out


def _limbs(x):
    """Three signed 18-bit limbs of integer-valued x (|x| <= 2^53): x = l0 + l1 2^18 + l2 2^36,
    l0, l1 in [-2^17, 2^17), |l2| <= 2^17 + 1."""
    v = x.astype(np.int64)
    out = []
    for _ in range(2):
        lo = ((v + (1 << 17)) & ((1 << 18) - 1)) - (1 << 17)
        out.append(lo)
        v = (v - lo) >> 18
    out.append(v)
    return out


def exact_product(Ai, Bi, use_int64=False):
    """C' = Ai Bi^T for integer-valued fp64 operands (|.| <= 2^53, K <= 2^17 columns) as an
    object array of Python ints.  Nine limb products: every entry of one is a sum of K terms
    below (2^17 + 1)^2, so below 2^52 -- exact in int64, and exact in an fp64 matrix multiply
    in any summation order (every partial sum is an integer below 2^53), which is the route
    taken unless use_int64 (the host test holds the two against each other)."""
    assert Ai.shape[1] == Bi.shape[1] and Ai.shape[1] <= (1 << 17)
    la, lb = _limbs(Ai), _limbs(Bi)
    if not use_int64:
        la = [l.astype(np.float64) for l in la]
        lb = [l.astype(np.float64) for l in lb]
    S = [None] * 5   # S[s] = sum of the limb products with a + b = s: below 3 2^52 < 2^63
    for a in range(3):
        for b in range(3):
            P = (la[a] @ lb[b].T).astype(np.int64)
            S[a + b] = P if S[a + b] is None else S[a + b] + P
    C = S[4].astype(object)
    for s in (3, 2, 1, 0):
        C = C * (1 << 18) + S[s].astype(object)
    return C


def centred(C, m):
    """The centred residue of the integers C modulo m, in [-(m // 2), (m - 1) // 2]."""
    r = (np.asarray(C, dtype=object) % m).astype(np.int64)
    return np.where(r >= (m + 1) // 2, r - m, r)


class Ref:
    """The exact product of two operands (dense, masked, R x Kv each, Kv <= K; b None: B is A)."""

    def __init__(self, a, b=None, *, K, nmod=16):
        self.K, self.nmod = K, nmod
        self.beta, self.M = consts(nmod, K)
        a = self._padded(a, K)
        self.ea = exponents(a, self.beta)
        self.Ai = int_operand(a, self.ea)
        if b is None:
            self.eb, self.Bi = self.ea, self.Ai
        else:
            b = self._padded(b, K)
            self.eb = exponents(b, self.beta)
            self.Bi = int_operand(b, self.eb)
        self.Cint = exact_product(self.Ai, self.Bi)
        self.nan = (self.ea == EX_NAN)[:, None] | (self.eb == EX_NAN)[None, :]

    @staticmethod
    def _padded(x, K):
        x = np.asarray(x, dtype=np.float64)
        assert x.shape[1] <= K
        return np.pad(x, ((0, 0), (0, K - x.shape[1])))

    @classmethod
    def from_ints(cls, Cint, ea, eb, *, K, nmod=16):
        """A reference whose exact C' is known in closed form (object array of Python ints)."""
        self = cls.__new__(cls)
        self.K, self.nmod = K, nmod
        self.beta, self.M = consts(nmod, K)
        self.ea, self.eb = np.asarray(ea, dtype=np.int64), np.asarray(eb, dtype=np.int64)
        self.Ai = self.Bi = None
        self.Cint = Cint
        self.nan = (self.ea == EX_NAN)[:, None] | (self.eb == EX_NAN)[None, :]
        return self

    def rows_from(self, r0):
        """The same product seen from row r0 on (a product that starts at tile row ti0)."""
        return Ref.from_ints(self.Cint[r0:], self.ea[r0:], self.eb, K=self.K, nmod=self.nmod)

    def residues(self, l):
        return centred(self.Cint, MODS[l])

    def padded_ex(self, which):
        e = self.ea if which == "a" else self.eb
        out = np.zeros(pad(e.size), dtype=np.int64)
        out[:e.size] = e
        return out


def _pow2(alpha):
    f, _ = math.frexp(abs(alpha))
    return f == 0.5


def compare(C, ref, alpha=1.0, Cold=None, where=None):
    """Check C (rows x cols, fp64) entrywise against ref's exact product within the bound of
    the module docstring; Cold: the accumulate form's old C.  where: boolean array of the
    entries to check (default all).  Returns (bad, worst): the boolean array of entries
    outside the bound (a NaN where a number is due, or the reverse, included) and the largest
    error / bound ratio seen (float, for printing; without Cold it is the fp64 estimate, which
    includes up to 2^-53 |P| of its own rounding of C').  The decision is exact: entries whose fp64
    estimate is within 2^-30 of the bound either way are decided in exact integers."""
    assert _pow2(alpha)
    C = np.asarray(C, dtype=np.float64)
    rows, cols = C.shape
    Cint = ref.Cint[:rows, :cols]
    nan = ref.nan[:rows, :cols]
    if where is None:
        where = np.ones((rows, cols), bool)
    ea = np.where(ref.ea == EX_NAN, 0, ref.ea)[:rows]
    eb = np.where(ref.eb == EX_NAN, 0, ref.eb)[:cols]
    esum = ea[:, None] + eb[None, :]
    bad = where & (np.isnan(C) != nan)
    bad |= where & ~nan & ~np.isfinite(C)
    todo = where & ~nan & np.isfinite(C)
    worst = 0.0
    M = ref.M

    SH = 1280   # everything times 2^SH is an integer (fp64 numbers are multiples of 2^-1074)

    def scaled(f):
        n, d = float(f).as_integer_ratio()
        return n << (SH - d.bit_length() + 1)

    sgn = 1 if alpha > 0 else -1
    la = int(math.log2(abs(alpha)))

    def exact_check(i, j):
        sh = SH - int(esum[i, j]) + la
        assert sh >= 0
        P = sgn * int(Cint[i, j]) << sh
        got = scaled(C[i, j])
        want = P + (scaled(Cold[i, j]) if Cold is not None else 0)
        # (err and bound times 2^131: 4 2^-53 |P| + 2^-78 M |alpha| 2^-esum + 2^-53 |C|)
        bound = (abs(P) << 80) + (M << (53 + sh)) + ((abs(got) << 78) if Cold is not None else 0)
        return abs(got - want) << 131, bound

    if Cold is not None:   # (few entries in the tests: every one exactly)
        for i, j in zip(*np.nonzero(todo)):
            err, bound = exact_check(i, j)
            if err > bound:
                bad[i, j] = True
            worst = max(worst, float(err / bound) if bound else (0.0 if err == 0 else math.inf))
        return bad, worst
    # scaled to the integers: d = C 2^(e_i + e_j) / alpha against C' (the scalings are exact
    # in fp64: powers of two, far from over- and underflow in the tests' ranges)
    with np.errstate(over="ignore"):   # (entries outside `where` may hold anything)
        d = np.ldexp(C, esum.astype(np.int32)) / alpha
    fC = np.vectorize(float, otypes=[np.float64])(Cint) if Cint.size else np.zeros((rows, cols))
    errf = np.abs(d - fC)                        # |d - C'| is within 2^-53 |C'| of this, and
    bound = 4.0 * 2.0 ** -53 * np.abs(fC) + float(Fraction(M, 1 << 78))   # (bound to ~2^-52 relative)
    slack = 2.0 ** -53 * np.abs(fC) + 2.0 ** -30 * bound
    sure_bad = todo & (errf - slack > bound)
    unsure = todo & ~sure_bad & (errf + slack > bound)
    bad |= sure_bad
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(todo & (bound > 0), errf / bound, 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    for i, j in zip(*np.nonzero(unsure)):
        err, bnd = exact_check(i, j)
        if err > bnd:
            bad[i, j] = True
    return bad, worst


def expected(ref, alpha=1.0):
    """fp64 alpha C' 2^-(e_i + e_j), each entry rounded once (NaN where a row or column is)."""
    assert _pow2(alpha)
    fC = np.vectorize(float, otypes=[np.float64])(ref.Cint)
    ea = np.where(ref.ea == EX_NAN, 0, ref.ea)
    eb = np.where(ref.eb == EX_NAN, 0, ref.eb)
    out = alpha * np.ldexp(fC, (-(ea[:, None] + eb[None, :])).astype(np.int32))
    out[ref.nan] = np.nan
    return out


def describe(bad, C, ref, alpha=1.0, limit=5):
    """A few of the wrong entries, for an assertion message: (row, column, got, expected)."""
    exp = expected(ref, alpha)
    idx = list(zip(*np.nonzero(bad)))[:limit]
    return "%d wrong, first (i, j, got, exact): %s" % (
        int(bad.sum()), [(int(i), int(j), float(C[i, j]), float(exp[i, j])) for i, j in idx])
