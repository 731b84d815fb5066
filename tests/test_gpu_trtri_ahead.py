"""Gradient evaluations with the split Cholesky: X11 = L11^-1 (the TRTRI's pairs inside [0, h))
and the top pair's T = L21 X11 run on the context stream while the sweep's second phase runs on
the high-priority one (potrf's ahead, trtri).  The operations and their
operands are those of the TRTRI after the sweep, only earlier and on another stream, so every
result must equal the GPEMU_TRTRI_AHEAD=0 context's bit for bit, with the same launches.

Contexts and shapes are tests/test_gpu_ozaki_chol.py's (NB tile columns, h the split column).
Which int8 pairs exist decides what runs ahead:

  n     NB  h   FLOORS (int8 from 512 rows)                          TRI_MIN=2048
  1024   8   4  X11 in fp64, T ahead                                 X11 in fp64 (top pair fp64)
  1400  11   8  pair (0, 4, 8) ahead on the int8 cores, then T       X11 in fp64
  2900  23  16  int8 pairs on both sides: T stays behind the sweep   X11 in fp64, T ahead
  1600  13   8  as 2900: the pair (8, 12, 13) runs on the int8 cores with its level
"""
import threading

import numpy as np
import pytest

import test_gpu_ozaki_chol as tc
from gp_emu_uqsa_amd import native
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

OFF = dict(GPEMU_TRTRI_AHEAD="0")
TOP = {**tc.FLOORS, "GPEMU_OZAKI_TRI_MIN": "2048"}


def _fixture(**env):
    @pytest.fixture(scope="module")
    def fx():
        c = tc._context(**env)
        yield c
        c.close()
    return fx


ahead = _fixture(**tc.FLOORS)
behind = _fixture(**tc.FLOORS, **OFF)
top_ahead = _fixture(**TOP)
top_behind = _fixture(**TOP, **OFF)
unsplit = _fixture(**tc.FLOORS, GPEMU_OZAKI_CHOL="0")
fp64 = _fixture(GPEMU_OZAKI="0")

SHAPES = [(1024, "gp4ml_fit"), (1024, "alt_r"), (1400, "gp4ml_fit"), (1400, "mucm_fix"), (1400, "alt_r"),
          (2900, "gp4ml_fit"), (2900, "mucm_fix")]
IDS = [f"{n}-{k}" for n, k in SHAPES]


def _bytes(res):
    return np.float64(res[0]).tobytes() + np.asarray(res[1], np.float64).tobytes() + np.float64(res[2]).tobytes()


def _count(n, min_tiles):
    return 1 + 2 * tc._pairs((n + 127) // 128, min_tiles) + 1


@pytest.mark.parametrize("n,case", SHAPES, ids=IDS)
def test_same_bytes_as_behind_the_sweep(ahead, behind, n, case):
    a = tc._grad(ahead, n, case, count=_count(n, 4))
    b = tc._grad(behind, n, case, count=_count(n, 4))
    assert _bytes(a) == _bytes(b), (a, b)


@pytest.mark.parametrize("n,case", [(1024, "gp4ml_fit"), (1400, "gp4ml_fit"), (2900, "gp4ml_fit"), (2900, "mucm_fix")])
def test_same_bytes_top_pair_only(top_ahead, top_behind, fp64, n, case):
    """Only the top pair (or none) on the int8 cores: at n = 2900 T reuses the sweep's L21 planes."""
    a = tc._grad(top_ahead, n, case, count=_count(n, 16))
    b = tc._grad(top_behind, n, case, count=_count(n, 16))
    assert _bytes(a) == _bytes(b), (a, b)
    tc._against(n, case, a, tc._grad(fp64, n, case), "ahead, top pair only")


def test_ragged_fourth_shape(ahead, behind):
    """n = 1600 (Rb = 640 -> Pb = 768), test_gpu_ozaki_chol.py's recipe at d = 5."""
    n, d = 1600, 5
    X, f, H = orc.synthetic_problem(n, d, seed=n + d)
    hp = np.array(list(np.linspace(0.5, 1.1, d)) + [1e-3, 1.1])
    out = []
    for c in (ahead, behind):
        c.set_data(X, f, H)
        out.append(c.objective(orc.GP4ML, orc.STD, hp))
    assert _bytes(out[0]) == _bytes(out[1]), out
    ref = orc.objective_fast(X, f, H, hp, orc.GP4ML, orc.STD, True)
    err = np.max(np.abs(out[0][1] - ref[1]) / tc._scale(ref[1]))
    print(f"n=1600: grad vs oracle {err:.2e}, llh vs oracle {abs(out[0][0] - ref[0]):.2e}")
    assert err <= 1e-7 and abs(out[0][0] - ref[0]) <= 1e-10 * max(1.0, abs(ref[0]))


def test_value_only_and_gradient_calls_alternate(ahead, behind):
    """A value-only call (nothing ahead) between gradient calls on one context."""
    n, case = 1400, "gp4ml_fit"
    variant, kind, _, _ = tc.CASES[case]
    X, f, H, r, hp, nu_fixed, _ = tc._problem(n, case)
    out = []
    for c in (ahead, behind):
        c.set_data(X, f, H, r)
        g1 = c.objective(variant, kind, hp, nu_fixed=nu_fixed)
        v = c.objective(variant, kind, hp, nu_fixed=nu_fixed, want_grad=False)
        g2 = c.objective(variant, kind, hp, nu_fixed=nu_fixed)
        assert _bytes(g1) == _bytes(g2)
        out.append((_bytes(g1), v[0]))
    assert out[0] == out[1]


@pytest.mark.parametrize("bad", [100, 800], ids=["a11", "schur"])
def test_not_positive_definite(ahead, unsplit, fp64, bad):
    """test_gpu_ozaki_chol.py's construction at n = 1024 (h 128 = 512): the failing pivot inside
    A11 (X11 and T then run on what is there) and in S.  The unsplit context's decision, twice
    in a row; a good matrix on the same context then gives the oracle's result."""
    X, f, H, r, hp = tc._non_pd_problem(bad)
    unsplit.set_data(X, f, H, r)
    with pytest.raises(native.NotPositiveDefinite):
        unsplit.objective(orc.GP4ML, orc.ALT, hp)
    ahead.set_data(X, f, H, r)
    for _ in range(2):
        with pytest.raises(native.NotPositiveDefinite):
            ahead.objective(orc.GP4ML, orc.ALT, hp)
    tc._against(1024, "gp4ml_fit", tc._grad(ahead, 1024, "gp4ml_fit", count=_count(1024, 4)),
                tc._grad(fp64, 1024, "gp4ml_fit"), "after non-PD")


@pytest.mark.parametrize("n", [1024, 1400, 2900])
def test_same_bytes_every_time(ahead, n):
    first = _bytes(tc._grad(ahead, n, "gp4ml_fit"))
    for _ in range(4):
        assert _bytes(tc._grad(ahead, n, "gp4ml_fit")) == first


def test_two_in_flight_give_their_solo_bytes():
    """Two contexts, each on its own thread, evaluating at once at n = 1400 (each then takes the
    per-step launches; three streams of work per context between the phases)."""
    n, cases = 1400, ("gp4ml_fit", "alt_r")
    ctxs = [tc._context(**tc.FLOORS) for _ in cases]
    try:
        solo = [_bytes(tc._grad(c, n, case)) for c, case in zip(ctxs, cases)]
        out, err = [None, None], []
        gate = threading.Barrier(2)

        def work(k):
            try:
                gate.wait()
                out[k] = [_bytes(tc._grad(ctxs[k], n, cases[k])) for _ in range(3)]
            except Exception as e:   # noqa: BLE001
                err.append(e)

        th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not err, err
        for k in range(2):
            assert all(b == solo[k] for b in out[k])
    finally:
        for c in ctxs:
            c.close()
