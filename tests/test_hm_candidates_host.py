"""Host checks of the candidate generators and reducers of the resident emulator set
(gpe_hm_cells, gpe_hm_cells_mv, gpe_hm_sample), no GPU:

- csrc/gpemu_hm_cand_plan.hpp through two stand-alone programs, built with the address and
  undefined-behaviour sanitizers where their runtime links (stand-alone binaries: nothing is
  preloaded), plainly otherwise: tests/host/hm_cells_check.cpp (the pieces a chunk cuts the cells
  into, the workspace sizes) and tests/host/hm_draw_check.cpp (PCG64's step, output, double,
  skip-ahead, row table and the affine map against numpy.random.default_rng, bit for bit);
- tests/implausibility_maps_ref.py, the NumPy restatement the GPU tests compare with, against
  history_match._imaxes plus min / (col < cm).sum, and its explicit rows against imp_plot's;
- EmulatorSet.maps outside the fused path and nonimp_sample's generator choice, on stand-in sets.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import implausibility_maps_ref as mapref
from test_objective_host import SAN, _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")


def _build(tmp_path, name):
    cxx = _cxx()
    if not cxx:
        pytest.skip("no C++ compiler: the host check cannot be built")
    exe = str(tmp_path / name)
    # -ffp-contract=off: g++ ignores the header's clang pragma and contracts by default in GNU mode
    base = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe]
    built = subprocess.run(base + SAN, capture_output=True, text=True)
    sanitized = built.returncode == 0
    if not sanitized:   # (no sanitizer runtime on this machine)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    print("sanitizers:", sanitized)
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.strip().splitlines()[-1]


def test_cells_check_program(tmp_path):
    assert _run(_build(tmp_path, "hm_cells_check")) == "hm_cells_check OK"


def _hex(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel())


def test_draw_check_program(tmp_path):
    exe = _build(tmp_path, "hm_draw_check")
    D, R, k1, mask = 13, 400, 777, (1 << 64) - 1
    lo = np.linspace(-1.5, 0.25, D)
    hi = lo + np.linspace(0.1, 3.7, D)
    for seed in (0, 4, 12345):
        rng = np.random.default_rng(seed)
        st = rng.bit_generator.state["state"]
        u = [rng.random(k1)]
        st1 = rng.bit_generator.state["state"]["state"]
        u.append(rng.random(R * D - k1))                       # a continued stream
        x = lo + np.random.default_rng(seed).random((R, D)) * (hi - lo)
        words = [st["state"] >> 64, st["state"] & mask, st["inc"] >> 64, st["inc"] & mask, k1, st1 >> 64, st1 & mask,
                 D, R]
        path = tmp_path / f"draw_{seed}.txt"
        path.write_text(" ".join("%x" % w for w in words) + "\n" + _hex(lo) + "\n" + _hex(hi) + "\n"
                        + _hex(np.concatenate(u)) + "\n" + _hex(x) + "\n")
        assert _run(exe, str(path)) == "hm_draw_check OK", seed
    assert struct.pack("<d", 0.5) == bytes.fromhex("000000000000e03f")   # (_hex writes IEEE bits)


def _hand_made_i2(cells, ns, p):
    rs = np.random.RandomState(2)
    I2 = rs.uniform(0.0, 16.0, size=(cells * ns, p))
    I2[4, 2] = np.nan                         # one NaN output in cell 0
    I2[ns + 3, 0] = -1.0                      # a negative denominator: sqrt gives NaN
    I2[2 * ns:2 * ns + 2, :] = np.nan         # all outputs NaN at two samples of cell 2
    I2[3 * ns + 1, 1] = I2[3 * ns + 1, 3]     # a tie
    I2[3 * ns + 2, :] = 9.0                   # every output exactly on the cut-off 3.0: not below
    I2[4 * ns + 5, 4] = np.inf
    I2[4 * ns + 6, 0] = -np.inf
    I2[5 * ns, 1] = -0.0                      # signed zeros count as equal
    I2[5 * ns + 1, :] = 0.0
    return I2


@pytest.mark.parametrize("use", [None, [True, True, False, True, True], [False] * 5])
def test_maps_reference_against_imaxes(use):
    from gp_emu_uqsa_amd.history_match import _imaxes
    cells, ns, p, cm = 6, 7, 5, 3.0
    I2 = _hand_made_i2(cells, ns, p)
    masked = I2.copy()
    if use is not None:
        masked[:, ~np.array(use)] = 0.0
    for maxno in (1, 2, 5):
        imp, below = mapref.maps(I2, cells, ns, maxno, cm, use)
        assert imp.shape == below.shape == (maxno, cells) and below.dtype == np.int64
        with np.errstate(invalid="ignore"):
            top = _imaxes(masked, maxno).reshape(cells, ns, maxno)
            for l in range(maxno):
                col = top[:, :, -(l + 1)]
                assert np.array_equal(imp[l], col.min(axis=1), equal_nan=True), (maxno, l)
                assert np.array_equal(below[l], (col < cm).sum(axis=1)), (maxno, l)
    if use is None:
        imp, below = mapref.maps(I2, cells, ns, 1, cm)
        assert np.isnan(imp[0, [0, 1, 2, 4]]).all() and np.isfinite(imp[0, [3, 5]]).all()   # (sqrt(-inf) is a NaN)
        imp5, below5 = mapref.maps(I2, cells, ns, 5, 5.0)        # level 4, cm above every number: NaNs alone are out
        assert below5[4, 2] == ns - 2 and below5[4, 0] == ns and below5[0, 0] == ns - 1
    if use is not None and not any(use):
        imp, below = mapref.maps(I2, cells, ns, 2, cm, use)
        assert np.all(imp == 0.0) and np.all(below == ns)


def test_reference_rows_are_imp_plots():
    """cell_rows against the vectorised construction of history_match.imp_plot."""
    rs = np.random.RandomState(1)
    D, g1, g2, n = 5, 3, 2, 4
    x1, x2, others = rs.uniform(size=g1), rs.uniform(size=g2), rs.uniform(size=(n, D - 2))
    for ca, cb in ((0, 1), (1, 3), (4, 2), (3, 0)):
        cells = g1 * g2
        x = np.empty((cells * n, D))
        x[:, ca] = np.repeat(np.repeat(x1, g2), n)
        x[:, cb] = np.repeat(np.tile(x2, g1), n)
        x[:, [k for k in range(D) if k not in (ca, cb)]] = np.tile(others, (cells, 1))
        assert np.array_equal(mapref.cell_rows(D, ca, cb, x1, x2, others), x)


def _StandInSet(D=3):
    """A set outside the fused path whose implausibility is a formula of the rows."""
    from gp_emu_uqsa_amd import history_match as hm

    class StandIn(hm.EmulatorSet):
        def __init__(self):
            self.minmax = {str(k): [0.0, 1.0] for k in range(D)}
            self.D = D
            self.fused = False
            self._set = None
            self.rows = None
            self.nan_row = None

        def implausibility(self, zs, var_extra, x, maxno=1):
            self.rows = x.copy()
            d = 10.0 * np.linalg.norm(x - 0.5, axis=1)
            if self.nan_row is not None:
                d[self.nan_row] = np.nan
            return np.column_stack([0.25 * d, 0.5 * d, d])[:, -maxno:]

    return StandIn()


def test_maps_outside_the_fused_path():
    from gp_emu_uqsa_amd import history_match as hm
    rs = np.random.RandomState(3)
    x1, x2, others, cm = rs.uniform(size=3), rs.uniform(size=2), rs.uniform(size=(4, 1)), 3.0
    for fn in (lambda S, **k: S.maps(None, None, cm, (2, 0), x1, x2, others, **k),
               lambda S, **k: hm.imp_maps(S, None, None, cm, (2, 0), x1, x2, others, **k)):
        S = _StandInSet()
        S.nan_row = 5
        IMP, ODP = fn(S, maxno=2)
        assert IMP.shape == ODP.shape == (2, 3, 2)
        rows = mapref.cell_rows(3, 2, 0, x1, x2, others)
        assert np.array_equal(S.rows, rows)
        d = 10.0 * np.linalg.norm(rows - 0.5, axis=1)
        d[5] = np.nan
        # the stand-in's columns are I itself: I^2 for the reference is their square
        imp, below = mapref.maps(np.column_stack([0.25 * d, 0.5 * d, d]) ** 2, 6, 4, 2, cm)
        top = np.column_stack([0.5 * d, d]).reshape(6, 4, 2)
        for l in range(2):
            assert np.array_equal(IMP[l].ravel(), top[:, :, -(l + 1)].min(axis=1), equal_nan=True)
            assert np.allclose(IMP[l].ravel(), imp[l], rtol=1e-15, atol=0.0, equal_nan=True)
            assert np.array_equal(ODP[l].ravel(), (top[:, :, -(l + 1)] < cm).sum(axis=1) / 4.0)
        assert np.isnan(IMP[:, 0, 1]).all() and np.isfinite(np.delete(IMP.reshape(2, 6), 1, axis=1)).all()


def test_joint_maps_outside_the_fused_path():
    """joint=(item, V): one level, I of implausibility_mv on the explicit rows, reduced per cell."""
    from gp_emu_uqsa_amd import history_match as hm
    rs = np.random.RandomState(5)
    x1, x2, others, cm = rs.uniform(size=3), rs.uniform(size=2), rs.uniform(size=(4, 1)), 3.0
    seen = {}

    def joint_measure(item, z, V, x, parts=False):
        seen.update(item=item, z=np.asarray(z), V=np.asarray(V), rows=x.copy())
        I = 8.0 * np.linalg.norm(x - 0.4, axis=1)
        I[9] = np.nan
        return I

    S = _StandInSet()
    S.emuls, S._multi = [None, None], [False, True]
    S.implausibility_mv = joint_measure
    with pytest.raises(ValueError):
        S.maps([1.0, 2.0], None, cm, (1, 2), x1, x2, others, joint=(0, np.eye(2)))      # item 0 is no MultiEmulator
    for IMP, ODP in (S.maps([1.0, 2.0], None, cm, (1, 2), x1, x2, others, maxno=3, joint=(1, [0.1, 0.2])),
                     hm.imp_maps(S, [1.0, 2.0], None, cm, (1, 2), x1, x2, others, joint=(1, np.diag([0.1, 0.2])))):
        assert IMP.shape == ODP.shape == (1, 3, 2)                                      # one level whatever maxno
        rows = mapref.cell_rows(3, 1, 2, x1, x2, others)
        assert seen["item"] == 1 and np.array_equal(seen["rows"], rows)
        assert np.array_equal(seen["z"], [1.0, 2.0]) and np.array_equal(seen["V"], np.diag([0.1, 0.2]))
        I = 8.0 * np.linalg.norm(rows - 0.4, axis=1)
        I[9] = np.nan
        I = I.reshape(6, 4)
        assert np.array_equal(IMP[0].ravel(), I.min(axis=1), equal_nan=True) and np.isnan(IMP[0, 1, 0])
        assert np.array_equal(ODP[0].ravel(), (I < cm).sum(axis=1) / 4.0)


def test_nonimp_sample_generator_choice():
    from gp_emu_uqsa_amd import history_match as hm
    a = hm.nonimp_sample(_StandInSet(), None, 3.0, None, count=20, seed=4, batch=100)
    b = hm.nonimp_sample(_StandInSet(), None, 3.0, None, count=20, seed=4, batch=37, generator="host")
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]            # None picks the host outside the fused path
    with pytest.raises(RuntimeError):
        hm.nonimp_sample(_StandInSet(), None, 3.0, None, count=20, generator="device")
    with pytest.raises(ValueError):
        hm.nonimp_sample(_StandInSet(), None, 3.0, None, count=20, generator="gpu")
