"""The Python layer over the device-made candidates: history_match.imp_plot, nonimp_data and
new_wave_design given an EmulatorSet, EmulatorSet.maps / imp_maps, and
nonimp_sample(generator="device"), on the two toysim3D emulators of test_gpu_history_match.py
with the fixture's zs, var_extra and cm = 3.

Bounds.  The set's route and the list's are two routes to one posterior: their implausibilities
agree to rtol 1e-7, the bound test_gpu_implausibility.py::test_api_level holds them to.  Counts
and accepted rows are equal provided no sample lies within 1e-7 cm of cm; each test asserts that
on the list route's values.  Checked beforehand on the CPU (oracle.gp_oracle.posterior_ref on the
two emulators, the seeded designs of the fixture): the nearest sample of imp_plot's three pairs
at seed 21, grid 4, olhcmult 20 is 1.5e-3 cm from cm at maxno 1 and 1.5e-3 cm at maxno 2; of the
fixture's data 5.1e-3 cm; of new_wave_design's design at seed 22, olhcmult 10, 4.0e-3 cm.
The device generator against the host generator is an equality: one stream, one set.
"""
import os
import shutil

import numpy as np
import pytest

import implausibility_maps_ref as mapref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "history_match.npz"))
ZS, VE, CM = list(G["zs"]), list(G["var_extra"]), float(G["cm"])
PAIRS = ("0_1", "0_2", "1_2")


@pytest.fixture()
def emuls(tmp_path, monkeypatch, capsys):
    import gp_emu_uqsa_amd as g
    shutil.copytree(os.path.join(HERE, "golden", "examples", "sensitivity_recon"), tmp_path / "w",
                    copy_function=shutil.copyfile)          # the checkout may be read-only
    os.chmod(tmp_path / "w", 0o755)
    monkeypatch.chdir(tmp_path / "w")
    for i in range(2):
        with open(f"toysim3D_beliefs{i}-1f", "a") as fh:
            fh.write("active_index 0 1 2\n")
    np.savetxt("toysim3D_input", G["data_in"])
    np.savetxt("toysim3D_output", G["data_out"])
    return [g.setup(f"toysim3D_config{i}_recon", datashuffle=False, scaleinputs=True) for i in range(2)]


def _loop(hm, emuls, x, maxno):
    """_imaxes of the _posterior_diag loop: the list route's values."""
    I2 = np.zeros((x.shape[0], len(emuls)))
    for o, E in enumerate(emuls):
        mean, var = hm._posterior_diag(E, x[:, E.beliefs.active_index])
        I2[:, o] = (mean - ZS[o]) ** 2 / (var + VE[o])
    return hm._imaxes(I2, maxno)


def _outside_the_band(I):
    return bool(np.all(np.abs(I - CM) > 1e-7 * CM))


def _files(maxno):
    return {f"{m}_{kind}_{tag}": np.loadtxt(f"{m}_{kind}_{tag}") for tag in PAIRS for m in range(1, maxno + 1)
            for kind in ("IMP", "ODP")}


def _grid(grid):
    return np.linspace(0.0, 1.0, grid, endpoint=False) + 0.5 / grid


@pytest.mark.parametrize("maxno", [1, 2])
def test_imp_plot_with_a_set(emuls, maxno):
    from gp_emu_uqsa_amd import history_match as hm
    np.random.seed(21)
    hm.imp_plot(emuls, ZS, CM, VE, maxno=maxno, olhcmult=20, grid=4, plot=False)
    want = _files(maxno)
    designs = {tag: np.loadtxt("imp_input_" + tag) for tag in PAIRS}
    # the condition of the ODP's equality, on the list route's values
    for tag in PAIRS:
        a, b = (int(c) for c in tag.split("_"))
        rows = mapref.cell_rows(3, a, b, _grid(4), _grid(4), designs[tag].reshape(-1, 1))
        top = _loop(hm, emuls, rows, maxno)
        for l in range(maxno):
            assert _outside_the_band(top[:, -(l + 1)]), (tag, l)
            assert np.array_equal(top[:, -(l + 1)].reshape(16, -1).min(axis=1), want[f"{l + 1}_IMP_{tag}"].ravel())
    S = hm.EmulatorSet(emuls)
    try:
        assert S.fused is True
        np.random.seed(21)
        hm.imp_plot(S, ZS, CM, VE, maxno=maxno, olhcmult=20, grid=4, plot=False)
        got = _files(maxno)
        for tag in PAIRS:
            assert np.array_equal(np.loadtxt("imp_input_" + tag), designs[tag])   # the same optLatinHyperCube calls
            for m in range(1, maxno + 1):
                assert np.allclose(got[f"{m}_IMP_{tag}"], want[f"{m}_IMP_{tag}"], rtol=1e-7, atol=0.0), (tag, m)
                assert np.array_equal(got[f"{m}_ODP_{tag}"], want[f"{m}_ODP_{tag}"]), (tag, m)
        # imp_maps: the maps of one pair, and the device's against the explicit rows through the set
        x1 = x2 = _grid(4)
        IMP, ODP = hm.imp_maps(S, ZS, VE, CM, (0, 2), x1, x2, designs["0_2"].reshape(-1, 1), maxno=maxno)
        assert IMP.shape == ODP.shape == (maxno, 4, 4)
        top = S.implausibility(ZS, VE, mapref.cell_rows(3, 0, 2, x1, x2, designs["0_2"].reshape(-1, 1)), maxno)
        for l in range(maxno):
            col = top[:, -(l + 1)].reshape(16, -1)
            assert np.array_equal(IMP[l].ravel(), col.min(axis=1))
            assert np.array_equal(ODP[l].ravel(), (col < CM).sum(axis=1) / float(col.shape[1]))
            assert np.array_equal(IMP[l], got[f"{l + 1}_IMP_0_2"])      # imp_plot wrote these maps (%.18e keeps the bits)
            assert np.array_equal(ODP[l], got[f"{l + 1}_ODP_0_2"])
        lst = hm.imp_maps(emuls, ZS, VE, CM, (0, 2), x1, x2, designs["0_2"].reshape(-1, 1), maxno=maxno)
        assert np.array_equal(lst[0], IMP) and np.array_equal(lst[1], ODP)           # a list makes its own set
    finally:
        S.close()


def test_a_set_that_is_not_fused_gives_the_lists_bits(emuls):
    from gp_emu_uqsa_amd import history_match as hm
    emuls[1].beliefs.basis_str[2] = "x**2"
    emuls[1].basis.exprs[2] = "x**2"
    emuls[1].basis.h[2] = emuls[1].basis._compile("x**2")
    np.random.seed(21)
    hm.imp_plot(emuls, ZS, CM, VE, maxno=2, olhcmult=20, grid=4, plot=False)
    want = _files(2)
    T = hm.EmulatorSet(emuls)
    try:
        assert T.fused is False
        np.random.seed(21)
        hm.imp_plot(T, ZS, CM, VE, maxno=2, olhcmult=20, grid=4, plot=False)
        got = _files(2)
        for key in want:
            assert np.array_equal(got[key], want[key]), key
        with pytest.raises(RuntimeError):
            hm.nonimp_sample(T, ZS, CM, VE, count=5, generator="device")
    finally:
        T.close()


def test_nonimp_data_and_new_wave_design_with_a_set(emuls):
    from gp_emu_uqsa_amd import history_match as hm
    din, dout = "toysim3D_input", "toysim3D_output"
    assert _outside_the_band(_loop(hm, emuls, np.ascontiguousarray(G["data_in"]), 1)[:, -1])
    count = hm.nonimp_data(emuls, ZS, CM, VE, [din, dout], maxno=1)
    want = np.loadtxt("nonimp_" + din), np.loadtxt("noninp_" + dout)
    np.random.seed(22)
    wave = hm.new_wave_design(emuls, ZS, CM, VE, ["nonimp_" + din, "noninp_" + dout], maxno=1, olhcmult=10, fileStr="list")
    design = np.loadtxt("olhc_des")
    assert _outside_the_band(_loop(hm, emuls, design, 1)[:, -1])
    S = hm.EmulatorSet(emuls)
    try:
        assert S.fused is True
        assert hm.nonimp_data(S, ZS, CM, VE, [din, dout], maxno=1, fileStr="set") == count == int(G["nonimp_count"])
        assert np.array_equal(np.loadtxt("set_nonimp_" + din), want[0])
        assert np.array_equal(np.loadtxt("set_noninp_" + dout), want[1])
        np.random.seed(22)
        assert hm.new_wave_design(S, ZS, CM, VE, ["nonimp_" + din, "noninp_" + dout], maxno=1, olhcmult=10,
                                  fileStr="set") == wave == int(G["wave_count"])
        assert np.array_equal(np.loadtxt("olhc_des"), design)
        assert np.array_equal(np.loadtxt("set_nonimp_" + din), np.loadtxt("list_nonimp_" + din))
    finally:
        S.close()


def test_nonimp_sample_on_the_device(emuls, monkeypatch):
    from gp_emu_uqsa_amd import history_match as hm
    S = hm.EmulatorSet(emuls)
    try:
        assert S.fused is True
        host = hm.nonimp_sample(S, ZS, CM, VE, count=50, batch=4096, generator="host")
        assert host[0].shape == (50, 3) and host[1] >= 50
        for batch in (4096, 1000, 37):                            # 37: the count is reached in the middle of a batch
            pts, tried = hm.nonimp_sample(S, ZS, CM, VE, count=50, batch=batch, generator="device")
            assert np.array_equal(pts, host[0]) and tried == host[1], batch
        for maxno, seed in ((2, 7), (1, 12345)):
            a = hm.nonimp_sample(S, ZS, CM, VE, count=30, maxno=maxno, seed=seed, batch=1000, generator="host")
            b = hm.nonimp_sample(S, ZS, CM, VE, count=30, maxno=maxno, seed=seed, batch=64, generator="device")
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        # max_tried exhausted: fewer than count, all that were tried
        a = hm.nonimp_sample(S, ZS, CM, VE, count=10 ** 6, batch=300, max_tried=1000, generator="host")
        b = hm.nonimp_sample(S, ZS, CM, VE, count=10 ** 6, batch=300, max_tried=1000, generator="device")
        c = hm.nonimp_sample(S, ZS, CM, VE, count=10 ** 6, batch=2 ** 20, max_tried=1000, generator="device")
        assert a[1] == b[1] == c[1] == 1000 and 0 < a[0].shape[0] < 1000
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
        # generator=None picks the device where the set is fused
        calls = []
        sample = S._set.sample
        monkeypatch.setattr(S._set, "sample", lambda *args, **kw: calls.append(1) or sample(*args, **kw))
        pts, tried = hm.nonimp_sample(S, ZS, CM, VE, count=50, batch=1000)
        assert calls and np.array_equal(pts, host[0]) and tried == host[1]
        n = len(calls)
        hm.nonimp_sample(S, ZS, CM, VE, count=50, batch=1000, generator="host")
        assert len(calls) == n
    finally:
        S.close()
