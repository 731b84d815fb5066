"""The objective's host arithmetic (csrc/gpemu_objective.hpp: kernel codes, the argument split,
the length-scale check, the closed form, the gradient from the contraction sums, the reader of
the one-launch kernels' result buffer -- what every path to an LLH and a gradient ends in)
checked by a stand-alone program, tests/host/objective_check.cpp: any C++17 compiler, no HIP,
no GPU.  Built with the address and undefined-behaviour sanitizers where their runtime links
(a stand-alone binary: nothing is preloaded), plainly otherwise.

The formulas run on inputs numpy forms in fp64 from the reference's recorded problems
(tests/golden/objective_n200_d3.npz): A (oracle.gp_oracle.kernel_var_ref), L, Z = L^-1 [f H],
its Gram, log|A| and the d + 3 sums as k_contract defines them over M = A^-1 - W W^T -
c alpha alpha^T, with W, alpha and c from the oracle's own algebra (objective_fast's), not from
the program.  The program's LLH, sigma^2 and gradient are held to the recorded ones under the
tolerances of tests/test_gpu_objective.py (its _grad_ok and cond(A) rule, imported)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gp_oracle as orc
from test_gpu_objective import CASES, _cond, _grad_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "objective_check.cpp")
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
GOLD = os.path.join(ROOT, "tests", "golden", "objective_n200_d3.npz")
ERR_ARG, ERR_HIP, NOT_PD = -1, -2, 1      # include/gpemu.h


def _cxx():
    cands = [os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++",
             os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")]
    for c in cands:
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(text) -> the program's output lines for the commands in text."""
    cxx = _cxx()
    if not cxx:
        pytest.skip("no C++ compiler: the host check of the objective cannot be built")
    exe = str(tmp_path_factory.mktemp("objective") / "objective_check")
    base = [cxx, "-std=c++17", "-O1", "-I", CSRC, SRC, "-o", exe]
    built = subprocess.run(base + SAN, capture_output=True, text=True)
    sanitized = built.returncode == 0
    if not sanitized:   # (no sanitizer runtime on this machine)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    print("sanitizers:", sanitized)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.strip().splitlines()
        assert lines[-1] == "objective_check OK"
        return lines[:-1]
    return run


def _hex(v):
    return " ".join(float(x).hex() for x in np.ravel(v))


def _fields(line, *names):
    """The doubles after each of the labels `names` (in order) of an output line."""
    tok = line.split()
    pos = [tok.index(nm) for nm in names] + [len(tok)]
    return [np.array([float.fromhex(t) for t in tok[pos[i] + 1:pos[i + 1]]]) for i in range(len(names))]


# ------------------------------------------------------------------ the formulas
def _golden_record(z, case, point):
    """One `value` command and what the program must print for it."""
    tag, kind, variant, fitn, use_r = case
    X, f = z["X"], z["f"]
    H = orc.linear_basis(X)
    n, d = X.shape
    q = H.shape[1]
    key = f"{tag}_p{point}"
    hp, nufixed = z[key + "_hp"], float(z[key + "_nufixed"])
    gp4ml = variant == orc.GP4ML
    delta, nu, sigma = orc.split_hp(hp, d, variant, fitn)
    nu = nu if nu is not None else nufixed
    s2 = sigma ** 2 if gp4ml else 1.0
    r = z["r"] if use_r else None
    C, e = orc.kernel_var_ref(X, delta, nu, kind, True)
    A = s2 * C
    if gp4ml and kind == orc.ALT and r is not None:
        A[np.diag_indices_from(A)] += r
    L = np.linalg.cholesky(A)
    Linv = sla.solve_triangular(L, np.eye(n), lower=True)
    Z = Linv @ np.column_stack([f, H])
    G = Z.T @ Z
    logdetA = 2.0 * np.sum(np.log(np.diag(L)))
    # the oracle's algebra (objective_fast): beta, Kq, c, then M
    zc, w = Z[:, 0], Z[:, 1:]
    Kq = np.linalg.cholesky(w.T @ w)
    B = sla.cho_solve((Kq, True), w.T @ zc)
    u = zc - w @ B
    quad = float(u @ u)
    c = 1.0 if gp4ml else (n - q) / ((quad / (n - q - 2.0)) * (n - q - 2.0))
    alpha = Linv.T @ u
    W = sla.solve_triangular(Kq, (Linv.T @ w).T, lower=True).T
    M = Linv.T @ Linv - W @ W.T - c * np.outer(alpha, alpha)
    ME = np.tril(M * _squareform(e, n), -1)      # the strictly lower entries of M E (k_contract's i > j)
    std_r = gp4ml and kind == orc.STD and r is not None
    red = [np.sum(ME * (X[:, k, None] - X[None, :, k]) ** 2 / delta[k] ** 2) for k in range(d)]
    red += [np.sum(ME), np.trace(M), float(np.diag(M) @ r) if std_r else 0.0]
    Kinv = sla.solve_triangular(Kq, np.eye(q), lower=True)
    T2 = np.zeros((q + 1, q + 1))
    T2[0, 0] = np.sqrt(c)
    T2[1:, 0] = -np.sqrt(c) * B
    T2[1:, 1:] = Kinv.T
    cmd = (f"value {q + 1} {d} {int(kind)} {float(nu).hex()} {int(fitn)} {int(gp4ml)} {float(s2).hex()} {n} "
           f"{hp.size} {int(std_r)} {float(logdetA).hex()} {_hex(G)} {_hex(red)}")
    rtol = max(1e-10, 4 * np.finfo(float).eps * _cond(X, hp, kind, variant, fitn, nufixed))
    want = dict(key=key, llh=float(z[key + "_llh"]), grad=z[key + "_grad"], sig2=float(z[key + "_sig2"]),
                rtol=rtol, T2=T2.ravel(order="F"), condQ=np.linalg.cond(w.T @ w), c=c)
    return cmd, want


def _squareform(e, n):
    E = np.zeros((n, n))
    E[np.triu_indices(n, 1)] = e
    return E + E.T


def test_formulas_match_the_recorded_results(check):
    z = np.load(GOLD)
    recs = [_golden_record(z, case, point) for case in CASES for point in (0, 1)]
    assert len(recs) == 18
    out = check("\n".join(cmd for cmd, _ in recs) + "\n")
    assert len(out) == 18
    for line, (_, w) in zip(out, recs):
        assert line.startswith("value ok"), (w["key"], line)
        val, T2, grad = _fields(line, "val", "T2", "grad")
        llh, sig2, cfac, _ = val
        print(w["key"], "llh err", abs(llh - w["llh"]) / max(1.0, abs(w["llh"])), "rtol", w["rtol"],
              "grad err", _grad_ok(grad, w["grad"])[1], "sig2 err", abs(sig2 - w["sig2"]) / abs(w["sig2"]))
        assert abs(llh - w["llh"]) <= w["rtol"] * max(1.0, abs(w["llh"])), (w["key"], llh, w["llh"])
        ok, err = _grad_ok(grad, w["grad"])
        assert ok, (w["key"], err, grad, w["grad"])
        assert abs(sig2 - w["sig2"]) <= 1e-10 * abs(w["sig2"]), (w["key"], sig2, w["sig2"])
        # small_t2 against the oracle's beta, Kq^-1 and c: entries of a Cholesky solve with Q
        # (q = 4), so within a small multiple of eps cond(Q) of the largest
        tol = 64 * np.finfo(float).eps * w["condQ"] * np.max(np.abs(w["T2"]))
        assert np.max(np.abs(T2 - w["T2"])) <= tol, (w["key"], T2, w["T2"])
        assert abs(cfac - w["c"]) <= 1e-12 * w["c"]


# ------------------------------------------------------------------ the argument split
def test_argument_split_table(check):
    cmds, want = [], []
    for d in (1, 3):
        for variant in (0, 1):
            base = d + 1 if variant == 0 else d
            for kernel in (0, 1):
                for n_hp in (base - 1, base, base + 1, base + 2):
                    hp = 0.5 + 0.25 * np.arange(n_hp)
                    cmds.append(f"args {variant} {kernel} {d} {n_hp} {0.125.hex()} {n_hp} {_hex(hp)}")
                    if n_hp in (base, base + 1):
                        fit = n_hp == base + 1
                        want.append((1 - variant, int(fit), hp[d] if fit else 0.125,
                                     hp[-1] * hp[-1] if variant == 0 else 1.0,
                                     1.0 if (variant == 0 and kernel == 1) else 0.0))
                    else:
                        want.append("n_hp inconsistent with d")
    for variant, n_hp in ((2, 4), (-1, 4), (2, 9)):   # (a bad variant is reported before a bad n_hp)
        cmds.append(f"args {variant} 0 3 {n_hp} 0x0p+0 {n_hp} {_hex(np.ones(n_hp))}")
        want.append("bad variant")
    out = check("\n".join(cmds) + "\n")
    assert len(out) == len(want) == 2 * 2 * 2 * 4 + 3
    for cmd, line, w in zip(cmds, out, want):
        if isinstance(w, str):
            assert line == f"args {ERR_ARG} {w}", (cmd, line)
        else:
            tok = line.split()
            assert tok[:4] == ["args", "0", str(w[0]), str(w[1])], (cmd, line)
            (val,) = _fields(line, "val")
            assert list(val) == [w[2], w[3], w[4]], (cmd, line, w)


# ------------------------------------------------------------------ inv_length_scales
def test_inv_length_scales(check):
    d = 5
    cmds, want = [], []
    with np.errstate(divide="ignore", over="ignore"):
        for v, bad in ((0.0, True), (-0.0, True), (np.nan, True), (-2.0, False), (5e-324, False), (np.inf, False)):
            for pos in (0, 2, 4):
                hp = np.array([0.5, 4.0, 0.25, 3.0, 8.0])
                hp[pos] = v
                cmds.append(f"inv {d} {_hex(hp)}")
                inv = 1.0 / hp
                if bad:
                    inv[pos:] = 7.0      # (untouched from the first bad one on)
                want.append((pos if bad else -1, inv))
    out = check("\n".join(cmds) + "\n")
    for cmd, line, (idx, inv) in zip(cmds, out, want):
        tok = line.split()
        assert int(tok[1]) == idx, (cmd, line)
        (got,) = _fields(line[:line.index(" msg ")], "out")
        assert np.array_equal(got, inv), (cmd, got, inv)
        msg = line[line.index(" msg ") + 5:]
        assert msg == (f"length scale delta[{idx}] is zero or NaN" if idx >= 0 else "-"), line


# ------------------------------------------------------------------ the one-launch reader
def _buffer(P, d, nld, nh, tag, logdets, info=0.0, qflag=0.0, partials=None, stale=None):
    h = np.full(P * P + nld + 1 + d + 4 + nh * 64, 99.0)
    h[:P * P] = np.arange(P * P)
    h[P * P:P * P + nld] = logdets
    h[P * P + nld] = info
    h[P * P + nld + 1 + d + 3] = qflag
    part = h[P * P + nld + 1 + d + 4:].reshape(nh, 64)
    part[:] = 0.0
    part[:, :d + 3] = 1.0 if partials is None else partials
    part[:, 63] = tag
    if stale is not None:
        part[stale, 63] = tag - 1.0
    return h


@pytest.mark.parametrize("nld,name", [(1, "k_tiny"), (3, "k_snb")])
def test_one_launch_reader(check, nld, name):
    P, d, nh, tag = 3, 2, 4, 41.0
    lds = [0.1, 0.2, 0.3][:nld]

    def cmd(**kw):
        h = _buffer(P, d, nld, nh, tag, lds, **kw)
        return f"read {P} {d} {nld} {nh} {tag.hex()} {name} {h.size} {_hex(h)}"
    big = np.ones((nh, d + 3))
    big[1, :] = 1e16      # 1 + 1e16 + 1 + 1 in helper order is 1e16; with 1e16 last it is 1e16 + 4
    big[:, 0] = [0.1, 0.2, 0.3, 0.4]
    out = check("\n".join([cmd(), cmd(info=-1.0), cmd(info=-2.0), cmd(info=17.0), cmd(qflag=1.0),
                           cmd(stale=2), cmd(partials=big)]) + "\n")
    acc = 0.0
    for v in lds:
        acc += v
    logdet = 2.0 * acc
    if nld == 1:
        assert logdet == 2.0 * lds[0]
    assert out[0].startswith("read status 0 ") and " q_refused 0 " in out[0] and " sums 0 " in out[0]
    (red,) = _fields(out[0], "red")
    assert out[0].split()[3] == "logdetA" and float.fromhex(out[0].split()[4]) == logdet
    assert list(red) == [float(nh)] * (d + 3)
    assert out[1] == f"read status {ERR_HIP} {name}: a workgroup wait timed out"
    assert out[2] == f"read status {ERR_HIP} {name}: workgroup 0 did not complete"
    assert out[3] == f"read status {NOT_PD} matrix not positive definite (pivot 17)"
    assert " q_refused 1 " in out[4]
    assert out[5].endswith(f" sums {ERR_HIP} {name}: helper 2 did not finish (a wait timed out)")
    (red,) = _fields(out[6], "red")
    in_order = [0.0] * (d + 3)
    for g in range(nh):
        for k in range(d + 3):
            in_order[k] += big[g, k]
    assert list(red) == in_order
    assert in_order[1] == 1e16 and (1.0 + 1.0 + 1.0) + 1e16 != 1e16     # (the order is visible)
    assert in_order[0] == ((0.1 + 0.2) + 0.3) + 0.4


# ------------------------------------------------------------------ kernel codes
def test_kernel_codes(check):
    nu = 0.3
    codes = [a | m32 | m52 for a in (0, 1) for m32 in (0, 0x10) for m52 in (0, 0x20)] + [2, 0x40, 0x11 | 0x80]
    cmds = [f"kernel {code} {predict} {nu.hex()}" for code in codes for predict in (0, 1)]
    out = check("\n".join(cmds) + "\n")
    i = 0
    for code in codes:
        for predict in (0, 1):
            tok = out[i].split()
            i += 1
            valid = (code & ~0x31) == 0 and (code & 0x30) != 0x30
            assert int(tok[1]) == int(valid), (code, out[i - 1])
            assert int(tok[2]) == (code & 1)
            if valid:
                assert int(tok[3]) == (1 if code & 0x10 else 2 if code & 0x20 else 0)
            (consts,) = _fields(out[i - 1], "consts")
            if code & 1:
                assert list(consts) == [1.0, 1.0 + nu * nu if predict else 1.0]
            else:
                assert list(consts) == [1.0 - nu, 1.0 if predict else 1.0 - nu]
