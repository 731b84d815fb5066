"""The host side of the int8 products (gpemu_ozaki.hpp: the moduli, beta, the CRT constants,
the tile lists, the TRTRI pair plans) checked by a stand-alone program with no HIP runtime
call, tests/host/oz_plan_check.cpp: it needs hipcc (the header holds the kernels too) but no
GPU.  Built with the host-side address and undefined-behaviour sanitizers where their runtime
links (a stand-alone binary: nothing is preloaded), plainly otherwise."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "oz_plan_check.cpp")
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")
SAN = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def _hipcc():
    cand = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return cand if os.path.exists(cand) else shutil.which("hipcc")


_RUN = {}   # the program is built and run once a session (test_oz_product_ref_host.py reads it too)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if "run" not in _RUN:
        _RUN["run"] = _build_and_run(tmp_path_factory)
    return _RUN["run"]


def _build_and_run(tmp_path_factory):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc: the host check of the int8 plans cannot be built")
    exe = str(tmp_path_factory.mktemp("oz_host") / "oz_plan_check")
    base = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", CSRC, SRC, "-o", exe]
    built = subprocess.run(base + SAN, capture_output=True, text=True)
    sanitized = built.returncode == 0
    if not sanitized:   # (no sanitizer runtime on this machine)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print("sanitizers:", sanitized)
    print(run.stdout[-4000:], run.stderr[-4000:])
    return run


def test_int8_constants_lists_and_plans(plan_check):
    assert plan_check.returncode == 0, plan_check.stdout[-4000:] + plan_check.stderr[-4000:]
    assert plan_check.stdout.strip().endswith("oz_plan_check OK")


def test_beta_claims_match_oz_consts(plan_check):
    """The operand bits quoted beside the fewer-moduli runs are what oz_consts gives:
    test_gpu_ozaki.py's docstring for 12 moduli at n_pad 4096 (40; it said 41), and the
    figures of DESIGN.md section 6.3 for 14 and 12 moduli at 16384 (47, 39)."""
    out = plan_check.stdout
    b12_4096 = int(re.search(r"beta12_4096=(\d+)", out).group(1))
    b12, b14 = (int(v) for v in re.search(r"beta12_16384=(\d+) beta14_16384=(\d+)", out).groups())
    with open(os.path.join(ROOT, "tests", "test_gpu_ozaki.py")) as fh:
        claim = re.search(r"GPEMU_OZAKI_MODULI=12 \(beta = (\d+) bits at n_pad = 4096\)", fh.read())
    assert claim and int(claim.group(1)) == b12_4096 == 40
    assert (b14, b12) == (47, 39)
