"""The host side of the grouped GEMM's launches (gpemu_gemm_sched.hpp: the kind table, the
descriptors of a launch, split_k, xcd_order / order_tiles / list_launch) checked by a
stand-alone program with no HIP runtime call, tests/host/gemm_sched_check.cpp: it needs hipcc
(the header includes the kernels') but no GPU.  Built with the host-side address and
undefined-behaviour sanitizers where their runtime links (a stand-alone binary: nothing is
preloaded), plainly otherwise.  Both the single-GPU schedules and the row-block ones are
assembled from these functions, so the tile orders pinned there hold for both."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "gemm_sched_check.cpp")
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")
SAN = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def _hipcc():
    cand = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return cand if os.path.exists(cand) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def sched_check(tmp_path_factory):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc: the host check of the GEMM launch layer cannot be built")
    exe = str(tmp_path_factory.mktemp("gemm_sched") / "gemm_sched_check")
    base = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", CSRC, SRC, "-o", exe]
    built = subprocess.run(base + SAN, capture_output=True, text=True)
    sanitized = built.returncode == 0
    if not sanitized:   # (no sanitizer runtime on this machine)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    print("sanitizers:", sanitized)
    return exe, env


def test_kinds_descriptors_orders_and_split(sched_check):
    exe, env = sched_check
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout[-4000:], run.stderr[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("gemm_sched_check OK")


def test_digests_option_prints_the_pinned_table(sched_check):
    """--digests prints what the program pins, one initialiser a line: the way to re-pin."""
    exe, env = sched_check
    run = subprocess.run([exe, "--digests"], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    with open(SRC) as fh:
        src = fh.read()
    lines = [ln.strip() for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 9
    for ln in lines:
        assert ln in src, ln
