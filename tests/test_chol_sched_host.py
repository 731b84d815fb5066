"""The factorisation plan (gpemu_chol_sched.hpp: build_chol_plan, which gpemu.hip's build_plan
uploads the result of) checked by a stand-alone program with no HIP runtime call,
tests/host/chol_sched_check.cpp: it needs hipcc (the header includes the kernels') but no GPU.
Built with the host-side address and undefined-behaviour sanitizers where their runtime links
(a stand-alone binary: nothing is preloaded), plainly otherwise.

It reads the real descriptors: for NB = 8 ... 130, the default widths / super-blocks, widths 1-8
and the super-block variants, every sweep -- (h, NB), (NB - h, NB - h), (NB, NB) and the nested
split's (q, NB), (h - q, NB - q) -- per step and by groups factors every column once and in
order, each having received every earlier column's update exactly once from a column already
factored, and writes nothing at or past its last column; every launch with a ticket stores a
list in which no tile waits on a later one and every counter is awaited for as many tiles as
post it; an optional part whose descriptors do not fit leaves the plan built without it; and the
whole plan of the pinned configurations has the digest it had before the builder moved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "chol_sched_check.cpp")
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")
SAN = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def _hipcc():
    cand = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return cand if os.path.exists(cand) else shutil.which("hipcc")


_BUILT = {}


def build_check(tmp_path_factory):
    """The program, built once per session (tests/test_chol_split_schedule.py runs it too)."""
    if "exe" in _BUILT:
        return _BUILT["exe"], _BUILT["env"]
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc: the host check of the factorisation plan cannot be built")
    exe = str(tmp_path_factory.mktemp("chol_sched") / "chol_sched_check")
    base = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-I", CSRC, SRC, "-o", exe]
    built = subprocess.run(base + SAN, capture_output=True, text=True)
    sanitized = built.returncode == 0
    if not sanitized:   # (no sanitizer runtime on this machine)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    print("sanitizers:", sanitized)
    _BUILT["exe"] = exe
    _BUILT["env"] = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    return _BUILT["exe"], _BUILT["env"]


@pytest.fixture(scope="module")
def sched_check(tmp_path_factory):
    return build_check(tmp_path_factory)


def test_coverage_waits_rollback_and_digests(sched_check):
    exe, env = sched_check
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout[-4000:], run.stderr[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("chol_sched_check OK")


def test_digests_option_prints_the_pinned_table(sched_check):
    """--digests prints what the program pins, one initialiser a line: the way to re-pin."""
    exe, env = sched_check
    run = subprocess.run([exe, "--digests"], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    with open(SRC) as fh:
        src = fh.read()
    lines = [ln.strip() for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 9
    for ln in lines:
        assert ln in src, ln
