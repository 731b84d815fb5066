"""How the library's device buffers grow (gpemu_host_alloc.hpp) checked against a stub
allocator that can fail, by the stand-alone program tests/host/grow_check.cpp: no HIP runtime
call and no GPU.  Built with the host-side address and undefined-behaviour sanitizers where
their runtime links (a stand-alone binary: nothing is preloaded), plainly otherwise."""
import os
import subprocess

import pytest

from test_ozaki_host import CSRC, ROOT, SAN, _hipcc

SRC = os.path.join(ROOT, "tests", "host", "grow_check.cpp")


def test_failed_growth_leaves_no_stale_capacity(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc: the host check cannot be built")
    exe = str(tmp_path / "grow_check")
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
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("grow_check OK")
