"""The TRTRI's block pairs by side of the split Cholesky's column (trtri_side_pairs) and
split_k's whole-level decision, for NB = 2 ... 130, checked by a stand-alone program with no HIP
runtime call, tests/host/trtri_sides_check.cpp: it needs hipcc (the headers hold the kernels
too) but no GPU.  Built with the host-side address and undefined-behaviour sanitizers where
their runtime links (a stand-alone binary: nothing is preloaded), plainly otherwise."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "trtri_sides_check.cpp")
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")
SAN = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def test_sides_cover_every_pair_once_with_the_levels_split_k(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hipcc = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc: the host check of the TRTRI sides cannot be built")
    exe = str(tmp_path / "trtri_sides_check")
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
    assert run.stdout.strip().endswith("trtri_sides_check OK")
