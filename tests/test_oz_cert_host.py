"""The 15-moduli certificate of the int8 products (gpemu_ozaki.hpp: oz_cert_term, oz_cert_ok,
the threshold T15 and oz_consts_cert) in its host form, checked against 128-bit integers by a
stand-alone program with no HIP runtime call, tests/host/oz_cert_check.cpp: it needs hipcc (the
header holds the kernels too) but no GPU.  Built with the host-side address and
undefined-behaviour sanitizers where their runtime links (a stand-alone binary: nothing is
preloaded), plainly otherwise."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "oz_cert_check.cpp")
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")
SAN = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def test_certificate(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hipcc = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc: the host check of the certificate cannot be built")
    exe = str(tmp_path / "oz_cert_check")
    base = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", CSRC, SRC, "-o", exe]
    built = subprocess.run(base + SAN, capture_output=True, text=True)
    sanitized = built.returncode == 0
    if not sanitized:
        # plainly only where the sanitizers' runtime is not installed (the linker says so); any
        # other failure of the sanitized build is a failure
        out = built.stdout + built.stderr
        assert re.search(r"(cannot find|no such file).*(asan|ubsan|clang_rt)", out, re.I | re.S), out
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print("sanitizers:", sanitized)
    print(run.stdout[-4000:], run.stderr[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("oz_cert_check OK")
    assert int(re.search(r"pairs=(\d+)", run.stdout).group(1)) == 100000
    assert int(re.search(r"certified=(\d+)", run.stdout).group(1)) > 10000
