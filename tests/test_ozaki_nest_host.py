"""The host side of the nested split Cholesky's int8 product (gpemu_ozaki.hpp: OzCholNest, the
capped-lower OzShape, its list, operation count, residue-tile index and buffer sizes) checked
by a stand-alone program with no HIP runtime call, tests/host/oz_nest_check.cpp, for every
n_pad from 1024 to 65536 at which the plan can nest: it needs hipcc (the header holds the
kernels too) but no GPU.  Built with the host-side address and undefined-behaviour sanitizers
where their runtime links (a stand-alone binary: nothing is preloaded), plainly otherwise."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "oz_nest_check.cpp")
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")
SAN = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def test_nested_split_plans(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hipcc = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc: the host check of the nested split's plan cannot be built")
    exe = str(tmp_path / "oz_nest_check")
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
    assert run.stdout.strip().endswith("oz_nest_check OK")
    # n_pad 1024 (NB 8, h 4, q 2) is the smallest that nests; NB in (4, 8] has q = 2, and from
    # there on every h = 2^k >= 4 has an even q: every size from 640 on that splits nests
    assert int(re.search(r"nested=(\d+)", run.stdout).group(1)) > 400
