"""The two-slot chunk pipeline of the posterior paths (csrc/gpemu_chunk_pipe.hpp) driven by a
stand-alone program, tests/host/chunk_pipe_check.cpp, with recording callbacks: any C++17
compiler, no HIP, no GPU.  Built with the address and undefined-behaviour sanitizers where their
runtime links (a stand-alone binary: nothing is preloaded), plainly otherwise.

The expected call sequence is written out here from the pipeline's rule, not from the header:
dev of chunk i into slot i % 2, then wait and host of chunk i - 1 (slot (i - 1) % 2), the last
chunk's wait and host after the loop, no drain; a failing dev or wait ends the sequence there
with one drain and its return code."""
import os
import subprocess

import pytest

from test_objective_host import SAN, _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "chunk_pipe_check.cpp")
CSRC = os.path.join(ROOT, "gp_emu_uqsa_amd", "csrc")
SHAPES = [(1, 256), (256, 256), (257, 256), (1000, 256), (8322, 8192)]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(text) -> the program's output lines for the commands in text."""
    cxx = _cxx()
    if not cxx:
        pytest.skip("no C++ compiler: the host check of the chunk pipeline cannot be built")
    exe = str(tmp_path_factory.mktemp("chunk_pipe") / "chunk_pipe_check")
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
        assert lines[-1] == "chunk_pipe_check OK"
        return [ln.split() for ln in lines[:-1]]
    return run


def expected(m, chunk, fail=None, at=None, code=0):
    """The calls of a run, in order, and its return code."""
    n = -(-m // chunk)
    calls = []

    def stop():
        return calls + ["drain", "rc", str(code)]
    for i in range(n + 1):
        if i < n:
            calls.append(f"d{i}/{i % 2}")
            if fail == "dev" and at == i:
                return stop()
        if i >= 1:
            calls.append(f"w{(i - 1) % 2}")
            if fail == "wait" and at == i - 1:
                return stop()
            calls.append(f"h{i - 1}/{(i - 1) % 2}")
    return calls + ["rc", "0"]


@pytest.mark.parametrize("m,chunk", SHAPES)
def test_call_sequence(check, m, chunk):
    (got,) = check(f"run {m} {chunk} none 0 0\n")
    n = -(-m // chunk)
    assert got == expected(m, chunk)
    # the properties, read off the recorded calls themselves
    devs = [c for c in got if c.startswith("d") and c != "drain"]
    hosts = [c for c in got if c.startswith("h")]
    assert len(devs) == n == (m + chunk - 1) // chunk
    assert devs == [f"d{i}/{i % 2}" for i in range(n)]                  # the slots alternate
    assert hosts == [f"h{i}/{i % 2}" for i in range(n)]                 # once each, in order
    for i in range(1, n):                                               # dev(i) before wait / host(i - 1)
        assert got.index(f"d{i}/{i % 2}") < got.index(f"h{i - 1}/{(i - 1) % 2}")
        assert got[got.index(f"h{i - 1}/{(i - 1) % 2}") - 1] == f"w{(i - 1) % 2}"
        if i + 1 < n:                                                   # and host(i - 1) before dev(i + 1)
            assert got.index(f"h{i - 1}/{(i - 1) % 2}") < got.index(f"d{i + 1}/{(i + 1) % 2}")
    assert got[-4:-2] == [f"w{(n - 1) % 2}", f"h{n - 1}/{(n - 1) % 2}"]
    assert "drain" not in got and got[-2:] == ["rc", "0"]


@pytest.mark.parametrize("m,chunk", SHAPES)
def test_injected_failures(check, m, chunk):
    n = -(-m // chunk)
    cases = [(kind, at) for kind, ats in (("dev", (0, 1, n - 1)), ("wait", (0, n - 1)))
             for at in sorted(set(a for a in ats if a < n))]
    codes = {("dev", 0): -2, ("dev", 1): 1, ("dev", n - 1): -4, ("wait", 0): -2, ("wait", n - 1): 7}
    out = check("".join(f"run {m} {chunk} {kind} {at} {codes[kind, at]}\n" for kind, at in cases))
    assert len(out) == len(cases)
    for (kind, at), got in zip(cases, out):
        code = codes[kind, at]
        assert got == expected(m, chunk, kind, at, code), (kind, at)
        assert got[-2:] == ["rc", str(code)]                            # that code comes back
        assert got.count("drain") == 1 and got[-3] == "drain"           # one drain, and nothing after it
        failed = f"d{at}/{at % 2}" if kind == "dev" else f"w{at % 2}"
        assert got[-4] == failed                                        # no dev, wait or host after the failure
        # what ran before it is the start of the successful run
        good = expected(m, chunk)
        assert got[:-3] == good[:len(got) - 3]
