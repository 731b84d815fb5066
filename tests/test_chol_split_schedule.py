"""Host-side check of the split Cholesky schedule (add_sweep(o, NC, NR), gpemu_chol_sched.hpp), on
the launches the real builder makes: tests/host/chol_sched_check.cpp builds the plan of every size
and, with --emit, lists launch by launch the factored columns with their pending sources and the
bulk updates (columns [a, b) by columns [g0, g0 + k)) as it reads them off the descriptors -- the
target columns from the C pointer, the source column from the A pointer, the width from K -- in
the sweep's local tile columns.  Checked here for NB = 8 ... 130, the default widths /
super-blocks and widths 1-8, for the per-step (fused) and the group launches:
  phase A = sweep(h, NB) (h the largest power of two below NB): no column >= h is written, and
      every column < h has received every earlier column exactly once when it is factored, each
      from a column factored before;
  phase C = sweep(NB - h, NB - h) is the unsplit schedule of NB - h columns: the same function
      the whole factorisation (NB, NB) uses, which passes the same check;
  the nested split's sweeps (q, NB) and (h - q, NB - q), q = h / 2, where h is a multiple of 4.
"""
import subprocess

import numpy as np
import pytest

from test_chol_sched_host import build_check

DEFAULT = ([(4, 48), (2, 24)], 2, 80)   # CholSchedParams: groups, sb, sb_min


@pytest.fixture(scope="module")
def sched_check(tmp_path_factory):
    return build_check(tmp_path_factory)


def emitted(exe, env, ci):
    """{(NB, NC, NR): [per-step launches, group launches]} of configuration ci; a launch is a list
    of ("bulk", a, b, g0, k) and ("factor", t, p0) entries in its problems' order."""
    run = subprocess.run([exe, "--emit", str(ci)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out = {}
    for line in run.stdout.splitlines():
        head, *ls = line.split(" |")
        tag, cfg, NB, NC, NR, grp = head.split()
        assert tag == "SWEEP" and int(cfg) == ci
        launches = []
        for l in ls:
            tok, launch, i = l.split(), [], 0
            while i < len(tok):
                n = 3 if tok[i] == "F" else 5
                launch.append(("factor" if tok[i] == "F" else "bulk",) + tuple(int(x) for x in tok[i + 1:i + n]))
                i += n
            launches.append(launch)
        out.setdefault((int(NB), int(NC), int(NR)), [None, None])[int(grp)] = launches
    return out


def check(launches, NC):
    """Every column < NC factored once, in order, having received each earlier column exactly
    once, each from a column factored before; nothing written at or past column NC."""
    got = np.zeros((NC, NC), dtype=np.int32)   # got[j, i]: updates of column j by column i
    done = 0                                   # columns [0, done) are factored
    for launch in launches:
        for e in launch:
            if e[0] == "factor":
                _, t, p0 = e
                assert t == done and t < NC and 0 <= p0 <= t
                got[t, p0:t] += 1
                assert np.all(got[t, :t] == 1), (t, got[t, :t])
                done += 1
            else:
                _, a, b, g0, k = e
                assert done <= a < b <= NC, (e, done)        # columns not yet factored, below NC
                assert 0 <= g0 and k > 0 and g0 + k <= done, (e, done)   # sources already factored
                got[a:b, g0:g0 + k] += 1
    assert done == NC
    assert np.all(np.tril(got, -1) == np.tril(np.ones((NC, NC), dtype=np.int32), -1))
    assert not np.any(np.triu(got))


CONFIGS = ([DEFAULT] + [([(w, 0)], 2, 80) for w in range(1, 9)] + [([(w, 0)], 1, 80) for w in (2, 4)] +
           [([(w, 0)], 3, 0) for w in (2, 4)])


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"w{c[0]}-sb{c[1]}-{c[2]}")
def test_split_schedule(sched_check, cfg):
    got = emitted(*sched_check, CONFIGS.index(cfg))   # (chol_sched_check.cpp's coverage_configs: the same list)
    for NB in range(8, 131):
        h = 1
        while 2 * h < NB:
            h *= 2
        sweeps = [(h, NB), (NB - h, NB - h), (NB, NB)]   # phase A, phase C, unsplit
        if h % 4 == 0:
            sweeps += [(h // 2, NB), (h - h // 2, NB - h // 2)]   # the nested split's
        for NC, NR in sweeps:
            fused, grp = got[(NB, NC, NR)]
            check(fused, NC)
            check(grp, NC)


def test_split_column():
    """h is the top TRTRI pair's: the largest power of two below NB (trtri_level_pairs)."""
    for NB in range(2, 600):
        h = 1
        while 2 * h < NB:
            h *= 2
        s = 2
        while s // 2 < NB:   # the last level: one pair (0, s / 2, NB)
            top = s // 2
            s *= 2
        assert h == top and h < NB <= 2 * h
