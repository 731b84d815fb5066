"""Host-side check of the split Cholesky schedule (build_plan's sweep(o, NC, NR), gpemu.hip): a
Python mirror of its column bookkeeping -- the groups, the super-blocks with their lazy far
updates and the balanced bulk segments -- for the per-step (fused) and the group launches.

sweep(NC, NR) here lists, launch by launch, the factored columns with their pending sources and
the bulk updates (columns [a, b) by columns [g0, g0 + k)), in local tile columns.  Checked for
NB = 8 ... 130, the default widths / super-blocks and widths 1-8:
  phase A = sweep(h, NB) (h the largest power of two below NB): no column >= h is written, and
      every column < h has received every earlier column exactly once when it is factored, each
      from a column factored before;
  phase C = sweep(NB - h, NB - h) is the unsplit schedule of NB - h columns: the same function
      the whole factorisation uses, which passes the same check, and whose groups do not depend
      on the origin.
"""
import numpy as np
import pytest

DEFAULT = ([(4, 48), (2, 24)], 2, 80)   # potrf_groups, potrf_sb, potrf_sb_min


def sweep(NC, NR, groups, sb, sb_min):
    """-> (fused launches, group launches); a launch is a list of ("bulk", a, b, g0, k) and
    ("factor", t, p0) entries in an order its waits allow."""
    gs, g = [], 0
    while g < NC:
        gs.append(g)
        w = 1
        for wd, lim in groups:
            if NR - g > lim:
                w = wd
                break
        g += max(1, min(w, NC - g))
    gs.append(NC)
    ng = len(gs) - 1
    sbs, sbe, src0 = [0] * ng, [0] * ng, [0] * ng
    cur = cnt = 0
    for gi in range(ng):
        w = gs[gi + 1] - gs[gi]
        if gi <= 1 or w < 2 or w != gs[gi] - gs[gi - 1] or cnt >= sb or NR - gs[gi] <= sb_min:
            cur, cnt = gs[gi], 0
        sbs[gi] = cur
        cnt += 1
    for gi in range(ng - 1, -1, -1):
        sbe[gi] = sbe[gi + 1] if gi + 1 < ng and sbs[gi + 1] == sbs[gi] else gs[gi + 1]
    for gi in range(1, ng):
        src0[gi] = sbs[gi - 1] if sbs[gi] == gs[gi] else gs[gi - 1]

    def cost(j, k):
        return float(NR - j) * k

    segs = [[] for _ in range(ng)]   # (a, b, g0, k): k source columns from g0
    for gi in range(1, ng):
        if gs[gi + 1] < sbe[gi]:
            segs[gi].append((gs[gi + 1], sbe[gi], src0[gi], gs[gi] - src0[gi]))
    for gi in range(1, ng):
        if sbs[gi] != gs[gi]:
            continue
        s0, s1, se = sbs[gi - 1], gs[gi], sbe[gi]
        kf = s1 - s0
        mem = [gj for gj in range(gi, ng) if sbs[gj] == sbs[gi]]
        fixed = []
        for gj in mem:
            kb = gs[gj] - src0[gj]
            fx = sum(cost(j, kb) for j in range(gs[gj] + 1, gs[gj + 1]))
            fx += sum(cost(j, k) for a, b, _, k in segs[gj] for j in range(a, b))
            fixed.append(fx)
        tot = sum(fixed) + sum(cost(j, kf) for j in range(se, NC))
        j = se
        for m, gj in enumerate(mem):
            want = max(0.0, tot / len(mem) - fixed[m])
            a, got = j, 0.0
            while j < NC and (m + 1 == len(mem) or got + 0.5 * cost(j, kf) <= want):
                got += cost(j, kf)
                j += 1
            if j > a:
                segs[gj].append((a, j, s0, kf))

    fused, grp = [], []
    for gi in range(ng):
        gb, ge = gs[gi], gs[gi + 1]
        W1 = ge - gb
        part = [[] for _ in range(W1)]
        if gi > 0:
            kb = gb - src0[gi]
            load = [float(NR - (gb + h + 1)) * kb if h + 1 < W1 else 0.0 for h in range(W1)]
            tot = sum(load)
            cols = []
            for si, (a, b, _, k) in enumerate(segs[gi]):
                for j in range(a, b):
                    cols.append((j, si))
                    tot += float(NR - j) * k
            u, cum = 0, 0.0
            for h in range(W1):
                cum += load[h]
                target = tot * (h + 1) / W1
                while u < len(cols):
                    j, si = cols[u]
                    _, _, g0, k = segs[gi][si]
                    cj = float(NR - j) * k
                    if h < W1 - 1 and cum + 0.5 * cj > target:
                        break
                    cum += cj
                    part[h].append((j, j + 1, g0, k))
                    u += 1
            assert u == len(cols)
        for h in range(W1):
            t = gb + h
            launch = [("factor", t, src0[gi] if h == 0 else gb)]
            if gi > 0:
                if h + 1 < W1:
                    launch.append(("bulk", t + 1, t + 2, src0[gi], gb - src0[gi]))
                launch += [("bulk",) + sg for sg in part[h]]
            fused.append(launch)
        if W1 < 2:
            grp.append(fused[-1])
            continue
        launch = []
        if gi > 0:
            launch += [("bulk", gb + h, gb + h + 1, src0[gi], gb - src0[gi]) for h in range(1, W1)]
        launch += [("factor", gb + h, src0[gi] if h == 0 else gb) for h in range(W1)]
        launch += [("bulk",) + sg for sg in segs[gi]]
        grp.append(launch)
    return fused, grp


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
def test_split_schedule(cfg):
    for NB in range(8, 131):
        h = 1
        while 2 * h < NB:
            h *= 2
        for NC, NR in ((h, NB), (NB - h, NB - h), (NB, NB)):   # phase A, phase C, unsplit
            fused, grp = sweep(NC, NR, *cfg)
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
