#!/usr/bin/env python
"""Time one multi-output member of a resident emulator set (gpe_hm_add_multi) against the route
the package had before it: a set of p gpe_hm_add members, one per output, built from the same
data, the same factor and the same B and Sigma-hat -- what ``MultiEmulator.single(j)`` items
cost.  Same candidates, one process.  One JSON line per (n, p), printed and appended to the log.

    python tools/implausibility_multi_time.py                     # n = 128, 300, 512; p = 4, 8, 16
    python tools/implausibility_multi_time.py --ns 300 --ps 8 --m 1000000 --reps 5

  multi_ms        gpe_hm_implausibility on the set of one multi-output member, the whole call
                  (upload, kernel, selection, download) between device synchronisations: median
                  of --reps after a warm-up call; multi_all_ms the single times
  singles_ms      the same call on the set of p single-output members (the baseline)
  one_single_ms   the same call on a set of one single-output member (the last output), maxno = 1
  mv_ms           gpe_hm_implausibility_mv on the multi-output member (the joint measure)
  speedup         singles_ms / multi_ms;  of_one_single  multi_ms / one_single_ms
  setup_multi_ms, setup_singles_ms   building each set: upload, factorisation, triangular
                  inverse and snapshot (once per wave, not per call)
  max_rel_diff    max |I_multi - I_singles| / I_singles over candidates and the maxno columns
                  (--maxno, default 1: the largest implausibility per candidate, as nonimp_data
                  asks; with maxno = p the call returns m x p values and the copies show)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, reps):
    from gp_emu_uqsa_amd import native
    wall, res = [], None
    for _ in range(reps):
        native.device_synchronize(0)
        t0 = time.perf_counter()
        res = call()
        native.device_synchronize(0)
        wall.append((time.perf_counter() - t0) * 1e3)
    return res, wall


def outputs(X, p, seed=3):
    """p smooth, linearly independent outputs of the inputs X plus a little noise."""
    n, d = X.shape
    rs = np.random.RandomState(seed)
    W = rs.normal(size=(d, p))
    ph = rs.uniform(0, 2 * np.pi, size=p)
    return np.ascontiguousarray(np.sin(X @ W * 1.5 + ph) + 0.3 * (X ** 2) @ rs.normal(size=(d, p))
                                + 0.02 * rs.normal(size=(n, p)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ns", default="128,300,512")
    ap.add_argument("--ps", default="4,8,16")
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--maxno", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "implausibility_multi_time.log"))
    args = ap.parse_args(argv)

    from gp_emu_uqsa_amd import native, synthetic
    d, m, nu = args.d, args.m, 1e-3
    q = d + 1
    delta = np.linspace(0.5, 1.1, d)
    hdim, hval = [-1] + list(range(d)), [1.0] + [0.0] * d
    active = list(range(d))
    x = np.random.default_rng(7).random((m, d))
    ctx = native.default_context()
    sync = lambda: native.device_synchronize(0)
    for n in (int(v) for v in args.ns.split(",")):
        X, _, H = synthetic.problem(n, d, seed=1)
        for p in (int(v) for v in args.ps.split(",")):
            F = outputs(X, p)
            ctx.set_data(X, F[:, 0], H)
            ctx.set_outputs(F)
            _, _, Sigma, B = ctx.objective_multi(native.KERNEL_STD, delta, nu_fixed=nu, want_grad=False)
            zs = F.mean(axis=0) + 0.5 * np.sqrt(np.diag(Sigma))
            ve = 0.05 * np.diag(Sigma)
            V = np.diag(ve) + 0.3 * np.sqrt(np.outer(ve, ve)) * (1.0 - np.eye(p))
            out = {"n": n, "d": d, "q": q, "p": p, "m": m, "maxno": min(args.maxno, p)}
            multi, singles, one = native.EmulatorSet(0), native.EmulatorSet(0), native.EmulatorSet(0)
            try:
                sync()
                t0 = time.perf_counter()
                ctx.set_data(X, F[:, 0], H)
                ctx.set_outputs(F)
                ctx.factor(native.KERNEL_STD, delta, nu, 1.0, 0.0)
                multi.add_multi(ctx, active, hdim, hval, B, Sigma)
                sync()
                out["setup_multi_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                for j in range(p):
                    ctx.set_data(X, F[:, j], H)
                    ctx.factor(native.KERNEL_STD, delta, nu, 1.0, 0.0)
                    singles.add(ctx, active, hdim, hval, B[:, j], float(np.sqrt(Sigma[j, j])))
                sync()
                out["setup_singles_ms"] = (time.perf_counter() - t0) * 1e3
                one.add(ctx, active, hdim, hval, B[:, p - 1], float(np.sqrt(Sigma[p - 1, p - 1])))
                k = out["maxno"]
                calls = {"multi": lambda: multi.implausibility(x, zs, ve, maxno=k),
                         "singles": lambda: singles.implausibility(x, zs, ve, maxno=k),
                         "one_single": lambda: one.implausibility(x, zs[p - 1:], ve[p - 1:], maxno=1),
                         "mv": lambda: multi.implausibility_mv(0, x, zs, V)}
                res = {}
                for name, call in calls.items():
                    call()   # warm-up
                    res[name], wall = timed(call, args.reps)
                    out[name + "_ms"], out[name + "_all_ms"] = statistics.median(wall), wall
                out["speedup"] = out["singles_ms"] / out["multi_ms"]
                out["of_one_single"] = out["multi_ms"] / out["one_single_ms"]
                out["max_rel_diff"] = float(np.max(np.abs(res["multi"] - res["singles"]) / res["singles"]))
                out["mv_i2_median"] = float(np.median(res["mv"]))
            finally:
                multi.close()
                singles.close()
                one.close()
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
