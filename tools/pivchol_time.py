#!/usr/bin/env python
"""Time gpe_posterior_pivchol on the synthetic problem bench.py uses, and the host routes it
replaces, and print one JSON line.

    python tools/pivchol_time.py                       # n = 16384, d = 10; shapes 16384:128 and 4096:4096
    python tools/pivchol_time.py --n 4096 --shapes 1024:64,1024:1024 --reps 3

Per shape m:k (m test points, at most k pivots; L is returned when k > 128):
  wall_ms    the whole call between gpe_device_synchronize brackets, best of --reps after a warm-up
  form_ms / steps_ms / trailing_ms   the call's device phases from one profiled call
             (gpe_phase_times: forming the covariance, the k one-launch pivot steps, the
             trailing updates S -= W W^T with the panels' copies into L)
  step_us, step_bytes, step_gbps   per pivot step: time, bytes moved (a column of S, the
             slab of the panel's earlier columns, d and the flags) and the bandwidth they give
  launches   kernel launches of the pivot loop (init + steps + trailing updates + panel copies)
  dpstrf_ms  scipy.linalg.lapack.dpstrf of the downloaded covariance on this host (--host)
  solve_ms   the np.linalg.solve route of Posterior.mahalanobis_distance (--host, k = m shapes)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--shapes", default="16384:128,4096:4096", help="comma-separated m:k")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="also time dpstrf / np.linalg.solve on the host")
    ap.add_argument("--host-max-m", type=int, default=16384, help="largest m the host routes are timed at")
    args = ap.parse_args(argv)

    from gp_emu_uqsa_amd import native, synthetic
    ctx = native.Context(0)
    X, f, H = synthetic.problem(args.n, args.d, seed=0)
    ctx.set_data(X, f, H)
    ctx.factor(native.KERNEL_STD, np.ones(args.d), 1e-3, 1.0, 0.0)
    beta = ctx.beta()
    sigma = 1.0
    out = {"n": args.n, "d": args.d, "shapes": []}
    for spec in args.shapes.split(","):
        m, k = (int(v) for v in spec.split(":"))
        xs = synthetic.design(m, args.d, seed=7)
        hs = synthetic.linear_basis(xs)
        ys = synthetic.outputs(xs, seed=7)
        want_L = k > 128

        def call():
            return ctx.posterior_pivchol(xs, hs, beta, sigma, k=k, want_L=want_L)

        call()   # warm-up: workspaces, L^-1
        wall = []
        for _ in range(args.reps):
            native.device_synchronize(0)
            t0 = time.perf_counter()
            res = call()
            native.device_synchronize(0)
            wall.append((time.perf_counter() - t0) * 1e3)
        ctx.set_profiling(True)
        call()
        ph = np.zeros(8)
        ctx._check(ctx.lib.gpe_phase_times(ctx._h, native._ptr(ph), 8), "gpe_phase_times")
        ctx.set_profiling(False)
        rank = res[4]
        mp = -(-m // 128) * 128
        npan = -(-k // 128)
        # a step in column j of its panel reads j earlier columns of the panel: (127 / 2) on
        # average over a full panel, (k - 1) / 2 when k < 128
        avg_cols = (min(k, 128) - 1) / 2.0
        step_bytes = mp * 8 * (1 + avg_cols + 1 + 2) + mp * 4 * 2
        step_us = ph[1] * 1e3 / max(rank, 1)
        row = {"m": m, "k": k, "rank": rank, "want_L": want_L, "wall_ms": min(wall), "form_ms": ph[0],
               "steps_ms": ph[1], "trailing_ms": ph[2], "step_us": step_us, "step_bytes": step_bytes,
               "step_gbps": step_bytes / (step_us * 1e-6) / 1e9,
               "launches": k + (npan - 1) + 1 + (npan if want_L else 0), "trailing_updates": npan - 1}
        if args.host and m <= args.host_max_m:
            from scipy.linalg import lapack
            mean, S = ctx.posterior(xs, hs, beta, sigma, full_var=True)
            t0 = time.perf_counter()
            _, piv, hrank, info = lapack.dpstrf(S, lower=1)
            row["dpstrf_ms"] = (time.perf_counter() - t0) * 1e3
            row["dpstrf_pivots_equal"] = int(np.sum(np.cumprod(piv[:rank] - 1 == res[1])))
            if k == m:
                e = ys - mean
                t0 = time.perf_counter()
                md = e.dot(np.linalg.solve(S, e))
                row["solve_ms"] = (time.perf_counter() - t0) * 1e3
                from scipy.linalg import solve_triangular
                t0 = time.perf_counter()
                dpc = solve_triangular(res[3][res[1]], e[res[1]], lower=True)
                row["errors_host_ms"] = (time.perf_counter() - t0) * 1e3
                row["mahalanobis_rel_diff"] = abs(np.sum(dpc ** 2) - md) / md
            del S
        out["shapes"].append(row)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
