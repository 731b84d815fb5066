#!/usr/bin/env python
"""Time gpe_posterior_groups beside gpe_posterior(full_var=0, precision=64) on the same points,
factor and process (the synthetic problem bench.py uses).  One JSON line per shape and family,
printed and appended to the log.

    python tools/posterior_groups_time.py                    # n = 16384, d = 10, G = 12, m = 12 * 8192 * 4
    python tools/posterior_groups_time.py --shapes 4096:12:98304 --kernels matern52 --example 8192

  groups_ms        gpe_posterior_groups, the whole call (upload, kernels, download, host finish)
                   between gpe_device_synchronize brackets: best of --reps after a warm-up call
  posterior_ms     gpe_posterior(full_var=0) the same way
  ratio            groups_ms / posterior_ms (the n^2 m product in front of both dominates)
  kernel_ms        the device time of k_post_groupgram + k_post_groupcov summed over the chunks of
                   one profiled call (gpe_phase_times: events around the pair, one synchronisation
                   per chunk), and kernel_ms_per_chunk
  v_bytes_per_s    n_pad * m * 8 / kernel time: the one pass over V
  max_diag_diff    max |cov[g, a, a] - posterior's variance| over the points
k_colnorm2, which the pair replaces, has no phase of its own: its time per chunk comes from a
kernel trace of this tool (the profiler's own statistics of a run started under it).

--example N adds mc_emulator_indices' work at N samples on the same factor: the Saltelli
groups of d + 2 points from sobol_points(d, N, 1, "uniform", 0.5, 1 / 12), one posterior_groups
call and sobol_group_estimates; example_ms is the whole of it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, reps):
    wall = []
    from gp_emu_uqsa_amd import native
    for _ in range(reps):
        native.device_synchronize(0)
        t0 = time.perf_counter()
        res = call()
        native.device_synchronize(0)
        wall.append((time.perf_counter() - t0) * 1e3)
    return res, wall


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="16384:12:393216", help="n:G:m,n:G:m,...")
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--kernels", default="gaussian")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--example", type=int, default=0, help="samples of the mc_emulator_indices example (0: skip)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "posterior_groups_time.log"))
    args = ap.parse_args(argv)

    from gp_emu_uqsa_amd import native, synthetic
    from gp_emu_uqsa_amd import sensitivity as sa
    codes = {"gaussian": 0, "matern32": native.KERNEL_MATERN32, "matern52": native.KERNEL_MATERN52}
    d = args.d
    ctx = native.Context(0)
    for shape in args.shapes.split(","):
        n, G, m = (int(v) for v in shape.split(":"))
        X, f, H = synthetic.problem(n, d, seed=0)
        xs = synthetic.design(m, d, seed=7)
        hs = synthetic.linear_basis(xs)
        ctx.set_data(X, f, H)
        for kernel in args.kernels.split(","):
            ctx.factor(native.KERNEL_STD | codes[kernel], np.ones(d), 1e-3, 1.0, 0.0)
            beta = ctx.beta()
            out = {"n": n, "d": d, "G": G, "m": m, "kernel": kernel}
            warm = (8192 // G) * G
            ctx.posterior_groups(xs[:warm], hs[:warm], beta, 1.0, G)   # warm-up: workspaces, L^-1
            (_, cov), wall = timed(lambda: ctx.posterior_groups(xs, hs, beta, 1.0, G), args.reps)
            out["groups_ms"], out["groups_all_ms"] = min(wall), wall
            ctx.posterior(xs[:8192], hs[:8192], beta, 1.0, full_var=False, precision=64)   # warm-up
            (_, var), wall = timed(lambda: ctx.posterior(xs, hs, beta, 1.0, full_var=False, precision=64), args.reps)
            out["posterior_ms"], out["posterior_all_ms"] = min(wall), wall
            out["ratio"] = out["groups_ms"] / out["posterior_ms"]
            out["max_diag_diff"] = float(np.max(np.abs(np.diagonal(cov, axis1=1, axis2=2).ravel() - var)))
            ctx.set_profiling(True)
            ctx.posterior_groups(xs, hs, beta, 1.0, G)
            ph = np.zeros(8)
            ctx._check(ctx.lib.gpe_phase_times(ctx._h, native._ptr(ph), 8), "gpe_phase_times")
            ctx.set_profiling(False)
            n_pad = (n + 127) // 128 * 128
            out["kernel_ms"], out["chunks"] = ph[0], int(ph[1])
            out["kernel_ms_per_chunk"] = ph[0] / max(ph[1], 1.0)
            out["v_bytes_per_s"] = n_pad * m * 8.0 / (ph[0] * 1e-3)
            if args.example:
                N = args.example
                t0 = time.perf_counter()
                A, B = sa.sobol_points(d, N, 1, "uniform", 0.5, 1.0 / 12.0)
                P = np.empty((N, d + 2, d))
                P[:, 0], P[:, 1] = A, B
                for i in range(d):
                    P[:, 2 + i] = A
                    P[:, 2 + i, i] = B[:, i]
                P = P.reshape(N * (d + 2), d)
                fm, C = ctx.posterior_groups(P, synthetic.linear_basis(P), beta, 1.0, d + 2)
                est = sa.sobol_group_estimates(fm.reshape(N, d + 2), C)
                out["example_ms"] = (time.perf_counter() - t0) * 1e3
                out["example"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in est.items()}
                out["example"]["N"] = N
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "a") as fh:
                fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
