#!/usr/bin/env python
"""Time gpe_posterior_mean beside gpe_posterior(full_var=0, precision=64), the only other way
to a posterior mean, on the same points, factor and process (the synthetic problem bench.py
uses).  One JSON line per shape and family, printed and appended to the log.

    python tools/posterior_mean_time.py                      # the three shapes, three families
    python tools/posterior_mean_time.py --shapes 4096:100000 --kernels gaussian --reps 5

  mean_ms          gpe_posterior_mean, the whole call (upload, kernels, download, host finish)
                   between gpe_device_synchronize brackets: best of --reps after a warm-up call
  posterior_ms     gpe_posterior the same way: best of --posterior-reps after a warm-up call on
                   the first 8192 points (one chunk: the workspaces, L^-1 and its int8 planes)
  speedup          posterior_ms / mean_ms
  kernel_ms        k_post_mean's device time summed over the chunks of one profiled call
                   (gpe_phase_times: events around the kernel, one synchronisation per chunk)
  pairs_per_s      n_pad * m / kernel time (n_pad: n rounded up to 128, the rows the kernel reads)
  valu_floor_ms    the time the inner loop's vector instructions alone take on every SIMD of the
                   chip: per pair VALU64 fp64 instructions at 4 cycles per wave of 64 (78.6
                   Tflop/s fp64 vector = 16 lanes per SIMD and clock) and VALU32 others at 2,
                   counted in the disassembly of the d = 10 instances (k_post_mean<12, FAM,
                   false>: two rows x two points per loop trip), at 1024 SIMDs x 2.4 GHz
  floor_fraction   valu_floor_ms / kernel_ms (only for d in 9..12, the instance counted)
  max_abs_diff     max |mean - posterior's mean| over the points
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (fp64 VALU, other VALU) instructions per pair in the inner loop of k_post_mean<12, FAM, false>
VALU_PER_PAIR = {"gaussian": (180 / 4, 14 / 4), "matern32": (244 / 4, 30 / 4), "matern52": (252 / 4, 30 / 4)}
SIMDS, CLOCK_HZ = 1024, 2.4e9


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
    ap.add_argument("--shapes", default="16384:1000000,4096:1000000,128:1000000", help="n:m,n:m,...")
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--kernels", default="gaussian,matern32,matern52")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--posterior-reps", type=int, default=1)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "posterior_mean_time.log"))
    args = ap.parse_args(argv)

    from gp_emu_uqsa_amd import native, synthetic
    codes = {"gaussian": 0, "matern32": native.KERNEL_MATERN32, "matern52": native.KERNEL_MATERN52}
    d = args.d
    ctx = native.Context(0)
    for shape in args.shapes.split(","):
        n, m = (int(v) for v in shape.split(":"))
        X, f, H = synthetic.problem(n, d, seed=0)
        xs = synthetic.design(m, d, seed=7)
        hs = synthetic.linear_basis(xs)
        ctx.set_data(X, f, H)
        for kernel in args.kernels.split(","):
            ctx.factor(native.KERNEL_STD | codes[kernel], np.ones(d), 1e-3, 1.0, 0.0)
            beta = ctx.beta()
            out = {"n": n, "d": d, "m": m, "kernel": kernel}
            ctx.posterior_mean(xs, hs, beta)   # warm-up
            mean, wall = timed(lambda: ctx.posterior_mean(xs, hs, beta), args.reps)
            out["mean_ms"], out["mean_all_ms"] = min(wall), wall
            ctx.posterior(xs[:8192], hs[:8192], beta, 1.0, full_var=False, precision=64)   # warm-up
            (pm, _), wall = timed(lambda: ctx.posterior(xs, hs, beta, 1.0, full_var=False, precision=64),
                                  args.posterior_reps)
            out["posterior_ms"], out["posterior_all_ms"] = min(wall), wall
            out["speedup"] = out["posterior_ms"] / out["mean_ms"]
            out["max_abs_diff"] = float(np.max(np.abs(mean - pm)))
            ctx.set_profiling(True)
            ctx.posterior_mean(xs, hs, beta)
            ph = np.zeros(8)
            ctx._check(ctx.lib.gpe_phase_times(ctx._h, native._ptr(ph), 8), "gpe_phase_times")
            ctx.set_profiling(False)
            n_pad = (n + 127) // 128 * 128
            out["kernel_ms"], out["chunks"] = ph[0], int(ph[1])
            out["pairs_per_s"] = n_pad * m / (ph[0] * 1e-3)
            if 9 <= d <= 12:
                v64, v32 = VALU_PER_PAIR[kernel]
                out["valu_floor_ms"] = n_pad * m / 64.0 * (4 * v64 + 2 * v32) / (SIMDS * CLOCK_HZ) * 1e3
                out["floor_fraction"] = out["valu_floor_ms"] / ph[0]
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "a") as fh:
                fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
