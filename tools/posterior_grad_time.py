#!/usr/bin/env python
"""Time gpe_posterior_grad beside gpe_posterior on the synthetic problem bench.py uses, and
print one JSON line.

    python tools/posterior_grad_time.py                    # n = 16384, d = 10, m = 65536
    python tools/posterior_grad_time.py --n 4096 --m 20000 --reps 3

  posterior_ms      gpe_posterior, diagonal variance, precision 64
  grad_ms           gpe_posterior_grad with the variance gradient
  grad_mean_ms      gpe_posterior_grad without it (dvar_out NULL: no second product)
      each the whole call between gpe_device_synchronize brackets, best of --reps after a
      warm-up call (workspaces, L^-1 and its int8 planes)
  kernel_ms_per_chunk   k_post_grad's device time per chunk of 8192 points from one profiled
      call of each kind (gpe_phase_times: events around the kernel, one synchronisation per
      chunk), with and without the variance sums
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
    ap.add_argument("--m", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel", default="gaussian", choices=["gaussian", "matern32", "matern52"])
    args = ap.parse_args(argv)

    from gp_emu_uqsa_amd import native, synthetic
    code = {"gaussian": 0, "matern32": native.KERNEL_MATERN32, "matern52": native.KERNEL_MATERN52}[args.kernel]
    ctx = native.Context(0)
    X, f, H = synthetic.problem(args.n, args.d, seed=0)
    ctx.set_data(X, f, H)
    ctx.factor(native.KERNEL_STD | code, np.ones(args.d), 1e-3, 1.0, 0.0)
    beta = ctx.beta()
    xs = synthetic.design(args.m, args.d, seed=7)
    hs = synthetic.linear_basis(xs)
    dhs = np.ones_like(hs)
    dhs[:, 0] = 0.0
    hdim = np.arange(-1, args.d, dtype=np.int32)
    calls = {
        "posterior_ms": lambda: ctx.posterior(xs, hs, beta, 1.0, full_var=False, precision=64),
        "grad_ms": lambda: ctx.posterior_grad(xs, hs, dhs, hdim, beta, 1.0, want_var=True),
        "grad_mean_ms": lambda: ctx.posterior_grad(xs, hs, dhs, hdim, beta, 1.0, want_var=False),
    }
    out = {"n": args.n, "d": args.d, "m": args.m, "kernel": args.kernel, "reps": args.reps}
    for name, call in calls.items():
        call()   # warm-up
        wall = []
        for _ in range(args.reps):
            native.device_synchronize(0)
            t0 = time.perf_counter()
            call()
            native.device_synchronize(0)
            wall.append((time.perf_counter() - t0) * 1e3)
        out[name] = min(wall)
        out[name[:-3] + "_all_ms"] = wall
    ctx.set_profiling(True)
    for name in ("grad_ms", "grad_mean_ms"):
        calls[name]()
        ph = np.zeros(8)
        ctx._check(ctx.lib.gpe_phase_times(ctx._h, native._ptr(ph), 8), "gpe_phase_times")
        out["kernel_ms_per_chunk" if name == "grad_ms" else "kernel_mean_ms_per_chunk"] = ph[0] / max(ph[1], 1.0)
        out["chunks"] = int(ph[1])
    ctx.set_profiling(False)
    ctx.close()
    out["grad_over_posterior"] = out["grad_ms"] / out["posterior_ms"]
    out["kernel_share_of_call"] = out["kernel_ms_per_chunk"] * out["chunks"] / out["grad_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
