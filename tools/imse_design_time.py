#!/usr/bin/env python
"""Time gpe_posterior_imse on the synthetic problem bench.py uses.  One JSON line per shape,
printed and appended to the log.

    python tools/imse_design_time.py                 # n = 16384, d = 10, k = 128; 12288:4096 and 8192:2048
    python tools/imse_design_time.py --n 4096 --shapes 1024:512 --k 64 --host 8

A shape is m_c:m_r (candidates : reference points), C is m_r x m_c.
  call_ms          the whole call (upload, covariance, picks, download) between
                   gpe_device_synchronize brackets: best of --reps after a warm-up call
  cov_ms, steps_ms, update_ms
                   gpe_phase_times of one profiled call: the covariance and the copy of C, the
                   column and sweep kernels, the trailing updates (one synchronisation per panel)
  step_ms_per_pick steps_ms / picks: k_im_col + k_im_sweep
  col_ms_per_pick  the column kernel's counterpart, k_pc_step of gpe_posterior_pivchol on the m_c
                   candidates alone, per step (the same rows, the same panel): an estimate of
                   k_im_col, which has no phase of its own
  sweep_ms_per_pick  step_ms_per_pick - col_ms_per_pick
  floor_ms         2 * 8 * m_r * m_c bytes at 6.0 TB/s; floor_fraction = floor_ms / sweep_ms_per_pick
  host_ms          with --host P: the NumPy model of the same algorithm (eager C) on the device's
                   own covariance, P picks timed and scaled to k (every pick is the same work)
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


def phases(ctx, call):
    from gp_emu_uqsa_amd import native
    ctx.set_profiling(True)
    call()
    ph = np.zeros(8)
    ctx._check(ctx.lib.gpe_phase_times(ctx._h, native._ptr(ph), 8), "gpe_phase_times")
    ctx.set_profiling(False)
    return ph


def host_model(S, mc, picks):
    """The algorithm of include/gpemu.h in NumPy with an eager C, uniform weights, tol = 0."""
    mr = S.shape[0] - mc
    w = np.full(mr, 1.0 / mr)
    d = np.diag(S)[:mc].copy()
    C = S[mc:, :mc].copy()
    L = np.zeros((mc, picks))
    chosen = np.zeros(mc, dtype=bool)
    piv = []
    for t in range(picks):
        score = np.where(chosen, -np.inf, w.dot(C * C) / d)
        p = int(np.argmax(score))
        root = np.sqrt(d[p])
        col = (S[:mc, p] - L[:, :t].dot(L[p, :t])) / root
        col[chosen] = 0.0
        L[:, t] = col
        lam = C[:, p] / root
        chosen[p] = True
        col[p] = 0.0
        C -= np.outer(lam, col)
        d -= col ** 2
        piv.append(p)
    return np.array(piv)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--shapes", default="12288:4096,8192:2048", help="mc:mr,mc:mr,...")
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host", type=int, default=0, help="picks of the NumPy model to time (0: skip)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "imse_design_time.log"))
    args = ap.parse_args(argv)

    from gp_emu_uqsa_amd import native, synthetic
    n, d, k = args.n, args.d, args.k
    ctx = native.Context(0)
    X, f, H = synthetic.problem(n, d, seed=0)
    ctx.set_data(X, f, H)
    ctx.factor(native.KERNEL_STD, np.ones(d), 1e-3, 1.0, 0.0)
    beta = ctx.beta()
    for shape in args.shapes.split(","):
        mc, mr = (int(v) for v in shape.split(":"))
        xs = synthetic.design(mc + mr, d, seed=7)
        hs = synthetic.linear_basis(xs)

        def call():
            return ctx.posterior_imse(xs, hs, beta, 1.0, mc, k, tol=0.0)
        out = {"n": n, "d": d, "mc": mc, "mr": mr, "k": k}
        call()   # warm-up: workspaces, L^-1
        res, wall = timed(call, args.reps)
        out["call_ms"], out["call_all_ms"], out["rank"] = min(wall), wall, res[5]
        ph = phases(ctx, call)
        out["cov_ms"], out["steps_ms"], out["update_ms"] = ph[0], ph[1], ph[2]
        out["step_ms_per_pick"] = ph[1] / max(res[5], 1)

        def pc():
            return ctx.posterior_pivchol(xs[:mc], hs[:mc], beta, 1.0, k=k, want_L=False)
        pc()
        out["col_ms_per_pick"] = phases(ctx, pc)[1] / k
        out["sweep_ms_per_pick"] = out["step_ms_per_pick"] - out["col_ms_per_pick"]
        out["floor_ms"] = 2 * 8.0 * mr * mc / 6.0e12 * 1e3
        out["floor_fraction"] = out["floor_ms"] / out["sweep_ms_per_pick"]
        if args.host:
            S = ctx.posterior(xs, hs, beta, 1.0, full_var=True)[1]
            t0 = time.perf_counter()
            hp = host_model(S, mc, args.host)
            out["host_picks"] = args.host
            out["host_ms"] = (time.perf_counter() - t0) * 1e3 * k / args.host
            out["host_picks_equal"] = bool(np.array_equal(hp, res[1][:args.host]))
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
