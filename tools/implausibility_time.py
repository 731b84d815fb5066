#!/usr/bin/env python
"""Time history matching over a resident emulator set (history_match.EmulatorSet, gpe_hm_*)
against the route the package had before it: the ``_implausible_rows`` loop, one
``model.Posterior`` per emulator, re-uploading and refactoring each training set because a
context holds one emulator -- what a user of nonimp_data / new_wave_design pays.  Same
emulators, same candidates, one process.  One JSON line per shape and family, printed and
appended to the log.

    python tools/implausibility_time.py                       # n = 300, 128, 512; gaussian, matern52
    python tools/implausibility_time.py --ns 300 --kernels gaussian --m 1000000 --reps 5

Each emulator is a synthetic problem (the one bench.py uses) on its own d of the D = d + p - 1
inputs, so the emulators differ and the candidate rows are wider than any of them.

  fused_ms        EmulatorSet.implausibility, the whole call (upload, kernels, selection,
                  download) between gpe_device_synchronize brackets: median of --reps after a
                  warm-up call; fused_all_ms the single times
  setup_ms        building the set: upload, factorisation, triangular inverse and snapshot of
                  every emulator (once per wave, not per call)
  loop_ms         _implausible_rows on the same candidates: median of --loop-reps after a warm-up
                  on the first 8192 candidates
  speedup         loop_ms / fused_ms
  flops           sum over the emulators of m n_pad^2, n_pad = n rounded up to 16: the multiply-
                  adds of the lower-triangular product L^-1 K* counted as two flops each
  tflops, of_mfma_ceiling   flops / fused_ms, and that against the 74.3 Tflop/s the fp64 MFMA
                  loop sustains on this chip: the whole call, transfers included
  max_rel_diff    max |I_fused - I_loop| / I_loop over candidates and the maxno columns
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_CEILING = 74.3e12


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


def emulator(n, d, cols, kernel, seed):
    """An Emulator as history_match reads it (beliefs, par, basis, K, training) on a synthetic
    problem, its inputs the columns `cols` of the candidate rows."""
    from gp_emu_uqsa_amd import kernels, model, native, synthetic
    X, f, H = synthetic.problem(n, d, seed=seed)
    delta = np.linspace(0.5, 1.1, d)
    ctx = native.default_context()
    ctx.set_data(X, f, H)
    ctx.factor({"gaussian": 0, "matern32": native.KERNEL_MATERN32, "matern52": native.KERNEL_MATERN52}[kernel],
               delta, 1e-3, 1.0, 0.0)
    beliefs = types.SimpleNamespace(
        active=[], basis_str=["1.0"] + ["x"] * d, basis_inf=list(range(d)), beta=list(ctx.beta()), delta=list(delta),
        sigma=0.9, nugget=1e-3, alt_nugget="F", kernel=kernel, active_index=list(cols),
        input_minmax=[[0.0, 1.0]] * d)
    par = model.Hyperparams(beliefs)
    basis = model.Basis(beliefs)
    K = kernels.for_beliefs(kernel, False)(d, par)
    training = model.Data(X, f, basis, par, beliefs, K)
    return types.SimpleNamespace(beliefs=beliefs, par=par, basis=basis, K=K, training=training)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ns", default="300,128,512")
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--p", type=int, default=4)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--maxno", type=int, default=1)
    ap.add_argument("--kernels", default="gaussian,matern52")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-reps", type=int, default=1)
    ap.add_argument("--no-loop", action="store_true", help="time the fused call only")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "implausibility_time.log"))
    args = ap.parse_args(argv)

    import contextlib
    import io
    from gp_emu_uqsa_amd import history_match as hm, native
    d, p, m = args.d, args.p, args.m
    D = d + p - 1
    x = np.random.default_rng(7).random((m, D))
    zs, ve, cm = [2.0 + 0.25 * o for o in range(p)], [0.01 + 0.005 * o for o in range(p)], 3.0
    for n in (int(v) for v in args.ns.split(",")):
        for kernel in args.kernels.split(","):
            quiet = io.StringIO()
            with contextlib.redirect_stdout(quiet):
                emuls = [emulator(n, d, range(o, o + d), kernel, seed=o) for o in range(p)]
                native.device_synchronize(0)
                t0 = time.perf_counter()
                S = hm.EmulatorSet(emuls)
                native.device_synchronize(0)
            out = {"n": n, "d": d, "p": p, "D": D, "m": m, "maxno": args.maxno, "kernel": kernel,
                   "setup_ms": (time.perf_counter() - t0) * 1e3, "fused": S.fused}
            S.implausibility(zs, ve, x, args.maxno)   # warm-up
            got, wall = timed(lambda: S.implausibility(zs, ve, x, args.maxno), args.reps)
            out["fused_ms"], out["fused_all_ms"] = statistics.median(wall), wall
            n16 = (n + 15) // 16 * 16
            out["flops"] = float(p) * m * n16 * n16
            out["tflops"] = out["flops"] / (out["fused_ms"] * 1e-3) / 1e12
            out["of_mfma_ceiling"] = out["tflops"] * 1e12 / MFMA_CEILING
            if not args.no_loop:
                def loop(xx):
                    I2 = np.zeros((xx.shape[0], p))
                    for o, E in enumerate(emuls):
                        mean, var = hm._posterior_diag(E, xx[:, S._cols[o]])
                        I2[:, o] = (mean - zs[o]) ** 2 / (var + ve[o])
                    return hm._imaxes(I2, args.maxno)
                with contextlib.redirect_stdout(quiet):
                    hm._implausible_rows(emuls, zs, ve, x[:8192], S.act_ref, args.maxno, cm)   # warm-up
                    keep, wall = timed(lambda: hm._implausible_rows(emuls, zs, ve, x, S.act_ref, args.maxno, cm),
                                       args.loop_reps)
                    want = loop(x[:200000])
                out["loop_ms"], out["loop_all_ms"] = statistics.median(wall), wall
                out["speedup"] = out["loop_ms"] / out["fused_ms"]
                out["accepted"] = int(keep.sum())
                out["same_mask"] = bool(np.array_equal(keep, got[:, -args.maxno] < cm))
                out["max_rel_diff"] = float(np.max(np.abs(got[:200000] - want) / want))
            S.close()
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
