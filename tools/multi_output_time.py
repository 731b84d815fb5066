"""Timing of the separable multi-output entries against the single-output ones they replace
(DESIGN.md 8c7): gpe_posterior_mean_multi at p outputs against p calls of gpe_posterior_mean,
gpe_objective_multi against gpe_objective(GPE_MUCM), per phase.

    python tools/multi_output_time.py --libs new=gp_emu_uqsa_amd/libgpemu.so [old=/path/libgpemu.so]
                                      [--rounds 3] [--n 16384] [--d 10] [--m 1000000]

Each library is measured in a child process of its own (GPEMU_LIB), the libraries alternating
over the rounds on the same GPU; one JSON line per child, then the medians and ranges.  A
library without the multi-output entries (the parent build) gives the single-output figures
only.  Wall times are a host clock around synchronous calls; kernel times are
gpe_phase_times()[0] with profiling on, in calls of their own.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import ctypes

    import numpy as np

    from gp_emu_uqsa_amd import native
    from oracle import gp_oracle as orc
    probe = ctypes.CDLL(native.LIB_PATH)
    native.SIGNATURES = {k: v for k, v in native.SIGNATURES.items() if hasattr(probe, k)}
    multi = "gpe_objective_multi" in native.SIGNATURES
    n, d, m = a.n, a.d, a.m
    X, f, H = orc.synthetic_problem(n, d, seed=1)
    rs = np.random.RandomState(2)
    Xs = rs.uniform(size=(m, d))
    Hs = orc.linear_basis(Xs)
    hp = np.concatenate([np.linspace(0.5, 1.1, d), [1e-3]])
    ctx = native.Context(0)
    ctx.set_data(X, f, H)
    out = {"multi": multi, "n": n, "d": d, "m": m}

    def wall(fn, reps):
        fn()                                   # warm-up: code objects, workspaces
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    def kernel(fn):
        ctx.set_profiling(True)
        fn()
        t = ctx.phase_times()
        ctx.set_profiling(False)
        return t

    # the objective: one gpe_objective(MUCM) with gradient, then the multi entry
    out["obj1_wall"] = wall(lambda: ctx.objective(native.MUCM, native.KERNEL_STD, hp), a.reps)
    out["obj1_phases"] = kernel(lambda: ctx.objective(native.MUCM, native.KERNEL_STD, hp))
    Fall = np.sin(X @ rs.normal(size=(d, 64)) * 1.5) + 0.05 * rs.normal(size=(n, 64)) + f[:, None]
    if multi:
        for p in a.pobj:
            ctx.set_outputs(Fall[:, :p])
            out[f"objm{p}_wall"] = wall(lambda: ctx.objective_multi(native.KERNEL_STD, hp), a.reps)
            out[f"objm{p}_phases"] = kernel(lambda: ctx.objective_multi(native.KERNEL_STD, hp))
    # the posterior mean: one call of the single entry, then the multi entry at each p
    ctx.factor(native.KERNEL_STD, hp[:d], hp[d])
    beta = ctx.beta()
    out["mean1_wall"] = wall(lambda: ctx.posterior_mean(Xs, Hs, beta), a.reps)
    out["mean1_kernel"] = kernel(lambda: ctx.posterior_mean(Xs, Hs, beta))["kbuild"]
    if multi:
        for p in a.pmean:
            ctx.set_outputs(Fall[:, :p])
            B = ctx.beta_multi()
            out[f"meanm{p}_wall"] = wall(lambda: ctx.posterior_mean_multi(Xs, Hs, B), a.reps)
            out[f"meanm{p}_kernel"] = kernel(lambda: ctx.posterior_mean_multi(Xs, Hs, B))["kbuild"]
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", default=["new=" + os.path.join(ROOT, "gp_emu_uqsa_amd", "libgpemu.so")])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--pmean", type=int, nargs="+", default=[1, 8, 16, 64])
    ap.add_argument("--pobj", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    libs = [s.split("=", 1) for s in a.libs]
    res = {name: [] for name, _ in libs}
    for r in range(a.rounds):
        for name, path in libs:
            env = dict(os.environ, GPEMU_LIB=os.path.abspath(path))
            cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:      # (no further GPU work after a failed child)
                sys.stdout.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"{name}: child failed with status {p.returncode}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            res[name].append(json.loads(line[7:]))
            print(name, "round", r, line[7:], flush=True)
    for name, _ in libs:
        print("==", name)
        for key in res[name][0]:
            vals = [x for rr in res[name] for x in (rr[key] if isinstance(rr[key], list) else [rr[key]])
                    if isinstance(x, (int, float)) and not isinstance(x, bool)]
            if key.endswith("_wall") or key.endswith("_kernel"):
                print(f"  {key:22s} median {statistics.median(vals):9.3f} ms   range {min(vals):9.3f} .. {max(vals):9.3f}")
            elif key.endswith("_phases"):
                ph = {k: statistics.median([rr[key][k] for rr in res[name]]) for k in res[name][0][key]}
                print(f"  {key:22s} " + "  ".join(f"{k} {v:.2f}" for k, v in ph.items()))


if __name__ == "__main__":
    main()
