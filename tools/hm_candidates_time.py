#!/usr/bin/env python
"""Time the candidates made and reduced on the device (gpe_hm_cells, gpe_hm_sample) against the
routes that make them on the host.  Same emulators (those of tools/implausibility_time.py: p
synthetic problems on their own d of the D = d + p - 1 inputs), one process, the routes
alternating: a warm-up of every route, then --reps rounds of one timing each.  One JSON line per
shape and part, printed and appended to the log.

    python tools/hm_candidates_time.py                        # n = 128, 300, 512; maps and sampler
    python tools/hm_candidates_time.py --ns 300 --parts maps --grid 20 --samples 800
    python tools/hm_candidates_time.py --ns 300 --parts sample --once device   # one route once: for a kernel trace

maps: one pair of inputs of imp_plot, grid x grid cells of --samples candidates each.
  device_ms   EmulatorSet.maps on the fused set: candidates by k_hm_mesh, k_hm_post, k_hm_cells
  rows_ms     the explicit rows on the host, EmulatorSet.implausibility on them (upload, kernels,
              m x maxno values back), NumPy's minimum and count per cell
  list_ms     imp_plot's list route: the explicit rows, the _posterior_diag loop (re-upload and
              refactorisation per emulator), _imaxes and NumPy's reduction
  same        IMP of the device against rows bit for bit, and the counts
sample: one batch of nonimp_sample (max_tried = batch) at two cut-offs, near 30 % and below
  1e-3 acceptance (quantiles of the level over 65536 host-made candidates).
  device_ms   generator="device": k_hm_draw, k_hm_post, count / ranks / scatter, accepted rows back
  host_ms     generator="host": default_rng().random, the affine map, upload, kernels, m values back
  same        the points and `tried` bit for bit
A route counts as faster where its slowest timing is below the other's fastest: *_faster.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def alternate(routes, reps):
    """{name: [ms, ...]} and the last results: a warm-up of every route, then reps rounds."""
    from implausibility_time import timed
    res, wall = {}, {k: [] for k in routes}
    for k, call in routes.items():
        call()
    for _ in range(reps):
        for k, call in routes.items():
            res[k], w = timed(call, 1)
            wall[k] += w
    return res, wall


def faster(a, b):
    return bool(max(a) < min(b))


def reduce_rows(top, cells, ns, maxno, cm):
    top = top.reshape(cells, ns, maxno)
    imp = np.stack([top[:, :, -(l + 1)].min(axis=1) for l in range(maxno)])
    below = np.stack([(top[:, :, -(l + 1)] < cm).sum(axis=1) for l in range(maxno)])
    return imp, below


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ns", default="128,300,512")
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--p", type=int, default=4)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--samples", type=int, default=800)
    ap.add_argument("--batch", type=int, default=2 ** 20)
    ap.add_argument("--maxno", type=int, default=1)
    ap.add_argument("--kernel", default="gaussian")
    ap.add_argument("--parts", default="maps,sample")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", default="", help="run this one route of each part once, untimed (for a kernel trace)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "hm_candidates_time.log"))
    args = ap.parse_args(argv)

    from gp_emu_uqsa_amd import history_match as hm
    from implausibility_time import emulator
    d, p, maxno = args.d, args.p, args.maxno
    D = d + p - 1
    zs, ve, cm = [2.0 + 0.25 * o for o in range(p)], [0.01 + 0.005 * o for o in range(p)], 3.0
    pair = (p - 1, p)                                             # two columns every emulator reads
    rng = np.random.default_rng(7)
    g, ns = args.grid, args.samples
    x1 = x2 = (np.arange(g) + 0.5) / g
    others = rng.random((ns, D - 2))
    cells = g * g

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as fh:
            fh.write(line + "\n")

    for n in (int(v) for v in args.ns.split(",")):
        quiet = io.StringIO()
        with contextlib.redirect_stdout(quiet):
            emuls = [emulator(n, d, range(o, o + d), args.kernel, seed=o) for o in range(p)]
            S = hm.EmulatorSet(emuls)
        assert S.fused
        base = {"n": n, "d": d, "p": p, "D": D, "maxno": maxno, "kernel": args.kernel}

        def rows():
            x = np.empty((cells * ns, D))
            x[:, pair[0]] = np.repeat(np.repeat(x1, g), ns)
            x[:, pair[1]] = np.repeat(np.tile(x2, g), ns)
            x[:, [k for k in range(D) if k not in pair]] = np.tile(others, (cells, 1))
            return x

        def by_device():
            imp, odp = S.maps(zs, ve, cm, pair, x1, x2, others, maxno=maxno)
            return imp.reshape(maxno, -1), odp.reshape(maxno, -1)

        def by_rows():
            imp, below = reduce_rows(S.implausibility(zs, ve, rows(), maxno), cells, ns, maxno, cm)
            return imp, below / float(ns)

        def by_list():
            x = rows()
            I2 = np.zeros((x.shape[0], p))
            with contextlib.redirect_stdout(quiet):
                for o, E in enumerate(emuls):
                    mean, var = hm._posterior_diag(E, x[:, S._cols[o]])
                    I2[:, o] = (mean - zs[o]) ** 2 / (var + ve[o])
            imp, below = reduce_rows(hm._imaxes(I2, maxno), cells, ns, maxno, cm)
            return imp, below / float(ns)

        if "maps" in args.parts.split(","):
            routes = {"device": by_device, "rows": by_rows, "list": by_list}
            if args.once:
                routes[args.once]()
            else:
                res, wall = alternate(routes, args.reps)
                out = dict(base, part="maps", grid=g, samples=ns, candidates=cells * ns)
                for k in routes:
                    out[k + "_ms"] = wall[k]
                out["device_faster_than_rows"] = faster(wall["device"], wall["rows"])
                out["device_faster_than_list"] = faster(wall["device"], wall["list"])
                out["same"] = bool(np.array_equal(res["device"][0], res["rows"][0], equal_nan=True)
                                   and np.array_equal(res["device"][1], res["rows"][1]))
                out["max_rel_diff_list"] = float(np.max(np.abs(res["device"][0] - res["list"][0]) / res["list"][0]))
                emit(out)
        if "sample" in args.parts.split(","):
            m = args.batch
            probe = S.implausibility(zs, ve, np.random.default_rng(0).random((65536, D)), maxno)[:, -maxno]
            for label, q in (("near_30_percent", 0.30), ("below_1e-3", 5e-4)):
                cut = float(np.quantile(probe, q))

                def sample(generator):
                    return hm.nonimp_sample(S, zs, cut, ve, count=10 ** 9, maxno=maxno, seed=0, batch=m, max_tried=m,
                                            generator=generator)
                routes = {"device": lambda: sample("device"), "host": lambda: sample("host")}
                if args.once:
                    routes[args.once]()
                    continue
                res, wall = alternate(routes, args.reps)
                out = dict(base, part="sample", batch=m, cm=cut, rate=label, accepted=int(res["device"][0].shape[0]),
                           device_ms=wall["device"], host_ms=wall["host"],
                           device_faster=faster(wall["device"], wall["host"]),
                           same=bool(np.array_equal(res["device"][0], res["host"][0]) and res["device"][1] == res["host"][1]))
                emit(out)
        S.close()


if __name__ == "__main__":
    main()
