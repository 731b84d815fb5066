"""Host wall time per objective of the three correlation families at n <= 512 (dev tool: the
one-launch paths k_tiny / k_snb against the general path, GPEMU_TINY=0, in one process).

(n, d) = (128, 10), (300, 10), (500, 10); gp4ml, std nugget fitted; with the gradient and
value only; 5 warm-up and 50 timed calls each.  Prints one line per case and a JSON summary
(ms per call; --json FILE also writes it).

    python tools/small_n_family_time.py [--json FILE]
"""
import json, os, sys, time
sys.path.insert(0, ".")
import numpy as np
from gp_emu_uqsa_amd import native, synthetic

FAMILIES = [("gaussian", 0), ("matern32", native.KERNEL_MATERN32), ("matern52", native.KERNEL_MATERN52)]
SHAPES = [(128, 10), (300, 10), (500, 10)]
WARMUP, TIMED = 5, 50


def contexts():
    """(one-launch, general): GPEMU_TINY is read when a context is created."""
    old = os.environ.pop("GPEMU_TINY", None)
    one = native.Context(0)
    os.environ["GPEMU_TINY"] = "0"
    gen = native.Context(0)
    if old is None:
        del os.environ["GPEMU_TINY"]
    else:
        os.environ["GPEMU_TINY"] = old
    return one, gen


def ms_per_call(ctx, kernel, hp, want):
    for _ in range(WARMUP):
        ctx.objective(native.GP4ML, kernel, hp, want_grad=want)
    t = time.perf_counter()
    for _ in range(TIMED):
        ctx.objective(native.GP4ML, kernel, hp, want_grad=want)
    return (time.perf_counter() - t) / TIMED * 1e3


def main():
    one, gen = contexts()
    rows = []
    for n, d in SHAPES:
        X, f, H = synthetic.problem(n, d, seed=0)
        one.set_data(X, f, H)
        gen.set_data(X, f, H)
        hp = np.concatenate([np.ones(d), [1e-3, 1.0]])
        for name, fam in FAMILIES:
            for want in (True, False):
                a = ms_per_call(one, native.KERNEL_STD | fam, hp, want)
                b = ms_per_call(gen, native.KERNEL_STD | fam, hp, want)
                rows.append(dict(n=n, d=d, family=name, grad=want, one_launch_ms=round(a, 4), general_ms=round(b, 4)))
                print(name, "n", n, "d", d, "grad" if want else "value", "one-launch", round(a, 3), "ms  general",
                      round(b, 3), "ms  ratio", round(b / a, 2), flush=True)
    one.close()
    gen.close()
    out = json.dumps(dict(warmup=WARMUP, timed=TIMED, rows=rows))
    print(out)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
