"""bench.py's plain run and --dump-outputs on one GPU, at a small size: the line carries the
headline and ms_per_step and none of the --full legs, and the dumped arrays are what the
timed path's last step returned (the objective at each try's point, same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.timeout(120)
def test_plain_run_dumps_last_step(tmp_path, ctx):
    import bench
    from gp_emu_uqsa_amd import native, synthetic
    n, d, K = 1000, 4, 2
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GPEMU_RDZV_DIR"):
        env.pop(k, None)
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--n", str(n), "--d", str(d), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=100, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0.0
    assert abs(line["value"] - K * 1000.0 / line["ms_per_step"]) <= 1e-9 * line["value"]
    assert "cpu_baseline" not in line
    extra = line.get("extra", {})
    for key in ("single_eval_ms", "value_only_ms", "other_configs", "rowblock", "rowblock_metric"):
        assert key not in extra, key
    assert sorted(os.listdir(out_dir)) == ["grad.npy", "llh.npy", "sigma2.npy"]
    llh, grad, s2 = (np.load(out_dir / f"{name}.npy") for name in ("llh", "grad", "sigma2"))
    assert llh.dtype == grad.dtype == s2.dtype == np.float64
    assert llh.shape == (K,) and s2.shape == (K,) and grad.shape == (K, d + 2)
    X, f, H = synthetic.problem(n, d, seed=0)
    ctx.set_data(X, f, H)
    for k in range(K):
        ref = ctx.objective(native.GP4ML, native.KERNEL_STD, bench.eval_point(d, k))
        # the same kernels on the same inputs; concurrent streams do not change the arithmetic
        assert abs(llh[k] - ref[0]) <= 1e-12 * abs(ref[0])
        assert np.max(np.abs(grad[k] - ref[1])) <= 1e-10 * np.max(np.abs(ref[1]))
        assert abs(s2[k] - ref[2]) <= 1e-12 * abs(ref[2])
