"""GPU: `bench.py --dump-outputs DIR` writes what its timed path computed in the last timed pass - the sampled
points' series and every point's last index - and they are those points' outputs: the same points through one
plan in natural order (no re-sort, no order rows to read them back through) carry the same bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_dumped_outputs_are_the_points_outputs(tmp_path):
    import torch
    from roadsurf_amd import abi, device, workload

    n, hours, seed, steps = 20_000, 6, 20240110, 2
    d = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--total-points", str(n),
           "--hours", str(hours), "--steps", str(steps), "--warmup", "0", "--seed", str(seed),
           "--dump-outputs", str(d)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)  # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["config"]["failed_points"] == 0
    assert "natural_order_value" not in line and "cpu_baseline" not in line  # a plain run: the headline only
    assert sum(f.stat().st_size for f in d.iterdir()) <= 64e6

    L = hours * workload.SPK + 1
    pts = np.load(d / "points.npy")
    assert pts.dtype == np.float64 and len(pts) > 0
    pts = pts.astype(np.int64)
    plan = device.Plan(n, abi.default_settings(L), abi.default_parameters(), 0)
    run = workload.SyntheticRun(plan, seed, hours, 240, plan_order=False)
    cols = torch.as_tensor(pts, device=plan.device)
    want = {k: np.full((len(pts), L), np.nan) for k in device.OUT_FIELDS}
    final = {}

    def on_launch(c, t0, ns):
        for k in device.OUT_FIELDS:
            want[k][:, t0 - 1:t0 - 1 + ns] = run.out.tensors[k][:ns, cols].T.cpu().numpy()
            if t0 - 1 + ns == L:
                final[k] = run.out.tensors[k][ns - 1, :n].cpu().numpy()

    run.run_pass(on_launch)
    plan.sync()
    assert plan.failed_count() == 0
    for k in device.OUT_FIELDS:
        got = np.load(d / (k + ".npy"))
        assert got.dtype == np.float64 and got.shape == (len(pts), L), k
        assert np.array_equal(got, want[k]), k
        got = np.load(d / ("final_" + k + ".npy"))
        assert got.dtype == np.float64 and got.shape == (n,), k
        assert np.array_equal(got, final[k]), k
    del run
    plan.close()
    torch.cuda.empty_cache()
