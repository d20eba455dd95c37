"""What per-point forecast summaries behind every launch cost (rs_hip_outputs_summary): bench.py's default flavour -
three plans, launches of 60 indices, slot-order rows with their order rows - with every launch's six streams x 60
rows also reduced into a [RS_SUM_COLS][points] accumulator in point order, on the plan's own stream between the launch
and its re-sort, or on a second stream through the kept order row with two output windows in turn; beside it the
pass without, and the existing per-point series (rs_hip_outputs_by_point) in the same process for a like-for-like
comparison.  The summary reads 48 B per point and row and reads and writes 136 B per point and call, where the
per-point series write the 48 B again.
usage: python tools/bench_summary_outputs.py [points] [passes] [modes, e.g. 0123]
A library without the summaries (an older build, ROADSURF_HIP_LIB) runs mode 0 only."""
import os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from roadsurf_amd import abi, device, lib, sharding, summary, workload

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
modes = [int(c) for c in (sys.argv[3] if len(sys.argv) > 3 else "0123")]
if not hasattr(lib.load(), "rs_hip_outputs_summary"):
    modes = [m for m in modes if m == 0]
hours, K, chunk = 48, 3, 60
simlen = hours * 120 + 1
dev = torch.device("cuda", 0)
s = abi.default_settings(simlen); p = abi.default_parameters()
spec = summary.SummarySpec(0.0, (0.0, 0.0, 0.0, 0.0, 0.0))
plans, runs = [], []
for j in range(K):
    off, nj = sharding.strong_shard(n, K, j)
    pl = device.Plan(nj, s, p, 0, stream=torch.cuda.Stream(dev))
    pl.set_variant(3)
    plans.append(pl)
    runs.append(workload.SyntheticRun(pl, 20240110, hours, chunk, point_offset=off, plan_order=True, forecast=True,
                                      forecast_mode=workload.DEFAULT_FORECAST_MODE))
accs = [torch.empty((lib.RS_SUM_COLS, r.plan.np_pad), dtype=torch.float64, device=dev) for r in runs]
dst = ([{k: torch.empty((r.plan.np_pad, chunk), dtype=torch.float64, device=dev) for k in device.OUT_FIELDS} for r in runs]
       if 3 in modes else None)
side = [torch.cuda.Stream(dev) for _ in runs]
wins = [[r.out, device.OutputWindow.empty(chunk, r.plan.np_pad, dev)] for r in runs]
done = [[None, None] for _ in runs]
TAGS = {0: "slot order + order rows (bench.py)",
        1: "summaries behind every launch, on the plan's stream (rs_hip_outputs_summary)",
        2: "summaries on a second stream through the kept order row, two output windows in turn",
        3: "per-point series behind every launch (rs_hip_outputs_by_point)"}


def behind(j, mode):
    r = runs[j]
    def on_launch(c, t0, ns):
        if mode == 1:  # between the launch and its re-sort: the plan's current order is the launch's
            r.plan.outputs_summary(r.out, ns, t0, 1, spec, accs[j])
            return
        if mode == 3:
            r.plan.outputs_by_point(r.out, ns, dst[j])
            return
        w = c & 1
        ev = torch.cuda.Event()
        ev.record(r.plan.stream)
        side[j].wait_event(ev)                      # behind the launch that filled window w
        r.plan.outputs_summary(wins[j][w], ns, t0, 1, spec, accs[j], order=r.orders[c], stream=side[j])
        done[j][w] = torch.cuda.Event()
        done[j][w].record(side[j])
        r.out = wins[j][w ^ 1]                      # the next launch writes the other window ...
        if done[j][w ^ 1] is not None:
            r.plan.stream.wait_event(done[j][w ^ 1])  # ... once its last reader is through
    return on_launch


def one_pass(mode):
    for j, r in enumerate(runs):
        r.out = wins[j][0]
        done[j][0] = done[j][1] = None
        if mode in (1, 2):
            r.plan.summary_reset(accs[j], stream=side[j] if mode == 2 else None)
    its = [r.iter_pass(behind(j, mode) if mode else None) for j, r in enumerate(runs)]
    while its:
        its = [it for it in its if next(it, None) is not None]


kept = {}
for mode in modes * 2:
    one_pass(mode)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(passes):
        one_pass(mode)
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / passes
    print(f"{TAGS[mode]}: {dt * 1e3:.1f} ms per pass -> {n * simlen / dt:.3e} point-timesteps/s", flush=True)
    if mode in (1, 2):
        kept[mode] = runs[0].plan.summary(accs[0])
if len(kept) == 2:  # both ways reduce the same rows of the same run
    print("plan 0: summaries on the plan's stream == on the second stream:", bool(np.array_equal(kept[1], kept[2])))
if kept:
    a = next(iter(kept.values()))
    print(f"plan 0: rows per point {a[:, 0].min():.0f}..{a[:, 0].max():.0f} of {simlen}, min Tsurf {a[:, 1].min():.3f}, "
          f"points that freeze {int((a[:, 5] > 0).sum())} of {len(a)}")
