"""What per-point aggregates over output periods behind every launch cost (rs_hip_outputs_periods): bench.py's default
flavour - three plans, launches of 60 indices, slot-order rows with their order rows - with every launch's six streams
x 60 rows also fed, in time order, to every point's hourly cells (periods of 120 indices from index 2 on, which end at
the hourly kept rows: a [48][RS_PER_COLS][points] accumulator in point order) on the plan's own stream between the
launch and its re-sort; beside it the pass without and the per-point summaries (rs_hip_outputs_summary), in the same
process, the modes alternating, medians reported.  The period reducer reads the same 48 B per point and row as the
summary reducer, without its four-way split of the rows over the wavefronts of a workgroup (the sum of a period is
ordered), and reads and writes 272 B per point and touched period where the summaries move 272 B per point and call: a
launch of 60 indices touches one hourly period or two.  The yardstick is the summaries' added time per pass.
usage: python tools/bench_period_outputs.py [points] [passes per round] [rounds] [output file]
The output file (default profiles/period_outputs.txt) gets the lines this prints."""
import os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from roadsurf_amd import abi, device, lib, periods, provenance, sharding, summary, workload

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 2
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "period_outputs.txt")
hours, K, chunk = 48, 3, 60
simlen = hours * 120 + 1
dev = torch.device("cuda", 0)
s = abi.default_settings(simlen); p = abi.default_parameters()
sspec = summary.SummarySpec(0.0, (0.0, 0.0, 0.0, 0.0, 0.0))
pspec = periods.PeriodSpec(2, 120, hours, 0.0, (0.0, 0.0, 0.0, 0.0, 0.0))
plans, runs = [], []
for j in range(K):
    off, nj = sharding.strong_shard(n, K, j)
    pl = device.Plan(nj, s, p, 0, stream=torch.cuda.Stream(dev))
    pl.set_variant(3)
    plans.append(pl)
    runs.append(workload.SyntheticRun(pl, 20240110, hours, chunk, point_offset=off, plan_order=True, forecast=True,
                                      forecast_mode=workload.DEFAULT_FORECAST_MODE))
saccs = [torch.empty((lib.RS_SUM_COLS, r.plan.np_pad), dtype=torch.float64, device=dev) for r in runs]
paccs = [torch.empty((hours, lib.RS_PER_COLS, r.plan.np_pad), dtype=torch.float64, device=dev) for r in runs]
TAGS = {0: "slot order + order rows (bench.py)",
        1: "hourly periods behind every launch, on the plan's stream (rs_hip_outputs_periods)",
        2: "summaries behind every launch, on the plan's stream (rs_hip_outputs_summary)"}
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def behind(j, mode):
    r = runs[j]
    def on_launch(c, t0, ns):  # between the launch and its re-sort: the plan's current order is the launch's
        if mode == 1:
            r.plan.outputs_periods(r.out, ns, t0, 1, pspec, paccs[j])
        else:
            r.plan.outputs_summary(r.out, ns, t0, 1, sspec, saccs[j])
    return on_launch


def one_pass(mode):
    for j, r in enumerate(runs):
        if mode == 1:
            r.plan.periods_reset(pspec, paccs[j])
        if mode == 2:
            r.plan.summary_reset(saccs[j])
    its = [r.iter_pass(behind(j, mode) if mode else None) for j, r in enumerate(runs)]
    while its:
        its = [it for it in its if next(it, None) is not None]


say(f"# python tools/bench_period_outputs.py {n} {passes} {rounds}; kernel sources {provenance.build_sha16()}")
say(f"# {n} points x {hours} h (SimLen {simlen}), {K} plans x launches of {chunk} (bench.py's default flavour), one device, one "
    f"process; {rounds} alternating rounds of {passes} passes per mode; periods: {hours} of 120 indices from index 2 on, "
    f"Tsurf < 0, storages > 0; accumulators {sum(a.numel() for a in paccs) * 8 / 1e9:.2f} GB")
times = {m: [] for m in TAGS}
for m in TAGS:  # warm-up
    one_pass(m)
torch.cuda.synchronize(dev)
for _ in range(rounds):
    for m in TAGS:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(passes):
            one_pass(m)
        torch.cuda.synchronize(dev)
        times[m].append((time.perf_counter() - t0) / passes)
med = {m: float(np.median(v)) for m, v in times.items()}
for m in TAGS:
    say(f"{TAGS[m]}: {med[m] * 1e3:.1f} ms per pass, median of {rounds} (all: "
        f"{' '.join(f'{x * 1e3:.1f}' for x in times[m])}) -> {n * simlen / med[m]:.3e} point-timesteps/s")
launches = len(runs[0].starts)
say(f"the periods cost {1e3 * (med[1] - med[0]):+.1f} ms per pass ({100 * (med[1] / med[0] - 1):+.1f} %), "
    f"{1e3 * (med[1] - med[0]) / launches:.2f} ms per launch cycle of {K} plans; the summaries "
    f"{1e3 * (med[2] - med[0]):+.1f} ms per pass ({100 * (med[2] / med[0] - 1):+.1f} %), "
    f"{1e3 * (med[2] - med[0]) / launches:.2f} ms per launch cycle")
say(f"ratio: the periods' added time is {(med[1] - med[0]) / (med[2] - med[0]):.2f} x the summaries' added time")
# what the cells of plan 0 say, counted on the device (the cells of a third of a million points are 2 GB)
a, npts = paccs[0], runs[0].plan.npoints
col = lambda c: a[:, c, :npts]
sm = runs[0].plan.summary(saccs[0])
cells = hours * npts
say(f"plan 0 ({npts} points x {hours} periods): rows per cell {int(col(0).min())}..{int(col(0).max())}; "
    f"cells with min Tsurf < 0 <= the sample {int(((col(1) < 0) & (col(5) >= 0)).sum())} of {cells}; "
    f"cells with max Ice > 0 {int((col(9) > 0).sum())}; points whose period minima reach the summaries' minimum "
    f"{int((col(1).min(dim=0).values.cpu().numpy() == sm[:, 1]).sum())} of {npts}")
with open(path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
