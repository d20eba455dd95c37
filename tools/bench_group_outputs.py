"""What per-group time series behind every launch cost (rs_hip_outputs_groups): bench.py's default flavour - three
plans, launches of 60 indices, slot-order rows with their order rows - with every launch's six streams x 60 rows also
reduced into one accumulator [rows][ngroups][cols] that the three plans share, on each plan's own stream between the
launch and its re-sort.  Beside it, in the same session: the pass without any reduction and the per-point summaries
(rs_hip_outputs_summary), which read the same 48 B per point and row.  Group rows:
  64 contiguous   64 districts of equal size, contiguous in point order (cells in LDS)
  64 random       64 districts dealt at random (cells in LDS)
  n/8 of 8        ensembles: 8 consecutive points are the members of one station (global cells)
each with and without 16 edges.  The accumulator has a row per time index (5761) for the districts; for the ensembles
every launch merges into the same 60 rows (a row per index would be tens of GB: such a consumer keeps hourly rows).  Behind the passes every reducer is timed alone on plan 0's last window (333 k points x
60 rows at 1 M points, through the plan's current order): 3 warm-up calls, then 20 calls between two events.
usage: python tools/bench_group_outputs.py [points] [passes]"""
import os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from roadsurf_amd import abi, device, groups, lib, sharding, summary, workload

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
hours, K, chunk = 48, 3, 60
simlen = hours * 120 + 1
dev = torch.device("cuda", 0)
s = abi.default_settings(simlen); p = abi.default_parameters()
th = summary.SummarySpec(0.0, (0.0, 0.0, 0.0, 0.0, 0.0))
EDGES = tuple(float(x) for x in np.linspace(-30.0, 15.0, 16))
plans, runs, offs = [], [], []
for j in range(K):
    off, nj = sharding.strong_shard(n, K, j)
    pl = device.Plan(nj, s, p, 0, stream=torch.cuda.Stream(dev))
    pl.set_variant(3)
    plans.append(pl)
    offs.append(off)
    runs.append(workload.SyntheticRun(pl, 20240110, hours, chunk, point_offset=off, plan_order=True, forecast=True,
                                      forecast_mode=workload.DEFAULT_FORECAST_MODE))
sum_accs = [torch.empty((lib.RS_SUM_COLS, r.plan.np_pad), dtype=torch.float64, device=dev) for r in runs]
point = np.arange(n)
ROWS = {"64 contiguous": (64, (point * 64 // n).astype(np.int32)),
        "64 random": (64, np.random.RandomState(1).randint(0, 64, n).astype(np.int32)),
        "n/8 of 8": ((n + 7) // 8, (point // 8).astype(np.int32))}
MODES = [("slot order + order rows (bench.py)", None),
         ("summaries behind every launch (rs_hip_outputs_summary)", "summary")]
for name, (ng, ids) in ROWS.items():
    for edges in ((), EDGES):
        spec = groups.GroupSpec(th, ng, edges)
        MODES.append((f"group series behind every launch, {name}, {len(edges)} edges ({lib.group_path(spec)})",
                      (spec, [torch.from_numpy(ids[off:off + r.plan.npoints]).to(dev) for off, r in zip(offs, runs)])))
gacc = {}


def behind(j, what):
    r = runs[j]
    def on_launch(c, t0, ns):  # between the launch and its re-sort: the plan's current order is the launch's
        if what == "summary":
            r.plan.outputs_summary(r.out, ns, t0, 1, th, sum_accs[j])
        else:
            acc = gacc[id(what)]
            r.plan.outputs_groups(r.out, ns, what[1][j], what[0], acc, t0 - 1 if acc.shape[0] == simlen else 0)
    return on_launch


def one_pass(what):
    if what == "summary":
        for j, r in enumerate(runs):
            r.plan.summary_reset(sum_accs[j])
    elif what is not None:  # one accumulator for the three plans: reset on plan 0's stream, the others wait for it
        if id(what) not in gacc:
            gacc.clear()
            # a row per time index where that is below 2 GB; the ensembles' launches all merge into the same 60 rows
            cells = what[0].ngroups * groups.cols(what[0])
            rows = simlen if simlen * cells * 8 < 2 << 30 else chunk
            gacc[id(what)] = torch.empty((rows, what[0].ngroups, groups.cols(what[0])), dtype=torch.float64, device=dev)
        plans[0].groups_reset(gacc[id(what)].shape[0], what[0], gacc[id(what)])
        ev = torch.cuda.Event()
        ev.record(plans[0].stream)
        for pl in plans[1:]:
            pl.stream.wait_event(ev)
    its = [r.iter_pass(behind(j, what) if what is not None else None) for j, r in enumerate(runs)]
    while its:
        its = [it for it in its if next(it, None) is not None]


def alone(call):
    for _ in range(3):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(plans[0].stream)
    for _ in range(20):
        call()
    b.record(plans[0].stream)
    b.synchronize()
    return a.elapsed_time(b) / 20


print(f"# {n} points x {hours} h, {K} plans x {chunk}, {passes} passes per figure behind one warm-up pass, every mode twice")
for tag, what in MODES * 2:
    one_pass(what)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(passes):
        one_pass(what)
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / passes
    line = f"{tag}: {dt * 1e3:.1f} ms per pass -> {n * simlen / dt:.3e} point-timesteps/s"
    r0 = runs[0]
    if what == "summary":
        ms = alone(lambda: r0.plan.outputs_summary(r0.out, chunk, 1, 1, th, sum_accs[0]))
        line += f"; alone {ms:.3f} ms per call of {r0.plan.npoints} points x {chunk} rows"
    elif what is not None:
        ms = alone(lambda: r0.plan.outputs_groups(r0.out, chunk, what[1][0], what[0], gacc[id(what)], 0))
        line += f"; alone {ms:.3f} ms per call of {r0.plan.npoints} points x {chunk} rows"
    print(line, flush=True)
    if what is not None and what != "summary" and what[0].ngroups == 64:
        # (before the timing calls above merged rows again: the passes' result is gone; check a fresh one)
        one_pass(what)
        torch.cuda.synchronize(dev)
        a = gacc[id(what)].cpu().numpy()
        full = bool((a[:, :, 0].sum(axis=1) == n).all())
        bins = "" if not what[0].edges else f", bins add up to the count: {bool((a[:, :, 14:].sum(axis=2) == a[:, :, 0]).all())}"
        print(f"    every row counts all {n} points: {full}; min Tsurf {a[:, :, 1].min():.3f}{bins}", flush=True)
