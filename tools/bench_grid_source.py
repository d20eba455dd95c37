"""What a gridded forecast source costs and saves (rs_driver_run_grid): bench.py's driver_path_relax call -
driver_workload's shape, relaxation, the library's fan-out of four blocks on one GPU, pageable host arrays - fed
  per-point   the forecast as [n_points][n_times] series (what the call took before; the yardstick of the session),
  grid/10     the same forecast as fields on a grid with about a tenth as many nodes as points, bilinear stencils,
  grid/1      ... with about as many nodes as points,
the points scattered uniformly over the grid (no two neighbours in memory are neighbours on the grid: the worst
case for the gather's reads).  The per-point series of a case are grid.to_raw_source of its fields, so all calls
of a case compute the same thing, and the host time of to_raw_source is what a caller no longer spends.

The parent process never touches the GPU.  It starts one child per step, each under its own time limit, and stops
at the first that fails:
  1. `--child time`: the three cases in one session, alternating, one warm call each, then `reps` timed ones (wall
     clock around calls that end with the results in host arrays); then one call per case with
     ROADSURF_HIP_DRIVER_TIMING=1 for the library's own phase report (those calls synchronise between phases: they
     are not among the timed ones).
  2. `--child trace CASE` under `rocprofv3 --kernel-trace --stats`, once per-point and once grid/10: the gather
     kernel's time beside the transposes it replaces (tracing slows the host: no wall time is taken from these).
Bytes uploaded are computed from the shapes.  The report goes to stdout and to profiles/grid_source.txt.
usage: python tools/bench_grid_source.py [points] [hours] [reps]"""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
CASES = ("per-point", "grid/10", "grid/1")


def build(n, hours, want=CASES):
    """{case: (sources, uploaded bytes, seconds of to_raw_source or None, what)} for the cases in `want`.  The model's
    fields are the workload's own forecast series, one per node (node j holds the series of point j)."""
    import numpy as np
    from roadsurf_amd import driver, driver_workload, grid

    w = driver_workload.DriverWorkload(n, hours, unique=None)
    ob = driver.RawSource(w.ob_t, w.ob, True)
    ob_bytes = sum(a.nbytes for a in w.ob.values())
    rs = np.random.RandomState(5)
    cases = {}
    for tag, nodes in (("grid/10", n // 10), ("grid/1", n)):
        nx = max(2, int(round(nodes ** 0.5)))
        ny = max(2, -(-nodes // nx))
        x, y = rs.uniform(0, nx - 1, n), rs.uniform(0, ny - 1, n)
        if tag not in want and not (tag == "grid/10" and "per-point" in want):
            continue
        idx = np.arange(nx * ny) % n
        fields = {k: np.ascontiguousarray(a[idx].T) for k, a in w.fc.items()}
        node, weight = grid.bilinear_stencil(x, y, nx, ny)
        gs = grid.GridSource(w.fc_t, fields, node, weight)
        up = sum(a.nbytes for a in gs.fields.values()) + gs.node.nbytes + gs.weight.nbytes + ob_bytes
        host = raw = None
        if "time" in want or (tag == "grid/10" and "per-point" in want):     # (the timing child reports it for both grids)
            t0 = time.perf_counter()
            raw = grid.to_raw_source(gs)
            host = time.perf_counter() - t0
        cases[tag] = ([gs, ob], up, host, f"{nx} x {ny} = {nx * ny} nodes")
        if tag == "grid/10" and "per-point" in want:
            cases["per-point"] = ([raw, ob], sum(a.nbytes for a in raw.fields.values()) + ob_bytes, None,
                                  "to_raw_source of grid/10")
    return w, cases


def call(w, src, out=None):
    from roadsurf_amd import abi, driver, driver_workload
    if not hasattr(w, "loc"):
        w.loc = w.local("relax")     # (made once: 72 B per point, not part of a call)
    return driver.run(src, w.settings("relax"), abi.default_parameters(), driver_workload.START,
                      driver_workload.START + driver_workload.OBS_HOURS * 3600, cal=w.cal, local=w.loc,
                      device=-1, out=out)


class StderrToFile:
    """the library reports its phases on the C stderr: fd 2 into a file for the length of the block"""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def child_time(n, hours, reps):
    import numpy as np
    import torch
    from roadsurf_amd import driver

    if not torch.cuda.is_available():
        raise SystemExit("bench_grid_source: no GPU - nothing is measured without one")
    os.environ.setdefault("ROADSURF_HIP_DEVICES", "0,0,0,0")     # bench.py's driver legs: four blocks on this GPU
    w, cases = build(n, hours, CASES + ("time",))
    print(f"rs_driver_run, relaxation, {n} points x {hours} h (SimLen {w.simlen}), forecast {len(w.fc_t)} raw times x "
          f"{len(w.fc)} variables, fan-out {os.environ['ROADSURF_HIP_DEVICES']}, pageable host arrays")
    res, times = {}, {c: [] for c in CASES}
    for rep in range(1 + reps):                                  # alternating; rep 0 warms every shape up
        for c in CASES:
            t0 = time.perf_counter()
            res[c] = call(w, cases[c][0], res.get(c))
            dt = time.perf_counter() - t0
            if rep:
                times[c].append(dt)
    base = sum(times["per-point"]) / reps
    for c in CASES:
        src, up, host, what = cases[c]
        mean = sum(times[c]) / reps
        print(f"{c:9s} ({what}): {mean:.3f} s per call, mean of {reps} (all: {' '.join('%.3f' % t for t in times[c])}) -> "
              f"{n * w.simlen / mean:.3e} point-timesteps/s, {mean / base:.3f} x the per-point call; uploaded "
              f"{up / 1e6:.1f} MB" + (f"; to_raw_source of the same case on the host: {host:.3f} s" if host is not None else ""))
    same = all(np.array_equal(res["grid/10"][k].view(np.int64), res["per-point"][k].view(np.int64)) for k in driver.OUT_FIELDS)
    print(f"grid/10 == per-point, all six outputs bit for bit: {same}; points simulated: "
          f"{int((res['per-point']['status'] == 0).sum())} / {int((res['grid/10']['status'] == 0).sum())} / "
          f"{int((res['grid/1']['status'] == 0).sum())}")
    os.environ["ROADSURF_HIP_DRIVER_TIMING"] = "1"
    for c in CASES:
        with StderrToFile() as cap:
            call(w, cases[c][0], res[c])
        print(f"-- ROADSURF_HIP_DRIVER_TIMING=1, one {c} call (one line per block; the laps synchronise):")
        for line in cap.text.splitlines():
            if line.startswith("rs_driver_run"):
                print("   " + line)
    if not same:
        raise SystemExit("bench_grid_source: the gridded call does not equal the per-point one")


def child_trace(n, hours, case):
    os.environ.setdefault("ROADSURF_HIP_DEVICES", "0,0,0,0")
    w, cases = build(n, hours, (case,))
    r = call(w, cases[case][0])
    call(w, cases[case][0], r)


def run_step(cmd, seconds, log):
    """one child under its own time limit; its stdout is returned and kept"""
    print("bench_grid_source: " + " ".join(cmd[-5:]), flush=True)
    p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    log.append(p.stdout)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit(f"bench_grid_source: `{' '.join(cmd)}` ended with {p.returncode}: stopping here")
    return p.stdout


def kernel_rows(trace_dir):
    rows = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows[r["Name"]] = (int(r["Calls"]), int(r["TotalDurationNs"]))
    return rows


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    hours = int(sys.argv[2]) if len(sys.argv) > 2 else 48
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    me = [sys.executable, os.path.abspath(__file__)]
    log = []
    run_step(me + ["--child", "time", str(n), str(hours), str(reps)], 900, log)
    out_dir = os.path.join(ROOT, "results", "grid_source_trace")
    lines = ["-- rocprofv3 --kernel-trace --stats, one run per case, two calls each (1 warm + 1): kernels of the input side"]
    for case in ("per-point", "grid/10"):
        d = os.path.join(out_dir, case.replace("/", "_"))
        run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me +
                 ["--child", "trace", str(n), str(hours), case], 600, [])
        rows = kernel_rows(d)
        if not rows:
            lines.append(f"   {case}: no kernel statistics found under {d}")
        for name, (calls, ns) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
            if any(k in name for k in ("gather_nodes_kernel", "transpose_kernel", "fill_pad_kernel", "humidity", "scan_")):
                lines.append(f"   {case:9s} {ns / 1e6:9.3f} ms in {calls:5d} launches  {name[:110]}")
    log.append("\n".join(lines) + "\n")
    text = "".join(log)
    sys.stdout.write(text)
    from roadsurf_amd import provenance
    with open(os.path.join(ROOT, "profiles", "grid_source.txt"), "w") as fh:
        fh.write(f"# python tools/bench_grid_source.py {n} {hours} {reps}; kernel sources {provenance.csrc_sha16()}\n" + text)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        if sys.argv[2] == "time":
            child_time(int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
        else:
            child_trace(int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    else:
        main()
