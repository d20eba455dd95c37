"""What the inputs at the kept rows and the dew-point deficit cost (rs_driver_run_kept): bench.py's
driver_path_relax_bench_weather call - driver_workload's shape on the headline's weather, relaxation, hourly rows,
the library's fan-out of four blocks on one GPU, pageable host arrays - made
  without     as rs_driver_run makes it: the six output series,
  with        ... and the air temperature and the dew point at the kept rows and the dew-point deficit: three more
              [n_points][n_out] arrays come home, each through a transpose on the device.
Both calls compute the same six series; the tool checks that on the bits, and the three extra arrays against the
definition (roadsurf_amd/kept.py) where the inputs allow it without a second implementation: the deficit is
dew_point_deficit of the call's own surface temperature and dew point.

The parent process never touches the GPU.  It starts one child under a time limit: both cases in one session,
alternating, one warm call each, then `reps` timed ones (wall clock around calls that end with the results in host
arrays, which are reused from call to call); the median of each case, the two rates and the difference are reported.
Bytes downloaded are computed from the shapes.  The report goes to stdout and to profiles/kept_rows.txt.
usage: python tools/bench_kept_rows.py [points] [hours] [reps]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
CASES = ("without", "with")
KEPT = ("tair", "tdew")


def child(n, hours, reps):
    import numpy as np
    import torch
    from roadsurf_amd import abi, driver, driver_workload, kept

    if not torch.cuda.is_available():
        raise SystemExit("bench_kept_rows: no GPU - nothing is measured without one")
    os.environ.setdefault("ROADSURF_HIP_DEVICES", "0,0,0,0")     # bench.py's driver legs: four blocks on this GPU
    w = driver_workload.DriverWorkload(n, hours, unique=None, weather="bench")
    src, s, p, loc = w.sources("relax"), w.settings("relax"), abi.default_parameters(), w.local("relax")
    step, n_out = driver.output_rows(s)
    print(f"rs_driver_run, relaxation, {n} points x {hours} h (SimLen {w.simlen}) on bench.py's weather, {n_out} kept rows "
          f"(step {step}), fan-out {os.environ['ROADSURF_HIP_DEVICES']}, pageable host arrays")

    def call(case, out):
        kw = dict(kept=KEPT, deficit=True) if case == "with" else {}
        return driver.run(src, s, p, driver_workload.START, driver_workload.START + driver_workload.OBS_HOURS * 3600,
                          cal=w.cal, local=loc, device=-1, out=out, **kw)

    res, times = {}, {c: [] for c in CASES}
    for rep in range(1 + reps):                                  # alternating; rep 0 warms both shapes up
        for c in CASES:
            t0 = time.perf_counter()
            res[c] = call(c, res.get(c))
            dt = time.perf_counter() - t0
            if rep:
                times[c].append(dt)
    med = {c: statistics.median(times[c]) for c in CASES}
    down = {"without": 6 * n * n_out * 8, "with": (6 + len(KEPT) + 1) * n * n_out * 8}
    for c in CASES:
        print(f"{c:8s}: {med[c]:.3f} s per call, median of {reps} (all: {' '.join('%.3f' % t for t in times[c])}) -> "
              f"{n * w.simlen / med[c]:.3e} point-timesteps/s; downloaded {down[c] / 1e6:.1f} MB of series")
    extra = med["with"] - med["without"]
    print(f"difference: {extra * 1e3:+.1f} ms per call ({100.0 * extra / med['without']:+.1f} %) for "
          f"{(down['with'] - down['without']) / 1e6:.1f} MB more and {len(KEPT) + 1} more transposes")
    a, b = res["without"], res["with"]
    same = all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in driver.OUT_FIELDS) and \
        np.array_equal(a["status"], b["status"])
    want = kept.dew_point_deficit(b["tsurf"], b["kept"]["tdew"])
    deficit_ok = np.array_equal(want.view(np.int64), b["deficit"].view(np.int64))
    ok = b["status"] == 0
    print(f"six outputs and status of the two calls equal bit for bit: {same}; deficit == dew_point_deficit(tsurf, tdew): "
          f"{deficit_ok}; points simulated: {int(ok.sum())}; deficits below / above 0 among them: "
          f"{int((b['deficit'][ok] < 0).sum())} / {int((b['deficit'][ok] > 0).sum())}")
    if not (same and deficit_ok):
        raise SystemExit("bench_kept_rows: the call with the kept rows does not equal the call without")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    hours = int(sys.argv[2]) if len(sys.argv) > 2 else 48
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), str(hours), str(reps)]
    print("bench_kept_rows: " + " ".join(cmd[-4:]), flush=True)
    p = subprocess.run(["timeout", "-k", "10", "900"] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-3000:])
        raise SystemExit(f"bench_kept_rows: the child ended with {p.returncode}: nothing is written")
    from roadsurf_amd import provenance
    with open(os.path.join(ROOT, "profiles", "kept_rows.txt"), "w") as fh:
        fh.write(f"# python tools/bench_kept_rows.py {n} {hours} {reps}; kernel sources {provenance.csrc_sha16()}\n" + p.stdout)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
