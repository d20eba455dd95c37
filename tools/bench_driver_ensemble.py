"""What the ensemble form of the driver saves (rs_driver_run_ensemble, driver.run_ensemble): S stations x M members,
`ha` h of analysis + `hf` h of forecast at 30 s, hourly sources on the headline's synthetic weather, relaxation on -
an hourly forecast the stations share (an hour before the start to an hour behind the end), hourly observations over
the analysis, and an hourly forecast of every member's own from hour `ha` on.  From the caller's host arrays to the
caller's host arrays, in one session, five alternating rounds behind a warm-up round, medians:
  plain            driver.run on driver.replicate_sources: S * M unrelated points, every series home
  ensemble         driver.run_ensemble, the stations' and the members' series home
  ensemble, cells  driver.run_ensemble with stats + probs and series=False: the members' rows never leave the device
One more ensemble call under ROADSURF_HIP_DRIVER_TIMING reports the column copies and the fan-outs.
Writes profiles/driver_ensemble.txt.
usage: python tools/bench_driver_ensemble.py [stations] [members] [analysis hours] [forecast hours]"""
import os, statistics, sys, tempfile, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from roadsurf_amd import abi, driver, driver_workload as dw, ensprob, ensstats

S = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000
M = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ha = int(sys.argv[3]) if len(sys.argv) > 3 else 48
hf = int(sys.argv[4]) if len(sys.argv) > 4 else 26
rounds = 5
hours = ha + hf
L = hours * 120 + 1
START = dw.START
torch.cuda.set_device(0)

# the stations: the headline's weather as hourly knots (knot h + 1 is hour h), observations every hour of the analysis
fc, ob10 = dw._bench_weather(S, hours + 3, ha * 6 + 1, 1)
fc_t = START - 3600 + 3600 * np.arange(hours + 3, dtype=np.int64)
ob = {k: np.ascontiguousarray(v[:, ::6]) for k, v in ob10.items()}
ob_t = START + 3600 * np.arange(ha + 1, dtype=np.int64)
rs = np.random.RandomState(3)
ob["tsurfobs"][rs.rand(*ob["tsurfobs"].shape) < 0.05] = -9999.9   # observations with holes
ob["tsurfobs"][:, -2:] = np.where(ob["tsurfobs"][:, -2:] < -9000, -3.0, ob["tsurfobs"][:, -2:])
shared = [driver.RawSource(fc_t, fc, False), driver.RawSource(ob_t, ob, True)]
# the members: other weather of the same generator from hour `ha` on, 2 * S distinct series tiled over the members
n = S * M
parent = np.repeat(np.arange(S, dtype=np.int32), M)
U = min(n, 2 * S)
mfc, _ = dw._bench_weather(U, hours + 3, 1, 2)
pick = (np.arange(n) * 7919) % U
mem = driver.RawSource(fc_t[ha + 1:], {k: np.ascontiguousarray(v[:, ha + 1:][pick]) for k, v in mfc.items()}, False)
del mfc, ob10
s = abi.default_settings(L)
s.use_relaxation = 1
p = abi.default_parameters()
tf = START + ha * 3600
B, first_row, n_tail = driver.member_rows(s, START, int(mem.times[0]))
step, n_out = driver.output_rows(s)
replicated = driver.replicate_sources(shared, mem, parent)
stats = ensstats.EnsSpec(S, M, (0.1, 0.5, 0.9))
probs = ensprob.ProbSpec(S, M, (ensprob.Condition.where(tsurf=(None, 0.0)), ensprob.Condition.where(ice=(0.0, None))))
res = {"plain": None, "ensemble": None, "cells": None}


def plain():
    res["plain"] = driver.run(replicated, s, p, START, tf, out=res["plain"])


def ensemble():
    res["ensemble"] = driver.run_ensemble(shared, mem, parent, s, p, START, tf, out=res["ensemble"])


def cells():
    res["cells"] = driver.run_ensemble(shared, mem, parent, s, p, START, tf, series=False, stats=stats, probs=probs,
                                       out=res["cells"])


def timed(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


calls = {"plain": plain, "ensemble": ensemble, "cells": cells}
for c in calls.values():
    timed(c)   # warm-up: the first call allocates
t = {k: [] for k in calls}
for _ in range(rounds):
    for k, c in calls.items():
        t[k].append(timed(c))

# the column copies and the fan-outs, as the library reports them (the report synchronises: a call of its own)
os.environ["ROADSURF_HIP_DRIVER_TIMING"] = "1"
sys.stderr.flush()
with tempfile.TemporaryFile() as tmp:
    saved = os.dup(2)
    os.dup2(tmp.fileno(), 2)
    try:
        ensemble()
    finally:
        os.dup2(saved, 2)
        os.close(saved)
    tmp.seek(0)
    report = [ln.strip() for ln in tmp.read().decode(errors="replace").splitlines() if "rs_driver_run_ensemble:" in ln]
del os.environ["ROADSURF_HIP_DRIVER_TIMING"]

pl, en, ce = res["plain"], res["ensemble"], res["cells"]
same = all(np.array_equal(en["members"][k].view(np.uint64), np.ascontiguousarray(pl[k][:, first_row:]).view(np.uint64))
           for k in driver.OUT_FIELDS)
rows = [pl[k][:, first_row:] for k in driver.OUT_FIELDS]
sub = slice(0, 200 * M)   # the definitions are numpy loops: the first 200 stations
want = ensstats.reduce_members(*[r[sub] for r in rows], parent[sub], ensstats.EnsSpec(200, M, stats.quantiles))
wantp, _ = ensprob.reduce_members_prob(*[r[sub] for r in rows], None, parent[sub], ensprob.ProbSpec(200, M, probs.conditions))
same_cells = (np.array_equal(ce["stats"][:, :200].view(np.uint64), want.view(np.uint64)) and
              np.array_equal(ce["probs"][:, :200].view(np.uint64), wantp.view(np.uint64)))
med = {k: statistics.median(v) for k, v in t.items()}
up_plain = sum(a.nbytes for r in replicated for a in r.fields.values())
up_ens = sum(a.nbytes for r in shared + [mem] for a in r.fields.values())
down_plain = 6 * n * n_out * 8
down_ens = 6 * (S * n_out + n * n_tail) * 8
down_cells = 6 * S * n_out * 8 + ce["stats"].nbytes + ce["probs"].nbytes
steps_plain, steps_ens = n * L, S * B + n * (L - B)
spread = lambda v: f"{min(v) * 1e3:.0f} .. {max(v) * 1e3:.0f}"
lines = [
    f"# {S} stations x {M} members = {n} points, {ha} h + {hf} h at 30 s (L = {L}, B = {B}, first_row = {first_row}, "
    f"{n_tail} of {n_out} kept rows are the members'), hourly sources on the headline's weather, relaxation on, fp64, "
    f"one device; host arrays to host arrays (pageable), medians of {rounds} alternating rounds behind a warm-up round",
    f"device: {torch.cuda.get_device_name(0)}",
    f"plain driver.run on replicate_sources, series home: {med['plain'] * 1e3:.0f} ms (rounds {spread(t['plain'])}); "
    f"{steps_plain} point-steps, {up_plain / 1e9:.2f} GB up, {down_plain / 1e9:.2f} GB down",
    f"ensemble call, series home: {med['ensemble'] * 1e3:.0f} ms (rounds {spread(t['ensemble'])}); "
    f"{steps_ens} point-steps, {up_ens / 1e9:.2f} GB up, {down_ens / 1e9:.2f} GB down",
    f"ensemble call with stats + probs, series=False: {med['cells'] * 1e3:.0f} ms (rounds {spread(t['cells'])}); "
    f"{up_ens / 1e9:.2f} GB up, {down_cells / 1e9:.3f} GB down",
    f"plain / ensemble: {med['plain'] / med['ensemble']:.2f}x; plain / ensemble with cells only: "
    f"{med['plain'] / med['cells']:.2f}x; for {steps_plain / steps_ens:.2f}x fewer point-steps",
    "all rounds, ms: " + "; ".join(f"{k} " + " ".join(f"{x * 1e3:.0f}" for x in v) for k, v in t.items()),
    "one ensemble call under ROADSURF_HIP_DRIVER_TIMING (synchronised laps): " + (" | ".join(report) or "no report"),
    f"the members' series are the plain run's from first_row on, bit for bit: {same}; stats and probs of the first 200 "
    f"stations equal ensstats.reduce_members / ensprob.reduce_members_prob on the plain rows: {same_cells}; accepted "
    f"members: {int((en['members']['status'] == 0).sum())} of {n}",
]
print("\n".join(lines))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "driver_ensemble.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
