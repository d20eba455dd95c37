"""What branching an ensemble forecast from one analysis run saves (rs_hip_state_fanout, roadsurf_amd/ensemble.py):
S stations x M members, `ha` h of analysis + `hf` h of forecast at 30 s, on the headline's synthetic weather - hourly
knots resident on the device, expanded into a forcing window per launch of 60 indices, natural order, fp64.
  plain      one plan of S * M points over [1, L]; every member carries its station's knots up to the branch
  ensemble   a plan of S points over [1, B], the fan-out, a plan of S * M points over [B + 1, L]
B = ha * 120: the knot of hour `ha` is the last the members of a station share.  Both sides read device-resident
knots and write the same output windows; five alternating rounds behind a warm-up round, medians.  The fan-out's own
time is taken between two events on the member plan's stream.  Writes profiles/ensemble_fanout.txt.
usage: python tools/bench_ensemble.py [stations] [members] [analysis hours] [forecast hours]"""
import os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
from roadsurf_amd import abi, device, ensemble

S = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000
M = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ha = int(sys.argv[3]) if len(sys.argv) > 3 else 48
hf = int(sys.argv[4]) if len(sys.argv) > 4 else 26
SPK, chunk, rounds = 120, 60, 5
L, B = (ha + hf) * SPK + 1, ha * SPK
dev = torch.device("cuda", 0)
s = abi.default_settings(L); p = abi.default_parameters()
parent = ensemble.parents(S, M)
n = len(parent)

st = device.Plan(S, s, p, 0)
mem = device.Plan(n, s, p, 0)      # the plain run's plan too: one side runs at a time
spec_s, kn_s = st.synth_knots(20240110, ha + hf + 2, steps_per_knot=SPK)
spec_m, kn_m = mem.synth_knots(20240111, ha + hf + 2, point_offset=S, steps_per_knot=SPK)
par = torch.from_numpy(parent).to(dev).long()
kn_m[:ha + 1, :, :n] = kn_s[:ha + 1].index_select(2, par)   # knots 0 .. ha: the station's
del par
wins = {pl: device.ForcingWindow.empty(chunk, pl.np_pad, dev, optional=()) for pl in (st, mem)}
win0 = {pl: device.ForcingWindow.empty(1, pl.np_pad, dev, optional=("tsurfobs",)) for pl in (st, mem)}
outs = {pl: device.OutputWindow.empty(chunk, pl.np_pad, dev) for pl in (st, mem)}
pps = {pl: pl.point_params(pl.uniform_tbottom(2024, 1, 10)) for pl in (st, mem)}
keep = list(pps.values())
last = {}


def leg(pl, spec, kn, lo, hi, init):
    if init:
        pl.expand(spec, kn, win0[pl], 1, 1)
        pl.init_state(win0[pl], pps[pl])
    t0 = lo
    while t0 <= hi:
        ns = min(chunk, hi - t0 + 1)
        pl.expand(spec, kn, wins[pl], t0, ns)
        pl.step(wins[pl], outs[pl], pps[pl], t0, ns, out_row0=t0 - 1)
        t0 += ns


fan = [torch.cuda.Event(enable_timing=True) for _ in range(2)]


def plain():
    leg(mem, spec_m, kn_m, 1, L, True)


def branched():
    leg(st, spec_s, kn_s, 1, B, True)
    fan[0].record(mem.stream)
    mem.fanout_from(st, parent)
    fan[1].record(mem.stream)
    leg(mem, spec_m, kn_m, B + 1, L, False)


def timed(call, tag):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    last[tag] = {k: v[:1].clone() for k, v in outs[mem].tensors.items()}   # the row of index L
    return dt


timed(plain, "plain"); timed(branched, "ensemble")   # warm-up
t = {"plain": [], "ensemble": []}
fan_ms = []
for _ in range(rounds):
    t["plain"].append(timed(plain, "plain"))
    t["ensemble"].append(timed(branched, "ensemble"))
    fan_ms.append(fan[0].elapsed_time(fan[1]))
same = all(torch.equal(last["plain"][k], last["ensemble"][k]) for k in device.OUT_FIELDS)
nfail = (st.failed_count(), mem.failed_count())
rows = 15 + 17                      # Tmp(1..NLayers) and the named rows: what an uncoupled fan-out copies
wrote, read = rows * n * 8, rows * S * 8   # every dst cell once; the members of a station read the same src cells
index = n * 4 * 2 + n * 4                  # the parent row uploaded and read, dst's order row where it has one
moved = wrote + read + index
mp, me, mf = (statistics.median(x) for x in (t["plain"], t["ensemble"], fan_ms))
lines = [
    f"# {S} stations x {M} members = {n} points, {ha} h + {hf} h at 30 s (L = {L}, B = {B}), launches of {chunk}, "
    f"natural order, fp64, knots resident on the device; medians of {rounds} alternating rounds",
    f"device: {torch.cuda.get_device_name(0)}",
    f"plain run of the {n} replicated points over [1, L]: {mp * 1e3:.1f} ms ({n * L} point-steps, {n * L / mp:.3e}/s)",
    f"ensemble (stations over [1, B], fan-out, members over [B + 1, L]): {me * 1e3:.1f} ms "
    f"({S * B + n * (L - B)} point-steps, {(S * B + n * (L - B)) / me:.3e}/s)",
    f"plain / ensemble: {mp / me:.2f}x in time for {n * L / (S * B + n * (L - B)):.2f}x fewer point-steps",
    f"the fan-out alone (parent check on the host aside; upload of the parent row, kernel): {mf:.3f} ms between events "
    f"for {moved / 1e6:.1f} MB moved - {rows} rows: {wrote / 1e6:.1f} MB written, {read / 1e6:.1f} MB of distinct "
    f"source cells read, {index / 1e6:.1f} MB of indices - = {moved / mf / 1e6:.0f} GB/s",
    f"all rounds, plain ms: {' '.join(f'{x * 1e3:.1f}' for x in t['plain'])}; ensemble ms: "
    f"{' '.join(f'{x * 1e3:.1f}' for x in t['ensemble'])}; fan-out ms: {' '.join(f'{x:.3f}' for x in fan_ms)}",
    f"the members' rows of index L are the plain run's, bit for bit: {same}; failed points (stations, members): {nfail}",
]
print("\n".join(lines))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "ensemble_fanout.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
