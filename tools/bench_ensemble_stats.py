"""What the per-station ensemble statistics cost behind every launch of an ensemble's members (rs_hip_outputs_ens,
roadsurf_amd/ensstats.py): S stations x M members, `ha` h of analysis + `hf` h of forecast at 30 s, the shape of
tools/bench_ensemble.py - hourly knots resident on the device, a forcing window per launch of 60 indices, natural
order, fp64.  The stations are stepped over [1, B] once; then the members' leg - the fan-out and the launches over
[B + 1, L] - is timed three ways in one process:
  plain    no reducer
  stats    rs_hip_outputs_ens behind every launch: mean, spread, quantiles 0.1 / 0.5 / 0.9 of Tsurf, mean storages
  groups   rs_hip_outputs_groups behind every launch, station = group (the kernel on global cells): counts and extremes
The three alternate; medians of five rounds behind a warm-up round.  Writes profiles/ensemble_stats.txt.
usage: python tools/bench_ensemble_stats.py [stations] [members] [analysis hours] [forecast hours]"""
import os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from roadsurf_amd import abi, device, ensemble, ensstats, groups, lib, summary

S = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000
M = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ha = int(sys.argv[3]) if len(sys.argv) > 3 else 48
hf = int(sys.argv[4]) if len(sys.argv) > 4 else 26
SPK, chunk, rounds = 120, 60, 5
L, B = (ha + hf) * SPK + 1, ha * SPK
rows = L - B
dev = torch.device("cuda", 0)
s = abi.default_settings(L); p = abi.default_parameters()
parent = ensemble.parents(S, M)
n = len(parent)

st = device.Plan(S, s, p, 0)
mem = device.Plan(n, s, p, 0)
spec_s, kn_s = st.synth_knots(20240110, ha + hf + 2, steps_per_knot=SPK)
spec_m, kn_m = mem.synth_knots(20240111, ha + hf + 2, point_offset=S, steps_per_knot=SPK)
par = torch.from_numpy(parent).to(dev).long()
kn_m[:ha + 1, :, :n] = kn_s[:ha + 1].index_select(2, par)   # knots 0 .. ha: the station's
del par
wins = {pl: device.ForcingWindow.empty(chunk, pl.np_pad, dev, optional=()) for pl in (st, mem)}
win0 = device.ForcingWindow.empty(1, st.np_pad, dev, optional=("tsurfobs",))
outs = {pl: device.OutputWindow.empty(chunk, pl.np_pad, dev) for pl in (st, mem)}
pps = {pl: pl.point_params(pl.uniform_tbottom(2024, 1, 10)) for pl in (st, mem)}
keep = list(pps.values())

espec = ensstats.EnsSpec(S, M, (0.1, 0.5, 0.9))
etab = mem.ens_table(parent, espec)
eacc = torch.empty((rows, S, ensstats.cols(espec)), dtype=torch.float64, device=dev)
gspec = groups.GroupSpec(summary.SummarySpec(), S, ())
gid = torch.from_numpy(parent).to(dev)
gacc = mem.groups_reset(rows, gspec)


def launches(pl, spec, kn, lo, hi, behind=None):
    t0 = lo
    while t0 <= hi:
        ns = min(chunk, hi - t0 + 1)
        pl.expand(spec, kn, wins[pl], t0, ns)
        pl.step(wins[pl], outs[pl], pps[pl], t0, ns, out_row0=t0 - 1)
        if behind:
            behind(ns, t0 - lo)
        t0 += ns


def with_stats(ns, r0):
    mem.outputs_ens(outs[mem], ns, etab, espec, eacc, r0)


def with_groups(ns, r0):
    mem.outputs_groups(outs[mem], ns, gid, gspec, gacc, r0)


HOOKS = {"plain": None, "stats": with_stats, "groups": with_groups}


def members_leg(tag):
    if tag == "groups":                 # (the group series merge: they start from the empty cell; not timed)
        mem.groups_reset(rows, gspec, gacc)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    mem.fanout_from(st, parent)         # the members at index B + 1 again: every pass steps the same thing
    launches(mem, spec_m, kn_m, B + 1, L, HOOKS[tag])
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


st.expand(spec_s, kn_s, win0, 1, 1)
st.init_state(win0, pps[st])
launches(st, spec_s, kn_s, 1, B)
for tag in HOOKS:                       # warm-up
    members_leg(tag)
t = {tag: [] for tag in HOOKS}
for _ in range(rounds):
    for tag in HOOKS:
        t[tag].append(members_leg(tag))
# the last launch's cells of the first stations against the definition, from the window that is still there
members_leg("stats")
ns_last = (rows - 1) % chunk + 1
some = min(S, 128)
series = [outs[mem].tensors[k][:ns_last, :some * M].T.contiguous().cpu().numpy() for k in device.OUT_FIELDS]
want = ensstats.reduce_members(*series, parent[:some * M], ensstats.EnsSpec(some, M, espec.quantiles))
mem.sync()
got = eacc[rows - ns_last:, :some].cpu().numpy()
same = bool(np.array_equal(got, want, equal_nan=True))
nfail = (st.failed_count(), mem.failed_count())
med = {tag: statistics.median(x) for tag, x in t.items()}
nlaunch = (rows + chunk - 1) // chunk
read = n * 6 * 8 * rows
lines = [
    f"# {S} stations x {M} members = {n} points, {ha} h + {hf} h at 30 s (L = {L}, B = {B}): the members' leg, "
    f"{rows} indices in {nlaunch} launches of {chunk}, natural order, fp64, knots resident on the device; "
    f"medians of {rounds} alternating rounds",
    f"device: {torch.cuda.get_device_name(0)}",
    f"members' leg without a reducer: {med['plain'] * 1e3:.1f} ms per pass",
    f"with the ensemble statistics behind every launch (mean, spread, quantiles 0.1 / 0.5 / 0.9, mean storages; "
    f"{lib.ens_cols(espec)} numbers per station and row): {med['stats'] * 1e3:.1f} ms per pass, "
    f"+{(med['stats'] - med['plain']) * 1e3:.1f} ms = +{(med['stats'] / med['plain'] - 1) * 100:.1f} %, "
    f"{(med['stats'] - med['plain']) / nlaunch * 1e3:.3f} ms per launch; the reducer reads {read / 1e9:.1f} GB of rows "
    f"per pass: {read / max(med['stats'] - med['plain'], 1e-9) / 1e9:.0f} GB/s",
    f"with the per-group series behind every launch (station = group, {groups.cols(gspec)} numbers, the kernel on "
    f"{lib.group_path(gspec)} cells): {med['groups'] * 1e3:.1f} ms per pass, "
    f"+{(med['groups'] - med['plain']) * 1e3:.1f} ms = +{(med['groups'] / med['plain'] - 1) * 100:.1f} %",
    f"stays on the device: the {n} member series of {rows} rows, {n * rows * 6 * 8 / 1e9:.1f} GB; comes home: "
    f"{eacc.numel() * 8 / 1e9:.2f} GB of statistics ({gacc.numel() * 8 / 1e9:.2f} GB of group series)",
    "all rounds, ms: " + "; ".join(f"{tag}: {' '.join(f'{x * 1e3:.1f}' for x in v)}" for tag, v in t.items()),
    f"the last launch's cells of the first {some} stations equal ensstats.reduce_members of its window, bit for bit: "
    f"{same}; failed points (stations, members): {nfail}",
]
print("\n".join(lines))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "ensemble_stats.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
