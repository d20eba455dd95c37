"""What the per-station probabilities of a condition cost behind every launch of an ensemble's members
(rs_hip_outputs_prob, roadsurf_amd/ensprob.py): the ensemble of tools/bench_ensemble_stats.py - S stations x M members,
`ha` h of analysis + `hf` h of forecast at 30 s, hourly knots resident on the device, a forcing window per launch of 60
indices, natural order, fp64.  The stations are stepped over [1, B] once; then the members' leg - the fan-out and the
launches over [B + 1, L] - is timed four ways in one process:
  plain    no reducer
  probs    rs_hip_outputs_prob behind every launch: tsurf < 0; ice > 0; tsurf < 2 and water > 0.05 - now and by now
  stats    rs_hip_outputs_ens behind every launch: mean, spread, quantiles 0.1 / 0.5 / 0.9 of Tsurf, mean storages
  groups   rs_hip_outputs_groups behind every launch, station = group (the kernel on global cells): counts and extremes
The four alternate; medians of five rounds behind a warm-up round, and the spread of the rounds.  Writes
profiles/ensemble_prob.txt.
usage: python tools/bench_ensemble_prob.py [stations] [members] [analysis hours] [forecast hours]"""
import os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from roadsurf_amd import abi, device, ensemble, ensprob, ensstats, groups, lib, summary

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

W = ensprob.Condition.where
pspec = ensprob.ProbSpec(S, M, (W(tsurf=(None, 0.0)), W(ice=(0.0, None)), W(tsurf=(None, 2.0), water=(0.05, None))))
espec = ensstats.EnsSpec(S, M, (0.1, 0.5, 0.9))
etab = mem.ens_table(parent, espec)                          # one table for both reducers
pacc = torch.empty((rows, S, ensprob.cols(pspec)), dtype=torch.float64, device=dev)
pever = mem.prob_reset()
pwork = torch.empty((mem.prob_work_ints(chunk),), dtype=torch.int32, device=dev)
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


def with_probs(ns, r0):
    mem.outputs_prob(outs[mem], ns, etab, pspec, pever, pacc, r0, work=pwork)


def with_stats(ns, r0):
    mem.outputs_ens(outs[mem], ns, etab, espec, eacc, r0)


def with_groups(ns, r0):
    mem.outputs_groups(outs[mem], ns, gid, gspec, gacc, r0)


HOOKS = {"plain": None, "probs": with_probs, "stats": with_stats, "groups": with_groups}


def members_leg(tag):
    if tag == "groups":                 # (the group series merge: they start from the empty cell; not timed)
        mem.groups_reset(rows, gspec, gacc)
    if tag == "probs":                  # (a pass starts with no condition held; 4 B per member, not timed either)
        mem.prob_reset(pever)
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
# the last launch's cells of the first stations against the definition, from the window that is still there: column 0
# and NOW are the window's own; BY_NOW of the last row is what the carry says of the members valid there
members_leg("probs")
ns_last = (rows - 1) % chunk + 1
some = min(S, 128)
series = [outs[mem].tensors[k][:ns_last, :some * M].T.contiguous().cpu().numpy() for k in device.OUT_FIELDS]
small = ensprob.ProbSpec(some, M, pspec.conditions)
want, _ = ensprob.reduce_members_prob(*series, None, parent[:some * M], small)
mem.sync()
got = pacc[rows - ns_last:, :some].cpu().numpy()
C_ = len(pspec.conditions)
carry = pever[:some * M].cpu().numpy()
valid_last = series[0][:, -1] != -9999.0
by_last = np.stack([np.bincount(parent[:some * M], weights=valid_last & (carry >> c & 1 > 0), minlength=some)
                    for c in range(C_)], axis=1)
same = bool(np.array_equal(got[:, :, :1 + C_], want[:, :, :1 + C_]) and np.array_equal(got[-1, :, 1 + C_:], by_last))
whole = pacc.cpu().numpy()
mixed = [int(((whole[:, :, 1 + c] > 0) & (whole[:, :, 1 + c] < whole[:, :, 0])).sum()) for c in range(C_)]
later = [int((whole[:, :, 1 + C_ + c] > whole[:, :, 1 + c]).sum()) for c in range(C_)]
nfail = (st.failed_count(), mem.failed_count())
med = {tag: statistics.median(x) for tag, x in t.items()}
nlaunch = (rows + chunk - 1) // chunk
read = n * 6 * 8 * rows


def cost(tag):
    extra = [x - y for x, y in zip(t[tag], t["plain"])]     # round by round: the rounds alternate
    return (f"{med[tag] * 1e3:.1f} ms per pass, +{(med[tag] - med['plain']) * 1e3:.1f} ms = "
            f"+{(med[tag] / med['plain'] - 1) * 100:.1f} %, {(med[tag] - med['plain']) / nlaunch * 1e3:.3f} ms per launch "
            f"(round by round +{min(extra) * 1e3:.1f} .. +{max(extra) * 1e3:.1f} ms)")


lines = [
    f"# {S} stations x {M} members = {n} points, {ha} h + {hf} h at 30 s (L = {L}, B = {B}): the members' leg, "
    f"{rows} indices in {nlaunch} launches of {chunk}, natural order, fp64, knots resident on the device; "
    f"medians of {rounds} alternating rounds",
    f"device: {torch.cuda.get_device_name(0)}",
    f"members' leg without a reducer: {med['plain'] * 1e3:.1f} ms per pass "
    f"(rounds {min(t['plain']) * 1e3:.1f} .. {max(t['plain']) * 1e3:.1f} ms)",
    f"with the probabilities behind every launch (tsurf < 0; ice > 0; tsurf < 2 and water > 0.05: valid members, now "
    f"and by now, {lib.prob_cols(pspec)} numbers per station and row): {cost('probs')}; the reducer reads "
    f"{read / 1e9:.1f} GB of rows per pass: {read / max(med['probs'] - med['plain'], 1e-9) / 1e9:.0f} GB/s",
    f"with the ensemble statistics behind every launch (mean, spread, quantiles 0.1 / 0.5 / 0.9, mean storages; "
    f"{lib.ens_cols(espec)} numbers per station and row), the yardstick - it reads the same rows: {cost('stats')}; "
    f"probs / stats = {(med['probs'] - med['plain']) / max(med['stats'] - med['plain'], 1e-9):.2f}",
    f"with the per-group series behind every launch (station = group, {groups.cols(gspec)} numbers, the kernel on "
    f"{lib.group_path(gspec)} cells): {cost('groups')}",
    f"stays on the device: the {n} member series of {rows} rows, {n * rows * 6 * 8 / 1e9:.1f} GB; comes home: "
    f"{pacc.numel() * 8 / 1e9:.2f} GB of counts ({eacc.numel() * 8 / 1e9:.2f} GB of statistics, "
    f"{gacc.numel() * 8 / 1e9:.2f} GB of group series); scratch of the probabilities: {pwork.numel() * 4 / 1e6:.0f} MB",
    "all rounds, ms: " + "; ".join(f"{tag}: {' '.join(f'{x * 1e3:.1f}' for x in v)}" for tag, v in t.items()),
    f"cells of {rows * S} with some but not all valid members under the condition, per condition: {mixed}; with more "
    f"members by now than now: {later}",
    f"the last launch's cells of the first {some} stations: column 0 and NOW equal ensprob.reduce_members_prob of its "
    f"window, BY_NOW of the last row equals the carry under the members valid there: {same}; failed points "
    f"(stations, members): {nfail}",
]
print("\n".join(lines))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "ensemble_prob.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
