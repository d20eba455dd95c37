"""GPU: what the register diet of the LEAN knot-reading two-wavefront kernel can break, and the re-sort chain's
kernels that were slimmed beside it.

(a) The surface wavefront reads part of its mailbox - humidity, short- and long-wave radiation, Tmp(3) - where a step
first uses it, behind the boundary-layer loop, instead of at the top of the index: right only while the ground
wavefront writes the OTHER buffer during that index.  The ground wavefront reads the bottom temperature again at every
index and its knot column through a 32-bit entry of the order row, and both form the point's row again for their
final stores.  So: the LEAN knot-reading flavour in plan order, the order row shuffled before every launch (the
re-read constants then go through the gather), against the one-point-per-lane window flavour in natural order on the
same points - all six outputs at every index and the carried state, bit for bit.  Launches of 1, 2, 3 and 121
indices (both buffer parities, a knot interval crossed inside a launch), each started on a knot, one index before a
knot and between knots; 1, 64, 65 and 129 points; a third of the points under precipitation around 0 C, a third wet
from the first hour's rain under a dry sky after it, so that a wavefront has lanes that read the rain, the snow and
the humidity beside lanes that do not; a bottom temperature of its own for every point.

(b) The plan's counting sort and the forecast keys it sorts: the order rows of the first launches of bench.py's
workload at 1 000 and 70 000 points with the default mode (378059: two stable passes, the ground digit first) are
those the library produced before the chain kernels were brought under 32 registers - recorded then, in
tests/golden/duo_sort_orders.json, as the row's SHA-256 (the whole row for 1 000 points' first re-sort)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import golden_helpers as gh
import knot_helpers as kh
import oracle_helpers as oh
from roadsurf_amd import abi, synth

pytestmark = pytest.mark.gpu
SPK = 120
OUT = oh.F64_OUT
LENGTHS = (1, 2, 3, 121)
STARTS = (0, SPK - 1, 57)  # (t0 - 1) mod SPK: on a knot, one index before a knot, between knots
SIZES = (1, 64, 65, 129)
START_HOUR = 17
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "duo_sort_orders.json")


def _launches():
    """[(t0, nsteps, wanted)]: every length at every start, the gaps filled by launches of their own"""
    todo = [(n, s) for n in LENGTHS for s in STARTS]
    out, t0 = [], 1
    while todo:
        n, s = min(todo, key=lambda c: ((c[1] - (t0 - 1)) % SPK, c[0]))
        gap = (s - (t0 - 1)) % SPK
        if gap:
            out.append((t0, gap, False))
            t0 += gap
        out.append((t0, n, True))
        t0 += n
        todo.remove((n, s))
    return out, t0 - 1


LAUNCHES, L = _launches()


def test_the_launch_list_is_what_the_docstring_says():
    got = {(ns, (t0 - 1) % SPK) for t0, ns, wanted in LAUNCHES if wanted}
    assert got == {(n, s) for n in LENGTHS for s in STARTS}
    assert sum(ns for _, ns, _ in LAUNCHES) == L and LAUNCHES[0][0] == 1
    assert all(a[0] + a[1] == b[0] for a, b in zip(LAUNCHES, LAUNCHES[1:]))
    assert {t0 & 1 for t0, ns, w in LAUNCHES if w and ns == 1} == {0, 1}
    assert any((t0 - 1) % SPK + ns > SPK for t0, ns, w in LAUNCHES if w)  # a knot crossed inside a launch


@functools.lru_cache(None)
def _knots(n):
    nk = (L - 1) // SPK + 2
    f = synth.synth_forcing(n, (nk - 1) * SPK + 1, seed=20241021, steps_per_knot=SPK, start_hour=START_HOUR)
    K = {k: np.ascontiguousarray(f[k][:, ::SPK]) for k in gh.KNOT_FIELDS}
    K["phase"] = np.ascontiguousarray(f["precphase"][:, ::SPK])
    K["tsurf0"] = f["tsurfobs"][:, 0].copy()
    j = np.arange(nk)
    for p in range(0, n, 3):  # precipitation at every other knot, the air around 0 C: rain, sleet and snow
        K["prec"][p] = np.where(j % 2 == 0, 1.5 + 0.1 * (p % 7), 0.0)
        K["tair"][p] = np.where(j % 3 == 0, 0.6, np.where(j % 3 == 1, -1.4, 0.2)) + 0.01 * (p % 5)
        K["tdew"][p] = K["tair"][p] - 0.3
        K["rhz"][p] = 97.0 - (p % 4)
        K["phase"][p] = -9999 if p % 6 == 0 else K["phase"][p]
        K["tsurf0"][p] = 0.3
    for p in range(1, n, 3):  # rain in the first hour, none after it: a wet surface under a dry sky
        K["prec"][p] = np.where(j == 0, 2.0, 0.0)
        K["tair"][p] = 3.0 + 0.1 * (p % 9) - 0.2 * j
        K["tdew"][p] = K["tair"][p] - 1.0
        K["rhz"][p] = 80.0 + (p % 11)
        K["phase"][p] = 1
        K["tsurf0"][p] = 2.0
    return K


def _run(n, variant, source, shuffle):
    """The block through the launches of LAUNCHES: (outputs [n][L], carried state rows [rows][n] in point order,
    failed, how many slots the shuffles moved)"""
    import torch
    from roadsurf_amd import device, lib, workload
    K = _knots(n)
    s, p = abi.default_settings(L), abi.default_parameters()
    plan = device.Plan(n, s, p, 0)
    plan.set_variant(variant)
    plan.set_history_score(False)
    dev, npad = plan.device, plan.np_pad
    try:
        knots = torch.from_numpy(kh.knot_block(K, npad)).to(dev)
        spec = lib.RsSynthSpec(0, 0, SPK, START_HOUR)
        f1 = kh.expand(K, 1, SPK, START_HOUR)
        win0 = device.ForcingWindow.empty(1, npad, dev, optional=("tdew", "tsurfobs"))
        for name, t in win0.tensors.items():
            if t is None or name == "hour":
                continue
            t.zero_()
            t[0, :n] = torch.from_numpy(np.ascontiguousarray(f1[name][:, 0])).to(dev)
        win0.tensors["hour"][0] = int(f1["hour"][0])
        tb_point = plan.uniform_tbottom(*kh.start_of(START_HOUR)[:3]) + 0.01 * np.arange(n)

        def params_in(row):
            t = torch.zeros((npad,), dtype=torch.float64, device=dev)
            t[:n] = torch.from_numpy(np.ascontiguousarray(tb_point[row])).to(dev)
            return plan.point_params(t)

        rows = max(ns for _, ns, _ in LAUNCHES)
        out = device.OutputWindow.empty(rows, npad, dev)
        win = device.ForcingWindow.empty(rows, npad, dev, optional=()) if source == "window" else None
        plan.reset_order()
        ident = np.arange(n)
        plan.init_state(win0, params_in(ident))
        got = {k: np.full((n, L), np.nan) for k in OUT}
        gen = torch.Generator().manual_seed(77 + n)
        moved = 0
        row = ident
        for c, (t0, ns, _) in enumerate(LAUNCHES):
            if shuffle:  # the plan's own sort on previews nobody forecast: a permutation, and the state moved with it
                ta = (torch.rand(npad, generator=gen, dtype=torch.float64) * 20.0 - 15.0).to(dev)
                vz = (torch.rand(npad, generator=gen, dtype=torch.float64) * 11.7 + 0.3).to(dev)
                pr = (torch.rand(npad, generator=gen, dtype=torch.float64) < 0.3).double().to(dev)
                plan.recluster_forecast([ta], [vz], [(START_HOUR + c) % 24], ta, 0.5, workload.DEFAULT_FORECAST_MODE,
                                        point_order=True, prec_rows=[pr])
            plan.sync()
            row = plan.order().cpu().numpy()[:n].astype(np.int64)
            assert np.array_equal(np.sort(row), ident)
            moved += int((row != ident).sum())
            pp = params_in(row)
            if source == "knots":
                plan.step_knots(spec, knots, out, pp, t0, ns, out_row0=t0 - 1)
            else:
                plan.expand_ordered(spec, knots, win, t0, ns)
                plan.step(win, out, pp, t0, ns, out_row0=t0 - 1)
            plan.sync()
            for k in OUT:
                got[k][row, t0 - 1:t0 - 1 + ns] = out.tensors[k][:ns, :n].cpu().numpy().T
        st = plan.state().numpy()
        keep = list(range(int(s.NLayers))) + list(range(lib.RS_MAX_LAYERS, lib.RS_MAX_LAYERS + 13))  # Tmp, TmpNw(1:2) ... failed
        state = np.empty((len(keep), n))
        state[:, row] = st[keep][:, :n]
        return got, state, plan.failed_count(), moved
    finally:
        plan.close()


@functools.lru_cache(None)
def _pair(n):
    ref = _run(n, 1, "window", False)   # one point per lane, forcing windows, natural order
    duo = _run(n, kh.DUO, "knots", True)  # two wavefronts, knots, shuffled plan order
    return ref, duo


@pytest.mark.parametrize("n", SIZES)
def test_late_mailbox_reads_and_reread_constants_keep_every_bit(n):
    (ref, ref_state, ref_failed, ref_moved), (duo, duo_state, duo_failed, duo_moved) = _pair(n)
    assert ref_moved == 0 and (duo_moved > 0) == (n > 1)
    assert ref_failed == 0 and duo_failed == 0
    for k in OUT:
        assert not np.isnan(ref[k]).any() and not np.isnan(duo[k]).any(), k
        ndiff = int((ref[k].view(np.uint64) != duo[k].view(np.uint64)).sum())
        print(f"n={n} {k}: {ndiff} of {ref[k].size} values differ in their bits")
        assert ndiff == 0, k
    nd = int((ref_state.view(np.uint64) != duo_state.view(np.uint64)).sum())
    print(f"n={n} carried state: {nd} of {ref_state.size} values differ in their bits")
    assert nd == 0


@pytest.mark.parametrize("n", SIZES)
def test_the_crafted_points_have_rain_snow_and_wet_surfaces_in_one_wavefront(n):
    """(what makes the late reads of rain, snow and humidity count: read from the reference flavour's rows)"""
    (ref, _, _, _), _ = _pair(n)
    snowy = (ref["snow"] > 0.0).any(axis=1)
    assert snowy[0::3].all()  # the points under precipitation around 0 C: the snow storage fills (and the water of some)
    if n > 1:
        assert (ref["water"][1::3, 2 * SPK:] > 0.0).any(axis=1).all()  # wet from the first hour's rain, hours behind it
        assert not snowy[1::3].any()
    if n >= 64:  # the third class keeps generator weather: lanes with a bare, dry road in the same wavefront
        bare = np.ones(n, bool)
        for k in OUT[1:]:
            bare &= ~(ref[k] > 0.0).any(axis=1)
        print(f"n={n}: {int(bare[:64].sum())} lanes of the first wavefront stay bare and dry")
        assert bare[:64].any()


# ---- (b) the sort ---------------------------------------------------------------------------------------------------

SORT_SIZES = (1000, 70000)
SORT_HOURS, SORT_CHUNK = 3, 60


def sort_orders(n):
    """The order rows of the launches of a short pass of bench.py's workload: [launch][n] int32"""
    from roadsurf_amd import device, workload
    Ls = SORT_HOURS * SPK + 1
    plan = device.Plan(n, abi.default_settings(Ls), abi.default_parameters(), 0)
    try:
        plan.set_variant(kh.DUO)
        run = workload.SyntheticRun(plan, 2024, SORT_HOURS, SORT_CHUNK, point_offset=123_000, plan_order=True, resort=True)
        assert run.forecast_mode == workload.DEFAULT_FORECAST_MODE == 378059
        rows = []
        run.run_pass(lambda c, t0, ns: rows.append(run.orders[c][:n].cpu().numpy().astype(np.int32)))
        plan.sync()
        assert plan.failed_count() == 0
        del run
    finally:
        plan.close()
    return rows


def digest(rows):
    return [hashlib.sha256(np.ascontiguousarray(r, dtype="<i4").tobytes()).hexdigest() for r in rows]


@pytest.mark.parametrize("n", SORT_SIZES)
def test_count_sort_and_forecast_keys_order_the_plan_as_before(n):
    gold = json.load(open(GOLDEN))[str(n)]
    rows = sort_orders(n)
    assert len(rows) == -(-(SORT_HOURS * SPK + 1) // SORT_CHUNK) == len(gold["sha256"])
    for r in rows:
        assert np.array_equal(np.sort(r), np.arange(n))
    assert any((r != np.arange(n)).any() for r in rows[1:])
    if "first_resort" in gold:
        assert np.array_equal(rows[1], np.asarray(gold["first_resort"], np.int32))
    assert digest(rows) == gold["sha256"]
