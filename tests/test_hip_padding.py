"""GPU: columns beyond npoints never reach a live point.

The kernels launch whole wavefronts over npoints_padded columns, and the caller owns every array it hands over.
Every case here is built twice (tests/padding_helpers.py): CLEAN, as the rest of the suite pads - zeros behind n -
and HOSTILE, with every caller-owned array inside guard bands, windows of np_pad + 64 columns, RsPointParams arrays
of exactly n elements (include/roadsurf.h) and poison in every element that is no live column.  Exact comparisons
throughout:

  (a) every output row of every live point and every live column of the state block is the same in both builds;
  (b) the fp64 clean build equals the reference (test_hip_parity's kind and comparison; the coupled cases take the
      reference build in which coupling acts, as tests/test_hip_coupling.py does);
  (c) after the hostile run the guard bands of every output, the columns [n, t_stride) of every output row and
      the whole of every input buffer (forcing, knots, parameter arrays) hold what they held before the launch.
      Only the pad columns of the state block are exempt: they are the plan's own;
  (d) plan.failed_count() and plan.first_failed_index() are the same in both builds, and with `failing` poison
      exactly what the live points give;
  (e) re-sorts with poisoned pad columns in the rows they read leave order()[:n] a permutation of the live points
      and order()[n:] the identity, and the outputs mapped back equal the natural-order run.

SimLen 241 (two hours and the final index, launches of 120, 120 and 1), n in 1, 63, 65, 129, 203, 257.  The seed
of a size comes from a fixed candidate list, by the oracle's series alone: the ragged last wavefront is bare and dry
for a quarter of the series and is not for another quarter (padding_helpers.prepare: every live point of the wave
at once, 64 points or the 128 of the fp32 two-points-per-lane kernels, on the case's own data, whose last wave is
given a dry first hour), so zero padding lets that wave take the wave-wide shortcuts and `opposite` padding forbids
them."""
import numpy as np
import pytest
import torch

import oracle_helpers as oh
import padding_helpers as ph
from padding_helpers import Case
from roadsurf_amd import abi, device
from test_hip_parity import _compare

pytestmark = pytest.mark.gpu

REG, LDS, DUO, HYBRID = 1, 2, 3, 4  # tests/test_step_selection.py pins what each selects

CASES = [
    Case("f64-reg-lean", variant=REG), Case("f64-lds-lean", variant=LDS), Case("f64-duo-lean", variant=DUO),
    Case("f64-reg-full", variant=REG, full=True), Case("f64-lds-full", variant=LDS, full=True),
    Case("f64-duo-full", variant=DUO, full=True), Case("f64-hybrid-full", variant=HYBRID, full=True),
    Case("f64-knots-lean", variant=DUO, src="knots"), Case("f64-knots-full", variant=DUO, src="knots", full=True),
    # sky-hybrid: without 32-bit window offsets a sky launch takes step_kernel_sky_h<4> (tests/test_step_selection.py,
    # row a32=0 full sky npoints=1000); run_case asserts that the limit is one the library honours and that every launch
    # is over it
    Case("f64-sky-duo", sky=True), Case("f64-sky-hybrid", sky=True, a32_limit="1024"),
    Case("f64-cpl-general", cpl="general"), Case("f64-cpl-chunk", cpl="chunk"),
    Case("f32-duo-lean", precision=32), Case("f32-duo-full", precision=32, full=True),
    Case("f32-knots-lean", precision=32, src="knots"), Case("f32-knots-full", precision=32, src="knots", full=True),
    Case("f32-duo-sky", precision=32, sky=True), Case("f32-lds", precision=32, variant=LDS),
    Case("f32-coupled-depth", precision=32, depth=True),
]
BY_NAME = {c.name: c for c in CASES}
THREE = ("f64-duo-lean", "f32-duo-full", "f32-knots-lean")  # the kernels every poison class runs on


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(ph.np_bits(a), ph.np_bits(b))


def _pair(case, cls, monkeypatch, by_point=False):
    """Both builds of a case at every size; every violated property of every size in one list."""
    if case.a32_limit:
        monkeypatch.setenv("ROADSURF_HIP_A32_LIMIT", case.a32_limit)
    failing = cls == "failing"
    wrong = []
    for n in ph.SIZES:
        seed, frac, ora = ph.prepare(case, n)
        assert 0.25 <= frac <= 0.75, (n, seed, frac)  # non-vacuity, from the oracle's series alone
        clean = ph.run_case(case, n, seed, None, failing, by_point)
        host = ph.run_case(case, n, seed, cls, failing, by_point)
        tag = f"{case.name}/{cls}/n={n}"
        # (a)
        for k in device.OUT_FIELDS:
            if not _same_bits(clean["out"][k], host["out"][k]):
                d = np.argwhere(ph.np_bits(clean["out"][k]) != ph.np_bits(host["out"][k]))
                wrong.append(f"{tag}: (a) {k} differs at {len(d)} places, first (point, row) {d[0].tolist()}")
        for which in ("state0", "state"):
            if not _same_bits(clean[which], host[which]):
                d = np.argwhere(ph.np_bits(clean[which]) != ph.np_bits(host[which]))
                wrong.append(f"{tag}: (a) {which} differs at {len(d)} places, first (row, point) {d[0].tolist()}")
        # (b)
        if case.precision == 64:
            if failing:
                f, s, p, ls, _ = ph.case_data(case, n, seed, failing)
                ora, _, _ = oh.run_oracle(ph.oracle_kind(case), f, s, p, ls)
            try:
                _compare(clean["out"], ora, tag)
            except AssertionError as e:
                wrong.append(f"{tag}: (b) {e}")
        # (c)
        for name, where in host["touched"]:
            wrong.append(f"{tag}: (c) {name} was written outside the live columns, first elements {where}")
        # (d)
        if clean["failed"] != host["failed"] or not np.array_equal(clean["first_failed"], host["first_failed"]):
            wrong.append(f"{tag}: (d) failed_count {clean['failed']} / {host['failed']}, first_failed_index differs at "
                         f"{np.flatnonzero(clean['first_failed'] != host['first_failed'])[:4].tolist()}")
        if failing:
            bad = host["bad"]
            if host["failed"] != len(bad) or set(np.flatnonzero(host["first_failed"]).tolist()) != set(bad):
                wrong.append(f"{tag}: (d) {host['failed']} failed points {np.flatnonzero(host['first_failed']).tolist()}, "
                             f"the live points give {sorted(bad)}")
            if case.src == "window" and any(int(host["first_failed"][pt]) != idx + 1 for pt, idx in bad.items()):
                wrong.append(f"{tag}: (d) first_failed_index {host['first_failed'][list(bad)].tolist()} for {bad}")
        if by_point:
            for r in (clean, host):
                for k in device.OUT_FIELDS:
                    d = r["dst"][k]
                    if not _same_bits(np.ascontiguousarray(d[:, 7:]), r["out"][k]):
                        wrong.append(f"{tag}: outputs_by_point {k}: not the rows of the window")
                    if not _same_bits(d[:, :7], np.full((n, 7), r["dst_fill"])):
                        wrong.append(f"{tag}: outputs_by_point {k}: wrote in front of dst_row0")
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_opposite_padding_changes_no_live_bit(case, monkeypatch):
    """(a)-(d) for every step kernel (and init_state, whose state is compared on its own) with pad columns that vote
    "no" in every wave-wide shortcut: snow, water and ice on a frozen profile, snowfall at every index."""
    _pair(case, "opposite", monkeypatch)


@pytest.mark.parametrize("cls", ["nan", "huge", "failing"])
@pytest.mark.parametrize("name", THREE)
def test_nan_huge_and_failing_padding(name, cls, monkeypatch):
    """(a)-(d) with NaN, with +inf (the largest finite value in the state block) and with an air temperature that
    CheckValues rejects in every column that is no live point; `failing`: two live points fail on purpose and the
    count and the indices are exactly theirs."""
    _pair(BY_NAME[name], cls, monkeypatch)


def test_outputs_by_point_reads_live_columns_only(monkeypatch):
    """rs_hip_outputs_by_point from an output window with poisoned pad columns into series of exactly n rows: every
    value where its point's series has it, nothing in front of dst_row0, in the guard bands or in the inputs."""
    _pair(BY_NAME["f64-duo-lean"], "opposite", monkeypatch, by_point=True)


@pytest.mark.parametrize("precision", [64, 32])
def test_expand_reads_live_knot_columns_only(precision):
    """rs_hip_expand_forcing from knots whose pad columns hold poison: the live columns of the window it writes are
    those of the clean build, and nothing else is written: not the window's columns behind n, not its guard bands, not
    the knots."""
    wdt = torch.float32 if precision == 32 else torch.float64
    s = abi.default_settings(ph.SIMLEN); p = abi.default_parameters()
    wrong = []
    for n in ph.SIZES:
        knot_case = Case("knots", precision=precision, variant=DUO, src="knots")
        seed, _, _ = ph.prepare(knot_case, n)
        got = {}
        for cls in (None, "opposite", "nan"):
            plan = device.Plan(n, s, p, 0)
            if precision == 32:
                plan.set_precision(32)
            A = ph.Arena(plan.device, n, plan.np_pad, cls)
            spec, knots = ph.make_knots(plan, A, seed, ph.wave_points(knot_case))
            t = {k: A.carve(k, (ph.SIMLEN, A.stride), wdt, A.fill(k, wdt), role="written")
                 for k in ("tair", "tdew", "vz", "rhz", "prec", "sw", "lw", "tsurfobs")}
            t["depth"] = None
            t["precphase"] = A.carve("precphase", (ph.SIMLEN, A.stride), torch.int32, A.fill("precphase", torch.int32), role="written")
            t["hour"] = A.carve("hour", (ph.SIMLEN,), torch.int32, 12)
            win = device.ForcingWindow(ph.SIMLEN, A.stride, t)
            snap = A.snapshot()
            plan.expand(spec, knots, win, 1, ph.SIMLEN)
            plan.sync()
            got[cls] = {k: v[:, :n].cpu().numpy() for k, v in t.items() if v is not None and k != "hour"}
            got[cls]["hour"] = t["hour"].cpu().numpy()
            if cls:
                for name, where in A.touched(snap, exempt=("hour",)):
                    wrong.append(f"n={n}/{cls}: {name} was written outside the live columns, first elements {where}")
            plan.close()
        for cls in ("opposite", "nan"):
            for k in got[None]:
                if not _same_bits(got[None][k], got[cls][k]):
                    wrong.append(f"n={n}/{cls}: {k} of the expanded window differs in live columns")
        f = oh.synth_forcing(n, ph.SIMLEN, seed=seed)  # the host twin of the generator (the dry spell leaves Tair alone)
        if precision == 64 and not _same_bits(got[None]["tair"].T.copy(), f["tair"]):
            wrong.append(f"n={n}: the expanded air temperature is not the host twin's")
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("mode", ["history", "forecast"])
@pytest.mark.parametrize("precision", [64, 32])
def test_resort_with_poisoned_pad_columns_stays_a_permutation_of_the_live_points(precision, mode):
    """(e): rs_hip_recluster reads the score row of the state block, rs_hip_recluster_forecast the state and knot
    rows of the caller's; both with `opposite` poison behind n (the state's score row holds the largest key).
    Launches of 80, 80 and 81 indices through rs_hip_step_knots, a re-sort after the first two."""
    s = abi.default_settings(ph.SIMLEN); p = abi.default_parameters()
    launches = ((1, 80), (81, 80), (161, 81))
    wdt = torch.float32 if precision == 32 else torch.float64
    wrong, moved = [], 0
    for n in ph.SIZES:
        knot_case = Case("natural", precision=precision, variant=DUO, src="knots")
        seed, _, _ = ph.prepare(knot_case, n)
        natural = ph.run_case(knot_case, n, seed, None)["out"]
        plan = device.Plan(n, s, p, 0)
        plan.set_variant(DUO)
        if precision == 32:
            plan.set_precision(32)
        plan.set_history_score(mode == "history")
        A = ph.Arena(plan.device, n, plan.np_pad, "opposite")
        spec, knots = ph.make_knots(plan, A, seed, ph.wave_points(knot_case))
        t0 = {k: A.rows(k, None, wdt, nrows=1) for k in ("tair", "tdew", "vz", "rhz", "prec", "sw", "lw", "tsurfobs")}
        t0["depth"] = None
        t0["precphase"] = A.rows("precphase", None, torch.int32, nrows=1)
        t0["hour"] = A.carve("hour", (1,), torch.int32, 12)
        win0 = device.ForcingWindow(1, A.stride, t0)
        plan.reset_order()
        plan.expand_ordered(spec, knots, win0, 1, 1)
        tb = plan.uniform_tbottom(2024, 1, 10)
        pp = plan.point_params(A.vec("tbottom", np.full(n, tb), torch.float64))
        out = A.output(ph.SIMLEN, wdt)
        plan.init_state(win0, pp)
        ph.poison_state(plan, n, "opposite", precision == 32)
        snap = A.snapshot()
        got = {k: np.full((n, ph.SIMLEN), np.nan, natural[k].dtype) for k in device.OUT_FIELDS}
        for c, (t, ns) in enumerate(launches):
            plan.step_knots(spec, knots, out, pp, t, ns, out_row0=0)
            plan.sync()
            order = plan.order().cpu().numpy().copy()
            if not np.array_equal(np.sort(order[:n]), np.arange(n)):
                wrong.append(f"n={n} launch {c}: order()[:n] is no permutation of the live points: {order[:n][:8].tolist()}")
                break
            if not np.array_equal(order[n:], np.arange(n, plan.np_pad)):
                wrong.append(f"n={n} launch {c}: order()[n:] is not the identity")
                break
            moved += int((order[:n] != np.arange(n)).sum())
            for k in device.OUT_FIELDS:
                got[k][order[:n], t - 1:t - 1 + ns] = out.tensors[k][t - 1:t - 1 + ns, :n].cpu().numpy().T
            if c + 1 < len(launches):
                if mode == "history":
                    plan.recluster()
                else:
                    k0 = (t + ns - 1) // ph.SPK
                    plan.recluster_forecast([knots[k0, 0], knots[k0 + 1, 0]], [knots[k0, 2], knots[k0 + 1, 2]],
                                            [k0 % 24, (k0 + 1) % 24], knots[k0, 0], 0.5, 1234, point_order=True,
                                            prec_rows=[knots[k0, 4], knots[k0 + 1, 4]])
        else:
            for k in device.OUT_FIELDS:
                if not _same_bits(got[k], natural[k]):
                    wrong.append(f"n={n}: {k} mapped back through the order differs from the natural-order run")
            for name, where in A.touched(snap):
                wrong.append(f"n={n}: {name} was written outside the live columns, first elements {where}")
            if plan.failed_count() != 0:
                wrong.append(f"n={n}: failed_count {plan.failed_count()}")
        plan.close()
    assert not wrong, "\n".join(wrong)
    assert moved > 0  # the re-sorts really moved points
