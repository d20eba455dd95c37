"""GPU: per-point aggregates over output periods reduced from the output rows on the device (rs_hip_outputs_periods)
against their definition, roadsurf_amd/periods.py (reduce_series).  Counts and extremes are selections, the sum is
ordered and the fp64 series equal the reference bit for bit: every comparison here is exact (NaN equal to NaN)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ensemble_helpers as eh
import oracle_helpers as oh
from roadsurf_amd import abi, device, ensemble, lib, periods

pytestmark = pytest.mark.gpu

OUT = device.OUT_FIELDS
TSURF_VALUES = np.array([-2.0, -0.5, 0.0, 0.0, 0.5, 1.5])   # few values, exact in fp32 too: ties and threshold hits
STORAGE_VALUES = np.array([0.0, 0.125, 0.125, 0.75])
TH = (0.0, (0.125, 0.0, 0.125, 0.75, 0.125))
NROWS, INDEX0 = 23, 2
SPEC = periods.PeriodSpec(4, 5, 3, *TH)   # indices 4 .. 18: rows before, rows behind, boundaries inside a call
GUARD, PAD_MARK, GUARD_MARK = 64, 555.0, 777.0


def _kind():
    return "ref" if oh.have_ref() else "port"


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _where(a, b):
    return np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))[:5]


def _made_series(n, nrows, seed, np_dtype):
    """Six series [n, nrows] in point order.  Point 0 holds values whose sum depends on the order of the additions;
    some points have a -9999.0 tail, one is invalid throughout, the last one holds a NaN."""
    rs = np.random.RandomState(seed)
    d = {"tsurf": TSURF_VALUES[rs.randint(0, len(TSURF_VALUES), (n, nrows))]}
    for k in OUT[1:]:
        d[k] = STORAGE_VALUES[rs.randint(0, len(STORAGE_VALUES), (n, nrows))]
    d["tsurf"][0] = np.resize([1e16, 1.0, 1.0, 0.3], nrows)
    for p in range(2, n, 5):
        d["tsurf"][p, rs.randint(0, nrows):] = -9999.0
    if n >= 3:
        d["tsurf"][n // 2] = -9999.0
    d["tsurf"][n - 1, 4] = np.nan
    d["snow"][n - 1, 0] = np.nan
    return {k: np.ascontiguousarray(v.astype(np_dtype)) for k, v in d.items()}


def _plan(n, precision):
    plan = device.Plan(n, abi.default_settings(10), abi.default_parameters(), 0)
    if precision == 32:
        plan.set_precision(32)
    return plan


def _window(plan, d, columns, t_dtype, stride):
    """[nrows][stride]: column s holds point columns[s] where that is a point, rubbish elsewhere and behind n."""
    n = plan.npoints
    nrows = d["tsurf"].shape[1]
    t = {k: torch.full((nrows, stride), 4321.0, dtype=t_dtype, device=plan.device) for k in OUT}
    live = np.flatnonzero((columns[:n] >= 0) & (columns[:n] < n))
    for k in OUT:
        t[k][:, torch.from_numpy(live).to(plan.device)] = torch.from_numpy(np.ascontiguousarray(d[k][columns[live]].T)).to(plan.device)
    return device.OutputWindow(nrows, stride, t)


def _guarded_acc(plan, spec):
    """An accumulator inside a larger buffer: reset - which writes all np_pad columns -, then marks in the columns
    of points >= n; guard values on both sides of the block."""
    n, size = plan.npoints, int(spec.nperiods) * lib.RS_PER_COLS * plan.np_pad
    buf = torch.full((size + 2 * GUARD,), GUARD_MARK, dtype=torch.float64, device=plan.device)
    acc = buf[GUARD:GUARD + size].view(int(spec.nperiods), lib.RS_PER_COLS, plan.np_pad)
    assert plan.periods_reset(spec, acc) is acc
    plan.sync()
    assert _same(acc.permute(2, 0, 1).cpu().numpy(), periods.empty(plan.np_pad, spec))
    assert bool((buf[:GUARD] == GUARD_MARK).all()) and bool((buf[-GUARD:] == GUARD_MARK).all())
    acc[:, :, n:] = PAD_MARK
    return buf, acc


def _guards_untouched(buf, acc, n):
    return (bool((acc[:, :, n:] == PAD_MARK).all()) and bool((buf[:GUARD] == GUARD_MARK).all())
            and bool((buf[-GUARD:] == GUARD_MARK).all()))


def _orders(n, np_pad, rs):
    """(order row, the points it names).  From three points on: a permutation with one entry of -1 and one of
    npoints, whose two points no slot names.  One point: the identity, then the two entries that name nothing."""
    if n < 3:
        rows = [np.arange(np_pad, dtype=np.int32) for _ in range(3)]
        rows[1][0], rows[2][0] = -1, n
        return [(rows[0], np.arange(n)), (rows[1], np.arange(0)), (rows[2], np.arange(0))]
    row = np.arange(np_pad, dtype=np.int32)
    row[:n] = rs.permutation(n)
    a, b = rs.choice(n, 2, replace=False)
    named = np.setdiff1d(np.arange(n), row[[a, b]])
    row[a], row[b] = -1, n
    return [(row, named)]


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [1, 65, 130])
@pytest.mark.parametrize("index_step", [1, 3])
def test_kernel_equals_the_definition_on_made_windows(n, precision, index_step):
    """No model: windows made with torch against reduce_series.  One point, a second partial wavefront, three
    wavefronts; 23 rows from index 2 on, of which the first lie before the periods and the last behind; t_stride
    above npoints_padded; a permuted kept order row with one entry of -1 and one of npoints, which write nothing;
    the plan's own order reads column s as point s; nothing but the named points' columns is written."""
    np_dtype, t_dtype = (np.float32, torch.float32) if precision == 32 else (np.float64, torch.float64)
    plan = _plan(n, precision)
    dev, stride = plan.device, plan.np_pad + 64
    d = _made_series(n, NROWS, 100 * n + index_step, np_dtype)
    index = INDEX0 + index_step * np.arange(NROWS)
    want = periods.reduce_series(*[d[k] for k in OUT], index, SPEC)
    per = periods.period_of(index, SPEC)
    assert (per < 0).any() and per[0] < 0 and per[-1] < 0 and set(per.tolist()) >= {0, 1, 2}
    if n > 1:   # ties, threshold hits, an invalid point and a failed one are there
        assert (want[:, :, periods.COUNT] == 0).all(axis=1).any() and (want[:, :, periods.N_BELOW] > 0).any()
        assert (want[:, 0, periods.COUNT] > 0).any() and (want[:, 2, periods.COUNT] == 0).any()
    assert np.isnan(want[n - 1, :, periods.TSUM]).any()
    for order_np, named in _orders(n, plan.np_pad, np.random.RandomState(n)):
        expect = periods.empty(n, SPEC)
        expect[named] = want[named]
        buf, acc = _guarded_acc(plan, SPEC)
        plan.outputs_periods(_window(plan, d, order_np, t_dtype, stride), NROWS, INDEX0, index_step, SPEC, acc,
                             order=torch.from_numpy(order_np).to(dev))
        plan.sync()
        got = plan.periods(acc, SPEC)
        assert _same(got, expect), (order_np[:4], _where(got, expect))
        assert _guards_untouched(buf, acc, n)
    # the plan's own order row (the identity here), on the plan's stream
    buf, acc = _guarded_acc(plan, SPEC)
    plan.outputs_periods(_window(plan, d, np.arange(plan.np_pad), t_dtype, stride), NROWS, INDEX0, index_step, SPEC, acc)
    plan.sync()
    got = plan.periods(acc, SPEC)
    assert _same(got, want), _where(got, want)
    assert _guards_untouched(buf, acc, n)
    plan.close()


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [1, 65, 130])
def test_rows_cut_into_calls_anywhere_give_the_accumulator_of_one_call(n, precision):
    """The same 23 rows in one call, in 23 calls of one row and in calls of seven rows - periods of five indices span
    calls, calls span periods: three identical accumulators, the ordered sum included, which equal the definition."""
    np_dtype, t_dtype = (np.float32, torch.float32) if precision == 32 else (np.float64, torch.float64)
    plan = _plan(n, precision)
    d = _made_series(n, NROWS, 7 * n, np_dtype)
    index = INDEX0 + np.arange(NROWS)
    want = periods.reduce_series(*[d[k] for k in OUT], index, SPEC)
    rev = periods.reduce_series(*[d[k][:, ::-1] for k in OUT], index[::-1], SPEC)
    assert not _same(rev[0, :, periods.TSUM], want[0, :, periods.TSUM])   # (point 0's sums do depend on the order)
    win = _window(plan, d, np.arange(plan.np_pad), t_dtype, plan.np_pad)
    bufs = []
    for rows_per_call in (NROWS, 1, 7):
        buf, acc = _guarded_acc(plan, SPEC)
        for lo in range(0, NROWS, rows_per_call):
            ns = min(rows_per_call, NROWS - lo)
            plan.outputs_periods(win, ns, INDEX0 + lo, 1, SPEC, acc, row=lo)
        plan.sync()
        got = plan.periods(acc, SPEC)
        assert _same(got, want), (rows_per_call, _where(got, want))
        assert _guards_untouched(buf, acc, n)
        bufs.append(buf.cpu().numpy())
    assert _same(bufs[0], bufs[1]) and _same(bufs[0], bufs[2])
    plan.close()


@pytest.mark.parametrize("precision", [64, 32])
def test_periods_of_one_index_reproduce_the_window(precision):
    """length = 1, nperiods = nrows: every cell is its row."""
    n = 130
    np_dtype, t_dtype = (np.float32, torch.float32) if precision == 32 else (np.float64, torch.float64)
    plan = _plan(n, precision)
    d = _made_series(n, NROWS, 3, np_dtype)
    spec = periods.PeriodSpec(INDEX0, 1, NROWS, *TH)
    acc = plan.periods_reset(spec)
    plan.outputs_periods(_window(plan, d, np.arange(plan.np_pad), t_dtype, plan.np_pad), NROWS, INDEX0, 1, spec, acc)
    got = plan.periods(acc, spec)
    index = INDEX0 + np.arange(NROWS)
    assert _same(got, periods.reduce_series(*[d[k] for k in OUT], index, spec))
    t = d["tsurf"].astype(np.float64)
    ok = t != -9999.0
    assert np.array_equal(got[:, :, periods.COUNT], ok.astype(float))
    assert _same(got[:, :, periods.LAST], t) and _same(got[:, :, periods.TSUM], np.where(ok, t, 0.0))
    assert np.array_equal(got[:, :, periods.LAST_INDEX], np.where(ok, index[None, :], 0))
    fin = ok & ~np.isnan(t)
    assert _same(got[:, :, periods.TMIN], np.where(fin, t, np.inf)) and _same(got[:, :, periods.TMAX], np.where(fin, t, -np.inf))
    for k, name in enumerate(OUT[1:]):
        s = d[name].astype(np.float64)
        assert _same(got[:, :, periods.STORAGE_MAX + k], np.where(ok & ~np.isnan(s), s, -np.inf))
    plan.close()


N_RUN, L_RUN = 300, 601
RUN_SPEC = periods.PeriodSpec(2, 120, 5)   # hourly, ending at the hourly kept rows: indices 2 .. 601
BAD_POINT, BAD_K = 131, 350                # a bad input at the 0-based index 350: index 351 keeps its row, the last


def _run_forcing():
    f = oh.synth_forcing(N_RUN, L_RUN, seed=31)
    f["tair"][BAD_POINT, BAD_K] = 250.0
    s = abi.default_settings(L_RUN); p = abi.default_parameters(); l = abi.default_local(); l.InitLenI = 1
    return f, s, p, l


def test_periods_behind_every_launch_equal_the_reference():
    """300 points x 600 indices in launches of 97 - periods of 120 indices span launches - against reduce_series of
    the reference's series; one point fails mid-run (CheckValues, src/InputOutput.f90:45-84) and its periods stop at
    its failing index."""
    f, s, p, l = _run_forcing()
    ora, _, _ = oh.run_oracle(_kind(), f, s, p, l)
    index = np.arange(1, L_RUN + 1)
    below = float(np.median(ora["tsurf"].min(axis=1)))
    spec = periods.PeriodSpec(RUN_SPEC.first_index, RUN_SPEC.length, RUN_SPEC.nperiods, below, (0.0,) * 5)
    want = periods.reduce_series(*[ora[k] for k in OUT], index, spec)
    nb = want[:, :, periods.N_BELOW]
    assert (nb > 0).any() and (nb == 0).any() and (want[:, :, periods.STORAGE_COUNT:] > 0).any()
    res, nfail = device.run_points(f, s, p, l, chunk=97, periods=spec)
    assert nfail == 1
    got = res["periods"]
    assert got.shape == (N_RUN, 5, periods.RS_PER_COLS)
    assert _same(got, want), _where(got, want)
    assert _same(got, periods.reduce_series(*[res[k] for k in OUT], index, spec))
    # the failed point: index 351 lies in period (351 - 2) // 120 = 2, whose first index is 242
    cells = got[BAD_POINT]
    assert cells[:, periods.COUNT].tolist() == [120, 120, BAD_K + 1 - 242 + 1, 0, 0]
    assert cells[2, periods.LAST_INDEX] == BAD_K + 1 and cells[2, periods.LAST] == ora["tsurf"][BAD_POINT, BAD_K]
    assert _same(cells[3:], periods.empty(1, spec)[0, 3:])
    assert (np.delete(got[:, :, periods.COUNT], BAD_POINT, axis=0) == 120).all()
    assert np.array_equal(np.delete(got[:, :, periods.LAST], BAD_POINT, axis=0),
                          np.delete(ora["tsurf"][:, 120::120], BAD_POINT, axis=0))   # the sample: the hourly kept rows


def test_fp32_plan_cells_equal_the_definition_on_its_own_outputs():
    f, s, p, l = _run_forcing()
    res, nfail = device.run_points(f, s, p, l, chunk=97, precision=32, periods=RUN_SPEC)
    assert nfail == 1
    for k in OUT:   # (the run's outputs are floats, handed back widened)
        assert np.array_equal(res[k], res[k].astype(np.float32).astype(np.float64))
    want = periods.reduce_series(*[res[k] for k in OUT], np.arange(1, L_RUN + 1), RUN_SPEC)
    assert _same(res["periods"], want), _where(res["periods"], want)
    assert res["periods"][BAD_POINT, :, periods.COUNT].tolist() == [120, 120, BAD_K + 1 - 242 + 1, 0, 0]


def test_run_ensemble_periods_equal_the_definition_on_its_own_members(monkeypatch):
    """70 stations x 5 members behind a shared analysis, launches of 60 indices with a re-sort behind every one: the
    accumulator is in point order, so the cells are reduce_series of the member series the same run returned.
    Periods from the members' first index on, the last one partial."""
    c = eh.lean_case()
    B, L = c["B"], c["L"]
    resorted = []
    plain_recluster = device.Plan.recluster

    def counting(self):
        plain_recluster(self)
        resorted.append(bool((self.order()[:self.npoints].cpu() != torch.arange(self.npoints, dtype=torch.int32)).any()))
    monkeypatch.setattr(device.Plan, "recluster", counting)
    spec = periods.PeriodSpec(B + 1, 120, 3, -3.0, (0.0,) * 5)
    assert B + 120 * 2 < L < B + 120 * 3
    res = ensemble.run_ensemble(c["stations"], c["tails"], B, c["settings"], c["params"], c["local"], None,
                                parent=c["parent"], recluster=True, chunk=60, periods=spec)
    assert len(resorted) > 8 and any(resorted)
    mem = res["members"]
    want = periods.reduce_series(*[mem[k] for k in OUT], B + 1 + np.arange(L - B), spec)
    got = res["periods"]
    assert got.shape == (len(c["parent"]), 3, periods.RS_PER_COLS)
    assert _same(got, want), _where(got, want)
    assert (got[:, :2, periods.COUNT] == 120).all() and (got[:, 2, periods.COUNT] == L - B - 240).all()
    assert np.array_equal(got[:, 2, periods.LAST], mem["tsurf"][:, -1])


def test_refusals_leave_the_accumulator_alone():
    """Every refusal of include/roadsurf.h: a status below 0 before any launch, the argument named in rs_last_error,
    the accumulator what it was; run_points refuses periods with coupling before any device work."""
    n = 65
    plan = _plan(n, 64)
    L = lib.load()
    assert L.rs_hip_period_cols() == lib.period_cols() == lib.RS_PER_COLS == periods.RS_PER_COLS == 17
    assert L.rs_hip_period_spec_bytes() == C.sizeof(lib.RsPeriodSpec) == 16 + 48
    d = _made_series(n, NROWS, 5, np.float64)
    win = _window(plan, d, np.arange(plan.np_pad), torch.float64, plan.np_pad)
    buf, acc = _guarded_acc(plan, SPEC)
    plan.outputs_periods(win, NROWS, INDEX0, 1, SPEC, acc)
    plan.sync()
    before = buf.clone()
    sp = lib.period_spec(SPEC)
    o = win.struct_from(0)
    accp = C.c_void_p(acc.data_ptr())

    def refused(rc, *named):
        assert rc < 0
        msg = lib.last_error()
        assert all(w in msg for w in named), msg
        plan.sync()
        assert torch.equal(buf.view(torch.int64), before.view(torch.int64))   # (bits: a cell holds a NaN)

    def feed(plan_=plan._h, src=C.byref(o), nrows=NROWS, index_step=1, spec=C.byref(sp), acc_=accp):
        return L.rs_hip_outputs_periods(plan_, src, nrows, INDEX0, index_step, None, spec, acc_, None)

    def bad(**kw):
        b = lib.period_spec(SPEC)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    refused(feed(plan_=None), "rs_hip_outputs_periods", "plan")
    refused(feed(src=None), "rs_hip_outputs_periods", "src")
    refused(feed(spec=None), "rs_hip_outputs_periods", "spec")
    refused(feed(acc_=None), "rs_hip_outputs_periods", "acc_device")
    refused(feed(nrows=0), "rs_hip_outputs_periods", "nrows")
    refused(feed(nrows=-3), "rs_hip_outputs_periods", "nrows")
    refused(feed(index_step=0), "rs_hip_outputs_periods", "index_step")
    for b, name in ((bad(first_index=0), "first_index"), (bad(length=0), "length"), (bad(nperiods=0), "nperiods"),
                    (bad(length=65536, nperiods=32768), "length * nperiods"), (bad(reserved=7), "reserved")):
        refused(feed(spec=C.byref(b)), "rs_hip_outputs_periods", "spec", name)
        refused(L.rs_hip_periods_reset(plan._h, C.byref(b), accp, None), "rs_hip_periods_reset", "spec", name)
        refused(L.rs_hip_period_check(C.byref(b)), "rs_hip_period_check", "spec", name)
    b = bad()
    b.th.storage_above[2] = float("nan")
    refused(feed(spec=C.byref(b)), "rs_hip_outputs_periods", "spec", "threshold")
    b = bad()
    b.th.tsurf_below = float("inf")
    refused(feed(spec=C.byref(b)), "rs_hip_outputs_periods", "spec", "threshold")
    narrow = win.struct_from(0)
    narrow.t_stride = n - 1
    refused(feed(src=C.byref(narrow)), "rs_hip_outputs_periods", "t_stride")
    hole = win.struct_from(0)
    hole.ice = None
    refused(feed(src=C.byref(hole)), "rs_hip_outputs_periods", "six streams")
    side = torch.cuda.Stream(plan.device)
    refused(L.rs_hip_outputs_periods(plan._h, C.byref(o), NROWS, INDEX0, 1, None, C.byref(sp), accp,
                                     C.c_void_p(side.cuda_stream)), "rs_hip_outputs_periods", "kept one")
    refused(L.rs_hip_periods_reset(None, C.byref(sp), accp, None), "rs_hip_periods_reset", "plan")
    refused(L.rs_hip_periods_reset(plan._h, None, accp, None), "rs_hip_periods_reset", "spec")
    refused(L.rs_hip_periods_reset(plan._h, C.byref(sp), None, None), "rs_hip_periods_reset", "acc_device")
    assert L.rs_hip_period_check(C.byref(sp)) == 0
    with pytest.raises(RuntimeError, match="length"):   # the wrapper checks the spec before it sizes an accumulator
        plan.periods_reset(periods.PeriodSpec(1, 0, 1))
    # rows that belong to no period are a feed of nothing, not a refusal
    assert feed(nrows=2) == 0 and L.rs_hip_outputs_periods(plan._h, C.byref(o), NROWS, 19, 1, None, C.byref(sp), accp, None) == 0
    plan.sync()
    assert torch.equal(buf.view(torch.int64), before.view(torch.int64))   # (bits: a cell holds a NaN)
    plan.close()
    # the runner: not with coupling, whose replays rewrite rows that earlier launches wrote
    f, s, p, l = _run_forcing()
    s.use_coupling = 1
    with pytest.raises(ValueError, match="no periods with coupling"):
        device.run_points(f, s, p, l, chunk=97, periods=RUN_SPEC)
    s.use_coupling = 0
    with pytest.raises(ValueError, match="nperiods"):
        device.run_points(f, s, p, l, chunk=97, periods=periods.PeriodSpec(2, 120, 0))
