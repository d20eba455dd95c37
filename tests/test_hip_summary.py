"""GPU: per-point forecast summaries reduced from the output rows on the device (rs_hip_outputs_summary,
rs_driver_run_summary) against their definition, roadsurf_amd/summary.py (reduce_series).  Summaries are selections
and counts, and the fp64 series equal the reference bit for bit: every comparison here is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import driver_helpers as dh
import oracle_helpers as oh
from roadsurf_amd import abi, device, driver, lib, summary, workload

pytestmark = pytest.mark.gpu

OUT = device.OUT_FIELDS
TSURF_VALUES = np.array([-2.0, -0.5, 0.0, 0.0, 0.5, 1.5])   # few values, exact in fp32 too: ties and threshold hits
STORAGE_VALUES = np.array([0.0, 0.125, 0.125, 0.75])
SPEC = summary.SummarySpec(0.0, (0.125, 0.0, 0.125, 0.75, 0.125))
INDEX0, INDEX_STEP = 7, 120


def _kind():
    return "ref" if oh.have_ref() else "port"


def _made_series(n, nrows, seed, np_dtype):
    """Six series [n, nrows] in point order: some points with a -9999.0 tail, one all invalid, one NaN."""
    rs = np.random.RandomState(seed)
    d = {"tsurf": TSURF_VALUES[rs.randint(0, len(TSURF_VALUES), (n, nrows))]}
    for k in OUT[1:]:
        d[k] = STORAGE_VALUES[rs.randint(0, len(STORAGE_VALUES), (n, nrows))]
    for p in range(0, n, 5):
        d["tsurf"][p, rs.randint(0, nrows):] = -9999.0
    if n >= 3:
        d["tsurf"][n // 2] = -9999.0
    d["tsurf"][n - 1, nrows // 2] = np.nan
    d["snow"][n - 1, 0] = np.nan
    return {k: np.ascontiguousarray(v.astype(np_dtype)) for k, v in d.items()}


def _guarded_acc(plan, n):
    """An accumulator inside a larger buffer: the reset pattern in the plan's columns, guard values in the
    columns of points >= n and around the block."""
    g = 64
    buf = torch.full((lib.RS_SUM_COLS * plan.np_pad + 2 * g,), 777.0, dtype=torch.float64, device=plan.device)
    acc = buf[g:g + lib.RS_SUM_COLS * plan.np_pad].view(lib.RS_SUM_COLS, plan.np_pad)
    plan.summary_reset(acc)
    plan.sync()
    assert np.array_equal(acc.T.cpu().numpy(), summary.empty(plan.np_pad))
    acc[:, n:] = 555.0
    return buf, acc, g


def _guards_untouched(buf, acc, g, n):
    return bool((acc[:, n:] == 555.0).all()) and bool((buf[:g] == 777.0).all()) and bool((buf[-g:] == 777.0).all())


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [1, 65, 2500])
def test_kernel_equals_the_definition_on_made_windows(n, precision):
    """No model: windows made with torch against reduce_series.  One point, a second partial wavefront, forty
    workgroups with a ragged last one; one row, rows that do not divide among a workgroup's wavefronts or its
    batches of rows in flight (33), more of them (90); t_stride above npoints_padded; a random permutation as a
    kept order row; three calls over disjoint row ranges in DESCENDING order equal one call; the plan's own
    order (NULL) reads column s as point s; nothing but the n points' columns is written."""
    np_dtype, t_dtype = (np.float32, torch.float32) if precision == 32 else (np.float64, torch.float64)
    s = abi.default_settings(10); p = abi.default_parameters()
    plan = device.Plan(n, s, p, 0)
    if precision == 32:
        plan.set_precision(32)
    dev, stride = plan.device, plan.np_pad + 64
    rs = np.random.RandomState(n)
    order_np = np.arange(plan.np_pad, dtype=np.int32)
    order_np[:n] = rs.permutation(n)
    order = torch.from_numpy(order_np).to(dev)
    for nrows in (1, 33, 90):
        d = _made_series(n, nrows, 100 * n + nrows, np_dtype)
        index = INDEX0 + INDEX_STEP * np.arange(nrows)
        want = summary.reduce_series(*[d[k] for k in OUT], index, SPEC)
        assert nrows == 1 or n == 1 or ((want[:, summary.FIRST_BELOW] > 0).any() and (want[:, summary.N_BELOW] == 0).any())

        def window(columns):  # [nrows][stride], column s = point columns[s]; the columns behind n hold rubbish
            t = {k: torch.full((nrows, stride), 4321.0, dtype=t_dtype, device=dev) for k in OUT}
            for k in OUT:
                t[k][:, :n] = torch.from_numpy(np.ascontiguousarray(d[k][columns[:n]].T)).to(dev)
            return device.OutputWindow(nrows, stride, t)
        win = window(order_np)
        buf, acc, g = _guarded_acc(plan, n)
        plan.outputs_summary(win, nrows, INDEX0, INDEX_STEP, SPEC, acc, order=order)
        plan.sync()
        got = plan.summary(acc)
        assert np.array_equal(got, want), (nrows, np.argwhere(got != want)[:5])
        assert _guards_untouched(buf, acc, g, n)
        if nrows >= 3:
            a, b = nrows // 4, nrows // 4 + 1
            buf, acc, g = _guarded_acc(plan, n)
            for lo, hi in ((b, nrows), (a, b), (0, a)):
                if hi > lo:
                    plan.outputs_summary(win, hi - lo, INDEX0 + INDEX_STEP * lo, INDEX_STEP, SPEC, acc, order=order, row=lo)
            plan.sync()
            got = plan.summary(acc)
            assert np.array_equal(got, want), (nrows, "three calls", np.argwhere(got != want)[:5])
            assert _guards_untouched(buf, acc, g, n)
        # the plan's own order row (the identity here), on the plan's stream
        buf, acc, g = _guarded_acc(plan, n)
        plan.outputs_summary(window(np.arange(plan.np_pad)), nrows, INDEX0, INDEX_STEP, SPEC, acc)
        plan.sync()
        assert np.array_equal(plan.summary(acc), want) and _guards_untouched(buf, acc, g, n)
    # what the entry refuses
    acc = plan.summary_reset()
    side = torch.cuda.Stream(dev)
    with pytest.raises(RuntimeError, match="kept one"):
        plan.outputs_summary(win, 1, 1, 1, SPEC, acc, stream=side)
    with pytest.raises(RuntimeError, match="t_stride"):
        plan.outputs_summary(device.OutputWindow(1, max(n - 1, 0), win.tensors), 1, 1, 1, SPEC, acc)
    with pytest.raises(RuntimeError, match="bad arguments"):
        plan.outputs_summary(win, 1, 0, 1, SPEC, acc)
    plan.sync()
    assert lib.load().rs_hip_summary_cols() == summary.RS_SUM_COLS == lib.RS_SUM_COLS
    plan.close()


def _pick_workload(n, hours):
    """Seed and Tsurf threshold from the oracle's series alone: a threshold that a good part of the points cross
    and a good part never do, and storages that are there."""
    L = hours * 120 + 1
    s = abi.default_settings(L); p = abi.default_parameters(); l = abi.default_local(); l.InitLenI = 1
    index = np.arange(1, L + 1)
    for seed in (3, 99, 7, 31, 1234):
        f = oh.synth_forcing(n, L, seed=seed)
        ora, _, _ = oh.run_oracle(_kind(), f, s, p, l)
        below = float(np.median(ora["tsurf"].min(axis=1)))
        spec = summary.SummarySpec(below, (0.0, 0.0, 0.0, 0.0, 0.0))
        want = summary.reduce_series(*[ora[k] for k in OUT], index, spec)
        crossed = int((want[:, summary.FIRST_BELOW] > 0).sum())
        if crossed >= n // 10 and n - crossed >= n // 10 and want[:, summary.STORAGE_COUNT:].any():
            return seed, s, p, spec, want
    raise AssertionError("no candidate seed gives a workload that exercises the summaries")


def test_summaries_behind_every_launch_equal_the_reference():
    """300 points x 6 h in plan order with forecast re-sorts, launches of 90 indices: the summary accumulated
    behind every launch - through the kept order row and through the plan's own in turn - equals reduce_series of the
    reference's series."""
    n, hours, chunk = 300, 6, 90
    seed, s, p, spec, want = _pick_workload(n, hours)
    # (the conditions that keep the comparison from passing vacuously, on the oracle's result)
    crossed = int((want[:, summary.FIRST_BELOW] > 0).sum())
    assert crossed >= n // 10 and n - crossed >= n // 10
    assert (want[:, summary.STORAGE_COUNT:] > 0).any()
    plan = device.Plan(n, s, p, 0)
    run = workload.SyntheticRun(plan, seed, hours, chunk, plan_order=True, forecast=True)
    acc = plan.summary_reset()
    calls = []

    def on_launch(c, t0, ns):
        plan.outputs_summary(run.out, ns, t0, 1, spec, acc, order=run.orders[c] if c % 2 else None)
        calls.append(c)
    run.run_pass(on_launch)
    plan.sync()
    assert len(calls) > 3 and bool((run.orders[-1][:n].cpu() != torch.arange(n, dtype=torch.int32)).any())
    got = plan.summary(acc)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    plan.close()


@pytest.mark.parametrize("chunk", [0, 97])
def test_a_failed_point_is_summarised_up_to_its_failing_index(chunk):
    """A bad input at 0-based index k (CheckValues, src/InputOutput.f90:45-84): the failing index keeps its row,
    the rows behind it read -9999.0 - the point's count is k + 1, its extremes come from those rows only, and
    its neighbours' summaries are those of the run without the bad value."""
    n, L = 300, 721
    f = oh.synth_forcing(n, L, seed=31)
    s = abi.default_settings(L); p = abi.default_parameters(); l = abi.default_local(); l.InitLenI = 1
    clean, _, _ = oh.run_oracle(_kind(), f, s, p, l)
    bad = {131: 350, 5: 96, 70: 97, 0: 0}
    for pt, k in bad.items():
        f["tair"][pt, k] = 250.0
    ora, _, _ = oh.run_oracle(_kind(), f, s, p, l)
    spec = summary.SummarySpec(float(np.median(clean["tsurf"].min(axis=1))), (0.0,) * 5)
    index = np.arange(1, L + 1)
    res, nfail = device.run_points(f, s, p, l, chunk=chunk, summary=spec)
    assert nfail == len(bad)
    got = res["summary"]
    want = summary.reduce_series(*[ora[k] for k in OUT], index, spec)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    want_clean = summary.reduce_series(*[clean[k] for k in OUT], index, spec)
    for pt, k in bad.items():
        assert got[pt, summary.COUNT] == k + 1
        head = summary.reduce_series(*[ora[q][pt:pt + 1, :k + 1] for q in OUT], index[:k + 1], spec)
        assert np.array_equal(got[pt:pt + 1], head)
        assert got[pt, summary.TMIN_INDEX] <= k + 1 and got[pt, summary.TMAX_INDEX] <= k + 1
        for nb in (pt - 1, pt + 1):
            if 0 <= nb < n and nb not in bad:
                assert np.array_equal(got[nb], want_clean[nb]) and got[nb, summary.COUNT] == L


def test_driver_summaries(monkeypatch):
    """rs_driver_run_summary on the driver tests' small scenario (stations that read_input rejects included) over the
    forecast part of the kept rows: equals reduce_series of the series the same call returned and of the checker's,
    rejected stations are empty, the identical summary comes back with no series asked for, in two tiles and
    from the fan-out, and asking for it changes neither the series nor how the call stepped."""
    n = 150
    src, L, t0, tf = dh.scenario(n, hours=12, seed=23)
    s = abi.default_settings(L); s.outputStep = 20; s.use_relaxation = 1
    p = abi.default_parameters()
    step, n_out = driver.output_rows(s)
    first, last = driver.forecast_rows(s, t0, tf)
    assert (first, last) == (18, n_out - 1) and step == 40
    index = np.arange(first, n_out) * step + 1
    ora = dh.oracle_run(_kind(), src, s, p, t0, tf)
    ok = ora["status"] == 0
    assert 0 < int((~ok).sum()) < n // 4
    spec = summary.SummarySpec(float(np.median(ora["tsurf"][ok][:, first:].min(axis=1))), (0.0,) * 5)
    want = summary.reduce_series(*[ora[k][:, first:] for k in OUT], index, spec)
    crossed = int((want[ok, summary.FIRST_BELOW] > 0).sum())
    assert crossed >= n // 10 and int(ok.sum()) - crossed >= n // 10 and (want[:, summary.STORAGE_COUNT:] > 0).any()

    L_ = driver._bind(lib.load())
    plain = driver.run(src, s, p, t0, tf)
    how_plain = (L_.rs_driver_last_tiles(), L_.rs_driver_last_raw_launches())
    both = driver.run(src, s, p, t0, tf, summary=spec, summary_rows=(first, last))
    assert (L_.rs_driver_last_tiles(), L_.rs_driver_last_raw_launches()) == how_plain
    for k in OUT:
        assert np.array_equal(both[k], plain[k]) and np.array_equal(both[k], ora[k]), k
    assert np.array_equal(both["status"], ora["status"])
    got = both["summary"]
    assert np.array_equal(got, summary.reduce_series(*[both[k][:, first:] for k in OUT], index, spec))
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(got[~ok], summary.empty(int((~ok).sum()))) and (got[ok, summary.COUNT] == n_out - first).all()

    only = driver.run(src, s, p, t0, tf, summary=spec, summary_rows=(first, last), series=False)
    assert (L_.rs_driver_last_tiles(), L_.rs_driver_last_raw_launches()) == how_plain
    assert "tsurf" not in only and np.array_equal(only["summary"], got) and np.array_equal(only["status"], ora["status"])

    fan = driver.run(src, s, p, t0, tf, summary=spec, summary_rows=(first, last), series=False, device=-1)
    assert np.array_equal(fan["summary"], got)

    monkeypatch.setenv("ROADSURF_HIP_TILE_POINTS", "100")
    tiled = driver.run(src, s, p, t0, tf, summary=spec, summary_rows=(first, last), series=False)
    assert L_.rs_driver_last_tiles() == 2
    assert np.array_equal(tiled["summary"], got)
    monkeypatch.delenv("ROADSURF_HIP_TILE_POINTS")

    # rows outside n_out, or no array to write to
    with pytest.raises(RuntimeError, match="first_row"):
        driver.run(src, s, p, t0, tf, summary=spec, summary_rows=(first, n_out))
    q = driver.RsDriverSummary(lib.summary_spec(spec), 0, 0, None)
    inp, keep = driver.make_input(src, t0, tf, driver.calendar(t0, L, int(s.DTSecs)))
    out = driver.RsDriverOutput(); out.n_out = n_out
    st = np.empty(n, np.int32); mi = np.empty(n, np.int32)
    out.status = st.ctypes.data_as(abi.c_int32_p); out.missing_index = mi.ctypes.data_as(abi.c_int32_p)
    assert L_.rs_driver_run_summary(C.byref(inp), C.byref(s), C.byref(p), driver._locals(n, None), C.byref(out),
                                    C.byref(q), 0) != 0
