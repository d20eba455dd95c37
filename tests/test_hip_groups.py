"""GPU: per-group time series reduced from the output rows on the device (rs_hip_outputs_groups,
rs_driver_run_groups) against their definition, roadsurf_amd/groups.py (reduce_groups).  Every column is a count, a
minimum or a maximum, and the fp64 series equal the reference bit for bit: every comparison here is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import driver_helpers as dh
import oracle_helpers as oh
from roadsurf_amd import abi, device, driver, groups, lib, summary, workload

pytestmark = pytest.mark.gpu

OUT = device.OUT_FIELDS
TSURF_VALUES = np.array([-2.0, -0.5, 0.0, 0.0, 0.5, 1.5])   # few values, exact in fp32 too: ties and threshold hits
STORAGE_VALUES = np.array([0.0, 0.125, 0.125, 0.75])
TH = summary.SummarySpec(0.0, (0.125, 0.0, 0.125, 0.75, 0.125))
EDGES = (-1.0, -0.5, 0.25, 0.5, 1.0)                        # five edges, -0.5 and 0.5 are values of the set
LDS_CELLS = 8192                                            # RS_GRP_LDS_CELLS: the switch between the two kernels


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


def _window(d, columns, n, nrows, stride, t_dtype, dev):
    """[nrows][stride], column s = point columns[s]; the columns behind n hold rubbish that would count."""
    t = {k: torch.full((nrows, stride), -1.0 if k == "tsurf" else 4321.0, dtype=t_dtype, device=dev) for k in OUT}
    for k in OUT:
        t[k][:, :n] = torch.from_numpy(np.ascontiguousarray(d[k][columns[:n]].T)).to(dev)
    return device.OutputWindow(nrows, stride, t)


GUARD, ROWS_BEFORE, ROWS_AFTER = 64, 2, 3


def _guarded_acc(plan, nrows, spec):
    """An accumulator of ROWS_BEFORE + nrows + ROWS_AFTER rows inside a larger buffer: the reset pattern in all of
    its rows, then guard values in the rows the calls must not write, and around the block."""
    rows, cells = ROWS_BEFORE + nrows + ROWS_AFTER, spec.ngroups * groups.cols(spec)
    buf = torch.full((rows * cells + 2 * GUARD,), 777.0, dtype=torch.float64, device=plan.device)
    acc = buf[GUARD:GUARD + rows * cells].view(rows, spec.ngroups, groups.cols(spec))
    plan.groups_reset(rows, spec, acc)
    plan.sync()
    assert np.array_equal(plan.groups(acc, spec), groups.empty(rows, spec))
    acc[:ROWS_BEFORE] = 555.0
    acc[ROWS_BEFORE + nrows:] = 555.0
    return buf, acc


def _result(plan, buf, acc, nrows, spec):
    """The rows the calls were to write, after checking that nothing else was written."""
    got = plan.groups(acc, spec)
    assert (got[:ROWS_BEFORE] == 555.0).all() and (got[ROWS_BEFORE + nrows:] == 555.0).all()
    assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[-GUARD:] == 777.0).all())
    return got[ROWS_BEFORE:ROWS_BEFORE + nrows]


def _group_rows(n, rs):
    """(name, ngroups, ids [n], edges): every point in one group; every point in its own group among n + 7; a few
    groups, a few hundred, and more groups than points at random, with ids of -1 and ids >= ngroups among them."""
    def random(ng):
        g = rs.randint(0, ng, n).astype(np.int32)
        g[rs.rand(n) < 0.1] = -1
        g[rs.rand(n) < 0.1] = ng + rs.randint(0, 3)
        return g
    return [("one group", 1, np.zeros(n, np.int32), ()),
            ("one group, bins", 1, np.zeros(n, np.int32), EDGES),
            ("random of 3, bins", 3, random(3), EDGES),
            ("random of 200", 200, random(200), ()),
            ("random of 200, bins", 200, random(200), EDGES),
            ("own group", n + 7, np.arange(n, dtype=np.int32), ()),
            ("random of n + 7, bins", n + 7, random(n + 7), EDGES)]


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [1, 65, 2500])
def test_kernel_equals_the_definition_on_made_windows(n, precision):
    """No model: windows made with torch against reduce_groups.  One point, a second partial wavefront, ten
    workgroups' worth of slots with a ragged last block; one row, rows that do not divide among the blocks of rows
    (33), more of them (90); 1, 3, 200 and n + 7 groups, which at n = 2500 is the kernel on global cells and
    elsewhere the one with the cells in LDS, 200 groups with bins taking a single row per workgroup; t_stride above
    npoints_padded with rubbish behind the points; a random permutation as a kept order row and the plan's own
    order; the accumulator inside a guarded buffer at acc_row0 = 2; three calls over disjoint row ranges in
    DESCENDING order equal one call; two plans of different n merge into one accumulator."""
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
    identity = np.arange(plan.np_pad)
    paths = set()
    for nrows in (1, 33, 90):
        d = _made_series(n, nrows, 100 * n + nrows, np_dtype)
        win, win_id = _window(d, order_np, n, nrows, stride, t_dtype, dev), _window(d, identity, n, nrows, stride, t_dtype, dev)
        for name, ng, gid_np, edges in _group_rows(n, rs):
            spec = groups.GroupSpec(TH, ng, edges)
            path = lib.group_path(spec)
            assert path == ("lds" if ng * groups.cols(spec) <= LDS_CELLS else "global"), name
            paths.add(path)
            gid = torch.from_numpy(gid_np).to(dev)
            want = groups.reduce_groups(*[d[k] for k in OUT], gid_np, spec)
            buf, acc = _guarded_acc(plan, nrows, spec)
            plan.outputs_groups(win, nrows, gid, spec, acc, ROWS_BEFORE, order=order)
            plan.sync()
            got = _result(plan, buf, acc, nrows, spec)
            assert np.array_equal(got, want), (nrows, name, np.argwhere(got != want)[:5])
            # the plan's own order row (the identity here), on the plan's stream
            buf, acc = _guarded_acc(plan, nrows, spec)
            plan.outputs_groups(win_id, nrows, gid, spec, acc, ROWS_BEFORE)
            plan.sync()
            got = _result(plan, buf, acc, nrows, spec)
            assert np.array_equal(got, want), (nrows, name, "own order", np.argwhere(got != want)[:5])
            if nrows == 33:
                a, b = nrows // 4, nrows // 4 + 1
                buf, acc = _guarded_acc(plan, nrows, spec)
                for lo, hi in ((b, nrows), (a, b), (0, a)):
                    plan.outputs_groups(win, hi - lo, gid, spec, acc, ROWS_BEFORE + lo, order=order, row=lo)
                plan.sync()
                got = _result(plan, buf, acc, nrows, spec)
                assert np.array_equal(got, want), (nrows, name, "three calls", np.argwhere(got != want)[:5])
        # a second plan of another size on the same device merges its points into the same accumulator
        n2 = 37
        plan2 = device.Plan(n2, s, p, 0)
        if precision == 32:
            plan2.set_precision(32)
        d2 = _made_series(n2, nrows, 7 * n + nrows, np_dtype)
        spec = groups.GroupSpec(TH, 3, EDGES)
        g1, g2 = rs.randint(-1, 4, n).astype(np.int32), rs.randint(-1, 4, n2).astype(np.int32)
        want = groups.reduce_groups(*[np.concatenate([d[k], d2[k]]) for k in OUT], np.concatenate([g1, g2]), spec)
        assert np.array_equal(want, groups.merge(groups.reduce_groups(*[d[k] for k in OUT], g1, spec),
                                                 groups.reduce_groups(*[d2[k] for k in OUT], g2, spec)))
        buf, acc = _guarded_acc(plan, nrows, spec)
        plan.outputs_groups(win, nrows, torch.from_numpy(g1).to(dev), spec, acc, ROWS_BEFORE, order=order)
        plan.sync()
        win2 = _window(d2, np.arange(plan2.np_pad), n2, nrows, plan2.np_pad + 64, t_dtype, dev)
        plan2.outputs_groups(win2, nrows, torch.from_numpy(g2).to(dev), spec, acc, ROWS_BEFORE)
        plan2.sync()
        got = _result(plan, buf, acc, nrows, spec)
        assert np.array_equal(got, want), (nrows, "two plans", np.argwhere(got != want)[:5])
        plan2.close()
    assert paths == ({"lds", "global"} if n == 2500 else {"lds"})

    # what the entries refuse
    spec = groups.GroupSpec(TH, 3, EDGES)
    gid = torch.zeros(n, dtype=torch.int32, device=dev)
    acc = plan.groups_reset(4, spec)
    side = torch.cuda.Stream(dev)
    for row0, rows in ((-1, 1), (4, 1), (2, 3)):
        with pytest.raises(RuntimeError, match="acc_rows"):
            plan.outputs_groups(win, rows, gid, spec, acc, row0)
    for bad in (groups.GroupSpec(TH, 0), groups.GroupSpec(TH, -3), groups.GroupSpec(TH, 3, tuple(range(32))),
                groups.GroupSpec(TH, 3, (0.0, 0.0)), groups.GroupSpec(TH, 3, (1.0, 0.5))):
        assert lib.load().rs_hip_group_cols(C.byref(lib.group_spec(bad))) < 0
        assert lib.load().rs_hip_group_path(C.byref(lib.group_spec(bad))) < 0
        bs = lib.group_spec(bad)
        o = win.struct(0)
        assert plan.L.rs_hip_outputs_groups(plan._h, C.byref(o), 1, C.c_void_p(gid.data_ptr()), None, C.byref(bs),
                                            C.c_void_p(acc.data_ptr()), 4, 0, None) != 0
        assert "bad spec" in lib.last_error()
        assert plan.L.rs_hip_group_reset(plan._h, C.c_void_p(acc.data_ptr()), 4, C.byref(bs), None) != 0
    with pytest.raises(RuntimeError, match="kept one"):
        plan.outputs_groups(win, 1, gid, spec, acc, 0, stream=side)
    with pytest.raises(RuntimeError, match="t_stride"):
        plan.outputs_groups(device.OutputWindow(1, max(n - 1, 0), win.tensors), 1, gid, spec, acc, 0)
    plan.sync()
    assert np.array_equal(plan.groups(acc, spec), groups.empty(4, spec))     # a refused call writes nothing
    assert lib.group_cols(spec) == groups.cols(spec) == lib.RS_GRP_COLS + 6
    assert lib.group_cols(groups.GroupSpec(TH, 3)) == groups.RS_GRP_COLS == lib.RS_GRP_COLS
    plan.close()


GROUP_BOUNDS = (0, 10, 30, 70, 120, 180, 250, 300)   # seven groups of unequal size over 300 points


def _group_ids(n, rs=None):
    gid = np.empty(n, np.int32)
    for g in range(len(GROUP_BOUNDS) - 1):
        gid[GROUP_BOUNDS[g]:GROUP_BOUNDS[g + 1]] = g
    return gid if rs is None else gid[rs.permutation(n)]


def _partly_below(cells):
    """(row, group) cells whose below-threshold count is strictly between 0 and the cell's valid count"""
    return (cells[:, :, groups.N_BELOW] > 0) & (cells[:, :, groups.N_BELOW] < cells[:, :, groups.COUNT])


def _pick_workload(n, hours):
    """Seed, Tsurf threshold and edges from the oracle's series alone: a threshold that splits a good part of the
    (row, group) cells, storages that are there, and edges that spread a cell over several bins."""
    L = hours * 120 + 1
    s = abi.default_settings(L); p = abi.default_parameters(); l = abi.default_local(); l.InitLenI = 1
    for seed in (3, 99, 7, 31, 1234):
        f = oh.synth_forcing(n, L, seed=seed)
        ora, _, _ = oh.run_oracle(_kind(), f, s, p, l)
        gid = _group_ids(n, np.random.RandomState(seed))
        edges = tuple(float(x) for x in np.unique(np.quantile(ora["tsurf"], (0.1, 0.3, 0.5, 0.7, 0.9))))
        if len(edges) != 5:
            continue
        spec = groups.GroupSpec(summary.SummarySpec(float(np.median(ora["tsurf"])), (0.0,) * 5), 7, edges)
        want = groups.reduce_groups(*[ora[k] for k in OUT], gid, spec)
        if (_partly_below(want).sum() * 10 >= want.shape[0] * want.shape[1]
                and (want[:, :, groups.STORAGE_COUNT:groups.STORAGE_COUNT + 5] > 0).any()
                and ((want[:, :, groups.BINS:] > 0).sum(axis=2) >= 3).any()):
            return seed, s, p, spec, gid, want
    raise AssertionError("no candidate seed gives a workload that exercises the group series")


def test_groups_behind_every_launch_equal_the_reference():
    """300 points x 6 h in plan order with forecast re-sorts, launches of 90 indices, seven groups of unequal size
    dealt over the points, five edges: the group series accumulated behind every launch - through the kept order
    row and through the plan's own in turn - equal reduce_groups of the reference's series."""
    n, hours, chunk = 300, 6, 90
    seed, s, p, spec, gid_np, want = _pick_workload(n, hours)
    # (the conditions that keep the comparison from passing vacuously, on the oracle's result)
    assert _partly_below(want).sum() * 10 >= want.shape[0] * want.shape[1]
    assert (want[:, :, groups.STORAGE_COUNT:groups.STORAGE_COUNT + 5] > 0).any()
    assert ((want[:, :, groups.BINS:] > 0).sum(axis=2) >= 3).any()
    assert lib.group_path(spec) == "lds"
    plan = device.Plan(n, s, p, 0)
    run = workload.SyntheticRun(plan, seed, hours, chunk, plan_order=True, forecast=True)
    gid = torch.from_numpy(gid_np).to(plan.device)
    acc = plan.groups_reset(want.shape[0], spec)
    calls = []

    def on_launch(c, t0, ns):
        plan.outputs_groups(run.out, ns, gid, spec, acc, t0 - 1, order=run.orders[c] if c % 2 else None)
        calls.append(c)
    run.run_pass(on_launch)
    plan.sync()
    assert len(calls) > 3 and bool((run.orders[-1][:n].cpu() != torch.arange(n, dtype=torch.int32)).any())
    got = plan.groups(acc, spec)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    plan.close()


@pytest.mark.parametrize("chunk", [0, 97])
def test_a_failed_point_leaves_its_group_at_the_row_behind_its_failing_index(chunk):
    """A bad input at 0-based index k (CheckValues, src/InputOutput.f90:45-84): the failing index keeps its row,
    the rows behind it read -9999.0 - from row k + 1 on the point's group has exactly one valid point less than in
    the run without the bad value, up to row k the same number, and the other groups' series are the clean run's."""
    n, L = 300, 721
    f = oh.synth_forcing(n, L, seed=31)
    s = abi.default_settings(L); p = abi.default_parameters(); l = abi.default_local(); l.InitLenI = 1
    clean, _, _ = oh.run_oracle(_kind(), f, s, p, l)
    bad = {131: 350, 5: 96, 70: 97, 0: 0}
    for pt, k in bad.items():
        f["tair"][pt, k] = 250.0
    ora, _, _ = oh.run_oracle(_kind(), f, s, p, l)
    gid = _group_ids(n)          # contiguous: points 0 and 5 in group 0, 70 in group 3, 131 in group 4
    assert [int(gid[pt]) for pt in bad] == [4, 0, 3, 0]
    edges = tuple(float(x) for x in np.quantile(clean["tsurf"], (0.1, 0.3, 0.5, 0.7, 0.9)))
    spec = groups.GroupSpec(summary.SummarySpec(float(np.median(clean["tsurf"])), (0.0,) * 5), 7, edges)
    res, nfail = device.run_points(f, s, p, l, chunk=chunk, groups=(spec, gid))
    assert nfail == len(bad)
    got = res["groups"]
    want = groups.reduce_groups(*[ora[k] for k in OUT], gid, spec)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    want_clean = groups.reduce_groups(*[clean[k] for k in OUT], gid, spec)
    rows = np.arange(L)
    for g in range(7):
        lost = sum((rows > k).astype(np.float64) for pt, k in bad.items() if gid[pt] == g)
        assert np.array_equal(got[:, g, groups.COUNT], want_clean[:, g, groups.COUNT] - lost), g
        if g not in (0, 3, 4):
            assert np.array_equal(got[:, g], want_clean[:, g]), g
    assert (got[351:, 4, groups.COUNT] == 59).all() and (got[:351, 4, groups.COUNT] == 60).all()


def test_driver_groups(monkeypatch):
    """rs_driver_run_groups on the driver tests' small scenario (stations that read_input rejects included) over the
    forecast part of the kept rows, four groups: equals reduce_groups of the series the same call returned and of the
    checker's, rejected stations count nowhere, the identical result comes back with no series asked for, together
    with the summaries, in two tiles and from the fan-out, and asking for it changes neither the series nor how the
    call stepped."""
    n = 150
    src, L, t0, tf = dh.scenario(n, hours=12, seed=23)
    s = abi.default_settings(L); s.outputStep = 20; s.use_relaxation = 1
    p = abi.default_parameters()
    step, n_out = driver.output_rows(s)
    first, last = driver.forecast_rows(s, t0, tf)
    assert (first, last) == (18, n_out - 1) and step == 40
    ora = dh.oracle_run(_kind(), src, s, p, t0, tf)
    ok = ora["status"] == 0
    assert 0 < int((~ok).sum()) < n // 4
    gid = np.random.RandomState(4).randint(0, 4, n).astype(np.int32)
    valid = ora["tsurf"][ok][:, first:]
    edges = tuple(float(x) for x in np.quantile(valid, (0.1, 0.3, 0.5, 0.7, 0.9)))
    th = summary.SummarySpec(float(np.median(valid)), (0.0,) * 5)
    spec = groups.GroupSpec(th, 4, edges)
    want = groups.reduce_groups(*[ora[k][:, first:] for k in OUT], gid, spec)
    assert _partly_below(want).sum() * 10 >= want.shape[0] * 4
    assert (want[:, :, groups.STORAGE_COUNT:groups.STORAGE_COUNT + 5] > 0).any()
    # rejected stations count nowhere: every cell counts its group's accepted stations, and some group has a rejected one
    per_group = np.array([int((ok & (gid == g)).sum()) for g in range(4)], np.float64)
    assert (want[:, :, groups.COUNT] == per_group[None, :]).all()
    assert (per_group < np.array([(gid == g).sum() for g in range(4)])).any()

    L_ = driver._bind(lib.load())
    plain = driver.run(src, s, p, t0, tf)
    how_plain = (L_.rs_driver_last_tiles(), L_.rs_driver_last_raw_launches())
    both = driver.run(src, s, p, t0, tf, groups=spec, group_of=gid, group_rows=(first, last))
    assert (L_.rs_driver_last_tiles(), L_.rs_driver_last_raw_launches()) == how_plain
    for k in OUT:
        assert np.array_equal(both[k], plain[k]) and np.array_equal(both[k], ora[k]), k
    assert np.array_equal(both["status"], ora["status"])
    got = both["groups"]
    assert got.shape == (n_out - first, 4, groups.cols(spec))
    assert np.array_equal(got, groups.reduce_groups(*[both[k][:, first:] for k in OUT], gid, spec))
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]

    only = driver.run(src, s, p, t0, tf, groups=spec, group_of=gid, group_rows=(first, last), series=False)
    assert (L_.rs_driver_last_tiles(), L_.rs_driver_last_raw_launches()) == how_plain
    assert "tsurf" not in only and np.array_equal(only["groups"], got) and np.array_equal(only["status"], ora["status"])

    with_sum = driver.run(src, s, p, t0, tf, groups=spec, group_of=gid, group_rows=(first, last), series=False,
                          summary=th, summary_rows=(first, last))
    assert np.array_equal(with_sum["groups"], got)
    alone = driver.run(src, s, p, t0, tf, series=False, summary=th, summary_rows=(first, last))
    assert np.array_equal(with_sum["summary"], alone["summary"])

    fan = driver.run(src, s, p, t0, tf, groups=spec, group_of=gid, group_rows=(first, last), series=False, device=-1)
    assert np.array_equal(fan["groups"], got)

    monkeypatch.setenv("ROADSURF_HIP_TILE_POINTS", "100")
    tiled = driver.run(src, s, p, t0, tf, groups=spec, group_of=gid, group_rows=(first, last), series=False)
    assert L_.rs_driver_last_tiles() == 2
    assert np.array_equal(tiled["groups"], got)
    monkeypatch.delenv("ROADSURF_HIP_TILE_POINTS")

    # rows outside n_out, no array to write to, no group row
    with pytest.raises(RuntimeError, match="first_row"):
        driver.run(src, s, p, t0, tf, groups=spec, group_of=gid, group_rows=(first, n_out))
    inp, keep = driver.make_input(src, t0, tf, driver.calendar(t0, L, int(s.DTSecs)))
    out = driver.RsDriverOutput(); out.n_out = n_out
    st = np.empty(n, np.int32); mi = np.empty(n, np.int32)
    out.status = st.ctypes.data_as(abi.c_int32_p); out.missing_index = mi.ctypes.data_as(abi.c_int32_p)
    series = np.empty((1, 4, groups.cols(spec)))
    for group_p, series_p in ((gid.ctypes.data_as(abi.c_int32_p), None), (None, series.ctypes.data_as(abi.c_double_p))):
        q = driver.RsDriverGroups(lib.group_spec(spec), group_p, 0, 0, series_p)
        assert L_.rs_driver_run_groups(C.byref(inp), C.byref(s), C.byref(p), driver._locals(n, None), C.byref(out),
                                       None, C.byref(q), 0) != 0
        assert "required" in lib.last_error()
