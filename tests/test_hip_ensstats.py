"""GPU: per-station ensemble statistics reduced from the member rows on the device (rs_hip_outputs_ens) against
their definition, roadsurf_amd/ensstats.py (reduce_members).  The kernel visits a station's members in the table's
order and rounds every operation on its own, as the definition does: every comparison here is
np.array_equal(..., equal_nan=True), no tolerance (-0.0 equals 0.0: which zero lands at which rank of the sort is not
part of the contract)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ensemble_helpers as eh
import oracle_helpers as oh
from roadsurf_amd import abi, device, ensemble, ensstats, lib

pytestmark = pytest.mark.gpu

OUT = device.OUT_FIELDS
QUANT = (0.0, 0.1, 0.5, 0.9, 1.0)
TSURF_VALUES = np.array([-2.0, -0.5, 0.0, 0.0, 0.5, 1.5])   # few values, exact in fp32 too: ties in the sort
STORAGE_VALUES = np.array([0.0, 0.125, 0.125, 0.75])
GUARD, ROWS_BEFORE, ROWS_AFTER = 64, 2, 3


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _where(got, want):
    return np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]


def _made_series(n, nrows, seed, np_dtype, kind):
    """Six series [n, nrows] in point order.  "set": a few values exact in fp32, so that sorts see ties; "normal":
    values whose sums and interpolations really round.  Both: some points with a -9999.0 tail, one all invalid, a NaN
    Tsurf and a NaN snow."""
    rs = np.random.RandomState(seed)
    if kind == "set":
        d = {"tsurf": TSURF_VALUES[rs.randint(0, len(TSURF_VALUES), (n, nrows))]}
        for k in OUT[1:]:
            d[k] = STORAGE_VALUES[rs.randint(0, len(STORAGE_VALUES), (n, nrows))]
    else:
        d = {"tsurf": rs.normal(-1.0, 3.0, (n, nrows))}
        for k in OUT[1:]:
            d[k] = np.abs(rs.normal(0.0, 0.4, (n, nrows)))
    for p in range(0, n, 5):
        d["tsurf"][p, rs.randint(0, nrows):] = -9999.0
    if n >= 3:
        d["tsurf"][n // 2] = -9999.0
    d["tsurf"][n - 1, nrows // 2] = np.nan
    d["snow"][n - 1, 0] = np.nan
    if n >= 7:
        d["snow"][n - 4, nrows - 1] = np.nan        # ... and one of a member that is used
    return {k: np.ascontiguousarray(v.astype(np_dtype)) for k, v in d.items()}


def _window(d, columns, n, nrows, stride, t_dtype, dev):
    """[nrows][stride] inside guarded buffers, column s = point columns[s]; the columns behind n hold rubbish that
    would count.  Returns the window and its buffers."""
    bufs, t = {}, {}
    for k in OUT:
        bufs[k] = torch.full((nrows * stride + 2 * GUARD,), 31337.0, dtype=t_dtype, device=dev)
        t[k] = bufs[k][GUARD:GUARD + nrows * stride].view(nrows, stride)
        t[k][:] = -1.0 if k == "tsurf" else 4321.0
        t[k][:, :n] = torch.from_numpy(np.ascontiguousarray(d[k][columns[:n]].T)).to(dev)
    return device.OutputWindow(nrows, stride, t), bufs


def _guarded_acc(plan, nrows, spec):
    """An accumulator of ROWS_BEFORE + nrows + ROWS_AFTER rows inside a larger buffer; there is no reset - a call
    writes every cell of its rows - so every cell starts as a value no cell can take."""
    rows, cells = ROWS_BEFORE + nrows + ROWS_AFTER, spec.ngroups * ensstats.cols(spec)
    buf = torch.full((rows * cells + 2 * GUARD,), 777.0, dtype=torch.float64, device=plan.device)
    acc = buf[GUARD:GUARD + rows * cells].view(rows, spec.ngroups, ensstats.cols(spec))
    acc[:] = 555.0
    return buf, acc


def _result(plan, buf, acc, nrows, spec):
    """The rows the calls were to write, after checking that nothing else was written."""
    got = plan.ens(acc, spec)
    assert (got[:ROWS_BEFORE] == 555.0).all() and (got[ROWS_BEFORE + nrows:] == 555.0).all()
    assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[-GUARD:] == 777.0).all())
    return got[ROWS_BEFORE:ROWS_BEFORE + nrows]


def _layouts(S, M, rs):
    """(name, ids [S * M], spec): the members of a station side by side; far apart, with a last station that has no
    member and room for more members than any station has; the same with ids of -1 and ids >= ngroups, no quantiles."""
    n = S * M
    irregular = ((np.arange(n) * 37 + 11) % S).astype(np.int32)
    outside = irregular.copy()
    outside[rs.rand(n) < 0.1] = -1
    outside[rs.rand(n) < 0.1] = S + 1 + rs.randint(0, 3)
    most = int(np.bincount(irregular).max())
    return [("parents", ensemble.parents(S, M), ensstats.EnsSpec(S, M, QUANT)),
            ("irregular", irregular, ensstats.EnsSpec(S + 1, min(64, most + 3), QUANT)),
            ("ids outside", outside, ensstats.EnsSpec(S + 1, most, ()))]


@pytest.mark.parametrize("precision", [64, 32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("S,M", [(1, 1), (13, 5), (65, 20), (3, 64)], ids=["n1", "n65", "n1300", "n192"])
def test_kernel_equals_the_definition_on_made_windows(S, M, precision):
    """No model: windows made with torch against reduce_members.  One point; 13 stations x 5, a second partial
    wavefront of slots; 65 x 20, a second, ragged block of stations; 3 x 64, the largest segment and the LDS maximum
    with one wavefront of rows per workgroup.  1, 5 and 33 rows (5 and 33 do not divide among the wavefronts); values
    from a small set and normal ones; three group layouts; a random permutation as a kept order row on a stream of the
    caller's with a work row of its own, and the plan's own order; t_stride above npoints_padded with rubbish behind
    the points; the accumulator inside a guarded buffer at acc_row0 = 2; three calls over disjoint row ranges equal
    one call."""
    n = S * M
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
    side = torch.cuda.Stream(dev)
    work_side = torch.empty(plan.np_pad, dtype=torch.int32, device=dev)
    layouts = _layouts(S, M, rs)
    for nrows in (1, 5, 33):
        for kind in ("set", "normal"):
            d = _made_series(n, nrows, 100 * n + nrows, np_dtype, kind)
            (win, wbufs), (win_id, _) = (_window(d, c, n, nrows, stride, t_dtype, dev) for c in (order_np, identity))
            for name, gid, spec in layouts:
                tag = (nrows, kind, name)
                want = ensstats.reduce_members(*[d[k] for k in OUT], gid, spec)
                table = plan.ens_table(gid, spec)
                assert np.array_equal(table.cpu().numpy(), ensstats.member_table(gid, spec)), tag
                # a kept order row, on a stream of the caller's with its own work row
                buf, acc = _guarded_acc(plan, nrows, spec)
                torch.cuda.synchronize(dev)
                plan.outputs_ens(win, nrows, table, spec, acc, ROWS_BEFORE, order=order, stream=side, work=work_side)
                side.synchronize()
                got = _result(plan, buf, acc, nrows, spec)
                assert _eq(got, want), (tag, _where(got, want))
                # the plan's own order row (the identity here), on the plan's stream
                buf, acc = _guarded_acc(plan, nrows, spec)
                plan.outputs_ens(win_id, nrows, table, spec, acc, ROWS_BEFORE)
                plan.sync()
                got = _result(plan, buf, acc, nrows, spec)
                assert _eq(got, want), (tag, "own order", _where(got, want))
                if nrows == 33:
                    a, b = nrows // 4, nrows // 4 + 1
                    buf, acc = _guarded_acc(plan, nrows, spec)
                    for lo, hi in ((b, nrows), (a, b), (0, a)):
                        plan.outputs_ens(win, hi - lo, table, spec, acc, ROWS_BEFORE + lo, order=order, row=lo)
                    plan.sync()
                    got = _result(plan, buf, acc, nrows, spec)
                    assert _eq(got, want), (tag, "three calls", _where(got, want))
            for k in OUT:                           # the window is read, never written
                assert bool((wbufs[k][:GUARD] == 31337.0).all()) and bool((wbufs[k][-GUARD:] == 31337.0).all())
    assert lib.ens_cols(layouts[0][2]) == ensstats.cols(layouts[0][2]) == lib.RS_ENS_COLS + len(QUANT)
    plan.close()


def _ens(c, **kw):
    return ensemble.run_ensemble(c["stations"], c["tails"], c["B"], c["settings"], c["params"], c["local"], None,
                                 parent=c["parent"], **kw)


@pytest.mark.parametrize("precision,recluster", [(64, False), (64, True), (32, True)],
                         ids=["fp64", "fp64-recluster", "fp32-recluster"])
def test_run_ensemble_stats_equal_the_definition_on_its_own_members(precision, recluster, monkeypatch):
    """70 stations x 5 members, launches of 100 indices, with and without a re-sort behind every launch: "stats" is
    reduce_members of the member series the same run returned, bit for bit, and everything else the run returns is
    what it returns without stats."""
    c = eh.lean_case()
    resorted = []
    plain_recluster = device.Plan.recluster

    def recluster_and_look(self):
        plain_recluster(self)
        o = self.order()[:self.npoints].cpu().numpy()
        resorted.append(not np.array_equal(o, np.arange(self.npoints)))
    monkeypatch.setattr(device.Plan, "recluster", recluster_and_look)
    spec = ensstats.EnsSpec(c["S"], c["M"], (0.1, 0.5, 0.9))
    res = _ens(c, chunk=100, recluster=recluster, precision=precision, stats=spec)
    assert any(resorted) == recluster                       # the members' slots really moved
    plain = _ens(c, chunk=100, recluster=recluster, precision=precision)
    assert "stats" not in plain and set(res) == set(plain) | {"stats"}
    assert res["failed"] == plain["failed"] == (0, 0)
    for leg in ("stations", "members"):
        for k in oh.F64_OUT:
            assert np.array_equal(res[leg][k], plain[leg][k]), (leg, k)
    got = res["stats"]
    assert got.shape == (c["L"] - c["B"], c["S"], ensstats.cols(spec)) and got.dtype == np.float64
    want = ensstats.reduce_members(*[res["members"][k] for k in OUT], c["parent"], spec)
    assert _eq(got, want), _where(got, want)
    # the comparison is not vacuous: every station has all its members, they differ, and the sums round
    assert (got[:, :, ensstats.N_USED] == c["M"]).all() and (got[:, :, ensstats.SPREAD] > 0).any()
    assert (got[:, :, ensstats.QUANT] < got[:, :, ensstats.QUANT + 2]).any()


def _refusal_fixture():
    n, nrows = 65, 4
    s = abi.default_settings(10); p = abi.default_parameters()
    plan = device.Plan(n, s, p, 0)
    d = _made_series(n, nrows, 3, np.float64, "normal")
    win, _ = _window(d, np.arange(plan.np_pad), n, nrows, plan.np_pad + 64, torch.float64, plan.device)
    gid = ensemble.parents(13, 5)
    spec = ensstats.EnsSpec(13, 5, QUANT)
    return plan, d, win, gid, spec, n, nrows


def test_every_refusal_has_its_message_and_writes_nothing():
    plan, d, win, gid, spec, n, nrows = _refusal_fixture()
    L, dev = plan.L, plan.device
    table = plan.ens_table(gid, spec)
    buf, acc = _guarded_acc(plan, nrows, spec)
    rows = acc.shape[0]
    work = torch.full((plan.np_pad,), 4242, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    sp = lib.ens_spec(spec)

    def call(plan_h=plan._h, o=win.struct(0), nr=nrows, tab=table, order=None, spec_=sp, acc_=acc, acc_rows=rows,
             row0=ROWS_BEFORE, work_=work, stream=None):
        return L.rs_hip_outputs_ens(plan_h, None if o is None else C.byref(o), nr,
                                    None if tab is None else C.c_void_p(tab.data_ptr()), order,
                                    None if spec_ is None else C.byref(spec_),
                                    None if acc_ is None else C.c_void_p(acc_.data_ptr()), acc_rows, row0,
                                    None if work_ is None else C.c_void_p(work_.data_ptr()), stream)

    def refused(message, **kw):
        assert call(**kw) == -1, (message, kw)
        assert message in lib.last_error(), (message, lib.last_error())

    for kw in (dict(plan_h=None), dict(o=None), dict(tab=None), dict(spec_=None), dict(acc_=None), dict(nr=0),
               dict(nr=-3)):
        refused("rs_hip_outputs_ens: bad arguments", **kw)
    for bad in (ensstats.EnsSpec(0, 5), ensstats.EnsSpec(13, 0), ensstats.EnsSpec(13, 65),
                ensstats.EnsSpec(13, 5, tuple(np.linspace(0, 1, 9))), ensstats.EnsSpec(13, 5, (0.5, 0.5)),
                ensstats.EnsSpec(13, 5, (0.9, 0.1)), ensstats.EnsSpec(13, 5, (1.5,)),
                ensstats.EnsSpec(13, 5, (float("nan"),))):
        refused("rs_hip_outputs_ens: bad spec", spec_=lib.ens_spec(bad))
    for row0, nr in ((-1, 1), (rows, 1), (rows - 2, 3)):
        refused("outside the accumulator's acc_rows", row0=row0, nr=nr)
    refused("outside the accumulator's acc_rows", acc_rows=0, row0=0)
    for k in OUT:
        o = win.struct(0)
        setattr(o, k, None)
        refused("rs_hip_outputs_ens: all six streams are required", o=o)
    o = win.struct(0)
    o.t_stride = n - 1
    refused("rs_hip_outputs_ens: t_stride below the plan's points", o=o)
    refused("rs_hip_outputs_ens: on a stream of the caller's the order row must be a kept one",
            stream=C.c_void_p(side.cuda_stream))
    refused("rs_hip_outputs_ens: work_device is required", work_=None)
    with pytest.raises(RuntimeError, match="kept one"):
        plan.outputs_ens(win, nrows, table, spec, acc, ROWS_BEFORE, stream=side)
    with pytest.raises(RuntimeError, match="acc_rows"):
        plan.outputs_ens(win, nrows, table, spec, acc, rows - 1)
    torch.cuda.synchronize(dev)
    # nothing was launched: the accumulator, its guards and the work row are what they were
    assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[-GUARD:] == 777.0).all())
    assert bool((acc == 555.0).all()) and bool((work == 4242).all())
    # ... and the same arguments, accepted, do write
    assert call() == 0, lib.last_error()
    plan.sync()
    got = _result(plan, buf, acc, nrows, spec)
    assert _eq(got, ensstats.reduce_members(*[d[k] for k in OUT], gid, spec))
    assert not bool((work[:n] == 4242).any())
    plan.close()


def test_a_damaged_table_or_order_row_stays_inside_bounds():
    """The bounds contract: an entry of npoints, a negative entry, a start beyond the table, a negative start, and an
    order row that names no point in one slot and a point beyond the plan in another.  The call returns; the guards
    around the accumulator, the table and the window are intact; the stations whose table is whole have their cells,
    and an entry or a point without a slot contributes nothing - the station's cell is the definition's without that
    member."""
    plan, d, win, gid, spec, n, nrows = _refusal_fixture()
    dev = plan.device
    ng = spec.ngroups
    whole = ensstats.member_table(gid, spec)
    assert np.array_equal(whole[:ng + 1], 5 * np.arange(ng + 1)) and np.array_equal(whole[ng + 1:], np.arange(n))
    bad = whole.copy()
    bad[ng + 1 + 2] = n          # station 0 loses point 2: an entry of npoints
    bad[ng + 1 + 8] = -7         # station 1 loses point 8: a negative entry
    bad[5] = 1_000_000           # start[5] beyond the table: stations 4 and 5 are anybody's
    bad[9] = -5                  # a negative start: stations 8 and 9
    tbuf = torch.full((len(bad) + 2 * GUARD,), 123456, dtype=torch.int32, device=dev)
    tbuf[GUARD:GUARD + len(bad)] = torch.from_numpy(bad).to(dev)
    table = tbuf[GUARD:GUARD + len(bad)]
    order_np = np.arange(plan.np_pad, dtype=np.int32)
    order_np[51] = -1            # point 51 (station 10) has no slot
    order_np[56] = n + 5         # ... nor has point 56 (station 11)
    order = torch.from_numpy(order_np).to(dev)
    gone = gid.copy()
    gone[[2, 8, 51, 56]] = -1
    want = ensstats.reduce_members(*[d[k] for k in OUT], gone, spec)
    buf, acc = _guarded_acc(plan, nrows, spec)
    wbuf = torch.full((plan.np_pad + 2 * GUARD,), 4242, dtype=torch.int32, device=dev)
    plan.outputs_ens(win, nrows, table, spec, acc, ROWS_BEFORE, order=order, work=wbuf[GUARD:GUARD + plan.np_pad])
    plan.sync()
    got = _result(plan, buf, acc, nrows, spec)
    sound = [g for g in range(ng) if g not in (4, 5, 8, 9)]
    assert _eq(got[:, sound], want[:, sound]), _where(got[:, sound], want[:, sound])
    assert (got[:, [0, 1, 10, 11], ensstats.N_VALID] <= 4).all()
    assert not (got == 555.0).any()                                      # every cell of the fed rows is written
    assert bool((tbuf[:GUARD] == 123456).all()) and bool((tbuf[-GUARD:] == 123456).all())
    assert np.array_equal(table.cpu().numpy(), bad)
    assert bool((wbuf[:GUARD] == 4242).all()) and bool((wbuf[-GUARD:] == 4242).all())
    plan.close()
