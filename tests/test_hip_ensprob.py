"""GPU: per-station probabilities of a condition over the ensemble members, reduced from the member rows on the device
(rs_hip_outputs_prob), against their definition, roadsurf_amd/ensprob.py (reduce_members_prob).  Every cell is a count
and the carry is bits: every comparison here is np.array_equal, no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ensemble_helpers as eh
import ensprob_helpers as ph
import oracle_helpers as oh
from roadsurf_amd import abi, device, ensemble, ensprob, ensstats, groups, lib, summary

pytestmark = pytest.mark.gpu

OUT = device.OUT_FIELDS
GUARD, ROWS_BEFORE, ROWS_AFTER = 64, 2, 3
BEYOND = 9191                                     # what the carry holds behind the plan's points


def _window(d, columns, n, nrows, stride, t_dtype, dev):
    """The six windows and the deficit, [nrows][stride] inside guarded buffers, column s = point columns[s]; the
    columns behind n hold values that would count.  Returns the window, the deficit rows and the buffers."""
    bufs, t = {}, {}
    for k in ph.SERIES:
        bufs[k] = torch.full((nrows * stride + 2 * GUARD,), 31337.0, dtype=t_dtype, device=dev)
        t[k] = bufs[k][GUARD:GUARD + nrows * stride].view(nrows, stride)
        t[k][:] = -1.0 if k in ("tsurf", "deficit") else 0.5
        t[k][:, :n] = torch.from_numpy(np.ascontiguousarray(d[k][columns[:n]].T)).to(dev)
    deficit = t.pop("deficit")
    return device.OutputWindow(nrows, stride, t), deficit, bufs


def _guarded_acc(plan, nrows, spec):
    """An accumulator of ROWS_BEFORE + nrows + ROWS_AFTER rows inside a larger buffer; a call writes every cell of its
    rows, so every cell starts as a value no cell can take."""
    rows, cells = ROWS_BEFORE + nrows + ROWS_AFTER, spec.ngroups * ensprob.cols(spec)
    buf = torch.full((rows * cells + 2 * GUARD,), 777.0, dtype=torch.float64, device=plan.device)
    acc = buf[GUARD:GUARD + rows * cells].view(rows, spec.ngroups, ensprob.cols(spec))
    acc[:] = 555.0
    return buf, acc


def _result(plan, buf, acc, nrows, spec):
    """The rows the calls were to write, after checking that nothing else was written."""
    got = plan.prob(acc, spec)
    assert (got[:ROWS_BEFORE] == 555.0).all() and (got[ROWS_BEFORE + nrows:] == 555.0).all()
    assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[-GUARD:] == 777.0).all())
    return got[ROWS_BEFORE:ROWS_BEFORE + nrows]


def _guarded_ints(count, dev, fill=4242):
    buf = torch.full((count + 2 * GUARD,), fill, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + count]


def _fresh_carry(plan, ever, stream=None):
    """The reset carry, with a mark behind the plan's points that no feed may touch."""
    plan.prob_reset(ever, stream=stream)
    (stream or plan.stream).synchronize()
    assert bool((ever == 0).all())
    ever[plan.npoints:] = BEYOND


def _carry(plan, ebuf, ever):
    assert bool((ebuf[:GUARD] == 4242).all()) and bool((ebuf[-GUARD:] == 4242).all())
    assert bool((ever[plan.npoints:] == BEYOND).all())          # columns at or beyond npoints are never written
    return ever[:plan.npoints].cpu().numpy()


def _intact(bufs, value):
    return all(bool((b[:GUARD] == value).all()) and bool((b[-GUARD:] == value).all()) for b in bufs)


@pytest.mark.parametrize("precision", [64, 32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("S,M", [(1, 1), (13, 5), (65, 20), (3, 64)], ids=["n1", "n65", "n1300", "n192"])
def test_kernels_equal_the_definition_on_made_windows(S, M, precision):
    """No model: windows made with torch against reduce_members_prob.  One point; 13 stations x 5, a second partial
    wavefront of slots; 65 x 20, a second, ragged block of stations; 3 x 64, the largest segment.  1, 5 and 33 rows
    (one row, one more than the rows in flight, and rows that do not divide among the wavefronts); one, three and eight
    conditions, the eight with one on the deficit; three group layouts; a random permutation as a kept order row on a
    stream of the caller's with scratch of its own, and the plan's own order; t_stride above npoints_padded with values
    behind the points that would count; accumulator, carry, scratch and window inside guarded buffers, the accumulator at
    acc_row0 = 2; three calls in time order equal one call, carry included; a reset starts BY_NOW afresh."""
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
    ebuf, ever = _guarded_ints(plan.np_pad, dev)
    lay = ph.layouts(S, M, rs)
    for nrows in (1, 5, 33):
        d = ph.made_series(n, nrows, 100 * n + nrows, np_dtype)
        win, dft, wbufs = _window(d, order_np, n, nrows, stride, t_dtype, dev)
        win_id, dft_id, wbufs_id = _window(d, identity, n, nrows, stride, t_dtype, dev)
        ints = plan.prob_work_ints(nrows)
        assert ints == plan.np_pad * (1 + nrows)
        sbuf, scratch = _guarded_ints(ints, dev)
        for name, gid, ng, mm in lay:
            table = plan.ens_table(gid, ensprob.ProbSpec(ng, mm, ph.conditions(1)))
            assert np.array_equal(table.cpu().numpy(), ensstats.member_table(gid, ensstats.EnsSpec(ng, mm))), name
            for nc in (1, 3, 8):
                spec = ensprob.ProbSpec(ng, mm, ph.conditions(nc))
                tag = (nrows, name, nc)
                want, want_ever = ph.reduce(d, gid, spec)
                # a kept order row, on a stream of the caller's with its own scratch
                buf, acc = _guarded_acc(plan, nrows, spec)
                _fresh_carry(plan, ever, side)
                torch.cuda.synchronize(dev)
                plan.outputs_prob(win, nrows, table, spec, ever, acc, ROWS_BEFORE, deficit=dft if nc == 8 else None,
                                  order=order, stream=side, work=scratch)
                side.synchronize()
                got = _result(plan, buf, acc, nrows, spec)
                assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:5])
                assert np.array_equal(_carry(plan, ebuf, ever), want_ever), tag
                assert _intact([sbuf], 4242), tag
                # the plan's own order row (the identity here), on the plan's stream, the plan's own scratch
                buf, acc = _guarded_acc(plan, nrows, spec)
                _fresh_carry(plan, ever)
                plan.outputs_prob(win_id, nrows, table, spec, ever, acc, ROWS_BEFORE,
                                  deficit=dft_id if nc == 8 else None)
                plan.sync()
                got = _result(plan, buf, acc, nrows, spec)
                assert np.array_equal(got, want), (tag, "own order", np.argwhere(got != want)[:5])
                assert np.array_equal(_carry(plan, ebuf, ever), want_ever), (tag, "own order")
                if nrows == 33:
                    a, b = nrows // 4, nrows // 4 + 1
                    buf, acc = _guarded_acc(plan, nrows, spec)
                    _fresh_carry(plan, ever)
                    for lo, hi in ((0, a), (a, b), (b, nrows)):
                        plan.outputs_prob(win, hi - lo, table, spec, ever, acc, ROWS_BEFORE + lo,
                                          deficit=dft if nc == 8 else None, order=order, row=lo)
                    plan.sync()
                    got = _result(plan, buf, acc, nrows, spec)
                    assert np.array_equal(got, want), (tag, "three calls", np.argwhere(got != want)[:5])
                    assert np.array_equal(_carry(plan, ebuf, ever), want_ever), (tag, "three calls")
                    # a reset between two feeds starts BY_NOW afresh: the rows from b on, as if nothing came before
                    _fresh_carry(plan, ever)
                    plan.outputs_prob(win, nrows - b, table, spec, ever, acc, ROWS_BEFORE + b,
                                      deficit=dft if nc == 8 else None, order=order, row=b)
                    plan.sync()
                    tail, tail_ever = ph.reduce(d, gid, spec, None, slice(b, nrows))
                    got = _result(plan, buf, acc, nrows, spec)
                    assert np.array_equal(got[b:], tail) and np.array_equal(got[:b], want[:b]), (tag, "reset")
                    assert np.array_equal(_carry(plan, ebuf, ever), tail_ever), (tag, "reset")
                    if n > 1 and nc == 8:
                        assert not np.array_equal(tail[:, :, 9:], want[b:, :, 9:]), tag      # (it does matter)
        # the windows are read, never written
        assert _intact(list(wbufs.values()) + list(wbufs_id.values()), 31337.0)
    plan.close()


def _refusal_fixture():
    n, nrows = 65, 4
    s = abi.default_settings(10); p = abi.default_parameters()
    plan = device.Plan(n, s, p, 0)
    d = ph.made_series(n, nrows, 3)
    win, dft, _ = _window(d, np.arange(plan.np_pad), n, nrows, plan.np_pad + 64, torch.float64, plan.device)
    gid = ensemble.parents(13, 5)
    spec = ensprob.ProbSpec(13, 5, ph.conditions(8))
    return plan, d, win, dft, gid, spec, n, nrows


def test_every_refusal_has_its_message_and_writes_nothing():
    plan, d, win, dft, gid, spec, n, nrows = _refusal_fixture()
    L, dev = plan.L, plan.device
    table = plan.ens_table(gid, spec)
    buf, acc = _guarded_acc(plan, nrows, spec)
    rows = acc.shape[0]
    ints = plan.prob_work_ints(nrows)
    work = torch.full((ints,), 4242, dtype=torch.int32, device=dev)
    ever = torch.full((plan.np_pad,), 1717, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    sp = lib.prob_spec(spec)
    no_deficit = lib.prob_spec(ensprob.ProbSpec(13, 5, ph.conditions(3)))

    def call(plan_h=plan._h, o=win.struct(0), deficit=dft, nr=nrows, tab=table, order=None, spec_=sp, ever_=ever,
             acc_=acc, acc_rows=rows, row0=ROWS_BEFORE, work_=work, work_ints=ints, stream=None):
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())                      # noqa: E731
        return L.rs_hip_outputs_prob(plan_h, None if o is None else C.byref(o), ptr(deficit), nr, ptr(tab), order,
                                     None if spec_ is None else C.byref(spec_), ptr(ever_), ptr(acc_), acc_rows, row0,
                                     ptr(work_), work_ints, stream)

    def refused(message, **kw):
        assert call(**kw) == -1, (message, kw)
        assert message in lib.last_error(), (message, lib.last_error())

    for kw in (dict(plan_h=None), dict(o=None), dict(tab=None), dict(spec_=None), dict(ever_=None), dict(acc_=None),
               dict(nr=0), dict(nr=-3)):
        refused("rs_hip_outputs_prob: bad arguments", **kw)
    ok = ph.conditions(3)
    Cn = ensprob.Condition
    for bad in (ensprob.ProbSpec(0, 5, ok), ensprob.ProbSpec(13, 0, ok), ensprob.ProbSpec(13, 65, ok),
                ensprob.ProbSpec(13, 5, ()), ensprob.ProbSpec(13, 5, ph.CONDITIONS + ok[:1]),
                ensprob.ProbSpec(13, 5, (Cn(0),)), ensprob.ProbSpec(13, 5, (ok[0], Cn(128))),
                ensprob.ProbSpec(13, 5, (Cn(1, (float("nan"),) + (0.0,) * 6),))):
        refused("rs_hip_outputs_prob: bad spec", spec_=lib.prob_spec(bad))
    for row0, nr in ((-1, 1), (rows, 1), (rows - 2, 3)):
        refused("outside the accumulator's acc_rows", row0=row0, nr=nr)
    refused("outside the accumulator's acc_rows", acc_rows=0, row0=0)
    for k in OUT:
        o = win.struct(0)
        setattr(o, k, None)
        refused("rs_hip_outputs_prob: all six streams are required", o=o)
    o = win.struct(0)
    o.t_stride = n - 1
    refused("rs_hip_outputs_prob: t_stride below the plan's points", o=o)
    refused("rs_hip_outputs_prob: on a stream of the caller's the order row must be a kept one",
            stream=C.c_void_p(side.cuda_stream))
    refused("rs_hip_outputs_prob: this spec uses the deficit (bit 6): deficit_device is required", deficit=None)
    refused("rs_hip_outputs_prob: work_device is required", work_=None)
    refused(f"rs_hip_outputs_prob: work_ints = {ints - 1} is below rs_hip_prob_work_ints = {ints}", work_ints=ints - 1)
    refused("is below rs_hip_prob_work_ints", work_ints=0)
    assert L.rs_hip_prob_reset(None, C.c_void_p(ever.data_ptr()), None) == -1
    assert "rs_hip_prob_reset: bad arguments" in lib.last_error()
    assert L.rs_hip_prob_reset(plan._h, None, None) == -1
    with pytest.raises(RuntimeError, match="kept one"):
        plan.outputs_prob(win, nrows, table, spec, ever, acc, ROWS_BEFORE, deficit=dft, stream=side, work=work)
    with pytest.raises(ValueError, match="a work of the caller's"):
        plan.outputs_prob(win, nrows, table, spec, ever, acc, ROWS_BEFORE, deficit=dft, stream=side)
    with pytest.raises(RuntimeError, match="acc_rows"):
        plan.outputs_prob(win, nrows, table, spec, ever, acc, rows - 1, deficit=dft)
    with pytest.raises(RuntimeError, match="deficit_device is required"):
        plan.outputs_prob(win, nrows, table, spec, ever, acc, ROWS_BEFORE)
    with pytest.raises(ValueError):
        plan.prob_work_ints(0)
    torch.cuda.synchronize(dev)
    # nothing was launched: the accumulator, its guards, the carry and the scratch are what they were
    assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[-GUARD:] == 777.0).all())
    assert bool((acc == 555.0).all()) and bool((work == 4242).all()) and bool((ever == 1717).all())
    # ... and the same arguments, accepted, do write; a spec without the deficit needs no deficit rows
    plan.prob_reset(ever)
    assert call() == 0, lib.last_error()
    plan.sync()
    got = _result(plan, buf, acc, nrows, spec)
    want, want_ever = ph.reduce(d, gid, spec)
    assert np.array_equal(got, want) and np.array_equal(ever[:n].cpu().numpy(), want_ever)
    assert not bool((work[:n] == 4242).any()) and not bool((work[plan.np_pad:plan.np_pad + n] == 4242).any())
    acc3 = torch.full((nrows, 13, 7), 555.0, dtype=torch.float64, device=dev)
    plan.prob_reset(ever)
    assert call(deficit=None, spec_=no_deficit, acc_=acc3, acc_rows=nrows, row0=0) == 0, lib.last_error()
    plan.sync()
    assert np.array_equal(acc3.cpu().numpy(), ph.reduce(d, gid, ensprob.ProbSpec(13, 5, ph.conditions(3)))[0])
    plan.close()


def test_a_damaged_table_or_order_row_stays_inside_bounds():
    """The bounds contract: an entry of npoints, a negative entry, a start beyond the table, a negative start, and an
    order row that names no point in one slot and a point beyond the plan in another.  The call returns; the guards
    around the accumulator, the table, the carry, the scratch and the window are intact; the stations whose table is
    whole have their cells, and an entry or a point without a slot contributes nothing - the station's cell is the
    definition's without that member; every cell of the fed rows is written."""
    plan, d, win, dft, gid, spec, n, nrows = _refusal_fixture()
    dev = plan.device
    ng = spec.ngroups
    whole = ensstats.member_table(gid, ensprob.table_spec(spec))
    assert np.array_equal(whole[:ng + 1], 5 * np.arange(ng + 1)) and np.array_equal(whole[ng + 1:], np.arange(n))
    bad = whole.copy()
    bad[ng + 1 + 2] = n          # station 0 loses point 2: an entry of npoints
    bad[ng + 1 + 8] = -7         # station 1 loses point 8: a negative entry
    bad[5] = 1_000_000           # start[5] beyond the table: stations 4 and 5 are anybody's
    bad[9] = -5                  # a negative start: stations 8 and 9
    tbuf, table = _guarded_ints(len(bad), dev, 123456)
    table[:] = torch.from_numpy(bad).to(dev)
    order_np = np.arange(plan.np_pad, dtype=np.int32)
    order_np[51] = -1            # point 51 (station 10) has no slot
    order_np[56] = n + 5         # ... nor has point 56 (station 11)
    order = torch.from_numpy(order_np).to(dev)
    gone = gid.copy()
    gone[[2, 8, 51, 56]] = -1
    want, want_ever = ph.reduce(d, gone, spec)
    buf, acc = _guarded_acc(plan, nrows, spec)
    wbuf, work = _guarded_ints(plan.prob_work_ints(nrows), dev)
    ebuf, ever = _guarded_ints(plan.np_pad, dev)
    _fresh_carry(plan, ever)
    plan.outputs_prob(win, nrows, table, spec, ever, acc, ROWS_BEFORE, deficit=dft, order=order, work=work)
    plan.sync()
    got = _result(plan, buf, acc, nrows, spec)
    sound = [g for g in range(ng) if g not in (4, 5, 8, 9)]
    assert np.array_equal(got[:, sound], want[:, sound]), np.argwhere(got[:, sound] != want[:, sound])[:5]
    assert (got[:, [0, 1, 10, 11], 0] <= 4).all()
    assert not (got == 555.0).any()                                      # every cell of the fed rows is written
    assert _intact([tbuf], 123456) and np.array_equal(table.cpu().numpy(), bad)
    assert _intact([wbuf], 4242)
    carry = _carry(plan, ebuf, ever)
    named = [q for q in range(n) if q not in (51, 56)]                   # a point no slot names keeps its carry
    assert np.array_equal(carry[named], want_ever[named]) and (carry[[51, 56]] == 0).all()
    plan.close()


def _ens(c, **kw):
    return ensemble.run_ensemble(c["stations"], c["tails"], c["B"], c["settings"], c["params"], c["local"], None,
                                 parent=c["parent"], **kw)


def _forecast_spec(c):
    return ensprob.ProbSpec(c["S"], c["M"], ph.FORECAST_CONDITIONS)


@functools.lru_cache(maxsize=None)
def _runs(precision, recluster):
    """(with probs, without) of the lean case in launches of 100 indices, each made once."""
    c = eh.lean_case()
    kw = dict(chunk=100, recluster=recluster, precision=precision)
    return _ens(c, probs=_forecast_spec(c), **kw), _ens(c, **kw)


@pytest.mark.parametrize("precision,recluster", [(64, False), (64, True), (32, True)],
                         ids=["fp64", "fp64-recluster", "fp32-recluster"])
def test_run_ensemble_probs_equal_the_definition_on_its_own_members(precision, recluster):
    """70 stations x 5 members, launches of 100 indices, with and without a re-sort behind every launch: "probs" is
    reduce_members_prob of the member series the same run returned, and everything else the run returns is what it
    returns without probs.  In fp64 that is also the definition applied to the reference's own run."""
    c = eh.lean_case()
    spec = _forecast_spec(c)
    res, plain = _runs(precision, recluster)
    assert "probs" not in plain and set(res) == set(plain) | {"probs"}
    assert res["failed"] == plain["failed"] == (0, 0)
    for leg in ("stations", "members"):
        for k in oh.F64_OUT:
            assert np.array_equal(res[leg][k], plain[leg][k]), (leg, k)
    got = res["probs"]
    assert got.shape == (c["L"] - c["B"], c["S"], ensprob.cols(spec)) and got.dtype == np.float64
    want, _ = ensprob.reduce_members_prob(*[res["members"][k] for k in OUT], None, c["parent"], spec)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    counts = ph.non_vacuity(got, spec, c["M"])
    if precision == 64:
        o = eh.lean_oracle()
        ref, _ = ensprob.reduce_members_prob(*[o[k][:, c["B"]:] for k in OUT], None, c["parent"], spec)
        assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
        for mixed, later in counts:
            assert mixed >= 1000 and later >= 100, counts
    else:
        assert all(mixed > 0 for mixed, _ in counts), counts


def test_probs_stats_and_groups_in_one_run_are_what_each_is_alone():
    c = eh.lean_case()
    spec = _forecast_spec(c)
    stats = ensstats.EnsSpec(c["S"], c["M"], (0.1, 0.5, 0.9))
    grp = (groups.GroupSpec(summary.SummarySpec(), c["S"]), c["parent"])
    both = _ens(c, chunk=100, probs=spec, stats=stats, groups=grp)
    assert np.array_equal(both["probs"], _runs(64, False)[0]["probs"])
    assert np.array_equal(both["stats"], _ens(c, chunk=100, stats=stats)["stats"], equal_nan=True)
    assert np.array_equal(both["groups"], _ens(c, chunk=100, groups=grp)["groups"])
    # the group series say the same where they can: the valid members, and Tsurf < 0 now
    assert np.array_equal(both["probs"][:, :, 0], both["groups"][:, :, groups.COUNT])
    assert np.array_equal(both["probs"][:, :, 1], both["groups"][:, :, groups.N_BELOW])


def test_run_points_forwards_probs():
    c = eh.lean_case()
    spec = _forecast_spec(c)
    n, L = 60, 200
    f = {k: np.ascontiguousarray(v[:n, :L] if np.ndim(v) == 2 else v[:L]) for k, v in c["rep"].items()}
    s = abi.default_settings(L)
    sp = ensprob.ProbSpec(12, 5, spec.conditions)
    res, nfail = device.run_points(f, s, c["params"], c["local"], chunk=70, probs=(sp, ensemble.parents(12, 5)))
    want, _ = ensprob.reduce_members_prob(*[res[k] for k in OUT], None, ensemble.parents(12, 5), sp)
    assert nfail == 0 and res["probs"].shape == (L, 12, 7) and np.array_equal(res["probs"], want)
    with pytest.raises(ValueError, match="deficit"):
        device.run_points(f, s, c["params"], c["local"], probs=(ensprob.ProbSpec(12, 5, ph.conditions(8)),
                                                                 ensemble.parents(12, 5)))
