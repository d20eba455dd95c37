"""GPU: the driver's inputs at the kept rows and the dew-point deficit (rs_driver_run_kept) against the CPU checker
(driver_helpers.oracle_read_input / oracle_run), the device's own read_input and the definition
(roadsurf_amd/kept.py).  Every comparison is on the bits."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import driver_helpers as dh
import grid_helpers as gh
import oracle_helpers as oh
from roadsurf_amd import abi, driver, grid, groups, kept, lib, summary

pytestmark = pytest.mark.gpu
M = -9999.9
GUARD = 777.25
ALL = driver.MERGED_FIELDS
SIZES = (1, 65, 203)
OUTPUT_STEPS = (1, 7, 60)          # minutes: step 2, 14 (SimLen 1441 is no multiple of it), 120
SEED = 7
MODES = {"plain": dict(), "relaxation": dict(use_relaxation=1), "coupling": dict(use_relaxation=1, use_coupling=1)}


def _kind(coupled):
    if coupled:
        return "ref_cpl" if os.path.exists(oh.REF_CPL_SO) else "port"
    return "ref" if os.path.exists(oh.REF_SO) else "port"


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _settings(L, output_step, mode="plain"):
    s = abi.default_settings(L)
    s.outputStep = output_step
    for k, v in MODES[mode].items():
        setattr(s, k, v)
    return s


@functools.lru_cache(maxsize=None)
def _sources(n, how):
    """(sources, L, start, forecast_time, sources as the checker takes them)"""
    if how == "grid":
        src, L, t0, tf = gh.grid_scenario(n, hours=12, seed=23)
        return src, L, t0, tf, [grid.to_raw_source(src[0]), src[1]]
    src, L, t0, tf = dh.scenario(n, hours=12, seed=SEED)
    if how == "ragged":
        src = [src[0], dh.ragged(src[1], seed=3)]
    return src, L, t0, tf, src


@functools.lru_cache(maxsize=None)
def _oracle(n, how, mode, output_step):
    """The checker's read_input and run of one case, computed once: merged [SimLen] series, the six outputs."""
    _, L, t0, tf, raw = _sources(n, how)
    s = _settings(L, output_step, mode)
    ri = dh.oracle_read_input(raw, s, t0, tf)
    run = dh.oracle_run(_kind(mode == "coupling"), raw, s, abi.default_parameters(), t0, tf)
    for a in list(ri["merged"].values()) + [run[k] for k in driver.OUT_FIELDS]:
        a.setflags(write=False)
    return ri, run


def _expected(n, how, mode, output_step):
    ri, run = _oracle(n, how, mode, output_step)
    step = run["step"]
    want = {k: kept.kept_rows(ri["merged"][k], step) for k in ALL}
    return want, kept.dew_point_deficit(run["tsurf"], want["tdew"]), ri, run


def _run(n, how, mode, output_step, **kw):
    src, L, t0, tf, _ = _sources(n, how)
    kw.setdefault("kept", ALL)
    kw.setdefault("deficit", True)
    return driver.run(src, _settings(L, output_step, mode), abi.default_parameters(), t0, tf, **kw)


def _check(res, n, how, mode, output_step, what=""):
    want, deficit, ri, run = _expected(n, how, mode, output_step)
    step, n_out = run["step"], run["tsurf"].shape[1]
    assert res["step"] == step == output_step * 2 and n_out == (1441 + step - 1) // step
    for k in ALL:
        assert res["kept"][k].shape == (n, n_out)
        assert _same_bits(res["kept"][k], want[k]), (what, k, np.argwhere(_bits(res["kept"][k]) != _bits(want[k]))[:5])
    assert _same_bits(res["deficit"], deficit), (what, np.argwhere(_bits(res["deficit"]) != _bits(deficit))[:5])
    assert np.array_equal(res["status"], run["status"]) and np.array_equal(res["missing_index"], run["missing_index"]), what
    for k in driver.OUT_FIELDS:
        if k in res:
            assert _same_bits(res[k], run[k]), (what, k)


# ---- 7. the cases hold what they are there for: asserted from the CHECKER's data alone (no device call)

def test_the_cases_hold_what_they_are_there_for():
    n = 203
    src, L, t0, tf, _ = _sources(n, "scenario")
    want, deficit, ri, run = _expected(n, "scenario", "coupling", 7)
    step = 14
    assert run["step"] == step and L == 1441 and L % step != 0
    # an interpolated value: a kept index strictly between two hourly forecast times (simulation index 0 is the
    # forecast's second stamp) whose value differs from both raw ends - LW comes from the forecast alone
    fc = src[0]
    assert fc.times[1] == t0 and fc.times[2] - fc.times[1] == 3600
    found = 0
    for r in range(want["lw"].shape[1]):
        i = r * step
        if i % 120 == 0:
            continue
        lo = 1 + i // 120
        a, b, v = fc.fields["lw"][:, lo], fc.fields["lw"][:, lo + 1], want["lw"][:, r]
        found += int(((v != a) & (v != b) & (v > -100) & (np.minimum(a, b) < v) & (v < np.maximum(a, b))).sum())
    assert found > 100
    # missing values among the compared ones
    assert (want["tsurfobs"] == M).any() and (want["tair"] == M).any() and (want["rhz"] > -100).any()
    # TSurfObs blanked inside a coupling window at a kept index: there without coupling, -9999.9 with it
    plain = kept.kept_rows(_oracle(n, "scenario", "relaxation", 7)[0]["merged"]["tsurfobs"], step)
    blanked = (plain > -100) & (want["tsurfobs"] == M)
    assert blanked.sum() > n and (blanked.any(axis=1) == (run["status"] == 0)).sum() > n // 2
    assert ((plain > -100) & (want["tsurfobs"] > -100)).any()      # ... and not everywhere
    for k in ALL[:-1]:                                           # nothing else differs
        assert _same_bits(want[k], kept.kept_rows(_oracle(n, "scenario", "relaxation", 7)[0]["merged"][k], step)), k
    # a rejected point whose kept air temperature is not blanked and whose deficit is -9999.0 throughout
    rejected = np.nonzero(run["status"] != 0)[0]
    intact = [p for p in rejected if (want["tair"][p] > -100).all() and (want["tdew"][p] > -100).all()]
    assert len(rejected) >= 5 and len(intact) >= 2
    assert (run["tsurf"][rejected] == -9999.0).all() and (deficit[rejected] == -9999.0).all()
    # deficits of both signs, and none missing for a simulated point
    ok = run["status"] == 0
    assert (deficit[ok] < 0).sum() > 50 and (deficit[ok] > 0).sum() > 50 and (deficit[ok] != -9999.0).all()
    # the other cases: the hourly rows too; per-point axes leave a series empty, one with a single stamp
    for os_ in OUTPUT_STEPS:
        w, d, _, r = _expected(n, "scenario", "plain", os_)
        assert (d[r["status"] == 0] < 0).any() and (d[r["status"] == 0] > 0).any() and (w["tsurfobs"] == M).any()
    rg = _sources(n, "ragged")[0][1]
    assert rg.times.ndim == 2 and rg.lengths.min() == 0 and (rg.lengths == 1).any() and rg.lengths.max() > 20
    w, d, ri2, r = _expected(n, "ragged", "relaxation", 7)
    assert (w["tsurfobs"] > -100).sum() > n and (w["tsurfobs"] == M).any() and 0 < (r["status"] != 0).sum() < n // 2


# ---- 1. ten variables

@pytest.mark.parametrize("output_step", OUTPUT_STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_ten_variables(n, output_step):
    """All ten kept variables equal the checker's merged series at every step-th index, and the device's own
    read_input of the same call, decimated; the deficit equals the definition over the checker's Tsurf."""
    res = _run(n, "scenario", "relaxation", output_step)
    _check(res, n, "scenario", "relaxation", output_step)
    src, L, t0, tf, _ = _sources(n, "scenario")
    own = driver.read_input(src, _settings(L, output_step, "relaxation"), t0, tf)
    for k in ALL:
        assert _same_bits(res["kept"][k], own["merged"][k][:, ::res["step"]]), k
    assert np.array_equal(own["status"], res["status"])


# ---- 2. per-point time axes: the sequential walk

@pytest.mark.parametrize("output_step", OUTPUT_STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_per_point_time_axes(n, output_step):
    res = _run(n, "ragged", "relaxation", output_step)
    _check(res, n, "ragged", "relaxation", output_step)
    src, L, t0, tf, _ = _sources(n, "ragged")
    own = driver.read_input(src, _settings(L, output_step, "relaxation"), t0, tf)
    for k in ALL:
        assert _same_bits(res["kept"][k], own["merged"][k][:, ::res["step"]]), k


# ---- 3. coupling: TSurfObs blanked inside the window, the deficit over the replayed Tsurf

@pytest.mark.parametrize("how", ["scenario", "ragged"])
@pytest.mark.parametrize("output_step", OUTPUT_STEPS)
def test_coupling(output_step, how):
    n = 203
    res = _run(n, how, "coupling", output_step)
    _check(res, n, how, "coupling", output_step)
    want, deficit, ri, run = _expected(n, how, "coupling", output_step)
    plain = kept.kept_rows(_oracle(n, how, "relaxation", output_step)[0]["merged"]["tsurfobs"], run["step"])
    blanked = (plain > -100) & (want["tsurfobs"] == M)
    assert blanked.any() and (res["kept"]["tsurfobs"][blanked] == M).all()
    # the replays rewrote rows: the coupled Tsurf is not the uncoupled one, and the deficit follows it
    uncoupled = _oracle(n, how, "relaxation", output_step)[1]["tsurf"]
    moved = (run["tsurf"] != uncoupled) & (run["tsurf"] != -9999.0)
    assert moved.any() and (res["deficit"][moved] != kept.dew_point_deficit(uncoupled, want["tdew"])[moved]).any()


# ---- 4. the deficit, and a call's other results do not depend on `kept`

@pytest.mark.parametrize("mode", ["plain", "coupling"])
def test_outputs_do_not_depend_on_kept(mode):
    n, output_step = 203, 7
    with_kept = _run(n, "scenario", mode, output_step)
    _check(with_kept, n, "scenario", mode, output_step)
    without = _run(n, "scenario", mode, output_step, kept=(), deficit=False)
    assert "kept" not in without and "deficit" not in without
    for k in driver.OUT_FIELDS:
        assert _same_bits(with_kept[k], without[k]), k
    assert np.array_equal(with_kept["status"], without["status"])
    assert np.array_equal(with_kept["missing_index"], without["missing_index"])
    for p in range(n):
        for f in ("tair_relax", "VZ_relax", "RH_relax", "couplingIndexI", "couplingTsurf", "InitLenI"):
            assert getattr(with_kept["local"][p], f) == getattr(without["local"][p], f), (p, f)
    # a rejected point: its inputs as read_input returns them, its deficit -9999.0
    rejected = np.nonzero(with_kept["status"] != 0)[0]
    assert (with_kept["deficit"][rejected] == -9999.0).all()
    assert any((with_kept["kept"]["tair"][p] > -100).all() for p in rejected)
    # no series at all
    only = _run(n, "scenario", mode, output_step, series=False)
    assert "tsurf" not in only
    _check(only, n, "scenario", mode, output_step, "series=False")
    only = _run(n, "scenario", mode, output_step, series=False, kept=("tair",), deficit=False)
    assert set(only["kept"]) == {"tair"} and "deficit" not in only and _same_bits(only["kept"]["tair"], with_kept["kept"]["tair"])
    only = _run(n, "scenario", mode, output_step, series=False, kept=(), deficit=True)
    assert only["kept"] == {} and _same_bits(only["deficit"], with_kept["deficit"])
    with pytest.raises(ValueError):
        _run(n, "scenario", mode, output_step, series=False, kept=(), deficit=False)
    with pytest.raises(KeyError):
        _run(n, "scenario", mode, output_step, kept=("depth",))


# ---- 5. other paths

@pytest.mark.parametrize("mode", ["relaxation", "coupling"])
def test_tiles_fanout_windows(mode, monkeypatch):
    n, output_step = 203, 7
    L_ = driver._bind(lib.load())
    monkeypatch.setenv("ROADSURF_HIP_TILE_POINTS", "200")
    _check(_run(n, "scenario", mode, output_step), n, "scenario", mode, output_step, "two tiles")
    assert L_.rs_driver_last_tiles() == 2
    _check(_run(n, "ragged", mode, output_step), n, "ragged", mode, output_step, "two tiles, per-point axes")
    monkeypatch.delenv("ROADSURF_HIP_TILE_POINTS")

    monkeypatch.setenv("ROADSURF_HIP_DEVICES", "0,0")
    monkeypatch.setenv("ROADSURF_HIP_MIN_SHARD", "64")
    _check(_run(n, "scenario", mode, output_step, device=-1), n, "scenario", mode, output_step, "fan-out")
    assert L_.rs_last_fanout() == 2
    monkeypatch.delenv("ROADSURF_HIP_DEVICES")
    monkeypatch.delenv("ROADSURF_HIP_MIN_SHARD")

    _run(n, "scenario", mode, output_step)
    assert L_.rs_driver_last_raw_launches() > 0
    monkeypatch.setenv("ROADSURF_HIP_DRIVER_WINDOWS", "1")
    _check(_run(n, "scenario", mode, output_step), n, "scenario", mode, output_step, "forcing windows")
    assert L_.rs_driver_last_raw_launches() == 0
    monkeypatch.delenv("ROADSURF_HIP_DRIVER_WINDOWS")

    monkeypatch.setenv("ROADSURF_HIP_CLUSTER", "0")
    _check(_run(n, "scenario", mode, output_step), n, "scenario", mode, output_step, "natural order")


def test_gridded_forecast():
    n, output_step = 203, 7
    src = _sources(n, "grid")[0]
    assert isinstance(src[0], grid.GridSource)
    for mode in ("relaxation", "coupling"):
        res = _run(n, "grid", mode, output_step)
        _check(res, n, "grid", mode, output_step, "gridded " + mode)
        assert 0 < (res["status"] != 0).sum() < n // 2


def test_with_summaries_and_groups():
    n, output_step, mode = 203, 7, "relaxation"
    src, L, t0, tf, _ = _sources(n, "scenario")
    s = _settings(L, output_step, mode)
    first, last = driver.forecast_rows(s, t0, tf)
    th = summary.SummarySpec(0.0, (0.0,) * 5)
    gspec = groups.GroupSpec(th, 4, (-2.0, 0.0, 2.0))
    gid = np.random.RandomState(4).randint(0, 4, n).astype(np.int32)
    kw = dict(summary=th, summary_rows=(first, last), groups=gspec, group_of=gid, group_rows=(first, last))
    both = _run(n, "scenario", mode, output_step, **kw)
    _check(both, n, "scenario", mode, output_step, "with summaries and groups")
    alone = _run(n, "scenario", mode, output_step, kept=(), deficit=False, **kw)
    assert _same_bits(both["summary"], alone["summary"]) and _same_bits(both["groups"], alone["groups"])
    none = _run(n, "scenario", mode, output_step, series=False, **kw)
    _check(none, n, "scenario", mode, output_step, "summaries, groups, no series")
    assert _same_bits(none["summary"], alone["summary"]) and _same_bits(none["groups"], alone["groups"])


# ---- 6. a subset request writes nothing else

@pytest.mark.parametrize("how", ["scenario", "ragged"])
def test_a_subset_leaves_the_rest_untouched(how):
    """The caller holds one block [11][n][n_out] pre-filled with a sentinel and hands over the dew point's slice
    alone, then the deficit's alone: every other slice keeps the sentinel."""
    n, output_step, mode = 65, 7, "coupling"
    src, L, t0, tf, _ = _sources(n, how)
    want, deficit, ri, run = _expected(n, how, mode, output_step)
    s = _settings(L, output_step, mode)
    p = abi.default_parameters()
    L_ = driver._bind(lib.load())
    assert L_.rs_driver_kept_fields() == 10
    n_out = run["tsurf"].shape[1]
    inp, keep = driver.make_input(src, t0, tf, driver.calendar(t0, L, int(s.DTSecs)))

    def call(slots, with_series):
        block = np.full((11, n, n_out), GUARD)
        kq = driver.RsDriverKept()
        for k in slots or ():
            ptr = block[k].ctypes.data_as(abi.c_double_p)
            if k == 10:
                kq.deficit = ptr
            else:
                kq.merged[k] = ptr
        out = driver.RsDriverOutput(); out.n_out = n_out
        st = np.full(n, 77, np.int32); mi = np.full(n, 77, np.int32)
        ts = np.full((n, n_out), GUARD)
        if with_series:
            out.tsurf = ts.ctypes.data_as(abi.c_double_p)
        out.status = st.ctypes.data_as(abi.c_int32_p); out.missing_index = mi.ctypes.data_as(abi.c_int32_p)
        rc = L_.rs_driver_run_kept(C.byref(inp), None, C.byref(s), C.byref(p), driver._locals(n, None), C.byref(out),
                                   None, None, C.byref(kq) if slots is not None else None, 0)
        assert rc == 0, lib.last_error()
        assert np.array_equal(st, run["status"]) and np.array_equal(mi, run["missing_index"])
        assert _same_bits(ts, run["tsurf"]) if with_series else (ts == GUARD).all()
        return block

    b = call((1,), True)
    assert _same_bits(b[1], want["tdew"]) and (np.delete(b, 1, axis=0) == GUARD).all()
    b = call((10,), False)
    assert _same_bits(b[10], deficit) and (b[:10] == GUARD).all()
    b = call((9, 0), False)
    assert _same_bits(b[9], want["tsurfobs"]) and _same_bits(b[0], want["tair"]) and (b[1:9] == GUARD).all() and (b[10] == GUARD).all()
    # all eleven pointers NULL, or no struct: the call without
    assert (call((), True) == GUARD).all() and (call(None, True) == GUARD).all()
    del keep
