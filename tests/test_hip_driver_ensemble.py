"""GPU: the ensemble form of the driver (driver.run_ensemble, rs_driver_run_ensemble) against its definition - a plain
``driver.run`` on ``driver.replicate_sources`` for the members, on the shared sources alone for the stations - bit for
bit: the six series at the members' own kept rows, status, missing_index and the decisions, the stations' rows before
the branch, the per-station statistics and probabilities, and every refusal with its reason.

The base shape is small and several tiles deep: 37 stations with 0..5 members each, SimLen 1 081, a kept row every
20 indices, tiles of 64 points and launches of 97 indices, so that tiles cut the station list and launches cut the
branch off the kept rows."""
import ctypes as C
import functools

import numpy as np
import pytest

import driver_helpers as dh
import grid_helpers as gh
from roadsurf_amd import abi, driver, ensprob, ensstats

pytestmark = pytest.mark.gpu

S, HOURS, OBS_HOURS = 37, 9, 6
L = HOURS * 120 + 1
COUNTS = np.array([(s * 7 + 3) % 6 for s in range(S)])
PARENT = np.repeat(np.arange(S, dtype=np.int32), COUNTS)
DECISIONS = ("InitLenI", "tair_relax", "VZ_relax", "RH_relax", "couplingIndexI", "couplingTsurf")
GUARD = 777.0
START = dh.START


@pytest.fixture(autouse=True)
def _small_tiles(monkeypatch):
    monkeypatch.setenv("ROADSURF_HIP_TILE_POINTS", "64")
    monkeypatch.setenv("ROADSURF_HIP_CHUNK_STEPS", "97")


def _u64(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _settings(relax=1, coupling=0, simlen=L):
    s = abi.default_settings(simlen)
    s.outputStep = 10
    s.use_relaxation = relax
    s.use_coupling = coupling
    return s


def member_source(n_members, times, seed=11, holes=True):
    """A forecast of the members' own on the shared axis `times`; two members have a hole in it."""
    rs = np.random.RandomState(seed)
    t = np.asarray(times, np.int64)
    shape = (n_members, len(t))
    tair = rs.uniform(-8, 4, shape)
    f = {"tair": tair, "tdew": tair - rs.uniform(0.2, 4, shape), "vz": rs.uniform(0.5, 9, shape),
         "prec": rs.uniform(0, 1, shape) * (rs.rand(*shape) < 0.3), "sw": rs.uniform(0, 200, shape),
         "lw": rs.uniform(200, 330, shape)}
    if holes and n_members > 4 and len(t) > 2:
        f["tair"][1, 1] = -9999.9
        f["lw"][n_members - 2, 1:3] = -9999.9
    return driver.RawSource(t, f)


def hourly(first_seconds):
    """hourly stamps from START + first_seconds to an hour behind the end of the run"""
    return START + np.arange(first_seconds, (HOURS + 1) * 3600 + 1, 3600, dtype=np.int64)


def _decisions(larr):
    return {k: np.array([getattr(l, k) for l in larr]) for k in DECISIONS}


def _copies(local, idx):
    out = []
    for i in idx:
        l = abi.LocalParameters()
        C.memmove(C.byref(l), C.byref(local[int(i)]), C.sizeof(l))
        out.append(l)
    return out


def compare(shared, mem, parent, s, t0, tf, local=None, horizons=None, position=None, **kw):
    """One ensemble call against the two plain calls that define it.  Returns (ensemble result, the members' plain
    result, the stations' plain result)."""
    p = abi.default_parameters()
    ens = driver.run_ensemble(shared, mem, parent, s, p, t0, tf, position=position, local=local, horizons=horizons, **kw)
    mlocal = None if local is None else _copies(local, parent)
    mhz = None if horizons is None else np.ascontiguousarray(horizons[parent])
    pm = driver.run(driver.replicate_sources(shared, mem, parent, position), s, p, t0, tf, local=mlocal, horizons=mhz)
    ps = driver.run(shared, s, p, t0, tf, local=local, horizons=horizons)
    B, first_row, n_tail = driver.member_rows(s, t0, int(mem.times[0]))
    assert (ens["branch_index"], ens["first_row"]) == (B, first_row)
    me, st = ens["members"], ens["stations"]
    for k in ("status", "missing_index"):
        assert np.array_equal(me[k], pm[k]), k
        assert np.array_equal(st[k], ps[k]), k
    dm, dpm, ds, dps = _decisions(me["local"]), _decisions(pm["local"]), _decisions(st["local"]), _decisions(ps["local"])
    for k in DECISIONS:
        assert np.array_equal(_u64(dm[k]), _u64(dpm[k])), k
        assert np.array_equal(_u64(ds[k]), _u64(dps[k])), k
    for k in driver.OUT_FIELDS:
        if kw.get("series", True):
            assert me[k].shape == (len(parent), n_tail)
            assert np.array_equal(_u64(me[k]), _u64(pm[k][:, first_row:])), k
        else:
            assert k not in me
        assert np.array_equal(_u64(st[k][:, :first_row]), _u64(ps[k][:, :first_row])), k
        assert (st[k][:, first_row:] == -9999.0).all(), k
    return ens, pm, ps


@functools.lru_cache(maxsize=None)
def base_sources():
    src, simlen, t0, tf = dh.scenario(S, hours=HOURS, obs_hours=OBS_HOURS)
    assert simlen == L
    return src, t0, tf


def test_base_shape_is_ragged_and_tiled():
    assert COUNTS.min() == 0 and COUNTS.max() == 5 and len(PARENT) > 64 and (COUNTS == 0).sum() >= 1


def test_relaxation():
    src, t0, tf = base_sources()
    ens, pm, ps = compare(src, member_source(len(PARENT), hourly(OBS_HOURS * 3600)), PARENT, _settings(), t0, tf)
    assert ens["branch_index"] == 720 and ens["first_row"] == 36
    assert (ps["status"] != 0).any() and (pm["status"] != 0).any() and (pm["status"] == 0).sum() > 64   # rejected points take part
    assert driver.rslib.load().rs_driver_last_tiles() >= 1


def test_coupling_and_relaxation_at_the_limit_of_the_rule():
    src, t0, tf = base_sources()
    ens, pm, ps = compare(src, member_source(len(PARENT), hourly(OBS_HOURS * 3600)), PARENT, _settings(coupling=1), t0, tf)
    B = ens["branch_index"]
    ci = _decisions(ps["local"])["couplingIndexI"][ps["status"] == 0]
    assert (ci + 1 == B).any() and (ci + 1 <= B).all() and (ci >= 1).any()


def _sky_local(n, seed=5):
    rs = np.random.RandomState(seed)
    local = []
    for i in range(n):
        lp = abi.default_local()
        lp.lat, lp.lon = 60.0 + 8.0 * rs.rand(), 20.0 + 10.0 * rs.rand()
        lp.sky_view = 1.0 if i % 4 == 0 else 0.35 + 0.6 * rs.rand()
        local.append(lp)
    return local, np.ascontiguousarray(rs.uniform(0.0, 35.0, (n, 360)))


def test_sky_view_with_horizons():
    src, t0, tf = base_sources()
    local, hz = _sky_local(S)
    # the sun is up over part of the members' leg: the run starts at midnight, the branch lies at 06:00
    compare(src, member_source(len(PARENT), hourly(OBS_HOURS * 3600)), PARENT, _settings(), t0, tf, local=local, horizons=hz)


def test_observations_on_per_point_axes():
    src, t0, tf = base_sources()
    shared = [src[0], dh.ragged(src[1])]
    compare(shared, member_source(len(PARENT), hourly(OBS_HOURS * 3600)), PARENT, _settings(), t0, tf)
    compare(shared, member_source(len(PARENT), hourly(OBS_HOURS * 3600)), PARENT, _settings(coupling=1), t0, tf)


def test_gridded_shared_source():
    src, simlen, t0, tf = gh.grid_scenario(S, hours=HOURS, obs_hours=OBS_HOURS)
    assert simlen == L
    compare(src, member_source(len(PARENT), hourly(OBS_HOURS * 3600)), PARENT, _settings(), t0, tf)


def test_branch_between_two_kept_rows_and_other_positions():
    src, t0, tf = base_sources()
    mem = member_source(len(PARENT), hourly(OBS_HOURS * 3600 + 7 * 60))
    ens, _, _ = compare(src, mem, PARENT, _settings(), t0, tf)
    assert ens["branch_index"] == 734 and ens["branch_index"] % 20 != 0 and ens["first_row"] == 37
    compare(src, mem, PARENT, _settings(), t0, tf, position=0)   # the shared forecast wins over the members' own
    compare(src, mem, PARENT, _settings(), t0, tf, position=2)   # the members' own wins over the observations


@pytest.mark.parametrize("which", ["B = 1", "B = L - 1"])
def test_branch_at_either_end(which):
    src, t0, tf = base_sources()
    if which == "B = 1":
        times = np.concatenate([[START + 30], hourly(3600)])
    else:
        times = START + 30 * (L - 1) + np.array([0, 3600], np.int64)
    ens, pm, ps = compare(src, member_source(len(PARENT), times), PARENT, _settings(), t0, tf)
    assert ens["branch_index"] == (1 if which == "B = 1" else L - 1)
    if which == "B = 1":
        # a station that a hole behind the branch rejects has members the members' own source completes
        assert ((ps["status"][PARENT] != 0) & (pm["status"] == 0)).any()
        assert ens["first_row"] == 1
    else:
        assert ens["first_row"] == 54 and ens["members"]["tsurf"].shape[1] == 1


def test_station_that_fails_during_the_analysis_takes_its_members_along():
    src, t0, tf = base_sources()
    fc = driver.RawSource(src[0].times, {k: v.copy() for k, v in src[0].fields.items()})
    bad = 10
    assert COUNTS[bad] >= 1
    fc.fields["sw"][bad, 4] = 5000.0    # hour 3: CheckValues' limit is 4000
    ens, pm, ps = compare([fc, src[1]], member_source(len(PARENT), hourly(OBS_HOURS * 3600)), PARENT, _settings(), t0, tf)
    assert ps["status"][bad] == 0 and (pm["status"][PARENT == bad] == 0).all()
    row = ps["tsurf"][bad]
    assert row[0] != -9999.0 and (row[20:] == -9999.0).all()          # it stopped during the analysis
    assert (ens["members"]["tsurf"][PARENT == bad] == -9999.0).all()   # and so did its members


def test_one_station_one_member():
    src, simlen, t0, tf = dh.scenario(1, hours=HOURS, obs_hours=OBS_HOURS)
    compare(src, member_source(1, hourly(OBS_HOURS * 3600)), np.zeros(1, np.int32), _settings(), t0, tf)


def test_257_stations_one_member_each():
    src, simlen, t0, tf = dh.scenario(257, hours=HOURS, obs_hours=OBS_HOURS)
    parent = np.arange(257, dtype=np.int32)
    compare(src, member_source(257, hourly(OBS_HOURS * 3600)), parent, _settings(), t0, tf)
    assert driver.rslib.load().rs_driver_last_tiles() == 5   # tiles of 64 stations


@pytest.mark.parametrize("series", [True, False])
def test_stats_and_probs_equal_the_definitions_on_the_plain_members_rows(series):
    src, t0, tf = base_sources()
    stats = ensstats.EnsSpec(S, 5, (0.1, 0.5, 0.9))
    probs = ensprob.ProbSpec(S, 8, (ensprob.Condition.where(tsurf=(None, -1.0)),
                                    ensprob.Condition.where(tsurf=(None, 0.0), water=(0.01, None)),
                                    ensprob.Condition.where(ice=(0.0, None))))
    ens, pm, _ = compare(src, member_source(len(PARENT), hourly(OBS_HOURS * 3600)), PARENT, _settings(), t0, tf,
                         stats=stats, probs=probs, series=series)
    first = ens["first_row"]
    rows = [pm[k][:, first:] for k in driver.OUT_FIELDS]   # tsurf, snow, water, ice, deposit, ice2
    want = ensstats.reduce_members(*rows, PARENT, stats)
    assert ens["stats"].shape == want.shape and np.array_equal(_u64(ens["stats"]), _u64(want))
    wantp, _ = ensprob.reduce_members_prob(*rows, None, PARENT, probs)
    assert ens["probs"].shape == wantp.shape and np.array_equal(_u64(ens["probs"]), _u64(wantp))
    assert wantp[..., 1:].any() and (wantp[:, COUNTS == 0] == 0).all() and (want[:, COUNTS == 0, 2:] == -9999.0).all()


# ---- refusals: each with its reason, the arrays passed in untouched -----------------------------------------------

def _guarded(n_tail):
    _, n_out = driver.output_rows(_settings())
    out = {}
    for name, n, w in (("stations", S, n_out), ("members", len(PARENT), n_tail)):
        out[name] = {k: np.full((n, w), GUARD) for k in driver.OUT_FIELDS}
        out[name].update(status=np.full(n, 77, np.int32), missing_index=np.full(n, 77, np.int32))
    return out


def _refused(match, shared=None, mem=None, parent=None, s=None, **kw):
    src, t0, tf = base_sources()
    shared = src if shared is None else shared
    mem = member_source(len(PARENT), hourly(OBS_HOURS * 3600)) if mem is None else mem
    s = _settings() if s is None else s
    parent = PARENT if parent is None else parent
    try:
        n_tail = driver.member_rows(s, t0, int(np.asarray(mem.times).flat[0]))[2]
    except ValueError:
        n_tail = 0
    out = _guarded(n_tail)
    local = driver._locals(S, None)
    before = bytes(local)
    with pytest.raises(RuntimeError, match=match):
        driver.run_ensemble(shared, mem, parent, s, abi.default_parameters(), t0, tf, local=local, out=out, **kw)
    assert bytes(local) == before
    for part in out.values():
        for k, a in part.items():
            assert (a == (77 if a.dtype == np.int32 else GUARD)).all(), k


def test_refusals_of_the_member_source():
    n = len(PARENT)
    base = member_source(n, hourly(OBS_HOURS * 3600))
    _refused("time axis shared by all members", mem=driver.RawSource(np.tile(base.times, (n, 1)), base.fields))
    _refused("must not be an observation source", mem=driver.RawSource(base.times, base.fields, True))
    _refused("must carry no tsurfobs", mem=driver.RawSource(base.times, dict(base.fields, tsurfobs=base.fields["tair"])))
    _refused("times\\[0\\] > start_time is required", mem=member_source(n, hourly(0)))
    _refused("times\\[0\\] > start_time is required", mem=member_source(n, hourly(-3600)))
    beyond = member_source(n, START + 30 * (L - 1) + 1 + np.array([0, 3600], np.int64))
    _refused(f"B = {L} outside \\[1, SimLen - 1 = {L - 1}\\]", mem=beyond)


def test_refusals_of_parent_position_sources_and_device():
    src, _, _ = base_sources()
    down = PARENT.copy()
    down[40] = down[39] - 1
    _refused(f"member 40: parent {down[40]} below member 39's parent {down[39]}", parent=down)
    out_of = PARENT.copy()
    out_of[-1] = S
    _refused(f"member {len(PARENT) - 1}: parent {S} outside", parent=out_of)
    _refused("more than RS_MAX_SOURCES", shared=[src[0], src[0], src[1], src[1]])
    _refused("position = 3 outside \\[0, n_sources = 2\\]", position=3)
    _refused("position = -1 outside", position=-1)
    _refused("device < 0", device=-1)


def test_refusal_of_a_coupling_window_that_reaches_the_branch():
    # the members' own source starts at hour 5, the road temperature observations go on to hour 6
    mem = member_source(len(PARENT), hourly(5 * 3600))
    _refused("station \\d+: couplingIndexI \\+ 1 = \\d+ > B = 600", mem=mem, s=_settings(coupling=1))


def test_refusal_of_a_station_with_more_members_than_a_tile(monkeypatch):
    monkeypatch.setenv("ROADSURF_HIP_TILE_POINTS", "4")
    first = int(np.nonzero(COUNTS > 4)[0][0])
    _refused(f"station {first} has 5 members, more than a tile of 4 points holds")


def test_refusals_of_stats_and_probs():
    first = int(np.nonzero(COUNTS > 3)[0][0])
    _refused(f"station {first} has {COUNTS[first]} members, more than max_members = 3", stats=ensstats.EnsSpec(S, 3))
    _refused("ngroups = n_stations = 37", stats=ensstats.EnsSpec(S + 1, 5))
    _refused(f"station {first} has {COUNTS[first]} members, more than max_members = 3",
             probs=ensprob.ProbSpec(S, 3, (ensprob.Condition.where(tsurf=(None, 0.0)),)))
    _refused("ngroups = n_stations = 37", probs=ensprob.ProbSpec(S - 1, 5, (ensprob.Condition.where(tsurf=(None, 0.0)),)))
    _refused("a condition uses the deficit", probs=ensprob.ProbSpec(S, 5, (ensprob.Condition.where(deficit=(None, 0.0)),)))
