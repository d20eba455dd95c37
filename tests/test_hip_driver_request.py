"""GPU: rs_driver_run_request against the six older entries of the driver, which are wrappers that fill the same
RsDriverRequest: the same members set give the same bits in every array a call writes, from one device and from the
fan-out, and a refused member is refused with the older entry's return code and message."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import driver_helpers as dh
import grid_helpers as gh
from roadsurf_amd import abi, driver, episodes, groups, lib, summary

pytestmark = pytest.mark.gpu

N, HOURS, SEED = 203, 12, 7
NGROUPS = 4
GUARD = 777.0
MEMBERS = ("summary", "groups", "kept", "episodes")
#: entry -> (takes `grids`, the members of the request its signature can express, in its argument order)
LEGACY = {
    "rs_driver_run": (False, ()),
    "rs_driver_run_summary": (False, MEMBERS[:1]),
    "rs_driver_run_groups": (False, MEMBERS[:2]),
    "rs_driver_run_grid": (True, MEMBERS[:2]),
    "rs_driver_run_kept": (True, MEMBERS[:3]),
    "rs_driver_run_episodes": (True, MEMBERS[:4]),
}


def _settings(L):
    s = abi.default_settings(L)
    s.outputStep = 7
    s.use_relaxation = 1
    s.use_coupling = 1
    return s


def _u64(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a   # (the int32 arrays compare exactly as they are)


@functools.lru_cache(maxsize=None)
def _case(gridded):
    """(sources, settings, start, forecast_time, (first, last) of the forecast rows, specs) of the driver tests' small
    scenario, per point or with its forecast delivered as fields.  The specs are built as tests/test_hip_summary.py,
    test_hip_groups.py and test_hip_episodes.py build theirs, their thresholds placed in the forecast rows of one
    plain call of the case: about half of the points cross them."""
    src, L, t0, tf = (gh.grid_scenario if gridded else dh.scenario)(N, hours=HOURS, seed=SEED)
    s = _settings(L)
    first, last = driver.forecast_rows(s, t0, tf)
    res = driver.run(src, s, abi.default_parameters(), t0, tf, deficit=True)
    ok = res["status"] == 0
    assert 0 < int((~ok).sum()) < N // 2   # rejected stations: the blanking is part of every comparison below
    valid = res["tsurf"][ok][:, first:]
    th = summary.SummarySpec(float(np.median(valid.min(axis=1))), (0.0,) * 5)
    edges = tuple(float(x) for x in np.quantile(valid, (0.1, 0.3, 0.5, 0.7, 0.9)))
    spec = {"summary": th, "groups": groups.GroupSpec(summary.SummarySpec(float(np.median(valid)), (0.0,) * 5), NGROUPS, edges),
            "episodes": episodes.EpisodeSpec.where(tsurf=(None, float(np.quantile(valid, 0.5))),
                                                   deficit=(None, float(np.quantile(res["deficit"][ok][:, first:], 0.7))),
                                                   peak="deficit", max_episodes=2)}
    assert episodes.needs_deficit(spec["episodes"])
    return src, s, t0, tf, (first, last), spec


class Call:
    """The arguments of one call on a case - its input, fresh output arrays filled with a guard, and the wanted members
    over arrays of their own - and what the call left in them."""

    def __init__(self, gridded, members, rows=None, spec=None):
        src, self.s, t0, tf, forecast, specs = _case(gridded)
        spec = dict(specs, **(spec or {}))
        rows = dict({m: forecast for m in MEMBERS}, **(rows or {}))
        self.p = abi.default_parameters()
        cal = driver.calendar(t0, self.s.SimLen, int(self.s.DTSecs))
        self.inp, self.grids, self.keep = driver.make_grid_input(src, t0, tf, cal)
        _, n_out = driver.output_rows(self.s)
        self.local = driver._locals(N, None)
        self.arrays = {k: np.full((N, n_out), GUARD) for k in driver.OUT_FIELDS}
        self.arrays.update(status=np.full(N, 77, np.int32), missing_index=np.full(N, 77, np.int32))
        self.out = driver.RsDriverOutput()
        self.out.n_out = n_out
        for k in driver.OUT_FIELDS:
            setattr(self.out, k, self.arrays[k].ctypes.data_as(abi.c_double_p))
        self.out.status = self.arrays["status"].ctypes.data_as(abi.c_int32_p)
        self.out.missing_index = self.arrays["missing_index"].ctypes.data_as(abi.c_int32_p)
        self.member = {}
        a = self.arrays
        if "summary" in members:
            a["summary"] = np.full((N, lib.RS_SUM_COLS), GUARD)
            self.member["summary"] = driver.RsDriverSummary(lib.summary_spec(spec["summary"]), *rows["summary"],
                                                            a["summary"].ctypes.data_as(abi.c_double_p))
        if "groups" in members:
            self.gid = np.random.RandomState(4).randint(0, NGROUPS, N).astype(np.int32)
            nrows = max(rows["groups"][1] - rows["groups"][0] + 1, 1)
            a["series"] = np.full((nrows, NGROUPS, groups.cols(specs["groups"])), GUARD)
            self.member["groups"] = driver.RsDriverGroups(lib.group_spec(spec["groups"]), self.gid.ctypes.data_as(abi.c_int32_p),
                                                          *rows["groups"], a["series"].ctypes.data_as(abi.c_double_p))
        if "kept" in members:
            k = self.member["kept"] = driver.RsDriverKept()
            for f, name in enumerate(driver.MERGED_FIELDS):
                a["kept_" + name] = np.full((N, n_out), GUARD)
                k.merged[f] = a["kept_" + name].ctypes.data_as(abi.c_double_p)
            a["deficit"] = np.full((N, n_out), GUARD)
            k.deficit = a["deficit"].ctypes.data_as(abi.c_double_p)
        if "episodes" in members:
            a["episodes"] = np.full((N, episodes.cols(specs["episodes"])), GUARD)
            self.member["episodes"] = driver.RsDriverEpisodes(lib.episode_spec(spec["episodes"]), *rows["episodes"],
                                                              a["episodes"].ctypes.data_as(abi.c_double_p))

    def _ref(self, m):
        return C.byref(self.member[m]) if m in self.member else None

    def legacy(self, entry, device=0):
        takes_grids, members = LEGACY[entry]
        assert set(self.member) <= set(members) and (takes_grids or self.grids is None), entry
        L_ = driver._bind(lib.load())
        args = [C.byref(self.inp)] + ([self.grids] if takes_grids else []) + \
            [C.byref(self.s), C.byref(self.p), self.local, C.byref(self.out)] + [self._ref(m) for m in members] + [device]
        return self._done(getattr(L_, entry)(*args))

    def request(self, device=0, how="members"):
        """how: "members" a request with the members set and the rest NULL; "null" no request at all"""
        L_ = driver._bind(lib.load())
        req = driver.RsDriverRequest(grids=self.grids)
        for m, q in self.member.items():
            setattr(req, m, C.pointer(q))
        assert how == "members" or (how == "null" and not self.member and self.grids is None)
        return self._done(L_.rs_driver_run_request(C.byref(self.inp), C.byref(self.s), C.byref(self.p), self.local,
                                                   C.byref(self.out), C.byref(req) if how == "members" else None, device))

    def _done(self, rc):
        self.rc, self.error = rc, lib.last_error()
        return self

    def untouched(self):
        return all((a == (77 if a.dtype == np.int32 else GUARD)).all() for a in self.arrays.values())


#: what read_input decides per point, and where it leaves it in LocalParameters
DECISIONS = {"tair_relax": "f8", "VZ_relax": "f8", "RH_relax": "f8", "couplingIndexI": "i4", "couplingTsurf": "f8",
             "InitLenI": "i4"}


def _decisions(local):
    dt = np.dtype({"names": list(DECISIONS), "formats": list(DECISIONS.values()),
                   "offsets": [getattr(abi.LocalParameters, f).offset for f in DECISIONS],
                   "itemsize": C.sizeof(abi.LocalParameters)})
    return np.frombuffer(local, dtype=dt)


def _assert_same(a, b, what):
    """every array either call wrote, and the six decisions of every local[p], on the bits"""
    assert (a.rc, b.rc) == (0, 0), (what, a.error, b.error)
    assert set(a.arrays) == set(b.arrays), what
    for k in a.arrays:
        assert a.arrays[k].shape == b.arrays[k].shape and np.array_equal(_u64(a.arrays[k]), _u64(b.arrays[k])), (what, k)
    da, db = _decisions(a.local), _decisions(b.local)
    for f in DECISIONS:
        assert np.array_equal(_u64(da[f]), _u64(db[f])), (what, f)


@functools.lru_cache(maxsize=None)
def _fullest_request():
    """the request with every member set, on the gridded case, from one device: made once, left unchanged"""
    r = Call(True, MEMBERS).request()
    assert r.rc == 0, r.error
    for a in r.arrays.values():
        a.setflags(write=False)
    return r


@pytest.mark.parametrize("entry", list(LEGACY))
def test_a_legacy_entry_equals_the_request_with_its_members(entry):
    """2a: the fullest argument set the entry's signature can express, against the request with the same members."""
    takes_grids, members = LEGACY[entry]
    old = Call(takes_grids, members).legacy(entry)
    new = _fullest_request() if entry == "rs_driver_run_episodes" else Call(takes_grids, members).request()
    _assert_same(old, new, entry)
    assert not (old.arrays["status"] == 77).any() and 0 < int((old.arrays["status"] != 0).sum()) < N // 2
    rejected = old.arrays["status"] != 0
    assert (old.arrays["tsurf"][rejected] == -9999.0).all() and (old.arrays["tsurf"][~rejected] > -100.0).all()
    # (what keeps the comparison from passing on arrays nobody wrote or that say nothing)
    for k, a in old.arrays.items():
        assert not (a == GUARD).any(), (entry, k)
    if "summary" in members:
        crossed = int((old.arrays["summary"][~rejected, summary.FIRST_BELOW] > 0).sum())
        assert crossed >= N // 10 and int((~rejected).sum()) - crossed >= N // 10
    if "groups" in members:
        assert (old.arrays["series"][:, :, groups.COUNT] > 0).all() and (old.arrays["series"][:, :, groups.BINS:] > 0).any()
    if "episodes" in members:
        assert (old.arrays["episodes"][~rejected, 0] > 0).any() and (old.arrays["episodes"][~rejected, 0] == 0).any()


def test_no_request_and_an_empty_request_are_rs_driver_run():
    """2b"""
    old = Call(False, ()).legacy("rs_driver_run")
    _assert_same(old, Call(False, ()).request(how="null"), "request NULL")
    _assert_same(old, Call(False, ()).request(), "five NULL members")


def test_the_fullest_request_from_the_fan_out(monkeypatch):
    """2c: two blocks on one device.  The group series too are compared exactly: the blocks' cells merge by minimum,
    maximum and sums of integers."""
    one = _fullest_request()
    monkeypatch.setenv("ROADSURF_HIP_DEVICES", "0,0")
    monkeypatch.setenv("ROADSURF_HIP_MIN_SHARD", "64")
    fan = Call(True, MEMBERS).request(device=-1)
    assert lib.load().rs_last_fanout() == 2
    _assert_same(one, fan, "fan-out")


#: the first forecast row and the number of kept rows of the case: 6 h of observations, every 14th of 1 441 indices
_FIRST, _N_OUT = 52, 103


def _refusal_cases():
    first, n_out = _FIRST, _N_OUT
    bad_group = groups.GroupSpec(summary.SummarySpec(), 0, ())
    yield "summary rows behind n_out", "rs_driver_run_summary", False, ("summary",), dict(rows={"summary": (first, n_out)})
    yield "summary without its array", "rs_driver_run_summary", False, ("summary",), dict(null=("summary", "summary"))
    yield "group rows behind n_out", "rs_driver_run_groups", False, ("groups",), dict(rows={"groups": (first, n_out)})
    yield "a bad group spec", "rs_driver_run_groups", False, ("groups",), dict(spec={"groups": bad_group})
    yield "groups without series", "rs_driver_run_groups", False, ("groups",), dict(null=("groups", "series"))
    yield "groups without group", "rs_driver_run_groups", False, ("groups",), dict(null=("groups", "group"))
    for rows in ((0, n_out), (5, 4), (-1, 4)):
        yield "episode rows %d..%d" % rows, "rs_driver_run_episodes", False, ("episodes",), dict(rows={"episodes": rows})
    for change in (dict(peak=7), dict(min_rows=0)):
        yield "a bad episode spec %s" % change, "rs_driver_run_episodes", False, ("episodes",), dict(change=change)
    yield "episodes without their array", "rs_driver_run_episodes", False, ("episodes",), dict(null=("episodes", "episodes"))
    yield "a gridded source with per-point axes", "rs_driver_run_grid", True, (), dict(per_point_axes=True)
    # two faults at once: the one that is reported is the same one
    yield "bad episodes, groups and summary together", "rs_driver_run_episodes", False, ("summary", "groups", "episodes"), \
        dict(rows={"summary": (first, n_out), "groups": (5, 4), "episodes": (-1, 4)})


@pytest.mark.parametrize("what,entry,gridded,members,fault", list(_refusal_cases()), ids=[c[0] for c in _refusal_cases()])
def test_a_refusal_is_the_legacy_entrys(what, entry, gridded, members, fault):
    """2d: the same bad argument at the older entry and in a request: the same return code, the same message (it
    names the older entry), and nothing written."""
    src, s, t0, tf, forecast, specs = _case(gridded)
    assert (forecast[0], driver.output_rows(s)[1]) == (_FIRST, _N_OUT)
    spec = dict(fault.get("spec", {}))
    if "change" in fault:
        spec["episodes"] = dataclasses.replace(specs["episodes"], **fault["change"])
    got = []
    for via in ("legacy", "request"):
        c = Call(gridded, members, rows=fault.get("rows"), spec=spec)
        if "null" in fault:
            setattr(c.member[fault["null"][0]], fault["null"][1], None)
        if fault.get("per_point_axes"):
            tpp = np.ascontiguousarray(np.tile(src[0].times, (N, 1)))
            c.inp.sources[0].times = tpp.ctypes.data_as(driver.c_int64_p)
            c.inp.sources[0].times_per_point = 1
        got.append(c.legacy(entry) if via == "legacy" else c.request())
        assert c.rc != 0 and c.untouched(), (what, via, c.error)
    assert (got[0].rc, got[0].error) == (got[1].rc, got[1].error), what
    assert got[0].error.startswith("rs_driver"), what
    if members:
        assert got[0].error.startswith("rs_driver_run_" + ("episodes" if "episodes" in members else members[0])), what
