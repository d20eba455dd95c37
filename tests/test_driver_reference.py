"""CPU: the driver data path against the reference's own C++ driver.

``oracle/_ref/libroadrunner_ref.so`` is the reference's example driver as it stands (all twelve sources of
examples/example1/src, strict flags, over the stand-in JSON / fmt headers of oracle/shim) with a small C surface
(oracle/driver_ref_harness.cpp).  A seeded generator writes whole driver inputs as files; the reference opens them,
and so do ``roadrunner.prepare`` -> ``driver.make_input`` -> ``oracle/driver_oracle.c``.  Everything is compared bit
for bit: the checker's merged series, decisions and statuses, the Python front end's settings, parameters, station
list, sky view and calendar, and - through the reference's runsimulation - whole runs.

The conditions in ``test_the_cases_are_not_vacuous`` are asserted on the reference's results alone."""
import numpy as np
import pytest

import driver_helpers as dh
import driver_ref_helpers as rh
from roadsurf_amd import abi, driver, roadrunner

R = rh.REJECTS
SPECS = [
    rh.Spec(seed=1, n=28, relaxation=True, coupling=True, rejects=R[0:5]),
    rh.Spec(seed=2, n=32, zone="eet", order=("obs", "fc"), relaxation=True, coupling=True, sky="both", params=True,
            rejects=R[5:9]),
    rh.Spec(seed=3, n=24, order=("fc", "obs", "obs2"), relaxation=True, coupling=True, cli_time=True, sky="sky",
            step=20, rejects=R[9:13]),
    rh.Spec(seed=4, n=40, zone="eet", order=("fc",), model=False, sky="hz", rejects=R[0:4]),
    rh.Spec(seed=5, n=30, order=("fc", "obs"), coupling=True, dtsecs=45, rejects=R[4:8]),
    rh.Spec(seed=6, n=26, zone="eet", order=("obs", "fc"), coupling=True, dtsecs=90, step=15, rejects=R[8:12]),
    rh.Spec(seed=7, n=36, order=("obs2", "fc", "obs"), relaxation=True, coupling=True, shared=True,
            coupling_minutes=None, rejects=("prec_hole", "vz_hole", "no_hum")),
    rh.Spec(seed=8, n=34, zone="eet", order=("fc", "obs"), relaxation=True, coupling=True, params=True, step=None,
            rejects=(R[12], R[1], R[6])),
]
IDS = [f"seed{s.seed}" for s in SPECS]


@pytest.fixture(scope="module")
def views(tmp_path_factory):
    """Every spec written, opened by the reference and by the project, once."""
    rh.require_reference()
    out = {}
    for spec in SPECS:
        tmp = tmp_path_factory.mktemp(f"seed{spec.seed}")
        with rh.timezone(rh.ZONES[spec.zone][0]):
            case = rh.make_case(tmp, spec)
            ref = rh.reference_view(case)
            singles = []
            if len(spec.order) > 1:
                for path in rh.single_source_configs(tmp, case):
                    one = rh.reference_view(dict(case, config=path))
                    first = {}
                    for row, sid in enumerate(one["ids"].tolist()):
                        first.setdefault(sid, row)
                    # that source's tair in the order of the whole run's stations (all missing where it has none)
                    singles.append(np.stack([one["merged"]["tair"][first[sid]] if sid in first
                                             else np.full(ref["simlen"], rh.M) for sid in ref["ids"].tolist()]))
            proj = rh.project_view(case)
        out[spec.seed] = {"case": case, "ref": ref, "proj": proj, "singles": singles, "tmp": tmp}
    return out


@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_front_end_settings_parameters_and_stations(views, spec):
    """roadrunner.make_settings / make_parameters / the station list against InputSettings.cpp, InputParameters.cpp,
    DataHandler::GetPointIDs / GetLocations."""
    v = views[spec.seed]
    ref, pc = v["ref"], v["proj"]["case"]
    assert (pc.forecast_time, pc.start_time, pc.end_time) == (ref["forecast_time"], ref["start_time"], ref["end_time"])
    for name in rh.SETTING_INTS:
        assert getattr(pc.settings, name) == ref["settings"][name], name
    for name in rh.SETTING_REALS:
        assert rh.same_bits(getattr(pc.settings, name), ref["settings"][name]), name
    mine = np.array([getattr(pc.params, name) for name in abi.INPUT_PARAMETER_NAMES])
    bad = [n for n, a, b in zip(abi.INPUT_PARAMETER_NAMES, mine, ref["parameters"]) if not rh.same_bits(a, b)]
    assert not bad, bad
    assert np.array_equal(pc.ids, ref["ids"])
    assert rh.same_bits(pc.lat, ref["lat"]) and rh.same_bits(pc.lon, ref["lon"])
    if spec.cli_time:  # roadrunner.cpp's own reading of -t
        with rh.timezone(v["case"]["tz"]):
            t = rh.Ref.lib().rr_ref_cli_time(b"20240110T0300", v["case"]["config"].encode())
            assert t == roadrunner.parse_local_time("20240110T0300", "-t") == v["case"]["cli_time"]


@pytest.mark.parametrize("spec", SPECS, ids=IDS)
def test_checker_read_input_equals_the_reference(views, spec):
    """oracle/driver_oracle.c over roadrunner.prepare's sources against read_input of the reference, per station."""
    v = views[spec.seed]
    ref, pc, ri = v["ref"], v["proj"]["case"], v["proj"]["read_input"]
    n = len(ref["ids"])
    assert n == spec.n and ri["status"].shape == (n,)
    assert np.all(ri["status"] != 7)
    assert np.array_equal(ri["status"] == 0, ref["success"])
    for name in driver.MERGED_FIELDS:
        a, b = ri["merged"][name], ref["merged"][name]
        bad = [int(ref["ids"][k]) for k in range(n) if not rh.same_bits(a[k], b[k])]
        assert not bad, (name, bad)
    for k in range(n):  # status and missing_index from the reference's own returned data
        assert (int(ri["status"][k]), int(ri["missing_index"][k])) == rh.scan_status(ref["merged"], k), int(ref["ids"][k])
        assert (rh.scan_status(ref["merged"], k)[0] == 0) == bool(ref["success"][k])
    mine = rh.local_fields(ri["local"])
    for name in rh.LOCAL_INTS:
        assert np.array_equal(mine[name], ref["local"][name]), name
    for name in rh.LOCAL_REALS:
        assert rh.same_bits(mine[name], ref["local"][name]), name
    # sky view and horizons (SkyView.cpp), PrecipitationForm, calendar
    assert np.all(ref["n_horizons"] == 360)
    hz = pc.horizons if pc.horizons is not None else np.zeros((n, 360))
    assert rh.same_bits(hz, ref["horizons"])
    assert np.all(ref["precphase"] == -9999)
    for name in driver.CALENDAR:
        got = ref["cal"][name]
        unset = np.all(got == -9999, axis=1)  # a station without a time stamp in any source keeps InputData's
        assert not np.any(unset & ref["success"])
        assert np.array_equal(got[~unset], np.broadcast_to(pc.cal[name], got.shape)[~unset]), name


def test_the_cases_are_not_vacuous(views):
    """On the reference's results alone."""
    total = accepted = 0
    statuses, placements = set(), set()
    for spec in SPECS:
        v = views[spec.seed]
        ref = v["ref"]
        n = len(ref["ids"])
        total += n
        accepted += int(ref["success"].sum())
        for k in range(n):
            statuses.add(rh.scan_status(ref["merged"], k)[0])
        if spec.coupling:
            cl = int(ref["settings"]["coupling_minutes"] * 60 / ref["settings"]["DTSecs"])
            ci = ref["local"]["couplingIndexI"]
            obs = ref["merged"]["tsurfobs"]
            for k in np.nonzero(ref["success"])[0]:
                if ci[k] == cl:
                    placements.add("at")
                elif ci[k] > cl:
                    placements.add("after")
                elif ci[k] == -9999 and np.any(obs[k] > -100):
                    placements.add("before")
        if len(spec.order) > 1:  # a tair series with values of two sources
            tair = ref["merged"]["tair"]
            singles = v["singles"]
            assert len(singles) == len(spec.order) and all(s.shape == tair.shape for s in singles)
            both = 0
            for k in range(n):
                owners = set()
                for j, s in enumerate(singles):
                    others = [o for i, o in enumerate(singles) if i != j]
                    mine = (tair[k] == s[k]) & (s[k] > -100) & np.all([o[k] != s[k] for o in others], axis=0)
                    if mine.any():
                        owners.add(j)
                both += len(owners) >= 2
            assert both >= 1, spec.seed
        if spec.relaxation:  # observation sources ending at different indices, one station without any
            init = ref["local"]["InitLenI"][ref["success"]]
            assert len(set(init.tolist())) >= 3
            assert np.any(ref["local"]["tair_relax"][ref["success"]] == rh.M)
    assert accepted >= 0.6 * total, (accepted, total)
    assert statuses >= {0, 1, 2, 3, 4, 5, 6}, statuses
    assert placements == {"before", "at", "after"}, placements


def test_two_zones_and_the_settings_cases(views):
    """What the generator promises about the settings side, read back from the reference."""
    s = {spec.seed: views[spec.seed]["ref"] for spec in SPECS}
    assert s[1]["simlen"] == 721 and s[5]["simlen"] == 481 and s[6]["simlen"] == 241
    assert s[4]["settings"]["outputStep"] == 60  # no model object: output.step is not read (InputSettings.cpp:90-94)
    assert s[3]["settings"]["outputStep"] == 20 and s[7]["settings"]["coupling_minutes"] == 180
    assert s[1]["settings"]["coupling_minutes"] == 60
    # the run of the second zone crosses the change of 31 March: local hours 1, 2, 4, 5, ...
    hours = s[2]["cal"]["hour"][np.nonzero(s[2]["success"])[0][0]]
    assert 3 not in set(hours.tolist()) and {2, 4} <= set(hours.tolist())
    assert s[2]["start_time"] == 1711839600  # 2024-03-30 23:00 UTC


E2E = [SPECS[3], SPECS[0], SPECS[1]]  # plain, relaxation + coupling, sky view (+ both, + parameters)


@pytest.mark.parametrize("spec", E2E, ids=["plain", "relaxation_coupling", "sky_view"])
def test_whole_run_equals_the_reference_driver(views, spec):
    """read_input (checker) + the reference's Fortran + save_output's rule against the reference's own read_input +
    runsimulation, at every step-th index."""
    v = views[spec.seed]
    pc = v["proj"]["case"]
    with rh.timezone(v["case"]["tz"]):
        want = rh.reference_run(v["case"])
    got = dh.oracle_run("ref_cpl", pc.sources, pc.settings, pc.params, pc.start_time, pc.forecast_time,
                        rh.copy_local(pc.local), pc.cal, pc.horizons)
    step = got["step"]
    assert step == int(v["ref"]["settings"]["outputStep"] * 60 / v["ref"]["settings"]["DTSecs"])
    assert np.array_equal(got["status"] == 0, want["success"]) and want["success"].sum() >= 10
    for name in driver.OUT_FIELDS:
        assert rh.same_bits(got[name], want[name][:, ::step]), name
        assert np.all(want[name][~want["success"]] == -9999.0)
    assert np.any(want["tsurf"][want["success"]][:, ::step] != -9999.0)


def test_observation_at_the_last_index_is_status_7():
    """An air-temperature observation at the last simulation index: GetLatestObsIndex returns SimLen and the
    reference reads data.tair[SimLen] (roadrunner.cpp:241-247).  Not run through the reference; the project's
    answer is status 7."""
    t0 = dh.START
    L = 121
    tt = [t0, t0 + 3600, t0 + 7200]
    fc = driver.RawSource(np.asarray(tt, np.int64), {k: np.full((1, 3), v) for k, v in
                          dict(tair=1.0, rhz=80.0, prec=0.0, sw=0.0, lw=300.0, vz=2.0).items()})
    ob = driver.RawSource(np.asarray(tt, np.int64), {"tair": np.full((1, 3), 2.0)}, True)
    s = abi.default_settings(L)
    s.use_relaxation = 1
    r = dh.oracle_read_input([fc, ob], s, t0, t0)
    assert r["status"][0] == 7 and r["local"][0].InitLenI == L
