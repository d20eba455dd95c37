"""CPU: the rules `python -m roadsurf_amd.roadrunner` takes from the reference's driver program, each against values
worked out by hand from the lines it mirrors (examples/example1/src: roadrunner.cpp, InputSettings.cpp,
InputParameters.cpp, JsonTools.cpp, SkyView.cpp, DataHandler.cpp, JsonSource.cpp).  Nothing here touches a GPU:
the parsing functions and the writer directly, and run_config / main only where they stop before rs_driver_run."""
import json
import os
import time

import numpy as np
import pytest

from roadsurf_amd import abi, driver
from roadsurf_amd import roadrunner as rr

GOLDEN_CONFIG = os.path.join(os.path.dirname(__file__), "golden", "roadrunner_example_config.json")
T0 = 1704844800  # 2024-01-10 00:00 UTC
FT = T0 + 48 * 3600  # 2024-01-12 00:00 UTC


@pytest.fixture
def tz(monkeypatch):
    """Set TZ for mktime / localtime (TZ=UTC unless a test asks for another zone)."""
    def set_tz(name):
        monkeypatch.setenv("TZ", name)
        time.tzset()
    set_tz("UTC")
    yield set_tz
    monkeypatch.undo()
    time.tzset()


def _write(path, obj):
    with open(path, "w") as fh:
        fh.write(obj if isinstance(obj, str) else json.dumps(obj))
    return str(path)


def _station(sid, lat, lon, stamps, **vars_):
    st = {"statId": sid, "lat": lat, "lon": lon, "time": stamps}
    st.update({k.replace("_", " "): v for k, v in vars_.items()})
    return st


def _stamps(t0, n, dt):
    return [time.strftime("%Y-%m-%d %H:%M", time.gmtime(t0 + i * dt)) for i in range(n)]


def _config(tmp_path, **over):
    cfg = {"time": {"analysis": 1, "forecast": 1},
           "input": [{"name": "fc", "path": str(tmp_path / "fc.json"), "type": "json", "source": "forecast"}],
           "output": {"filename": str(tmp_path / "out.json")}}
    cfg.update(over)
    return _write(tmp_path / "config.json", cfg)


def _forecast(tmp_path, ids=(1, 2, 3), t0=FT - 7200, n=5):
    st = [_station(s, 60.0 + s, 25.0 - s, _stamps(t0, n, 3600), Temperature_2m=[1.0 * s] * n) for s in ids]
    return _write(tmp_path / "fc.json", st)


# ---- configuration file ----------------------------------------------------------------------------------------

def test_comments_are_stripped_from_the_reference_config(tz):
    """JsonTools.cpp:66-80: a default Json::CharReaderBuilder, which allows comments; example_config.json has
    `//` comments, read here as the reference's file stands."""
    cfg = rr.read_json(GOLDEN_CONFIG)
    assert cfg["missing_limit"] == 50
    assert cfg["time"] == {"analysis": 48, "forecast": 26}
    assert cfg["model"] == {"use_coupling": 1, "use_relaxation": 1, "DTSecs": 30.0}
    assert cfg["output"] == {"start": 0, "step": 60, "filename": "example_output.json"}
    assert [s["path"] for s in cfg["input"]] == ["example_forecast.json", "example_observations.json"]
    assert [s["source"] for s in cfg["input"]] == ["forecast", "observations"]
    # ... /* */ too, and nothing inside a string is a comment
    text = '/* a */ {"u": "http://x/*y*/", // b\n "v": /* c */ 2}'
    assert rr.parse_json(text, "t") == {"u": "http://x/*y*/", "v": 2}
    # the reference's own configuration under -t 20240112T0000: 48 h + 26 h at 30 s
    s, start, end = rr.make_settings(cfg, rr.get_forecast_time(cfg, rr.parse_local_time("20240112T0000", "-t")))
    assert (start, end) == (T0, T0 + 74 * 3600)
    assert (s.SimLen, s.DTSecs, s.use_coupling, s.use_relaxation, s.outputStep) == (8881, 30.0, 1, 1, 60)
    assert (s.NLayers, s.coupling_minutes, s.tsurfOutputDepth, s.force_tsurf) == (15, 180, -9999.9, 0)


def test_default_analysis_and_forecast_hours(tz):
    """InputSettings.cpp:46,59: 24 h back, 48 h ahead; SimLen = 1 + int(72 h / DTSecs)."""
    s, start, end = rr.make_settings({}, FT)
    assert (start, end) == (FT - 24 * 3600, FT + 48 * 3600)
    assert s.SimLen == 1 + 72 * 120 == 8641
    s, start, end = rr.make_settings({"time": {"analysis": 2}, "model": {"DTSecs": 45.0}}, FT)
    assert (start, end) == (FT - 7200, FT + 48 * 3600)
    assert s.SimLen == 1 + int(50 * 3600 / 45.0) == 4001
    # int(total / DTSecs) truncates: 3 h / 7000 s = 1.54 -> 2 steps
    s, _, _ = rr.make_settings({"time": {"analysis": 1, "forecast": 2}, "model": {"DTSecs": 7000}}, FT)
    assert s.SimLen == 2


def test_t_overrides_time_now(tz):
    """InputSettings.cpp:13-26: -t wins over time.now; both are local time (mktime)."""
    cfg = {"time": {"now": "20240115T1230"}}
    assert rr.get_forecast_time(cfg, FT) == FT
    assert rr.get_forecast_time(cfg) == 1705321800  # 2024-01-15 12:30 UTC
    tz("EET-2")  # two hours east of UTC, no daylight saving
    assert rr.get_forecast_time(cfg) == 1705321800 - 7200
    assert rr.parse_local_time("20240112T0000", "-t") == FT - 7200


def test_no_t_and_no_time_now_is_the_current_minute_made_the_reference_way(tz):
    """InputSettings.cpp:29-33: gmtime(now), seconds zeroed, mktime - the UTC fields read as local time."""
    now = FT + 125.7  # 2024-01-12 00:02:05.7 UTC
    assert rr.get_forecast_time({}, now=now) == FT + 120
    tz("EET-2")
    assert rr.get_forecast_time({"time": {"now": ""}}, now=now) == FT + 120 - 7200


def test_output_step_is_read_only_with_a_model_object(tz):
    """InputSettings.cpp:90-94 tests the `model` object, not `output`: the reference's slip, reproduced."""
    s, _, _ = rr.make_settings({"output": {"step": 30}}, FT)
    assert s.outputStep == 60
    s, _, _ = rr.make_settings({"output": {"step": 30}, "model": {}}, FT)
    assert s.outputStep == 30
    assert driver.output_rows(s) == (60, (s.SimLen + 59) // 60)


def test_coupling_minutes_at_or_below_zero_are_ignored(tz):
    """InputSettings.cpp:101-103."""
    for cm, want in ((0, 180), (-30, 180), (90, 90), (45.9, 45)):
        s, _, _ = rr.make_settings({"time": {"coupling_minutes": cm}}, FT)
        assert s.coupling_minutes == want, cm


def test_model_overrides_take_ints_and_doubles(tz):
    """InputSettings.cpp:83-88 with the two override overloads (JsonTools.cpp:8-39): asInt truncates a real and
    reads a bool as 0/1, asDouble takes an int."""
    s, _, _ = rr.make_settings({"model": {"use_coupling": True, "use_relaxation": 1.9, "DTSecs": 60,
                                          "tsurfOutputDepth": 0.05, "NLayers": 10.7,
                                          "couplingEffectReduction": 7200, "ignored": 3}}, FT)
    assert (s.use_coupling, s.use_relaxation, s.NLayers) == (1, 1, 10)
    assert (s.DTSecs, s.tsurfOutputDepth, s.couplingEffectReduction) == (60.0, 0.05, 7200.0)
    assert type(s.DTSecs) is float and s.SimLen == 1 + 72 * 60
    with pytest.raises(rr.ConfigError, match="DTSecs"):
        rr.make_settings({"model": {"DTSecs": "30"}}, FT)


def test_parameters_are_derived_from_dtsecs_then_overridden(tz):
    """InputParameters.cpp:9-21 first (with the settings' DTSecs), then the overrides of :41-108: an overridden
    MaxPormms leaves WDampLim / WWetLim / WWearLim / MaxWatmms at their values for MaxPormms = 1.0."""
    s, _, _ = rr.make_settings({"model": {"DTSecs": 60.0}}, FT)
    p = rr.make_parameters(s, {"MaxPormms": 2.5, "Albedo_Surroundings": 0.3, "MaxExtmms": 4, "sky_view_file": None})
    assert p.MaxPormms == 2.5 and p.Albedo_surroundings == 0.3 and p.MaxExtmms == 4.0
    assert p.WDampLim == 0.1 and p.WWetLim == 0.9 and p.WWearLim == 0.1 and p.MaxWatmms == 2.0
    assert p.MinPrecmm == 0.05 * 60.0 / 3600.0 and p.MinWatmms == 0.01 * 60.0 / 3600.0
    assert p.MinSnowmms == 0.1 * 60.0 / 3600.0 and p.MinDepmms == 0.01 * 60.0 / 3600.0
    assert p.MinIcemms == 0.05 * 60.0 / 3600.0
    # abi.default_parameters is InputParameters.cpp:13-21 as written
    d = abi.default_parameters(60.0)
    for k in abi.INPUT_PARAMETER_NAMES:
        if k not in ("MaxPormms", "Albedo_surroundings", "MaxExtmms"):
            assert getattr(p, k) == getattr(d, k), k
    # without a parameters object: the derived defaults; the missing-value constants are not overridable
    p0 = rr.make_parameters(s, None)
    assert bytes(p0) == bytes(d)
    assert rr.make_parameters(s, {"MissValR": 1.0, "WDampLim": 7.0}).MissValR == -99.99
    assert rr.make_parameters(s, {"WDampLim": 7.0}).WDampLim == 0.1
    assert len(rr.PARAMETER_OVERRIDES) == 58  # the override lines of InputParameters.cpp:41-108
    assert rr.make_parameters(s, {"Albedo_surroundings": 0.3}).Albedo_surroundings == 0.15
    assert rr.make_parameters(s, {"TClimG": 3, "Snow2IceFac": 0.25}).TClimG == 3.0


def test_missing_limit_output_start_and_params_are_read_and_ignored(tz, tmp_path):
    _forecast(tmp_path)
    base = rr.prepare(_config(tmp_path))
    odd = rr.prepare(_config(tmp_path, missing_limit=1, output={"filename": "x.json", "start": 600},
                             input=[{"name": "fc", "path": str(tmp_path / "fc.json"), "type": "json",
                                     "params": ["Humidity"]}]))
    assert bytes(base.settings) == bytes(odd.settings) and bytes(base.params) == bytes(odd.params)
    assert np.array_equal(base.sources[0].fields["tair"], odd.sources[0].fields["tair"])


def test_source_types_other_than_json_are_refused(tz, tmp_path):
    """GenericSourceFactory.cpp:29-43."""
    _forecast(tmp_path)
    cfg = _config(tmp_path, input=[{"name": "a", "path": "fc.json", "type": "netcdf"}])
    with pytest.raises(rr.ConfigError, match="Unknown data source type 'netcdf'"):
        rr.run_config(cfg)
    with pytest.raises(rr.ConfigError, match="has no type"):
        rr.run_config(_config(tmp_path, input=[{"name": "a", "path": "fc.json"}]))
    with pytest.raises(rr.ConfigError, match="'input' must be set"):
        rr.run_config(_config(tmp_path, input=None))


# ---- sources and stations ----------------------------------------------------------------------------------------

def test_a_station_a_later_source_lacks_gets_all_missing_rows(tz, tmp_path):
    """DataHandler.cpp:73-82, JsonSource.cpp:322-370: a later source is matched by statId; where it has no such
    station the reference leaves the data alone - all-missing rows on a shared axis, an empty series on
    per-point axes.  Stations, order, lat/lon are source 0's; the observation flag is `source`."""
    _forecast(tmp_path, ids=(7, 3, 5))
    ob = [_station(5, 0.0, 0.0, _stamps(T0, 3, 600), Temperature_2m=[5.5, None, 5.7], RoadTemperature=[1, 2, 3]),
          _station(7, 0.0, 0.0, _stamps(T0, 3, 600), Temperature_2m=[7.5, 7.6, 7.7])]
    _write(tmp_path / "ob.json", ob)
    inputs = [{"name": "fc", "path": str(tmp_path / "fc.json"), "type": "json", "source": "forecast"},
              {"name": "ob", "path": str(tmp_path / "ob.json"), "type": "json", "source": "observations"}]
    case = rr.prepare(_config(tmp_path, input=inputs))
    assert case.ids.tolist() == [7, 3, 5]
    assert case.lat.tolist() == [67.0, 63.0, 65.0] and case.lon.tolist() == [18.0, 22.0, 20.0]
    assert [(case.local[q].lat, case.local[q].lon) for q in range(3)] == [(67.0, 18.0), (63.0, 22.0), (65.0, 20.0)]
    fc, o = case.sources
    assert not fc.is_observation and o.is_observation
    assert np.ndim(o.times) == 1 and o.times.tolist() == [T0, T0 + 600, T0 + 1200]
    assert o.fields["tair"].tolist() == [[7.5, 7.6, 7.7], [-9999.9] * 3, [5.5, -9999.9, 5.7]]
    assert o.fields["tsurfobs"].tolist() == [[-9999.9] * 3, [-9999.9] * 3, [1.0, 2.0, 3.0]]
    # per-point axes: the missing station has an empty series
    ob[1]["time"] = _stamps(T0 + 600, 3, 600)
    _write(tmp_path / "ob.json", ob)
    o = rr.prepare(_config(tmp_path, input=inputs)).sources[1]
    assert np.ndim(o.times) == 2 and o.lengths.tolist() == [3, 0, 3]
    assert o.times[0].tolist() == [T0 + 600, T0 + 1200, T0 + 1800] and o.times[2].tolist() == [T0, T0 + 600, T0 + 1200]
    assert o.fields["tair"][0].tolist() == [7.5, 7.6, 7.7] and o.fields["tair"][2].tolist() == [5.5, -9999.9, 5.7]
    # a later source without any station
    _write(tmp_path / "ob.json", [])
    assert len(rr.prepare(_config(tmp_path, input=inputs)).sources) == 1


def test_stations_only_a_later_source_has_are_not_simulated(tz, tmp_path):
    _forecast(tmp_path, ids=(1, 2))
    _write(tmp_path / "ob.json", [_station(s, 0.0, 0.0, _stamps(T0, 2, 600), Humidity=[80.0, 81.0]) for s in (9, 2, 8)])
    inputs = [{"name": "fc", "path": str(tmp_path / "fc.json"), "type": "json"},
              {"name": "ob", "path": str(tmp_path / "ob.json"), "type": "json", "source": "observations"}]
    case = rr.prepare(_config(tmp_path, input=inputs))
    assert case.ids.tolist() == [1, 2] and len(case.local) == 2
    assert all(s.fields[k].shape[0] == 2 for s in case.sources for k in s.fields)
    assert case.sources[1].fields["rhz"].tolist() == [[-9999.9] * 2, [80.0, 81.0]]


def test_input_times_are_local_time(tz, tmp_path):
    """JsonSource.cpp:247-250: mktime.  Under TZ=EET-2 the same stamps are two hours earlier in UTC."""
    _forecast(tmp_path)
    t_utc = rr.prepare(_config(tmp_path), FT).sources[0].times.copy()
    tz("EET-2")
    assert (rr.prepare(_config(tmp_path), FT).sources[0].times == t_utc - 7200).all()


# ---- sky view and local horizons -------------------------------------------------------------------------------

def test_sky_view_range_rule_and_a_horizon_only_station(tz, tmp_path):
    """SkyView.cpp:42-55: a factor outside [0, 1] becomes 1.0; :90-119: a station only in the horizon file gets
    1.0; a station in the sky-view file only keeps zero horizons, one in neither LocalParameters' default."""
    _forecast(tmp_path, ids=(1, 2, 3, 4, 5, 6))
    _write(tmp_path / "sky.txt", "1 a 60.0 25.0 0.25\n2 b 60.0 25.0 1.5\n3 c 60 25 -0.2\n"
                                 "4  d 60.0 25.0 1.0\n1 again 0 0 0.5\n")
    h5 = np.arange(360) * 0.1
    h1 = np.full(360, 2.5)
    rows = [f"5 e 60.0 25.0 " + " ".join(repr(x) for x in h5.tolist()), "", "1 a 60.0 25.0 " + " ".join(["2.5"] * 360)]
    _write(tmp_path / "hz.txt", "\n".join(rows) + "\n")
    pars = {"sky_view_file": str(tmp_path / "sky.txt"), "local_horizon_file": str(tmp_path / "hz.txt")}
    case = rr.prepare(_config(tmp_path, parameters=pars))
    assert [case.local[q].sky_view for q in range(6)] == [0.25, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert case.horizons.shape == (6, 360)
    assert np.array_equal(case.horizons[0], h1) and np.array_equal(case.horizons[4], h5)
    assert not case.horizons[[1, 2, 3, 5]].any()
    # a sky-view file alone: no horizon table at all (the kernels read a missing one as zeros)
    case = rr.prepare(_config(tmp_path, parameters={"sky_view_file": str(tmp_path / "sky.txt")}))
    assert case.horizons is None and case.local[0].sky_view == 0.25


def test_a_horizon_row_without_360_angles_is_refused(tz, tmp_path):
    """SkyView.cpp:70-89 would hand the model a vector of 359 angles to read 360 from."""
    _forecast(tmp_path)
    _write(tmp_path / "hz.txt", "1 a 60.0 25.0 " + " ".join(["1.0"] * 359) + "\n")
    cfg = _config(tmp_path, parameters={"local_horizon_file": str(tmp_path / "hz.txt")})
    with pytest.raises(rr.ConfigError, match="359 local horizon angles, 360 needed"):
        rr.run_config(cfg)
    assert rr.main([cfg]) == 1


# ---- output layout ---------------------------------------------------------------------------------------------

def _result(status, n_out=3):
    n = len(status)
    res = {k: np.arange(n * n_out, dtype=np.float64).reshape(n, n_out) / 7.0 + j
           for j, k in enumerate(driver.OUT_FIELDS)}
    res.update(status=np.asarray(status, np.int32), ids=np.arange(100, 100 + n), lat=60.0 + np.arange(n) / 3.0,
               lon=np.full(n, 25.1), times=["2024-01-10T00:00", "2024-01-10T01:00", "2024-01-10T02:00"][:n_out])
    return res


@pytest.mark.parametrize("status, layout", [
    ([0, 1, 0, 3, 0], [100, None, 102, None, 104]),  # interior rejections: null entries
    ([1, 0, 0, 2, 2], [None, 101, 102]),              # trailing rejections: absent
    ([0], [100]),
])
def test_writer_null_layout(tmp_path, status, layout):
    """roadrunner.cpp:318-326: forecast[loc_index][...] = ... grows a jsoncpp array with nulls."""
    res = _result(status)
    path = str(tmp_path / "out.json")
    rr.write_output(path, res)
    text = open(path).read()
    got = json.loads(text)
    assert [None if e is None else e["statId"] for e in got] == layout
    assert text == json.dumps(rr.forecast_json(res), indent=3, sort_keys=True)
    assert text.startswith("[\n   ") and "\n      \"Deposit\": [\n         " in text
    for p, e in enumerate(got):
        if e is None:
            continue
        assert list(e) == sorted(["statId", "lat", "lon", "time", "RoadTemperature", "Water", "Ice", "Snow", "Deposit"])
        assert e["lat"] == res["lat"][p] and e["lon"] == 25.1 and e["time"] == res["times"]
        for name, k in rr.OUTPUT_FIELDS:
            assert np.array_equal(np.array(e[name]).view(np.int64), res[k][p].view(np.int64)), name


def test_writer_with_no_accepted_station_writes_null(tmp_path):
    path = str(tmp_path / "out.json")
    rr.write_output(path, _result([1, 2, 1]))
    assert json.load(open(path)) is None and rr.forecast_json(_result([1])) is None


def test_writer_non_finite_numbers_as_jsoncpp_writes_them(tmp_path):
    res = _result([0, 0])
    res["tsurf"][1, :] = [np.nan, np.inf, -np.inf]
    path = str(tmp_path / "out.json")
    rr.write_output(path, res)
    got = json.load(open(path))
    assert got[1]["RoadTemperature"] == [None, float("inf"), float("-inf")]
    assert got[0]["RoadTemperature"] == res["tsurf"][0].tolist()


def test_output_times_are_utc_every_step(tz, tmp_path):
    """roadrunner.cpp:303-308: gmtime of start + i*DTSecs for i = 0, step, ... < SimLen."""
    _forecast(tmp_path)
    tz("EET-2")
    case = rr.prepare(_config(tmp_path, time={"analysis": 1, "forecast": 2}), FT)
    assert case.start_time == FT - 3600 and case.settings.SimLen == 361
    assert case.times == ["2024-01-11T23:00", "2024-01-12T00:00", "2024-01-12T01:00", "2024-01-12T02:00"]
    assert case.cal["hour"][0] == 1 and case.cal["day"][0] == 12  # ... while the simulation's calendar is local
    # time_t += double (roadrunner.cpp:139-145): a DTSecs of 30.5 truncates at every step
    want = [time.strftime("%Y-%m-%dT%H:%M", time.gmtime(FT + d)) for d in (0, 60, 120)]
    assert rr.output_times(FT, 5, 30.5, 2) == want
    assert rr.output_times(FT, 122, 30.5, 120)[1] == time.strftime("%Y-%m-%dT%H:%M", time.gmtime(FT + 120 * 30))


# ---- command line ----------------------------------------------------------------------------------------------

def test_help_and_unknown_options_print_the_usage_and_exit_0(capsys):
    """roadrunner.cpp:79-88,108-110."""
    assert rr.main(["-h"]) == 0
    out = capsys.readouterr().out
    assert out.startswith("Usage:") and "-j" in out and "ignored" in out and "ROADSURF_HIP_DEVICES" in out
    assert rr.main(["-x", "config.json"]) == 0
    assert capsys.readouterr().out.startswith("Usage:")
    assert rr.main(["-j", "8", "-h"]) == 0


def test_missing_config_and_missing_output_filename_exit_1(tz, tmp_path, capsys):
    """roadrunner.cpp:115-125,360-362,545-549: `Error: <message>` on standard error, exit 1."""
    assert rr.main([]) == 1
    assert capsys.readouterr().err == "Error: Configuration file not given\n"
    missing = str(tmp_path / "nosuch.json")
    assert rr.main(["-j", "4", missing]) == 1
    assert capsys.readouterr().err == f"Error: Configuration file '{missing}' missing\n"
    _forecast(tmp_path)
    cfg = _config(tmp_path, output={"step": 60})
    assert rr.main(["-t", "20240112T0000", "-c", cfg]) == 1
    assert capsys.readouterr().err == "Error: Output filename not set\n"
    _write(tmp_path / "bad.json", "{ // unterminated\n")
    assert rr.main([str(tmp_path / "bad.json")]) == 1
    assert capsys.readouterr().err.startswith(f"Error: failed to read {tmp_path / 'bad.json'}")
