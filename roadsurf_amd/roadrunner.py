"""``python -m roadsurf_amd.roadrunner``: the reference's driver program over ``rs_driver_run``.

Same command line, configuration file, input files, sky-view / local-horizon files and output layout as the
reference's ``roadrunner`` (``examples/example1/src/roadrunner.cpp``), but every station of the run goes to the
GPUs in ONE ``rs_driver_run`` call (``driver.run(..., device=-1)``) instead of one ``runsimulation`` per station.
The host side reads and writes files only; interpolation, overlay, Tdew/RH, the read_input decisions, the
simulation and the output decimation run on the device.

Known differences from the reference (README):

* numbers are written as the shortest text that parses back to the same double, not with 7 digits;
* ``-j`` is accepted and ignored: the work is spread over the devices of ``ROADSURF_HIP_DEVICES``;
* where the reference reads past an array or uses an unset value, this program refuses the input with a message:
  a local-horizon row without exactly 360 angles, an incomplete sky-view row, a time that does not parse, more
  data sources than ``rs_driver_run`` takes (``driver.RS_MAX_SOURCES``).

Quirks of the reference that are reproduced on purpose: ``output.step`` is read only when a ``model`` object
exists; a rejected station between accepted ones is a ``null`` entry of the output array, rejected stations behind
the last accepted one are absent and a run without any accepted station writes ``null``; output times are UTC
although input times are local time.
"""
from __future__ import annotations

import dataclasses
import getopt
import json
import os
import re
import sys
import time as _time

import numpy as np

from . import abi, driver
from . import lib as rslib

USAGE = """Usage: python -m roadsurf_amd.roadrunner [options] [configfile]

Run road model using the given configuration.

-j number of parallel jobs (accepted and ignored: all stations run as one batch, spread over the GPUs of
   ROADSURF_HIP_DEVICES, not over threads)
-t simulation time, YYYYmmddTHHMM in local time (TZ)
-c configuration file
-v print the seconds spent parsing, loading the library, in rs_driver_run and writing"""

MISSING = -9999.9
_INT_MIN, _INT_MAX = -2 ** 31, 2 ** 31 - 1

#: settings a ``model`` object overrides (InputSettings.cpp:83-88): name -> int field?
MODEL_OVERRIDES = (("use_coupling", True), ("use_relaxation", True), ("DTSecs", False),
                   ("tsurfOutputDepth", False), ("NLayers", True), ("couplingEffectReduction", False))
#: parameters a ``parameters`` object overrides, (JSON key, InputParameters field), InputParameters.cpp:41-108:
#: every field but the missing values and the derived ones, all double; one key differs from its field's name
PARAMETER_OVERRIDES = tuple(
    ("Albedo_Surroundings" if n == "Albedo_surroundings" else n, n) for n in abi.INPUT_PARAMETER_NAMES
    if n not in ("MissValI", "MissValR", "MinPrecmm", "MinWatmms", "MinSnowmms", "MaxWatmms", "WDampLim",
                 "WWetLim", "WWearLim", "MinDepmms", "MinIcemms"))
#: output member -> driver.run field (roadrunner.cpp:318-326)
OUTPUT_FIELDS = (("RoadTemperature", "tsurf"), ("Water", "water"), ("Ice", "ice"), ("Snow", "snow"),
                 ("Deposit", "deposit"))


class ConfigError(RuntimeError):
    """An input the reference refuses (or would misread): ``main`` prints it as ``Error: <message>``."""


# ---- JSON as jsoncpp's default Json::CharReaderBuilder reads it (JsonTools.cpp:66-84) -------------------------

_STRING_OR_COMMENT = re.compile(r'"(?:[^"\\]|\\.)*"|//[^\n\r]*|/\*.*?\*/', re.S)


def strip_comments(text: str) -> str:
    """``//`` and ``/* */`` comments outside strings become blanks (allowComments is on by default)."""
    def keep(m):
        s = m.group(0)
        return s if s[0] == '"' else " "
    return _STRING_OR_COMMENT.sub(keep, text)


def _no_special_float(name):
    raise ValueError(f"{name} is not a JSON number")


def parse_json(text: str, what: str):
    """Comments allowed, a leading byte-order mark skipped, anything behind the root value ignored (failIfExtra is
    off by default), NaN / Infinity refused (allowSpecialFloats is off)."""
    text = strip_comments(text.lstrip("﻿"))
    dec = json.JSONDecoder(parse_constant=_no_special_float)
    try:
        value, _ = dec.raw_decode(text, len(text) - len(text.lstrip()))
    except ValueError as e:
        raise ConfigError(f"failed to read {what}: {e}") from None
    return value


def read_json(path: str):
    """read_json (JsonTools.cpp:47-84)."""
    try:
        with open(path, encoding="utf-8") as fh:
            text = fh.read()
    except OSError:
        raise ConfigError(f"Failed to open '{path}' for reading") from None
    return parse_json(text, path)


def _resolve(node, *keys, default=None):
    """Json::Path(".a.b").resolve(root, default): the default where a key or an object on the way is missing."""
    for k in keys:
        if not isinstance(node, dict) or k not in node:
            return default
        node = node[k]
    return node


def _get(obj, key):
    """Json::Value::get(key, null) on an object or null."""
    if obj is None:
        return None
    if not isinstance(obj, dict):
        raise ConfigError(f"'{key}': looked up in a JSON value that is not an object")
    return obj.get(key)


def as_int(v, what: str) -> int:
    """Json::Value::asInt: null 0, bools 0/1, reals truncated toward zero, strings refused."""
    if v is None:
        return 0
    if isinstance(v, (bool, int, float)) and _INT_MIN <= v <= _INT_MAX:
        return int(v)
    if isinstance(v, (int, float)):
        raise ConfigError(f"{what}: {v!r} is out of the range of int")
    raise ConfigError(f"{what}: {v!r} is not convertible to int")


def as_double(v, what: str) -> float:
    """Json::Value::asDouble: null 0.0, bools 0/1, numbers as they are, strings refused."""
    if v is None:
        return 0.0
    if isinstance(v, (bool, int, float)):
        return float(v)
    raise ConfigError(f"{what}: {v!r} is not convertible to double")


def override(target, obj, name: str, field: str | None = None, is_int: bool = False) -> bool:
    """override(int* / double*, json, name) (JsonTools.cpp:8-39): a value given and not null replaces the field."""
    v = _get(obj, name)
    if v is None:
        return False
    setattr(target, field or name, as_int(v, name) if is_int else as_double(v, name))
    return True


# ---- times and settings (roadrunner.cpp:58-127, InputSettings.cpp:10-104) ----------------------------------

def parse_local_time(s: str, what: str) -> int:
    """strptime(s, "%Y%m%dT%H%M") + mktime with tm_isdst = -1: ``s`` is local time (TZ)."""
    try:
        tm = _time.strptime(s, "%Y%m%dT%H%M")
    except ValueError:
        raise ConfigError(f"{what}: '{s}' is not a time of the form YYYYmmddTHHMM") from None
    return int(_time.mktime(tm))


def get_forecast_time(cfg, cli_time: int = 0, now: float | None = None) -> int:
    """get_forecast_time (InputSettings.cpp:10-35): ``-t`` (any nonzero time), else ``time.now``, else the current
    time rounded down to the minute - the reference's way: the fields of gmtime handed to mktime, i.e. read as
    local time with daylight saving off."""
    if cli_time:
        return int(cli_time)
    s = _resolve(cfg, "time", "now")
    if s is not None and not isinstance(s, str):
        raise ConfigError(f"time.now: {s!r} is not a string")
    if s:
        return parse_local_time(s, "time.now")
    g = _time.gmtime(_time.time() if now is None else now)
    return int(_time.mktime((g.tm_year, g.tm_mon, g.tm_mday, g.tm_hour, g.tm_min, 0, g.tm_wday, g.tm_yday, 0)))


def make_settings(cfg, forecast_time: int) -> tuple[abi.InputSettings, int, int]:
    """InputSettings(json, options) (InputSettings.cpp:69-104).  Returns (settings, start_time, end_time)."""
    analysis = as_int(_resolve(cfg, "time", "analysis", default=24), "time.analysis")
    forecast = as_int(_resolve(cfg, "time", "forecast", default=48), "time.forecast")
    start, end = forecast_time - analysis * 3600, forecast_time + forecast * 3600
    s = abi.default_settings(0)  # InputSettings.h:13-23
    model = _get(cfg, "model")
    if model is not None:
        for name, is_int in MODEL_OVERRIDES:
            override(s, model, name, is_int=is_int)
    # Deliberately as the reference has it: InputSettings.cpp:90-94 tests `json` (the "model" object), not
    # `json2` ("output"), so output.step is read only when the configuration has a model object.
    if model is not None:
        override(s, _get(cfg, "output"), "step", "outputStep", is_int=True)
    if not s.DTSecs > 0:
        raise ConfigError(f"model.DTSecs must be > 0, not {s.DTSecs!r}")
    s.SimLen = 1 + int((end - start) / s.DTSecs)  # time_t / double, truncated
    if s.SimLen < 1:
        raise ConfigError(f"the simulation has no time steps (time.analysis {analysis} h, time.forecast {forecast} h)")
    cm = as_int(_resolve(cfg, "time", "coupling_minutes", default=0), "time.coupling_minutes")
    if cm > 0:
        s.coupling_minutes = cm
    return s, start, end


def make_parameters(settings: abi.InputSettings, pcfg) -> abi.InputParameters:
    """InputParameters(settings, json) (InputParameters.cpp:9-110): the DTSecs-derived defaults first
    (abi.default_parameters evaluates InputParameters.cpp:13-21 as written), then the overrides - so an overridden
    MaxPormms does not move WDampLim, WWetLim, WWearLim or MaxWatmms."""
    p = abi.default_parameters(settings.DTSecs)
    if pcfg is None:
        return p
    for key, field in PARAMETER_OVERRIDES:
        override(p, pcfg, key, field)
    return p


# ---- sources (DataHandler.cpp:34-101, GenericSourceFactory.cpp:14-44, JsonSource.cpp:206-414) ----------------

def source_specs(cfg) -> list[tuple[str, str, bool]]:
    """(name, path, is_observation) of every ``input[]`` entry, in order, checked as the reference checks them."""
    inp = _get(cfg, "input")
    if inp is None:
        raise ConfigError("Config variable 'input' must be set")
    if not isinstance(inp, list):
        raise ConfigError("Config variable 'input' must be an array of JSON objects defining data sources")
    specs = []
    for src in inp:
        if not isinstance(src, dict):
            raise ConfigError("Data sources must be defined with JSON objects")
        name = src.get("name")
        if name is None:
            raise ConfigError("Encountered an element in 'sources' without a name")
        typ = src.get("type")
        if typ is None:
            raise ConfigError(f"Data source '{name}' has no type")
        if typ != "json":
            raise ConfigError(f"Unknown data source type '{typ}'")
        path = src.get("path")
        specs.append((str(name), "" if path is None else str(path), src.get("source") == "observations"))
    if not specs:
        raise ConfigError("Config variable 'input' holds no data source")
    if len(specs) > driver.RS_MAX_SOURCES:
        raise ConfigError(f"{len(specs)} data sources: rs_driver_run takes at most {driver.RS_MAX_SOURCES}")
    return specs


def read_source(path: str, is_observation: bool):
    """One input file: (RawSource, ids, lats, lons).  Times are local time (JsonSource.cpp:247-250 uses mktime)."""
    if not os.path.isfile(path):
        raise ConfigError(f"Failed to open '{path}' for reading")
    return driver.read_json_source(path, is_observation, utc=False)


def match_source(src: driver.RawSource, ids, station_ids) -> driver.RawSource:
    """The source's rows in the order of ``station_ids`` (source 0's stations), found by statId as
    JsonSource::GetWeather finds them (the first station of that id).  A station the source lacks gets all-missing
    rows on a shared axis, or an empty series on per-point axes: the reference leaves its data as it is."""
    first = {}
    for i, sid in enumerate(ids):
        first.setdefault(int(sid), i)
    idx = np.fromiter((first.get(int(sid), -1) for sid in station_ids), np.int64, len(station_ids))
    if len(ids) == len(station_ids) and np.array_equal(idx, np.arange(len(ids))):
        return src
    have = idx >= 0
    take = np.where(have, idx, 0)
    fields = {k: np.where(have[:, None], a[take], MISSING) for k, a in src.fields.items()}
    if np.ndim(src.times) == 1:
        return driver.RawSource(src.times, fields, src.is_observation)
    return driver.RawSource(np.ascontiguousarray(src.times[take]), fields, src.is_observation,
                            np.where(have, src.lengths[take], 0).astype(np.int32))


# ---- sky view and local horizons (SkyView.cpp:14-138) --------------------------------------------------------

def read_sky_view(pcfg) -> dict:
    """statId -> [sky_view, horizons (360 float64) or None] from ``parameters.sky_view_file`` (rows
    ``id name lat lon sky_view``; a factor outside [0, 1] becomes 1.0; the first row of an id counts) and
    ``parameters.local_horizon_file`` (rows ``id name lat lon h0 ... h359``; the last row of an id counts, an id
    only there gets sky view 1.0).  A station in neither keeps LocalParameters' default and zero horizons."""
    data = {}
    if pcfg is None:
        return data
    sv = _get(pcfg, "sky_view_file")
    if sv is not None:
        sv = str(sv)
        try:
            with open(sv) as fh:
                tok = fh.read().split()
        except OSError:
            raise ConfigError(f"Failed to open '{sv}'") from None
        if len(tok) % 5:
            raise ConfigError(f"{sv}: {len(tok)} values, not rows of five (id name lat lon sky_view)")
        try:
            for r in range(0, len(tok), 5):
                sid, f = int(tok[r]), float(tok[r + 4])
                data.setdefault(sid, [f if 0.0 <= f <= 1.0 else 1.0, None])
        except ValueError as e:
            raise ConfigError(f"{sv}: {e}") from None
    hf = _get(pcfg, "local_horizon_file")
    if hf is not None:
        hf = str(hf)
        try:
            fh = open(hf)
        except OSError:
            raise ConfigError(f"Failed to open '{hf}'") from None
        with fh:
            for lineno, line in enumerate(fh, 1):
                tok = line.split()
                if not tok:
                    continue
                if len(tok) != 364:
                    raise ConfigError(f"{hf}:{lineno}: {max(0, len(tok) - 4)} local horizon angles, 360 needed "
                                      "(id name lat lon h0 ... h359)")
                try:
                    sid = int(tok[0])
                    hz = np.array([float(x) for x in tok[4:]])
                except ValueError as e:
                    raise ConfigError(f"{hf}:{lineno}: {e}") from None
                if sid in data:
                    data[sid][1] = hz
                else:
                    data[sid] = [1.0, hz]
    return data


# ---- the run ------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Case:
    """Everything one run needs, as the reference holds it before its station loop."""
    settings: abi.InputSettings
    params: abi.InputParameters
    forecast_time: int
    start_time: int
    end_time: int
    sources: list
    ids: np.ndarray
    lat: np.ndarray
    lon: np.ndarray
    local: object
    horizons: np.ndarray | None
    output_filename: str | None
    cal: dict  # the simulation calendar, local time (JsonSource.cpp:297-308)
    times: list  # the output's time strings


def prepare(config_path: str, forecast_time: int | None = None, need_output: bool = False) -> Case:
    """Read the configuration, the input files and the sky-view files, in the reference's order (main ->
    InputSettings -> DataHandler::init -> run_locations_sync).  ``forecast_time``: what ``-t`` gives."""
    cfg = read_json(config_path)
    if not isinstance(cfg, dict):
        raise ConfigError(f"{config_path}: the configuration is not a JSON object")
    ft = get_forecast_time(cfg, forecast_time or 0)
    s, start, end = make_settings(cfg, ft)
    raw = [read_source(path, obs) for _, path, obs in source_specs(cfg)]
    _, ids0, lat, lon = raw[0]
    ids0 = np.asarray(ids0, np.int64)
    # (a file without stations has data for none of them)
    sources = [match_source(src, ids, ids0) for src, ids, _, _ in raw if len(ids)] if len(ids0) else []
    fname = _resolve(cfg, "output", "filename")
    if need_output and fname is None:
        raise ConfigError("Output filename not set")
    p = make_parameters(s, _get(cfg, "parameters"))
    sky = read_sky_view(_get(cfg, "parameters"))
    n = len(ids0)
    local = driver._locals(n, None)  # LocalParameters' defaults (LocalParameters.h:17-25)
    hz = None
    for q in range(n):
        lp = local[q]
        lp.lat, lp.lon = float(lat[q]), float(lon[q])
        e = sky.get(int(ids0[q]))
        if e is not None:
            lp.sky_view = e[0]
            if e[1] is not None:
                if hz is None:
                    hz = np.zeros((n, 360))
                hz[q] = e[1]
    cal = driver.calendar(start, s.SimLen, int(s.DTSecs), utc=False) if n else None
    return Case(s, p, ft, start, end, sources, ids0, np.asarray(lat, np.float64), np.asarray(lon, np.float64),
                local, hz, None if fname is None else str(fname), cal,
                output_times(start, s.SimLen, s.DTSecs, driver.output_rows(s)[0]))


def output_times(start_time: int, simlen: int, dtsecs: float, step: int) -> list[str]:
    """get_times (roadrunner.cpp:135-148: time_t += double) at every ``step``-th index, as save_output formats
    them (roadrunner.cpp:303-308): gmtime, i.e. UTC although the inputs are local time."""
    out, t = [], start_time
    for i in range(simlen):
        if i % step == 0:
            out.append(_time.strftime("%Y-%m-%dT%H:%M", _time.gmtime(t)))
        t = int(t + dtsecs)
    return out


def run_case(case: Case) -> dict:
    """One driver.run over all stations (rs_driver_run, fanned out over ROADSURF_HIP_DEVICES).  Returns
    driver.run's arrays plus ``ids``, ``lat``, ``lon``, ``times`` (the output's time strings) and
    ``output_filename``."""
    s = case.settings
    if len(case.ids):
        res = driver.run(case.sources, s, case.params, case.start_time, case.forecast_time, local=case.local,
                         cal=case.cal, horizons=case.horizons, device=-1)
    else:
        step, n_out = driver.output_rows(s)
        res = {k: np.zeros((0, n_out)) for k in driver.OUT_FIELDS}
        res.update(status=np.zeros(0, np.int32), missing_index=np.zeros(0, np.int32), local=case.local, step=step)
    res.update(ids=case.ids, lat=case.lat, lon=case.lon, times=case.times, output_filename=case.output_filename)
    return res


def run_config(config_path: str, forecast_time: int | None = None) -> dict:
    """Read ``config_path`` and run it; nothing is written (``write_output`` does that)."""
    return run_case(prepare(config_path, forecast_time))


# ---- output (roadrunner.cpp:285-347) -------------------------------------------------------------------------

def forecast_json(res: dict):
    """The forecast as the reference's jsoncpp value holds it: ``forecast[loc_index][...] = ...`` grows the array
    with null, so a rejected station before the last accepted one is null, the ones behind it are absent, and no
    accepted station at all leaves the value null."""
    ok = np.nonzero(np.asarray(res["status"]) == 0)[0]
    if not len(ok):
        return None
    out = [None] * (int(ok[-1]) + 1)
    for p in ok:
        e = {"statId": int(res["ids"][p]), "lat": float(res["lat"][p]), "lon": float(res["lon"][p]),
             "time": list(res["times"])}
        for name, k in OUTPUT_FIELDS:
            e[name] = [_special(x) for x in res[k][p].tolist()]
        out[p] = e
    return out


def _special(x: float):
    return x if np.isfinite(x) else (None if x != x else x)


def _num(x: float) -> str:
    """A double as jsoncpp writes a non-finite one (null, +-1e+9999), else the shortest round-trip text."""
    if x != x:
        return "null"
    if x in (float("inf"), float("-inf")):
        return "1e+9999" if x > 0 else "-1e+9999"
    return repr(x)


def write_output(path: str, res: dict) -> None:
    """Write ``forecast_json(res)`` as json.dump(indent=3, sort_keys=True) would - three-space indentation, members
    in jsoncpp's (sorted) order - but row by row, fast enough for a million stations."""
    ok = np.nonzero(np.asarray(res["status"]) == 0)[0]
    with open(path, "w") as fh:
        if not len(ok):
            fh.write("null")
            return
        i2, i3 = "\n" + " " * 6, "\n" + " " * 9
        times = "[" + i3 + ("," + i3).join(json.dumps(t) for t in res["times"]) + i2 + "]"
        members = sorted([(name, k) for name, k in OUTPUT_FIELDS] + [("lat", None), ("lon", None),
                                                                    ("statId", None), ("time", None)])
        fin = {k: bool(np.isfinite(res[k][ok]).all()) for _, k in OUTPUT_FIELDS}
        okset = set(ok.tolist())
        fh.write("[")
        for p in range(int(ok[-1]) + 1):
            fh.write("\n   " if p == 0 else ",\n   ")
            if p not in okset:
                fh.write("null")
                continue
            parts = []
            for name, k in members:
                if k is not None:
                    row = res[k][p].tolist()
                    txt = ("," + i3).join(map(repr, row) if fin[k] else map(_num, row))
                    v = "[" + i3 + txt + i2 + "]"
                elif name == "statId":
                    v = str(int(res["ids"][p]))
                elif name == "time":
                    v = times
                else:
                    v = _num(float(res[name][p]))
                parts.append(f'"{name}": {v}')
            fh.write("{" + i2 + ("," + i2).join(parts) + "\n   }")
        fh.write("\n]")


# ---- command line ---------------------------------------------------------------------------------------------

def main(argv=None) -> int:
    """roadrunner's main (roadrunner.cpp:525-551): 0 on success, after -h or an unknown option; 1 with
    ``Error: <message>`` on standard error otherwise."""
    argv = sys.argv[1:] if argv is None else list(argv)
    try:
        try:
            opts, args = getopt.gnu_getopt(argv, "hvj:t:c:")
        except getopt.GetoptError as e:  # roadrunner.cpp:108-110: the usage, and a normal exit
            print(f"roadrunner: {e}", file=sys.stderr)
            print(USAGE + "\n")
            return 0
        config, cli_time, verbose = "", 0, False
        for o, a in opts:
            if o == "-h":
                print(USAGE + "\n")
                return 0
            if o == "-t":
                cli_time = parse_local_time(a, "-t")
            elif o == "-c":
                config = a
            elif o == "-v":
                verbose = True
            # -j: accepted and ignored
        if not config and args:
            config = args[0]
        if not config:
            raise ConfigError("Configuration file not given")
        if not os.path.exists(config):
            raise ConfigError(f"Configuration file '{config}' missing")

        t0 = _time.perf_counter()
        case = prepare(config, cli_time, need_output=True)
        t1 = _time.perf_counter()
        L = rslib.load()  # (imports torch, maps the library; the HIP runtime starts in rs_hip_device_count)
        L.rs_hip_device_count()
        t2 = _time.perf_counter()
        res = run_case(case)
        t3 = _time.perf_counter()
        write_output(case.output_filename, res)
        t4 = _time.perf_counter()
        if verbose:
            n, ok = len(res["ids"]), int((res["status"] == 0).sum())
            print(f"roadrunner: {n} stations ({ok} accepted) x {case.settings.SimLen} steps: parse {t1 - t0:.3f} s, "
                  f"load {t2 - t1:.3f} s, rs_driver_run {t3 - t2:.3f} s, write {t4 - t3:.3f} s", flush=True)
        return 0
    except Exception as e:  # roadrunner.cpp:547-551
        print(f"Error: {e}", file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main())
