"""Helpers for the tests that hold the driver data path to the reference's own C++ driver.

* ``Ref``: ctypes binding of ``oracle/_ref/libroadrunner_ref.so`` (the reference's twelve driver sources + our
  ``oracle/driver_ref_harness.cpp``, built by ``oracle/build_ref.sh`` over the stand-in headers of ``oracle/shim``).
* ``make_case``: a seeded generator of whole driver inputs - a configuration, one to three source files and optional
  sky-view / local-horizon files - written as the files the reference's ``roadrunner`` reads.
* ``reference_view`` / ``project_view``: the same configuration opened by the reference and by
  ``roadrunner.prepare`` -> ``driver.make_input`` -> ``oracle/driver_oracle.c``.

The generator stays inside what the stand-in JSON library can be trusted with: every value array is as long as
"time" and holds numbers only (no null entries), see DESIGN.md 4.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import json
import os
import time as _time

import numpy as np
import pytest

import driver_helpers as dh
import oracle_helpers as oh
from roadsurf_amd import abi, driver, roadrunner

REF_DRIVER_SO = os.path.join(oh.ORACLE_DIR, "_ref", "libroadrunner_ref.so")
M = -9999.9
#: name, POSIX TZ string (no tzdata needed), time.now in that zone's local time
ZONES = {
    "utc": ("UTC", "20240110T0300"),
    # 05:00 EEST = 02:00 UTC; three hours back is 01:00 EET: the run crosses the change of 31 March, 03:00 -> 04:00
    "eet": ("EET-2EEST,M3.5.0/3,M10.5.0/4", "20240331T0500"),
}
ANALYSIS_H = FORECAST_H = 3
#: read_input's order of complaints (roadrunner.cpp:188-229): status code -> merged series
STATUS_ORDER = ((1, "tair"), (2, "rhz"), (3, "prec"), (4, "sw"), (5, "lw"), (6, "vz"))
LOCAL_REALS = ("tair_relax", "VZ_relax", "RH_relax", "couplingTsurf", "lat", "lon", "sky_view")
LOCAL_INTS = ("couplingIndexI", "InitLenI")
SETTING_INTS = ("SimLen", "use_coupling", "use_relaxation", "NLayers", "coupling_minutes", "outputStep")
SETTING_REALS = ("DTSecs", "tsurfOutputDepth", "couplingEffectReduction")


@contextlib.contextmanager
def timezone(tz: str):
    """TZ for mktime / localtime, in this process's C library and in Python alike."""
    old = os.environ.get("TZ")
    os.environ["TZ"] = tz
    _time.tzset()
    try:
        yield
    finally:
        if old is None:
            del os.environ["TZ"]
        else:
            os.environ["TZ"] = old
        _time.tzset()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bits(a, b) -> bool:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


# ---- the reference ------------------------------------------------------------------------------------------------

def require_reference() -> str:
    """The reference driver library, or a skip where there is no reference build at all; a build that lacks just
    this library is an error with the way out in the message."""
    if os.path.exists(REF_DRIVER_SO):
        return REF_DRIVER_SO
    if os.path.exists(oh.REF_CPL_SO):
        pytest.fail(f"{REF_DRIVER_SO} is missing beside {oh.REF_CPL_SO}: build it with `bash oracle/build_ref.sh` "
                    "(or `python -c \"import __graft_entry__ as g; g.build()\"`) where the reference's sources are")
    pytest.skip("no reference build (oracle/_ref)")


class Ref:
    """One configuration opened by the reference: main() up to run(), then run_locations_sync up to its loop."""
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = C.CDLL(require_reference())
            L.rr_ref_error.restype = C.c_char_p
            L.rr_ref_open.restype = C.c_void_p
            L.rr_ref_open.argtypes = [C.c_char_p, C.c_int64]
            L.rr_ref_close.argtypes = [C.c_void_p]
            L.rr_ref_cli_time.restype = C.c_int64
            L.rr_ref_cli_time.argtypes = [C.c_char_p, C.c_char_p]
            L.rr_ref_settings.argtypes = [C.c_void_p, abi.c_int32_p, abi.c_double_p, C.POINTER(C.c_int64)]
            L.rr_ref_parameters.restype = C.c_int32
            L.rr_ref_parameters.argtypes = [C.c_void_p, abi.c_double_p, C.c_int32]
            L.rr_ref_n_stations.restype = C.c_int32
            L.rr_ref_n_stations.argtypes = [C.c_void_p]
            L.rr_ref_stations.argtypes = [C.c_void_p, abi.c_int32_p, abi.c_double_p, abi.c_double_p]
            L.rr_ref_read_input.restype = C.c_int32
            L.rr_ref_read_input.argtypes = [C.c_void_p, C.c_int32, abi.c_double_p, abi.c_int32_p, abi.c_double_p,
                                            abi.c_int32_p, abi.c_double_p, abi.c_int32_p, abi.c_int32_p]
            L.rr_ref_run.restype = C.c_int32
            L.rr_ref_run.argtypes = [C.c_void_p, C.c_int32, abi.c_double_p, abi.c_int32_p]
            cls._lib = L
        return cls._lib

    def __init__(self, config_path: str, cli_time: int = 0):
        L = self.lib()
        with oh.quiet_stdout():  # "Reading data source named ..."
            self.h = L.rr_ref_open(os.fsencode(config_path), int(cli_time))
        if not self.h:
            raise RuntimeError("reference: " + L.rr_ref_error().decode())
        ints = np.zeros(len(SETTING_INTS), np.int32)
        reals = np.zeros(len(SETTING_REALS))
        times = np.zeros(3, np.int64)
        L.rr_ref_settings(self.h, ints.ctypes.data_as(abi.c_int32_p), reals.ctypes.data_as(abi.c_double_p),
                          times.ctypes.data_as(C.POINTER(C.c_int64)))
        self.settings = dict(zip(SETTING_INTS, ints.tolist()), **dict(zip(SETTING_REALS, reals.tolist())))
        self.forecast_time, self.start_time, self.end_time = (int(t) for t in times)
        self.simlen = int(ints[0])
        p = np.zeros(len(abi.INPUT_PARAMETER_NAMES))
        n = L.rr_ref_parameters(self.h, p.ctypes.data_as(abi.c_double_p), len(p))
        assert n == len(p), "InputParameters: the harness and abi.INPUT_PARAMETER_NAMES disagree on the members"
        self.parameters = p
        self.n = L.rr_ref_n_stations(self.h)
        self.ids = np.zeros(self.n, np.int32)
        self.lat, self.lon = np.zeros(self.n), np.zeros(self.n)
        if self.n:
            L.rr_ref_stations(self.h, self.ids.ctypes.data_as(abi.c_int32_p), self.lat.ctypes.data_as(abi.c_double_p),
                              self.lon.ctypes.data_as(abi.c_double_p))

    def close(self):
        if self.h:
            self.lib().rr_ref_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def read_input(self) -> dict:
        """read_input of every station: ``merged`` name -> [n][SimLen], ``cal`` name -> [n][SimLen],
        ``precphase`` [n][SimLen], ``horizons`` [n][360], ``n_horizons`` [n], ``local`` name -> [n], ``success`` [n]."""
        L, n, S = self.lib(), self.n, self.simlen
        series = np.zeros((n, 10, S))
        cal = np.zeros((n, 7, S), np.int32)
        hz = np.zeros((n, 360))
        nhz = np.zeros(n, np.int32)
        ld = np.zeros((n, len(LOCAL_REALS)))
        li = np.zeros((n, len(LOCAL_INTS)), np.int32)
        ok = np.zeros(n, np.int32)
        with oh.quiet_stdout():  # "2m temperature missing at ..."
            for k in range(n):
                rc = L.rr_ref_read_input(self.h, k, series[k].ctypes.data_as(abi.c_double_p),
                                         cal[k].ctypes.data_as(abi.c_int32_p), hz[k].ctypes.data_as(abi.c_double_p),
                                         nhz[k:].ctypes.data_as(abi.c_int32_p), ld[k].ctypes.data_as(abi.c_double_p),
                                         li[k].ctypes.data_as(abi.c_int32_p), ok[k:].ctypes.data_as(abi.c_int32_p))
                if rc:
                    raise RuntimeError("reference: " + L.rr_ref_error().decode())
        local = {name: ld[:, j].copy() for j, name in enumerate(LOCAL_REALS)}
        local.update({name: li[:, j].copy() for j, name in enumerate(LOCAL_INTS)})
        return {"merged": {name: np.ascontiguousarray(series[:, j]) for j, name in enumerate(driver.MERGED_FIELDS)},
                "cal": {name: np.ascontiguousarray(cal[:, j]) for j, name in enumerate(driver.CALENDAR)},
                "precphase": np.ascontiguousarray(cal[:, 6]), "horizons": hz, "n_horizons": nhz, "local": local,
                "success": ok.astype(bool)}

    def run(self) -> dict:
        """read_input + runsimulation of every station at full resolution: name -> [n][SimLen], ``success`` [n]."""
        L, n, S = self.lib(), self.n, self.simlen
        out = np.zeros((n, 6, S))
        ok = np.zeros(n, np.int32)
        with oh.quiet_stdout():
            for k in range(n):
                if L.rr_ref_run(self.h, k, out[k].ctypes.data_as(abi.c_double_p), ok[k:].ctypes.data_as(abi.c_int32_p)):
                    raise RuntimeError("reference: " + L.rr_ref_error().decode())
        res = {name: np.ascontiguousarray(out[:, j]) for j, name in enumerate(driver.OUT_FIELDS)}
        res["success"] = ok.astype(bool)
        return res


def scan_status(merged: dict, k: int):
    """(status, missing_index) of station k from the InputData the reference returned: the first complaint of
    read_input's loop (roadrunner.cpp:183-231), which returns at once - so what it returned is the merged data."""
    S = merged["tair"].shape[1]
    bad = np.zeros((len(STATUS_ORDER), S), bool)
    for j, (_, name) in enumerate(STATUS_ORDER):
        v = merged[name][k]
        bad[j] = np.isnan(v) | (v < -9000)
    cols = np.nonzero(bad.any(axis=0))[0]
    if not len(cols):
        return 0, -1
    i = int(cols[0])
    return STATUS_ORDER[int(np.argmax(bad[:, i]))][0], i


# ---- the generator ------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Spec:
    seed: int
    n: int = 28
    zone: str = "utc"
    order: tuple = ("fc", "obs")  # the sources, in the configuration's order; "obs2" = a second observation file
    relaxation: bool = False
    coupling: bool = False
    coupling_minutes: int | None = 60
    dtsecs: int = 30
    model: bool = True  # a "model" object at all (without it output.step is not read)
    step: int | None = 30  # output.step, minutes
    cli_time: bool = False  # a different time.now in the file than what -t gives
    sky: str | None = None  # "sky", "hz" or "both"
    params: bool = False
    shared: bool = False  # every station of a file on the same time axis
    rejects: tuple = ()  # fc axis / value kinds that make read_input refuse a station


#: what read_input refuses (names of the branches of _fc_station below)
REJECTS = ("ends_at_end", "starts_late", "ends_early", "single", "empty", "before", "after", "no_hum", "prec_hole",
           "no_sw", "lw_m100", "vz_hole", "tair_m100")


def _stamp(t: int) -> str:
    return _time.strftime("%Y-%m-%d %H:%M", _time.localtime(t))


def _walk(rs, n, lo, hi, step):
    v = np.clip(rs.uniform(lo, hi) + np.cumsum(rs.normal(0, step, n)), lo, hi)
    return [float(x) for x in v]


def _fc_station(rs, kind, start, end, shared, sky):
    """One station of the forecast file: (times, variables).  ``sky``: the run has sky-view factors, under which the
    model also wants direct short-wave and net long-wave radiation at every step (src/InputOutput.f90:68-71)."""
    H = 3600
    wide = list(range(start - H, end + H + 1, H))
    if shared or kind in ("wide", "no_hum", "prec_hole", "no_sw", "lw_m100", "vz_hole", "tair_m100", "tair_gap_early"):
        t = wide
    elif kind == "first_at_start":
        t = list(range(start, end + H + 1, H))
    elif kind == "ten_minutes":
        t = list(range(start - 600, end + 601, 600))
    elif kind == "irregular":
        mins = np.sort(rs.choice(np.arange(-30, (end - start) // 60 + 30), 40, replace=False))
        t = [start - 45 * 60] + [start + 60 * int(m) for m in mins] + [end + 45 * 60]
    elif kind == "ends_at_end":
        t = list(range(start - H, end + 1, H))
    elif kind == "starts_late":
        t = list(range(start + H, end + H + 1, H))
    elif kind == "ends_early":
        t = list(range(start - H, end - H + 1, H))
    elif kind == "single":
        t = [start + 2 * H]
    elif kind == "empty":
        t = []
    elif kind == "before":
        t = list(range(start - 5 * H, start - H + 1, H))
    elif kind == "after":
        t = list(range(end + H, end + 4 * H + 1, H))
    else:
        raise KeyError(kind)
    m = len(t)
    tair = _walk(rs, m, -25.0, 12.0, 1.5)
    v = {"Temperature 2m": tair,
         "WindSpeed": _walk(rs, m, 0.2, 14.0, 1.0),
         "Precipitation": [0 if rs.rand() < 0.5 else float(rs.uniform(0, 3)) for _ in range(m)],  # integer literals too
         "RadiationGlobal": _walk(rs, m, 0.0, 500.0, 60.0),
         "RadiationLW": _walk(rs, m, 180.0, 380.0, 15.0)}
    hum = "none" if kind == "no_hum" else ("rh", "tdew", "both")[rs.randint(3)]
    if hum in ("rh", "both"):
        v["Humidity"] = [int(x) if rs.rand() < 0.3 else x for x in _walk(rs, m, 35.0, 100.0, 5.0)]
    if hum in ("tdew", "both"):
        v["DewPoint"] = [a - float(rs.uniform(0, 6)) for a in tair]
    edge = rs.rand() < 0.3  # values at and around the thresholds (the model itself then gives up on some of these)
    if sky or rs.rand() < 0.5:
        v["RadiationDirectSW"] = _walk(rs, m, 0.0, 300.0, 40.0)
        if m > 3 and edge:
            v["RadiationDirectSW"][2] = -150.0  # missing anywhere but in the net long-wave radiation
    if sky or rs.rand() < 0.6:
        v["RadiationNetSurfaceLW"] = _walk(rs, m, -140.0, 20.0, 20.0)
        if m > 4:
            v["RadiationNetSurfaceLW"][1] = -150.0  # a valid value there
            if edge:
                v["RadiationNetSurfaceLW"][3] = -1000.0  # exactly the threshold: missing
                v["RadiationNetSurfaceLW"][4] = -999.5
    if rs.rand() < 0.5:
        v["PrecipitationForm"] = [int(rs.randint(0, 7)) for _ in range(m)]
    j = m - 3  # a stamp in the forecast part, with stamps on both sides
    if kind == "no_sw":
        del v["RadiationGlobal"]
    elif kind == "prec_hole":
        v["Precipitation"][j] = M
    elif kind == "lw_m100":
        v["RadiationLW"][j] = -100.0  # exactly the threshold: missing
    elif kind == "vz_hole":
        v["WindSpeed"][j] = M
    elif kind == "tair_m100":
        v["Temperature 2m"][j] = -100.0
    elif kind == "tair_gap_early":  # no forecast air temperature in the first hour: an observation source shows through
        v["Temperature 2m"][1] = M
    elif kind == "wide" and m > 5 and rs.rand() < 0.12:
        v["Temperature 2m"][1] = -99.9999  # just inside
        if "DewPoint" in v:
            v["DewPoint"][1] = -99.99995
    return t, v


def _obs_station(rs, k, start, ft, dt, shared, second):
    """One station of an observation file: 10-minute stamps from ten minutes before the start to ten minutes behind
    the forecast time (irregular minutes for some); air temperature and road temperature each stop at a stamp of
    their own.  Nothing is observed at or behind the forecast time's index."""
    last = (ft - start) // 600  # stamp j is start - 600 + 600 j
    if not shared and k % 5 == 3:
        mins = np.sort(rs.choice(np.arange(1, (ft - start) // 60 - 2), 25, replace=False))
        t = [start] + [start + 60 * int(x) for x in mins] + [ft + 240]  # first stamp AT the start
    elif not shared and k % 7 == 5:
        t = list(range(start + 1200, ft + 601, 600))  # first stamp behind the start
    else:
        t = list(range(start - 600, ft + 601, 600))
    m = len(t)
    tair = _walk(rs, m, -25.0, 12.0, 0.8)
    v = {"Temperature 2m": tair, "WindSpeed": _walk(rs, m, 0.2, 14.0, 0.6)}
    if k % 4 == 1:
        v["DewPoint"] = [a - float(rs.uniform(0, 4)) for a in tair]
    else:
        v["Humidity"] = _walk(rs, m, 35.0, 100.0, 3.0)
    road = _walk(rs, m, -20.0, 15.0, 0.7)
    # road temperature stops at 50 min (before the 60-minute window), 60 min (exactly), later, or is absent
    cuts = (6, 7, 12, last, None, 7, 10)
    rc = cuts[k % len(cuts)] if m == last + 3 else m - 2
    if rc is not None:
        v["RoadTemperature"] = [x if j <= rc else M for j, x in enumerate(road)]
    ac = (last - 1 - (k % 6)) if not second else last  # air temperature: different last stamps
    ac = min(ac, m - 2)
    if k % 11 == 4:
        ac = -1  # no air temperature observation at all
    for name in ("Temperature 2m", "WindSpeed", "Humidity", "DewPoint"):
        if name in v:
            v[name] = [x if j <= ac else M for j, x in enumerate(v[name])]
    if k % 3 == 0 and m > 6:
        v["WindSpeed"][3] = M  # a missing neighbour on one side of two segments
    if k % 9 == 2:
        del v["Temperature 2m"]
    return t, v


def make_case(tmp, spec: Spec) -> dict:
    """Write one whole driver input under ``tmp``.  Call inside ``timezone(ZONES[spec.zone][0])``: the stamps of the
    source files are local time.  Returns {"config", "cli_time", "tz"}."""
    tmp = str(tmp)
    rs = np.random.RandomState(spec.seed)
    tz, now = ZONES[spec.zone]
    ft = roadrunner.parse_local_time(now, "now")
    start, end = ft - ANALYSIS_H * 3600, ft + FORECAST_H * 3600
    n = spec.n
    ids = [int(x) for x in rs.choice(np.arange(1000, 9000), n + 4, replace=False)]
    master, extra = ids[:n - 1], ids[n - 1:]
    kinds = ["wide"] * len(master)
    special = list(spec.rejects) + ["tair_gap_early"] + ([] if spec.shared else ["first_at_start", "ten_minutes",
                                                                                 "irregular"])
    for k, kind in zip(rs.permutation(len(master))[:len(special)], special):
        kinds[int(k)] = kind
    lat = {i: float(rs.uniform(59.5, 69.5)) for i in ids}
    lon = {i: float(rs.uniform(20.0, 30.0)) for i in ids}
    files = {}
    for si, name in enumerate(spec.order):
        members = list(master)
        if si > 0:  # a later file: shuffled, two stations missing, one station that only it has
            members = [members[int(j)] for j in rs.permutation(len(members))][2:] + [extra[si]]
        stations = []
        for sid in members:
            k = ids.index(sid)
            if name == "fc":
                t, v = _fc_station(rs, kinds[k] if sid in master else "wide", start, end, spec.shared, spec.sky is not None)
            else:
                t, v = _obs_station(rs, k, start, ft, spec.dtsecs, spec.shared, name == "obs2")
                if name == "obs2" and k % 2:
                    t, v = [], {}
            e = {"statId": sid, "lat": lat[sid], "lon": lon[sid], "time": [_stamp(x) for x in t]}
            e.update(v)
            stations.append(e)
        # a repeated statId: the first one wins (a copy of another station's data under the id of the first)
        dup = dict(stations[int(rs.randint(len(stations)))])
        dup["statId"] = stations[0]["statId"]
        dup["lat"] += 0.125
        stations.insert(int(rs.randint(1, len(stations) + 1)), dup)
        path = os.path.join(tmp, f"{name}.json")
        with open(path, "w") as fh:
            json.dump(stations, fh)
        files[name] = path
    cfg = {"time": {"now": now, "analysis": ANALYSIS_H, "forecast": FORECAST_H},
           "output": {"filename": os.path.join(tmp, "forecast.json")},
           "input": [{"name": name, "path": files[name], "type": "json",
                      "source": "forecast" if name == "fc" else "observations"} for name in spec.order]}
    if spec.coupling_minutes is not None:
        cfg["time"]["coupling_minutes"] = spec.coupling_minutes
    if spec.step is not None:
        cfg["output"]["step"] = spec.step
    if spec.model:
        cfg["model"] = {"use_relaxation": int(spec.relaxation), "use_coupling": int(spec.coupling)}
        if spec.dtsecs != 30:
            cfg["model"]["DTSecs"] = spec.dtsecs
    # The time always comes the way -t gives it.  time.now alone cannot be held to the reference: get_forecast_time
    # (InputSettings.cpp:17-25) hands mktime a struct tm whose tm_sec nothing has set, so the reference's own
    # forecast time is then whatever lay on the stack ("not pinned").
    cli_time = ft
    if spec.cli_time:  # the file's time.now is another day: -t has to win
        cfg["time"]["now"] = "20231224T1800"
    pr = {}
    if spec.params:
        pr.update({"Albedo": 0.12, "Albedo_Surroundings": 0.2, "ZMom": 0.35, "TClimG": 5.5, "Emiss": 0.93,
                   "MaxPormms": 1.25, "NightOn": 20, "PLimSnow": 0.25})
    if spec.sky in ("sky", "both"):
        rows = [(sid, float(rs.choice([0.0, 1.0, 0.35, 0.85, 1.3, -0.2, float(rs.uniform(0.2, 1.0))])))
                for sid in master if rs.rand() < 0.6] + [(extra[3], 0.5)]
        rows.insert(len(rows) // 2, (rows[0][0], 0.0625))  # a repeated id: the first row counts
        text = "\n".join(f"{sid} st{sid} {lat[sid]!r} {lon[sid]!r} {f!r}" for sid, f in rows)
        pr["sky_view_file"] = os.path.join(tmp, "skyview.txt")
        with open(pr["sky_view_file"], "w") as fh:
            fh.write(text + ("\n" if spec.seed % 2 else ""))
    if spec.sky in ("hz", "both"):
        who = [sid for sid in master if rs.rand() < 0.5] + [extra[0]]
        who.append(who[1])  # a repeated id: the last row counts
        lines = []
        for sid in who:
            hz = np.round(np.clip(rs.normal(6, 8, 360), 0, 60), 1)
            lines.append(f"{sid} st{sid} {lat[sid]!r} {lon[sid]!r} " + " ".join(repr(float(x)) for x in hz))
        pr["local_horizon_file"] = os.path.join(tmp, "horizons.txt")
        with open(pr["local_horizon_file"], "w") as fh:
            fh.write("\n".join(lines) + ("\n" if spec.seed % 4 == 0 else ""))
    if pr:
        cfg["parameters"] = pr
    config = os.path.join(tmp, "config.json")
    with open(config, "w") as fh:
        json.dump(cfg, fh, indent=1)
    return {"config": config, "cli_time": cli_time, "tz": tz, "spec": spec, "cfg": cfg}


def single_source_configs(tmp, case: dict) -> list:
    """One configuration per source of ``case``, each with that source alone (for telling which source a merged
    value came from, on the reference's results alone)."""
    out = []
    for j, src in enumerate(case["cfg"]["input"]):
        cfg = dict(case["cfg"], input=[src])
        path = os.path.join(str(tmp), f"config_only_{j}.json")
        with open(path, "w") as fh:
            json.dump(cfg, fh)
        out.append(path)
    return out


# ---- the two sides ------------------------------------------------------------------------------------------------

def copy_local(local):
    arr = (abi.LocalParameters * len(local))()
    C.memmove(arr, local, C.sizeof(arr))
    return arr


def reference_view(case: dict) -> dict:
    with Ref(case["config"], case["cli_time"]) as r:
        v = r.read_input()
        v.update(ids=r.ids, lat=r.lat, lon=r.lon, settings=r.settings, parameters=r.parameters,
                 forecast_time=r.forecast_time, start_time=r.start_time, end_time=r.end_time, simlen=r.simlen)
    return v


def reference_run(case: dict) -> dict:
    with Ref(case["config"], case["cli_time"]) as r:
        return r.run()


def project_view(case: dict) -> dict:
    """roadrunner.prepare -> driver.make_input -> oracle/driver_oracle.c."""
    pc = roadrunner.prepare(case["config"], case["cli_time"] or None)
    ri = dh.oracle_read_input(pc.sources, pc.settings, pc.start_time, pc.forecast_time, copy_local(pc.local))
    return {"case": pc, "read_input": ri}


def local_fields(larr) -> dict:
    return {name: np.array([getattr(lp, name) for lp in larr]) for name in LOCAL_REALS + LOCAL_INTS}
