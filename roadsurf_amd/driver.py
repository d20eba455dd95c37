"""Host mirror of the reference driver's data path (layer 4 of ``include/roadsurf.h``).

The names follow ``examples/example1/src``: a *source* is what ``JsonSource`` holds after
parsing (raw series on the source's own time axis), ``read_input`` is what
``roadrunner.cpp:156-278`` returns for a point (series at simulation resolution plus the
relaxation / coupling decisions) and ``run`` is ``read_input`` + ``runsimulation`` +
``save_output``'s decimation for a whole batch, with the per-value work on the GPU
(``roadsurf_amd/csrc/rs_driver.hip``).  Only file formats are handled here on the host:
``read_json_source`` / ``save_output`` read and write the reference's JSON schema
(``JsonSource.cpp:182-316``, ``roadrunner.cpp:285-347``).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import time as _time

import numpy as np

from . import abi
from . import grid as rsgrid
from . import lib as rslib

RS_MAX_SOURCES = 4
#: order of ``merged`` in rs_driver_expand
MERGED_FIELDS = ("tair", "tdew", "vz", "rhz", "prec", "sw", "lw", "sw_dir", "lw_net", "tsurfobs")
#: member order of RsRawSource
RAW_FIELDS = ("tair", "rhz", "tdew", "vz", "prec", "lw_net", "lw", "sw", "sw_dir", "tsurfobs")
OUT_FIELDS = ("tsurf", "snow", "water", "ice", "deposit", "ice2")
CALENDAR = ("year", "month", "day", "hour", "minute", "second")
#: variable names of the reference's JSON input (JsonSource.cpp:192-194) -> our field names;
#: "PrecipitationForm" is read by the reference but never handed on (JsonSource.cpp:323-373)
JSON_VARIABLES = {
    "Temperature 2m": "tair", "Humidity": "rhz", "DewPoint": "tdew", "WindSpeed": "vz",
    "Precipitation": "prec", "RadiationNetSurfaceLW": "lw_net", "RadiationLW": "lw",
    "RadiationGlobal": "sw", "RadiationDirectSW": "sw_dir", "RoadTemperature": "tsurfobs",
}

c_int64_p = C.POINTER(C.c_int64)


class RsRawSource(C.Structure):
    _fields_ = [("n_times", C.c_int32), ("is_observation", C.c_int32), ("times", c_int64_p)] + [
        (n, abi.c_double_p) for n in RAW_FIELDS
    ] + [("times_per_point", C.c_int32), ("lengths", abi.c_int32_p)]


class RsDriverInput(C.Structure):
    _fields_ = [
        ("n_points", C.c_int32), ("n_sources", C.c_int32), ("sources", C.POINTER(RsRawSource)),
        ("start_time", C.c_int64), ("forecast_time", C.c_int64),
    ] + [(n, abi.c_int32_p) for n in CALENDAR] + [("horizons", abi.c_double_p)]


class RsDriverOutput(C.Structure):
    _fields_ = [("n_out", C.c_int32)] + [(n, abi.c_double_p) for n in OUT_FIELDS] + [
        ("status", abi.c_int32_p), ("missing_index", abi.c_int32_p)
    ]


class RsDriverSummary(C.Structure):
    _fields_ = [("spec", rslib.RsSummarySpec), ("first_row", C.c_int32), ("last_row", C.c_int32),
                ("summary", abi.c_double_p)]


class RsDriverGroups(C.Structure):
    _fields_ = [("spec", rslib.RsGroupSpec), ("group", abi.c_int32_p), ("first_row", C.c_int32),
                ("last_row", C.c_int32), ("series", abi.c_double_p)]


class RsGridSource(C.Structure):
    _fields_ = [("n_nodes", C.c_int64)] + [(n, abi.c_double_p) for n in RAW_FIELDS] + [
        ("stencil", C.c_int32), ("node", abi.c_int32_p), ("weight", abi.c_double_p)]


class RsDriverKept(C.Structure):
    _fields_ = [("merged", abi.c_double_p * len(MERGED_FIELDS)), ("deficit", abi.c_double_p)]


class RsDriverEpisodes(C.Structure):
    _fields_ = [("spec", rslib.RsEpisodeSpec), ("first_row", C.c_int32), ("last_row", C.c_int32),
                ("episodes", abi.c_double_p)]


class RsDriverRequest(C.Structure):
    _fields_ = [("grids", C.POINTER(C.POINTER(RsGridSource))), ("summary", C.POINTER(RsDriverSummary)),
                ("groups", C.POINTER(RsDriverGroups)), ("kept", C.POINTER(RsDriverKept)),
                ("episodes", C.POINTER(RsDriverEpisodes))]


class RsDriverEnsemble(C.Structure):
    _fields_ = [("n_members", C.c_int32), ("position", C.c_int32), ("parent", abi.c_int32_p), ("member", RsRawSource),
                ("member_out", RsDriverOutput), ("member_local", C.POINTER(abi.LocalParameters)),
                ("stats_spec", C.POINTER(rslib.RsEnsSpec)), ("stats", abi.c_double_p),
                ("probs_spec", C.POINTER(rslib.RsProbSpec)), ("probs", abi.c_double_p),
                ("branch_index", C.c_int32), ("first_row", C.c_int32)]


@dataclasses.dataclass
class RawSource:
    """One data source: ``fields`` name -> [n_points][n_times] float64 (absent name = variable
    not in the source) and ``times`` epoch seconds, either [n_times] shared by all points or
    [n_points][n_times] with one axis per point; ``lengths`` [n_points] then says how many
    leading entries of each row are real (rows are padded to a common width)."""
    times: np.ndarray
    fields: dict
    is_observation: bool = False
    lengths: np.ndarray | None = None


def calendar(start_time: int, simlen: int, dtsecs: int, utc: bool = True) -> dict:
    """Calendar arrays of the simulation times (JsonSource.cpp:297-308 uses localtime)."""
    conv = _time.gmtime if utc else _time.localtime
    ax = {k: np.empty(simlen, np.int32) for k in CALENDAR}
    for i in range(simlen):
        tt = conv(start_time + i * dtsecs)
        ax["year"][i], ax["month"][i], ax["day"][i] = tt.tm_year, tt.tm_mon, tt.tm_mday
        ax["hour"][i], ax["minute"][i], ax["second"][i] = tt.tm_hour, tt.tm_min, tt.tm_sec
    return ax


def output_rows(settings: abi.InputSettings) -> tuple[int, int]:
    """(step, n_out) of save_output, roadrunner.cpp:290,303."""
    step = int(settings.outputStep * 60 / settings.DTSecs)
    if step < 1:
        raise ValueError("outputStep*60/DTSecs < 1")
    return step, (settings.SimLen + step - 1) // step


def forecast_rows(settings: abi.InputSettings, start_time: int, forecast_time: int) -> tuple[int, int]:
    """(first_row, last_row) of the kept rows at or behind ``forecast_time``: the forecast part of a run, what
    ``run(..., summary_rows=...)`` is usually given."""
    step, n_out = output_rows(settings)
    i = max(0, -(-(int(forecast_time) - int(start_time)) // int(settings.DTSecs)))  # first 0-based index at or behind it
    return min(-(-i // step), n_out - 1), n_out - 1


def make_input(sources, start_time: int, forecast_time: int, cal: dict | None = None,
               horizons: np.ndarray | None = None, n_points: int | None = None):
    """Build the C struct.  Returns (RsDriverInput, keepalive list).  ``n_points``: the number of points where it is
    known beforehand (``make_grid_input``: a source without fields of its own does not tell)."""
    if not 1 <= len(sources) <= RS_MAX_SOURCES:
        raise ValueError(f"1..{RS_MAX_SOURCES} sources")
    keep = []
    arr = (RsRawSource * len(sources))()
    for k, s in enumerate(sources):
        t = np.ascontiguousarray(s.times, np.int64)
        keep.append(t)
        width = t.shape[-1]
        arr[k].n_times = width
        arr[k].is_observation = 1 if s.is_observation else 0
        arr[k].times = t.ctypes.data_as(c_int64_p)
        arr[k].times_per_point = 1 if t.ndim == 2 else 0
        if t.ndim == 2:
            if n_points is None:
                n_points = t.shape[0]
            elif t.shape[0] != n_points:
                raise ValueError("all sources must hold the same points")
            if s.lengths is not None:
                ln = np.ascontiguousarray(s.lengths, np.int32)
                if ln.shape != (t.shape[0],) or ln.min() < 0 or ln.max() > width:
                    raise ValueError("lengths: [n_points] values in 0..n_times")
                keep.append(ln)
                arr[k].lengths = ln.ctypes.data_as(abi.c_int32_p)
        elif s.lengths is not None:
            raise ValueError("lengths needs per-point time axes")
        for name, a in s.fields.items():
            if name not in RAW_FIELDS:
                raise KeyError(name)
            a = np.ascontiguousarray(a, np.float64)
            if a.ndim != 2 or a.shape[1] != width:
                raise ValueError(f"{name}: expected [n_points][{width}], got {a.shape}")
            if n_points is None:
                n_points = a.shape[0]
            elif a.shape[0] != n_points:
                raise ValueError("all sources must hold the same points")
            keep.append(a)
            setattr(arr[k], name, a.ctypes.data_as(abi.c_double_p))
    if n_points is None:
        raise ValueError("no data")
    inp = RsDriverInput()
    inp.n_points = n_points
    inp.n_sources = len(sources)
    inp.sources = arr
    inp.start_time = int(start_time)
    inp.forecast_time = int(forecast_time)
    keep.append(arr)
    if cal is not None:
        for k in CALENDAR:
            a = np.ascontiguousarray(cal[k], np.int32)
            keep.append(a)
            setattr(inp, k, a.ctypes.data_as(abi.c_int32_p))
    if horizons is not None:
        h = np.ascontiguousarray(horizons, np.float64)
        if h.shape != (n_points, 360):
            raise ValueError("horizons: [n_points][360]")
        keep.append(h)
        inp.horizons = h.ctypes.data_as(abi.c_double_p)
    return inp, keep


def make_grid_input(sources, start_time: int, forecast_time: int, cal: dict | None = None,
                    horizons: np.ndarray | None = None):
    """``make_input`` for a list that may hold ``grid.GridSource`` entries among the ``RawSource`` ones.  Returns
    (RsDriverInput, grids, keepalive list): ``grids`` is the ``RsGridSource *[n_sources]`` of RsDriverRequest::grids
    (NULL entry = per-point source), or None when no source is gridded.  A gridded source's RsRawSource carries
    its time axis and is_observation only."""
    gridded = [isinstance(s, rsgrid.GridSource) for s in sources]
    if not any(gridded):
        inp, keep = make_input(sources, start_time, forecast_time, cal, horizons)
        return inp, None, keep
    n_points = {s.n_points for s, g in zip(sources, gridded) if g}
    if len(n_points) != 1:
        raise ValueError("all sources must hold the same points")
    plain = [RawSource(s.times, {}, s.is_observation) if g else s for s, g in zip(sources, gridded)]
    inp, keep = make_input(plain, start_time, forecast_time, cal, horizons, n_points=n_points.pop())
    structs = (RsGridSource * len(sources))()
    grids = (C.POINTER(RsGridSource) * len(sources))()
    for k, (s, g) in enumerate(zip(sources, gridded)):
        if not g:
            continue
        for name, a in s.fields.items():
            if name not in RAW_FIELDS:
                raise KeyError(name)
            setattr(structs[k], name, a.ctypes.data_as(abi.c_double_p))
        structs[k].n_nodes = s.n_nodes
        structs[k].stencil = s.node.shape[1]
        structs[k].node = s.node.ctypes.data_as(abi.c_int32_p)
        structs[k].weight = s.weight.ctypes.data_as(abi.c_double_p)
        grids[k] = C.pointer(structs[k])
        keep.append(s)
    keep.append(structs)
    return inp, grids, keep


def _locals(n: int, local) -> C.Array:
    """LocalParameters[n]: None -> defaults, one struct -> replicated, a list, or a ready
    ctypes array (used as is: it is also where the decisions are written back)."""
    if isinstance(local, C.Array):
        if len(local) != n:
            raise ValueError("local: wrong length")
        return local
    if local is None:
        local = abi.default_local()
    if isinstance(local, abi.LocalParameters):
        arr = (abi.LocalParameters * n)()
        tmpl = bytes(local)
        C.memmove(arr, tmpl * n, len(tmpl) * n)
        return arr
    return (abi.LocalParameters * n)(*local)


def _bind(L):
    """Argument types of the driver's entries: rs_driver_run_request, and the older entries (the tests call them), each
    of which is the run's five arguments, the members of RsDriverRequest it can express - the grids in front - and the
    device."""
    P = C.POINTER
    if not hasattr(L, "rs_driver_run_request"):
        raise RuntimeError("this libroadsurf_hip.so has no request form of the driver (rs_driver_run_request)")
    run = [P(RsDriverInput), P(abi.InputSettings), P(abi.InputParameters), P(abi.LocalParameters), P(RsDriverOutput)]
    grids, s, g, k, e = P(P(RsGridSource)), P(RsDriverSummary), P(RsDriverGroups), P(RsDriverKept), P(RsDriverEpisodes)
    L.rs_driver_run_request.argtypes = run + [P(RsDriverRequest), C.c_int32]
    for name, front, members in (("rs_driver_run", [], []), ("rs_driver_run_summary", [], [s]),
                                 ("rs_driver_run_groups", [], [s, g]), ("rs_driver_run_grid", [grids], [s, g]),
                                 ("rs_driver_run_kept", [grids], [s, g, k]),
                                 ("rs_driver_run_episodes", [grids], [s, g, k, e])):
        getattr(L, name).argtypes = run[:1] + front + run[1:] + members + [C.c_int32]
    expand = [P(abi.InputSettings), P(abi.LocalParameters), abi.c_double_p, abi.c_int32_p, abi.c_int32_p, C.c_int32]
    L.rs_driver_expand.argtypes = run[:1] + expand
    L.rs_driver_expand_grid.argtypes = run[:1] + [grids] + expand
    L.rs_driver_kept_fields.restype = C.c_int32
    return L


def _need_grids(L) -> None:
    if L.rs_hip_grid_max_stencil() != rsgrid.MAX_STENCIL:
        raise RuntimeError("this libroadsurf_hip.so has no gridded sources (rs_hip_grid_max_stencil)")


def read_input(sources, settings: abi.InputSettings, start_time: int, forecast_time: int,
               local=None, device: int = 0) -> dict:
    """What ``read_input`` (roadrunner.cpp:156-278) produces for every point, computed on the
    GPU: ``merged`` name -> [n][SimLen], ``status``, ``missing_index``, ``local``.  ``sources`` may hold
    ``grid.GridSource`` entries (rs_driver_expand_grid)."""
    L = _bind(rslib.load())
    inp, grids, keep = make_grid_input(sources, start_time, forecast_time)
    n, simlen = inp.n_points, settings.SimLen
    larr = _locals(n, local)
    merged = np.empty((len(MERGED_FIELDS), n, simlen), np.float64)
    status = np.empty(n, np.int32)
    mi = np.empty(n, np.int32)
    if grids is not None:
        _need_grids(L)
        rslib.check(L.rs_driver_expand_grid(C.byref(inp), grids, C.byref(settings), larr,
                                            merged.ctypes.data_as(abi.c_double_p),
                                            status.ctypes.data_as(abi.c_int32_p),
                                            mi.ctypes.data_as(abi.c_int32_p), device), "rs_driver_expand_grid")
    else:
        rslib.check(L.rs_driver_expand(C.byref(inp), C.byref(settings), larr,
                                       merged.ctypes.data_as(abi.c_double_p),
                                       status.ctypes.data_as(abi.c_int32_p),
                                       mi.ctypes.data_as(abi.c_int32_p), device), "rs_driver_expand")
    del keep
    return {"merged": {k: merged[i] for i, k in enumerate(MERGED_FIELDS)}, "status": status,
            "missing_index": mi, "local": larr}


def run(sources, settings: abi.InputSettings, params: abi.InputParameters, start_time: int,
        forecast_time: int, local=None, cal: dict | None = None,
        horizons: np.ndarray | None = None, device: int = 0, out: dict | None = None,
        summary=None, summary_rows: tuple[int, int] | None = None, series: bool = True,
        groups=None, group_of=None, group_rows: tuple[int, int] | None = None,
        kept=(), deficit: bool = False, episodes=None, episode_rows: tuple[int, int] | None = None) -> dict:
    """read_input + runsimulation + save_output's decimation for all points.  Returns the six
    outputs as [n][n_out] arrays plus ``status``, ``missing_index``, ``local`` and ``step``.  One call of
    rs_driver_run_request, whatever is asked for: the entries named below are the older ones that take the same member.
    ``device`` < 0 fans the points out over ROADSURF_HIP_DEVICES; ``out`` = a result dict of an
    earlier call with the same shapes, whose arrays are written again (no fresh allocation; its ``kept`` and
    ``deficit`` arrays too).
    ``summary`` = a summary.SummarySpec: the result also has ``summary``, float64 [n][RS_SUM_COLS], the per-point
    summaries (roadsurf_amd/summary.py) of the kept rows ``summary_rows`` = (first_row, last_row) - default all
    of them, ``forecast_rows`` gives the forecast part - reduced on the device (rs_driver_run_summary);
    ``series=False`` then leaves the six series out of the result: nothing but the summaries is downloaded.
    ``groups`` = a groups.GroupSpec with ``group_of`` = every point's group id, int32 [n]: the result also has
    ``groups``, float64 [rows][ngroups][cols], the per-group series (roadsurf_amd/groups.py) of the kept rows
    ``group_rows`` = (first_row, last_row), default all of them (rs_driver_run_groups); counts as a summary for
    ``series=False``.
    ``sources`` may hold ``grid.GridSource`` entries, mixed with ``RawSource`` ones: their fields go to the device
    as they are and are gathered to the points there (rs_driver_run_grid); the result is that of the same call on
    ``grid.to_raw_source`` of them.
    ``kept`` = names among ``MERGED_FIELDS``: the result also has ``kept``, name -> float64 [n][n_out], the inputs the
    model saw at the kept rows - ``read_input``'s ``merged`` at every ``step``-th index (roadsurf_amd/kept.py), for
    every point, rejected ones included - made on the device from the raw series (rs_driver_run_kept).
    ``deficit=True``: the result also has ``deficit``, float64 [n][n_out], ``kept.dew_point_deficit`` of the final
    surface temperature rows and the kept dew point.  Either counts as a summary for ``series=False``.
    ``episodes`` = an episodes.EpisodeSpec: the result also has ``episodes``, float64 [n][cols], the finished per-point
    threshold episodes (roadsurf_amd/episodes.py; ``episodes.decode`` reads them) of the kept rows ``episode_rows`` =
    (first_row, last_row) - default the forecast part, ``forecast_rows`` - reduced on the device
    (rs_driver_run_episodes); a spec that needs the deficit has it made there whether or not ``deficit`` is asked
    for.  Counts as a summary for ``series=False``."""
    L = _bind(rslib.load())
    kept = tuple(kept or ())
    for name in kept:
        if name not in MERGED_FIELDS:
            raise KeyError(name)
    want_kept = bool(kept) or bool(deficit)
    if want_kept and L.rs_driver_kept_fields() != len(MERGED_FIELDS):
        raise RuntimeError("this libroadsurf_hip.so has no kept input rows (rs_driver_kept_fields)")
    if cal is None:
        cal = calendar(start_time, settings.SimLen, int(settings.DTSecs))
    inp, grids, keep = make_grid_input(sources, start_time, forecast_time, cal, horizons)
    if grids is not None:
        _need_grids(L)
    n = inp.n_points
    step, n_out = output_rows(settings)
    larr = _locals(n, local)
    if not series and summary is None and groups is None and not want_kept and episodes is None:
        raise ValueError("series=False needs a summary, groups, kept, deficit or episodes")
    earlier = out if out is not None else {}

    def rows(old):  # an [n][n_out] array of the earlier result, or a fresh one
        ok = old is not None and old.shape == (n, n_out) and old.dtype == np.float64 and old.flags.c_contiguous
        return old if ok else np.full((n, n_out), np.nan)
    if out is not None and series and out["tsurf"].shape == (n, n_out):
        res = {k: out[k] for k in OUT_FIELDS + ("status", "missing_index")}
    else:
        res = {k: np.full((n, n_out), np.nan) for k in OUT_FIELDS} if series else {}
        res["status"] = np.empty(n, np.int32)
        res["missing_index"] = np.empty(n, np.int32)
    out = RsDriverOutput()
    out.n_out = n_out
    if series:  # (a NULL series pointer = not wanted)
        for k in OUT_FIELDS:
            setattr(out, k, res[k].ctypes.data_as(abi.c_double_p))
    out.status = res["status"].ctypes.data_as(abi.c_int32_p)
    out.missing_index = res["missing_index"].ctypes.data_as(abi.c_int32_p)
    req = RsDriverRequest(grids=grids)  # (its members keep what they point to alive)
    if summary is not None:
        if L.rs_hip_summary_cols() != rslib.RS_SUM_COLS:
            raise RuntimeError("this libroadsurf_hip.so has no summaries (rs_hip_summary_cols)")
        first, last = (0, n_out - 1) if summary_rows is None else summary_rows
        res["summary"] = np.full((n, rslib.RS_SUM_COLS), np.nan)
        req.summary = C.pointer(RsDriverSummary(rslib.summary_spec(summary), int(first), int(last),
                                                res["summary"].ctypes.data_as(abi.c_double_p)))
    if groups is not None:
        gfirst, glast = (0, n_out - 1) if group_rows is None else (int(group_rows[0]), int(group_rows[1]))
        gid = np.ascontiguousarray(group_of, dtype=np.int32)
        if gid.shape != (n,):
            raise ValueError("group_of: one group id per point")
        res["groups"] = np.full((max(glast - gfirst + 1, 1), int(groups.ngroups), rslib.group_cols(groups)), np.nan)
        req.groups = C.pointer(RsDriverGroups(rslib.group_spec(groups), gid.ctypes.data_as(abi.c_int32_p), gfirst, glast,
                                              res["groups"].ctypes.data_as(abi.c_double_p)))
    if episodes is not None:
        efirst, elast = forecast_rows(settings, start_time, forecast_time) if episode_rows is None else episode_rows
        res["episodes"] = np.full((n, rslib.episode_cols(episodes)), np.nan)
        req.episodes = C.pointer(RsDriverEpisodes(rslib.episode_spec(episodes), int(efirst), int(elast),
                                                  res["episodes"].ctypes.data_as(abi.c_double_p)))
    if want_kept:
        kq = RsDriverKept()
        res["kept"] = {name: rows(earlier.get("kept", {}).get(name)) for name in kept}
        for name, a in res["kept"].items():
            kq.merged[MERGED_FIELDS.index(name)] = a.ctypes.data_as(abi.c_double_p)
        if deficit:
            res["deficit"] = rows(earlier.get("deficit"))
            kq.deficit = res["deficit"].ctypes.data_as(abi.c_double_p)
        req.kept = C.pointer(kq)
    rslib.check(L.rs_driver_run_request(C.byref(inp), C.byref(settings), C.byref(params), larr, C.byref(out),
                                        C.byref(req), device), "rs_driver_run_request")
    del keep
    res["local"] = larr
    res["step"] = step
    return res


# ---- the ensemble form: one analysis per station, members over the forecast alone --------

def branch_index(start_time: int, dtsecs: int, simlen: int, member_time0: int) -> int:
    """``B``, the last 1-based time index the members share with their station, for a member source whose first raw
    time is ``member_time0``: ``JsonSource::interpolate`` writes nothing to a simulation time before a source's first
    raw time, so with ``k_b`` the smallest 0-based simulation index with ``start_time + k*dtsecs >= member_time0`` the
    indices ``k < k_b`` do not see the source, and ``B = k_b``.  ValueError where the member source starts at or
    before ``start_time`` (index 1 is the stations') or ``B`` leaves ``[1, simlen - 1]``."""
    start_time, dtsecs, simlen, member_time0 = int(start_time), int(dtsecs), int(simlen), int(member_time0)
    if dtsecs < 1 or simlen < 1:
        raise ValueError("branch_index: DTSecs >= 1 and SimLen >= 1 are required")
    if member_time0 <= start_time:
        raise ValueError(f"branch_index: the member source starts at {member_time0}, at or before start_time = "
                         f"{start_time}: times[0] > start_time is required")
    k = -(-(member_time0 - start_time) // dtsecs)
    if not 1 <= k <= simlen - 1:
        raise ValueError(f"branch_index: B = {k} outside [1, SimLen - 1 = {simlen - 1}]: both the stations and the "
                         "members need an index")
    return k


def member_rows(settings: abi.InputSettings, start_time: int, member_time0: int) -> tuple[int, int, int]:
    """(B, first_row, n_tail) of an ensemble call: kept row r is the 0-based index ``r*step`` (roadrunner.cpp:303),
    so ``first_row = ceil(B / step)`` is the first kept row that is a member's own and ``n_tail = n_out - first_row``
    the rows a member has."""
    step, n_out = output_rows(settings)
    B = branch_index(start_time, int(settings.DTSecs), settings.SimLen, member_time0)
    first_row = -(-B // step)
    return B, first_row, n_out - first_row


def check_parent(parent, n_stations: int) -> np.ndarray:
    """``parent`` as int32 [n_members]: non-decreasing - the members of a station side by side, a station may have
    none - with every entry in ``[0, n_stations)``; ValueError names the first member that is not."""
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    if parent.ndim != 1 or len(parent) < 1:
        raise ValueError("parent: one station per member, at least one member")
    for q, s in enumerate(parent):
        if not 0 <= s < n_stations:
            raise ValueError(f"member {q}: parent {int(s)} outside [0, n_stations = {n_stations})")
        if q and s < parent[q - 1]:
            raise ValueError(f"member {q}: parent {int(s)} below member {q - 1}'s parent {int(parent[q - 1])}: parent "
                             "must be non-decreasing")
    return parent


def default_position(shared_sources) -> int:
    """Where the member source goes by default: directly behind the non-observation shared sources that lead the
    list, before the first observation one."""
    k = 0
    while k < len(shared_sources) and not shared_sources[k].is_observation:
        k += 1
    return k


def replicate_sources(shared_sources, member_source: RawSource, parent, position: int | None = None) -> list:
    """The input of the plain run an ensemble call is defined by: every shared source row-gathered by ``parent`` as
    bit copies (``a[parent]``: fields, per-point time axes and lengths; of a ``grid.GridSource`` the stencils - its
    fields are shared as they are), and the member source inserted at ``position`` of the overlay order, where later
    sources win.  Pure numpy."""
    parent = np.asarray(parent, np.int64)
    position = default_position(shared_sources) if position is None else int(position)
    if not 0 <= position <= len(shared_sources):
        raise ValueError(f"position = {position} outside [0, {len(shared_sources)}]")
    out = []
    for s in shared_sources:
        if isinstance(s, rsgrid.GridSource):
            out.append(rsgrid.GridSource(s.times, s.fields, np.ascontiguousarray(s.node[parent]),
                                         np.ascontiguousarray(s.weight[parent]), s.is_observation))
            continue
        t = np.asarray(s.times)
        out.append(RawSource(np.ascontiguousarray(t[parent]) if t.ndim == 2 else t,
                             {k: np.ascontiguousarray(np.asarray(a)[parent]) for k, a in s.fields.items()},
                             s.is_observation,
                             None if s.lengths is None else np.ascontiguousarray(np.asarray(s.lengths)[parent])))
    out.insert(position, member_source)
    return out


def _bind_ensemble(L):
    if not hasattr(L, "rs_driver_run_ensemble"):
        raise RuntimeError("this libroadsurf_hip.so has no ensemble form of the driver (rs_driver_run_ensemble)")
    L.rs_driver_ensemble_bytes.restype = C.c_int64
    if L.rs_driver_ensemble_bytes() != C.sizeof(RsDriverEnsemble):
        raise RuntimeError("RsDriverEnsemble: the library's struct and the binding's differ in size")
    P = C.POINTER
    L.rs_driver_run_ensemble.argtypes = [P(RsDriverInput), P(P(RsGridSource)), P(abi.InputSettings),
                                         P(abi.InputParameters), P(abi.LocalParameters), P(RsDriverOutput),
                                         P(RsDriverEnsemble), C.c_int32]
    return L


def run_ensemble(shared_sources, member_source: RawSource, parent, settings: abi.InputSettings,
                 params: abi.InputParameters, start_time: int, forecast_time: int, position: int | None = None,
                 local=None, horizons: np.ndarray | None = None, device: int = 0, series: bool = True,
                 stats=None, probs=None, out: dict | None = None) -> dict:
    """The ensemble form of ``run`` (rs_driver_run_ensemble): ``shared_sources`` hold the stations - per-point or
    gridded, as ``run`` takes them - and ``member_source`` [n_members][n_times] on one shared time axis is what the
    members of a station see in addition, at ``position`` of the overlay order (default ``default_position``);
    ``parent`` [n_members] names every member's station, non-decreasing.  The analysis is stepped once per station, the
    carried state fanned out on the device, the members stepped over the forecast alone.  By definition the members get
    what ``run(replicate_sources(...), ...)`` returns - status, missing_index, the decisions in ``local`` and the six
    series at the kept rows from ``first_row`` on - and the stations what ``run(shared_sources, ...)`` returns at the
    kept rows before ``first_row`` (later rows read -9999.0).

    Returns a dict: ``stations`` like ``run``'s result (arrays [n_stations][n_out]), ``members`` likewise with arrays
    [n_members][n_tail] (``series=False``: no series in it, and none downloaded), ``branch_index``, ``first_row``,
    and with ``stats`` = an ``ensstats.EnsSpec`` / ``probs`` = an ``ensprob.ProbSpec`` (``ngroups`` = the stations) the
    cells ``stats[n_tail][n_stations][cols]`` / ``probs[n_tail][n_stations][cols]`` of ``ensstats.reduce_members`` /
    ``ensprob.reduce_members_prob`` over the members' rows, group = parent.  ``local``: the stations' parameters (in:
    lat, lon, sky_view; out: the decisions); a member has its station's.  ``out``: the result of an earlier call of
    the same shapes, whose arrays are written again.  The library refuses - RuntimeError with its reason - what would
    not keep the analysis shared (include/roadsurf.h lists the refusals)."""
    L = _bind_ensemble(_bind(rslib.load()))
    cal = calendar(start_time, settings.SimLen, int(settings.DTSecs))
    inp, grids, keep = make_grid_input(shared_sources, start_time, forecast_time, cal, horizons)
    if grids is not None:
        _need_grids(L)
    S = inp.n_points
    step, n_out = output_rows(settings)
    position = default_position(shared_sources) if position is None else int(position)
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    if parent.ndim != 1 or len(parent) < 1:
        raise ValueError("parent: one station per member, at least one member")
    nmem = len(parent)
    mt = np.ascontiguousarray(member_source.times, np.int64)
    # the rows a member has; where the library will refuse the branch, any shape does (the call names the reason)
    try:
        _, _, n_tail = member_rows(settings, start_time, int(mt.flat[0]) if mt.size else start_time)
    except ValueError:
        n_tail = 0
    minp, mkeep = make_input([member_source], start_time, forecast_time, n_points=nmem)
    earlier = out or {}
    est, eme = earlier.get("stations", {}), earlier.get("members", {})

    def rows(old, n, w):
        ok = old is not None and old.shape == (n, w) and old.dtype == np.float64 and old.flags.c_contiguous
        return old if ok else np.full((n, w), np.nan)

    def ints(old, n):
        ok = old is not None and old.shape == (n,) and old.dtype == np.int32
        return old if ok else np.empty(n, np.int32)
    st_res = {k: rows(est.get(k), S, n_out) for k in OUT_FIELDS}
    me_res = {k: rows(eme.get(k), nmem, n_tail) for k in OUT_FIELDS} if series else {}
    for res, e, n in ((st_res, est, S), (me_res, eme, nmem)):
        res["status"] = ints(e.get("status"), n)
        res["missing_index"] = ints(e.get("missing_index"), n)
    sout = RsDriverOutput()
    sout.n_out = n_out
    ens = RsDriverEnsemble()
    ens.member_out.n_out = n_tail
    for o, res in ((sout, st_res), (ens.member_out, me_res)):
        for k in OUT_FIELDS:
            if k in res:
                setattr(o, k, res[k].ctypes.data_as(abi.c_double_p))
        o.status = res["status"].ctypes.data_as(abi.c_int32_p)
        o.missing_index = res["missing_index"].ctypes.data_as(abi.c_int32_p)
    larr = _locals(S, local)
    marr = (abi.LocalParameters * nmem)()
    ens.n_members = nmem
    ens.position = position
    ens.parent = parent.ctypes.data_as(abi.c_int32_p)
    ens.member = minp.sources[0]
    ens.member_local = marr
    result = {"stations": st_res, "members": me_res}
    if stats is not None:
        sp = rslib.ens_spec(stats)
        cols = L.rs_hip_ens_cols(C.byref(sp))
        result["stats"] = np.full((n_tail, S, max(cols, 1)), np.nan)
        ens.stats_spec = C.pointer(sp)
        ens.stats = result["stats"].ctypes.data_as(abi.c_double_p)
    if probs is not None:
        pp = rslib.prob_spec(probs)
        cols = L.rs_hip_prob_cols(C.byref(pp))
        result["probs"] = np.full((n_tail, S, max(cols, 1)), np.nan)
        ens.probs_spec = C.pointer(pp)
        ens.probs = result["probs"].ctypes.data_as(abi.c_double_p)
    rslib.check(L.rs_driver_run_ensemble(C.byref(inp), grids, C.byref(settings), C.byref(params), larr, C.byref(sout),
                                         C.byref(ens), device), "rs_driver_run_ensemble")
    del keep, mkeep
    st_res.update(local=larr, step=step)
    me_res.update(local=marr, step=step)
    result.update(branch_index=int(ens.branch_index), first_row=int(ens.first_row))
    return result


# ---- file formats (host only) ------------------------------------------------------------

def read_json_source(path: str, is_observation: bool = False, utc: bool = True):
    """Parse one input file of the reference's JSON schema (JsonSource.cpp:206-286): a list of
    stations ``{"statId", "lat", "lon", "time": ["%Y-%m-%d %H:%M", ...], "<variable>": [...]}``.
    Returns (RawSource, station ids, lats, lons).  If all stations carry the same time stamps
    the source gets one shared axis, otherwise per-point axes (padded rows + lengths); values
    absent or null become -9999.9."""
    import calendar as _cal

    with open(path) as fh:
        stations = json.load(fh)
    if not stations:  # a file without stations: a source of no points
        return RawSource(np.zeros(0, np.int64), {}, is_observation), [], np.zeros(0), np.zeros(0)
    ids, lats, lons, axes = [], [], [], []
    cols = {v: [] for v in JSON_VARIABLES.values()}
    present = set()
    seconds = {}  # time stamp -> epoch seconds: stations share their stamps, strptime is the slow part

    def epoch(s):
        tm = _time.strptime(s, "%Y-%m-%d %H:%M")
        t = seconds[s] = _cal.timegm(tm) if utc else int(_time.mktime(tm))
        return t

    for st in stations:
        tt = [seconds[s] if s in seconds else epoch(s) for s in st.get("time", [])]
        axes.append(np.asarray(tt, np.int64))
        ids.append(int(st["statId"]))
        lats.append(float(st["lat"]))
        lons.append(float(st["lon"]))
        for jname, name in JSON_VARIABLES.items():
            v = st.get(jname)
            if v is None:
                cols[name].append(np.full(len(tt), -9999.9))
            else:
                present.add(name)
                cols[name].append(np.asarray([-9999.9 if x is None else float(x) for x in v]))
    shared = all(np.array_equal(axes[0], a) for a in axes[1:])
    if shared:
        fields = {k: np.stack(v) for k, v in cols.items() if k in present}
        src = RawSource(axes[0], fields, is_observation)
    else:
        lengths = np.asarray([len(a) for a in axes], np.int32)
        width = int(max(1, lengths.max()))
        times = np.full((len(axes), width), np.iinfo(np.int64).min, np.int64)
        fields = {k: np.full((len(axes), width), -9999.9) for k in cols if k in present}
        for p, a in enumerate(axes):
            times[p, :len(a)] = a
            for k in fields:
                fields[k][p, :len(a)] = cols[k][p]
        src = RawSource(times, fields, is_observation, lengths)
    return src, ids, np.asarray(lats), np.asarray(lons)


def save_output(path: str, result: dict, ids, lats, lons, start_time: int, dtsecs: int, extra: dict | None = None) -> None:
    """Write the forecast like save_output/write_output (roadrunner.cpp:285-347): one object per
    simulated point with the kept times and RoadTemperature/Water/Ice/Snow/Deposit.  Numbers are
    written with Python's shortest round-trip repr (the reference asks jsoncpp for 7 digits).
    ``extra`` = {"tair", "tdew", "deficit"}, [n][n_out] each - ``dict(res["kept"], deficit=res["deficit"])`` of a
    ``run(..., kept=("tair", "tdew"), deficit=True)``: every station also gets "AirTemperature", "DewPoint" and
    "DewPointDeficit", what the reference's operational program stores beside the surface temperature
    (examples/example2/src/QueryDataTools.cpp:323-347).  Without it the file is what it always was."""
    step = result["step"]
    n_out = result["tsurf"].shape[1]
    tstr = [_time.strftime("%Y-%m-%dT%H:%M", _time.gmtime(start_time + r * step * dtsecs))
            for r in range(n_out)]
    forecast = []
    for p in range(len(ids)):
        if result["status"][p] != 0:
            continue  # roadrunner.cpp:393: nothing is written for a rejected point
        forecast.append({
            "statId": int(ids[p]), "lat": float(lats[p]), "lon": float(lons[p]), "time": tstr,
            "RoadTemperature": result["tsurf"][p].tolist(), "Water": result["water"][p].tolist(),
            "Ice": result["ice"][p].tolist(), "Snow": result["snow"][p].tolist(),
            "Deposit": result["deposit"][p].tolist(),
        })
        if extra is not None:
            forecast[-1].update({
                "AirTemperature": np.asarray(extra["tair"])[p].tolist(), "DewPoint": np.asarray(extra["tdew"])[p].tolist(),
                "DewPointDeficit": np.asarray(extra["deficit"])[p].tolist(),
            })
    with open(path, "w") as fh:
        json.dump(forecast, fh, indent=3)
