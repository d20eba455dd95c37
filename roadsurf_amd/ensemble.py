"""Ensemble forecasts branched from one analysis run: the definition in numpy, and a runner.

``S`` stations share an analysis - the forcing of the time indices ``1 .. B`` - and every station has ``M`` forecast
members whose forcing differs behind ``B`` only.  The plain way to run them is ``S * M`` unrelated points, every
member carrying a copy of its station's analysis (``replicate`` builds exactly that input: it is the definition of
what an ensemble run returns).  ``run_ensemble`` steps the analysis once per station instead, copies every station's
carried state into its members on the device (``Plan.fanout_from``, rs_hip_state_fanout in include/roadsurf.h) and
steps the members over ``B + 1 .. L`` alone.  The carried state block is all a launch inherits, so the two agree bit
for bit; both plans are made with ``SimLen = L``, because the model's last-index step belongs to index ``L`` only.

Two rules keep the analysis shared ("Ensemble fan-out"):

* with coupling every ``couplingIndexI + 1 <= B``: a replay reads the forcing of the index behind its window;
* with relaxation, member targets that differ from the station's need ``InitLenI >= B``: the targets act at every
  index behind ``InitLenI``.

Sky view is a per-point parameter like the others: a member has its station's geometry and local horizons.
"""
from __future__ import annotations

import numpy as np

from . import abi
from .legs import RELAX_FIELDS, Leg, coupling_stages, feature_set

SHARED_FIELDS = ("InitLenI", "couplingIndexI", "couplingTsurf", "lat", "lon", "sky_view")


def parents(S: int, M: int) -> np.ndarray:
    """The station of every member, members of a station side by side: int32 [S * M]."""
    return np.repeat(np.arange(S, dtype=np.int32), M)


def replicate(station_forcing: dict, member_tail: dict, parent, B: int) -> dict:
    """The forcing ``[len(parent)][L]`` of the equivalent plain run: columns ``< B`` are the parent station's, columns
    ``>= B`` the member's own ``member_tail[name][len(parent)][L - B]``.  One-dimensional entries are the shared time
    axes: the station's first ``B`` values, then the tail's."""
    parent = np.asarray(parent, np.int64)
    out = {}
    if station_forcing.get("local_horizons") is not None:  # per point, not per index: the station's
        out["local_horizons"] = np.ascontiguousarray(np.asarray(station_forcing["local_horizons"])[parent])
    for name, tail in member_tail.items():
        head = np.asarray(station_forcing[name])
        tail = np.asarray(tail)
        if tail.ndim == 1:
            if head.shape[0] < B:
                raise ValueError(f"replicate: {name}: the stations' axis is shorter than B = {B}")
            out[name] = np.ascontiguousarray(np.concatenate([head[:B], tail]).astype(head.dtype, copy=False))
            continue
        if tail.ndim != 2 or tail.shape[0] != len(parent) or head.ndim != 2 or head.shape[1] < B:
            raise ValueError(f"replicate: {name}: stations [S][>= B] and tails [len(parent)][L - B] are required")
        out[name] = np.ascontiguousarray(np.concatenate([head[parent, :B], tail], axis=1).astype(head.dtype, copy=False))
    return out


def _locals(local, n):
    return [local] * n if isinstance(local, abi.LocalParameters) else list(local)


def member_locals(station_local, member_local, parent):
    """Per member: its station's parameters, with the member's own relaxation targets where ``member_local`` gives
    them.  Anything else in ``member_local`` must be the station's."""
    parent = np.asarray(parent, np.int64)
    out = []
    ml = None if member_local is None else _locals(member_local, len(parent))
    for m, q in enumerate(parent):
        st = station_local[q]
        li = abi.LocalParameters()
        for name, _ in abi.LocalParameters._fields_:
            setattr(li, name, getattr(st, name))
        if ml is not None:
            for name in SHARED_FIELDS:
                if getattr(ml[m], name) != getattr(st, name):
                    raise ValueError(f"run_ensemble: member {m} differs from its station {int(q)} in {name}: "
                                     "only the three relaxation targets may differ")
            for name in RELAX_FIELDS:
                setattr(li, name, getattr(ml[m], name))
        out.append(li)
    return out


def check(S, L, B, settings, station_local, member_local, parent, precision=64, recluster=False, stats=None,
          probs=None, periods=None) -> None:
    """The refusals of ``run_ensemble`` (ValueError), all of them before any device work."""
    if not 1 <= B <= L - 1:
        raise ValueError(f"run_ensemble: B = {B} outside [1, L - 1 = {L - 1}]: both the analysis and the members "
                         "need an index")
    parent = np.asarray(parent)
    if parent.ndim != 1 or len(parent) < 1 or parent.min() < 0 or parent.max() >= S:
        raise ValueError(f"run_ensemble: parent must name stations in [0, {S})")
    if precision not in (32, 64):
        raise ValueError("run_ensemble: precision is 32 or 64")
    if stats is not None:
        from . import ensstats
        if int(stats.ngroups) != S:
            raise ValueError(f"run_ensemble: stats.ngroups = {int(stats.ngroups)}, but there are S = {S} stations: the "
                             "statistics are per station")
        try:
            ensstats.member_table(parent, stats)   # (and the spec's own limits)
        except ValueError as e:
            raise ValueError(f"run_ensemble: stats: {e}") from None
    if probs is not None:
        from . import ensprob, ensstats
        try:
            ensprob.check_spec(probs)
        except ValueError as e:
            raise ValueError(f"run_ensemble: probs: {e}") from None
        if int(probs.ngroups) != S:
            raise ValueError(f"run_ensemble: probs.ngroups = {int(probs.ngroups)}, but there are S = {S} stations: the "
                             "probabilities are per station")
        try:
            ensstats.member_table(parent, ensprob.table_spec(probs))
        except ValueError as e:
            raise ValueError(f"run_ensemble: probs: {e}") from None
        if ensprob.needs_deficit(probs):
            raise ValueError("run_ensemble: probs: a condition uses the deficit, and the runner has no deficit rows "
                             "(such conditions belong to the device API, whose caller supplies them)")
    if periods is not None:
        from . import periods as periods_
        try:
            periods_.check_spec(periods)
        except ValueError as e:
            raise ValueError(f"run_ensemble: periods: {e}") from None
    coupled = settings.use_coupling == 1
    if coupled and precision == 32:
        raise ValueError("run_ensemble: coupling is fp64 only (the time-chunked coupling calls need the fp64 flavour)")
    if coupled and recluster:
        raise ValueError("run_ensemble: no recluster with coupling (a replay rewrites rows of earlier launches)")
    if coupled:
        for q, l in enumerate(station_local):
            on = not (l.couplingTsurf < -100 or l.couplingIndexI < 1)
            if on and l.couplingIndexI + 1 > B:
                raise ValueError(f"run_ensemble: station {q}: couplingIndexI + 1 = {l.couplingIndexI + 1} > B = {B}: "
                                 "a coupling replay reads the index behind its window, which must be shared")
    if member_local is not None:
        ml = member_locals(station_local, member_local, parent)  # (raises where more than the targets differ)
        if settings.use_relaxation == 1:
            for m, q in enumerate(parent):
                st = station_local[q]
                if st.InitLenI < B and any(getattr(ml[m], k) != getattr(st, k) for k in RELAX_FIELDS):
                    raise ValueError(f"run_ensemble: member {m} has relaxation targets of its own while its station "
                                     f"{int(q)} has InitLenI = {st.InitLenI} < B = {B}: the targets act at every "
                                     "index behind InitLenI, so the analysis would not be shared")


def run_ensemble(station_forcing: dict, member_tail: dict, B: int, settings: abi.InputSettings,
                 params: abi.InputParameters, station_local, member_local=None, parent=None, chunk: int = 0,
                 variant: int = 0, precision: int = 64, recluster: bool = False, groups=None, device: int = 0,
                 timing: dict | None = None, stats=None, probs=None, periods=None):
    """Step ``S`` stations over ``[1, B]``, fan their carried state out to ``len(parent)`` members on the device and
    step those over ``[B + 1, L]``: what ``device.run_points(replicate(...))`` returns for the members, bit for bit,
    without stepping any station's analysis more than once.

    ``station_forcing[name][S][>= B]`` and ``member_tail[name][len(parent)][L - B]`` are host arrays in the reference
    layout (time axes one-dimensional, shared); ``settings.SimLen = L``.  ``station_local``: one LocalParameters or
    ``S`` of them; a member has its station's, except that ``member_local`` (one, or one per member) may give it
    relaxation targets of its own.  ``parent`` defaults to ``parents(S, len(tail) // S)``.  ``chunk``: indices per
    launch (0: a leg in one launch); ``recluster``: ``Plan.recluster()`` behind every launch; ``groups``:
    ``(groups.GroupSpec, ids int32 [len(parent)])`` - the members' rows are also reduced per group on the device;
    ``stats``: an ``ensstats.EnsSpec`` with ``ngroups = S`` - the members' rows are also reduced per STATION on the
    device (group = parent), behind every launch: mean, spread and quantiles of Tsurf, mean storages; ``probs``: an
    ``ensprob.ProbSpec`` with ``ngroups = S`` whose conditions do not use the deficit - the members under each
    condition are also counted per STATION on the device, now and by now, behind every launch in row order;
    ``periods``: a ``periods.PeriodSpec`` in absolute time indices (``first_index = B + 1``: the first period starts
    with the members' first index) - the members' rows are also fed to the per-point aggregates over output periods.

    Returns a dict: ``stations[name][S][B]``, ``members[name][len(parent)][L - B]`` (row r is time index
    ``B + 1 + r``), ``failed`` = (stations, members) counts, with ``groups`` the series ``[L - B, ngroups, cols]`` and
    with ``stats`` the cells ``stats[L - B, S, cols]`` of ``ensstats.reduce_members`` and with ``probs`` the cells
    ``probs[L - B, S, cols]`` of ``ensprob.reduce_members_prob`` (row r is time index ``B + 1 + r``) and with
    ``periods`` the cells ``periods[len(parent), nperiods, RS_PER_COLS]`` of ``periods.reduce_series``.
    Raises ValueError - before any device work - where the analysis would not be shared (``check``)."""
    S = station_forcing["tair"].shape[0]
    nmem, tail_len = member_tail["tair"].shape
    L = int(settings.SimLen)
    if not 1 <= B <= L - 1:
        raise ValueError(f"run_ensemble: B = {B} outside [1, L - 1 = {L - 1}]: both the analysis and the members "
                         "need an index")
    if B + tail_len != L:
        raise ValueError(f"run_ensemble: settings.SimLen = {L}, but B + the tails' length = {B + tail_len}")
    if parent is None:
        if nmem % S:
            raise ValueError("run_ensemble: without parent the members are S * M")
        parent = parents(S, nmem // S)
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    if len(parent) != nmem:
        raise ValueError("run_ensemble: one parent per member tail")
    sl = _locals(station_local, S)
    if len(sl) != S:
        raise ValueError("run_ensemble: one LocalParameters, or one per station")
    check(S, L, B, settings, sl, member_local, parent, precision, recluster, stats, probs, periods)
    if station_forcing["tair"].shape[1] < B:
        raise ValueError(f"run_ensemble: the stations' forcing is shorter than B = {B}")
    ml = member_locals(sl, member_local, parent)
    # the stations' leg reads the first B columns and axis entries; a member has its station's horizons
    head = {k: np.asarray(v)[..., :B] for k, v in station_forcing.items() if k != "local_horizons"}
    tail = dict(member_tail)
    hz = station_forcing.get("local_horizons")
    if hz is not None:
        head["local_horizons"], tail["local_horizons"] = hz, np.asarray(hz)[parent]
    coupled = settings.use_coupling == 1
    need_full, sky_on = feature_set(settings, sl, [head, member_tail])  # one feature set for both legs
    from . import device as dv
    dv.require_gpu()
    common = dict(need_full=need_full, sky_on=sky_on, precision=precision, variant=variant, recluster=recluster,
                  device=device, tbottom_date=tuple(int(station_forcing[k][0]) for k in ("year", "month", "day")))
    st = Leg(head, settings, params, sl, first=1, **common)
    mem = Leg(tail, settings, params, ml, first=B + 1, groups=groups,
              stats=None if stats is None else (stats, parent),
              probs=None if probs is None else (probs, parent), periods=periods, **common)
    st.init()
    st.run(coupling_stages(settings, sl, B, chunked=True), chunk)
    if coupled:  # every window is closed, and the members go on in lock step from where every point resumes, B + 1
        st.plan.coupling_windows_closed(True)
    ev = None
    if timing is not None:
        ev = [st.torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(mem.plan.stream)
    mem.plan.fanout_from(st.plan, parent)
    if ev:
        ev[1].record(mem.plan.stream)
    mem.chunks(B + 1, L, chunk, "step_cpl" if coupled else "step")
    res = {"stations": st.results(), "members": mem.results()}
    res["failed"] = (st.plan.failed_count(), mem.plan.failed_count())
    res.update(mem.reduced())
    if ev:
        timing["fanout_ms"] = float(ev[0].elapsed_time(ev[1]))
    st.plan.close()
    mem.plan.close()
    return res
