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

RELAX_FIELDS = ("tair_relax", "VZ_relax", "RH_relax")
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


def check(S, L, B, settings, station_local, member_local, parent, precision=64, recluster=False, stats=None) -> None:
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


class _Leg:
    """One plan and the rows of forcing it steps: row r of its windows is time index ``first + r``."""

    def __init__(self, n, first, forcing, hour, settings, params, local, need_full, precision, variant, recluster,
                 device, tbottom_date, groups=None, sky=None, stats=None):
        import ctypes as C
        import torch
        from . import device as dv, lib
        self.dv, self.torch = dv, torch
        self.n, self.first, self.recluster = n, first, recluster
        self.nrows = forcing["tair"].shape[1]
        self.plan = plan = dv.Plan(n, settings, params, device)
        if variant:
            plan.set_variant(variant)
        if precision == 32:
            plan.set_precision(32)
        self.wdt = wdt = torch.float32 if precision == 32 else torch.float64
        self.dev = dev = plan.device
        self.npad = npad = plan.np_pad
        nrows = self.nrows

        def pad_t(a, dtype):  # [n, nrows] -> device [nrows, npad]
            t = torch.zeros((nrows, npad), dtype=dtype, device=dev)
            t[:, :n] = torch.from_numpy(np.ascontiguousarray(a)).to(dev).T
            return t

        nat = {k: pad_t(forcing[k], wdt) for k in ("tair", "vz", "rhz", "prec", "sw", "lw", "tsurfobs")}
        nat["tdew"] = pad_t(forcing["tdew"], wdt) if need_full else None
        nat["depth"] = pad_t(forcing["depth"], wdt) if need_full and bool((forcing["depth"] >= 0).any()) else None
        nat["precphase"] = pad_t(forcing["precphase"], torch.int32)
        self.nat = nat
        self.hour = torch.from_numpy(np.ascontiguousarray(hour, np.int32)).to(dev)

        def pp_vec(vals, dtype):
            t = torch.zeros((npad,), dtype=dtype, device=dev)
            t[:n] = torch.tensor(vals, dtype=dtype)
            return t

        relax_on = settings.use_relaxation == 1
        coupled = settings.use_coupling == 1
        # (one tensor for every RsPointParams of the leg: Plan.point_params keeps only its latest arguments alive)
        self.tb = torch.full((npad,), float(plan.uniform_tbottom(*tbottom_date)), dtype=torch.float64, device=dev)
        self.pvec = None
        if need_full:
            self.pvec = [pp_vec([l.InitLenI for l in local], torch.int32)]
            self.pvec += [pp_vec([getattr(l, k) for l in local], torch.float64) if relax_on else None
                          for k in RELAX_FIELDS]
            self.pvec += [pp_vec([l.couplingIndexI for l in local], torch.int32) if coupled else None,
                          pp_vec([l.couplingTsurf for l in local], torch.float64) if coupled else None]
        # sky view (sky: the leg's six time axes and the points' local horizons [n][360] or None): the two radiation
        # streams in the plan's precision, the sun rows of the leg's indices, the points' geometry in fp64
        self.sun = self.sky = None
        if sky is not None:
            Lh = lib.load()
            nat["sw_dir"] = pad_t(forcing["sw_dir"], wdt)
            nat["lw_net"] = pad_t(forcing["lw_net"], wdt)
            sun = np.zeros((nrows, 6))  # RS_SUN_COLS
            ax = [np.ascontiguousarray(sky["axes"][k], np.int32) for k in ("year", "month", "day", "hour", "minute", "second")]
            assert all(a.shape == (nrows,) for a in ax)
            Lh.rs_sun_table(nrows, *[C.c_void_p(a.ctypes.data) for a in ax], C.c_void_p(sun.ctypes.data))
            self.sun = torch.from_numpy(sun).to(dev)
            larr = (abi.LocalParameters * n)(*local)
            geo = [np.zeros(n) for _ in range(3)]
            Lh.rs_point_geometry(n, larr, *[C.c_void_p(g.ctypes.data) for g in geo])
            self.sky = {"sky_view": pp_vec([l.sky_view for l in local], torch.float64)}
            for k, g in zip(("sin_lat", "cos_lat", "lon_rad"), geo):
                self.sky[k] = pp_vec(g.tolist(), torch.float64)
            if sky.get("horizons") is not None:
                h = torch.zeros((360, npad), dtype=torch.float64, device=dev)
                h[:, :n] = torch.from_numpy(np.ascontiguousarray(sky["horizons"], np.float64)).to(dev).T
                self.sky["horizons"] = h
        self.out = dv.OutputWindow.empty(nrows, npad, dev, dtype=wdt)
        if not recluster:
            self.win = self._window(nat, self.hour, self.sun, nrows)
            self.pp = self._pp(None)
        self.gspec = self.gid = self.gacc = None
        if groups is not None:
            self.gspec = groups[0]
            self.gid = torch.from_numpy(np.ascontiguousarray(groups[1], dtype=np.int32)).to(dev)
            assert self.gid.shape == (n,)
            self.gacc = plan.groups_reset(nrows, self.gspec)
        self.espec = self.etab = self.eacc = None
        if stats is not None:  # (stats: the spec and the station of every point; a cell is written, so no reset)
            self.espec = stats[0]
            self.etab = plan.ens_table(np.ascontiguousarray(stats[1], dtype=np.int32), self.espec)
            self.eacc = torch.empty((nrows, int(self.espec.ngroups), lib.ens_cols(self.espec)), dtype=torch.float64,
                                    device=dev)

    def _window(self, tens, hour, sun, nrows):
        tens = dict(tens, hour=hour)
        if sun is not None:
            tens["sun"] = sun
        return self.dv.ForcingWindow(nrows, self.npad, tens)

    def _pp(self, order):
        if self.pvec is None:
            return self.plan.point_params(self.tb)
        vecs = self.pvec if order is None else [None if v is None else v.index_select(0, order) for v in self.pvec]
        sky = self.sky
        if sky is not None and order is not None:  # the vectors by slot; the horizons stay, slot s reads column order[s]
            sky = {k: (v if k == "horizons" else v.index_select(0, order)) for k, v in self.sky.items()}
            if "horizons" in sky:
                sky["horizon_index"] = order.to(self.torch.int32)
        return self.plan.point_params(self.tb, *vecs, sky)

    def init(self):
        # (before any re-sort: slot order is point order)
        self.plan.init_state(self._window(self.nat, self.hour, self.sun, self.nrows), self._pp(None))

    def launch(self, t0, ns, call="step"):
        """Time indices [t0, t0 + ns) through Plan.step / step_cpl / cpl_replay; with ``recluster`` the window and the
        per-point parameters go in the plan's current slot order, the rows come back through the kept order row, and
        the plan is re-sorted behind the launch."""
        dv, plan, r0 = self.dv, self.plan, t0 - self.first
        assert 0 <= r0 and r0 + ns <= self.nrows
        if self.recluster:
            order = plan.order().clone().long()
            tens = {k: (None if v is None else v[r0:r0 + ns].index_select(1, order)) for k, v in self.nat.items()}
            win = self._window(tens, self.hour[r0:r0 + ns].contiguous(),
                               None if self.sun is None else self.sun[r0:r0 + ns].contiguous(), ns)
            wrow = 0
            out, orow0, srow = dv.OutputWindow.empty(ns, self.npad, self.dev, dtype=self.wdt), t0 - 1, 0
            pp = self._pp(order)
        else:
            win, wrow, out, orow0, srow, pp = self.win, r0, self.out, self.first - 1, r0, self.pp
        getattr(plan, call)(win, out, pp, t0, ns, window_row=wrow, out_row0=orow0)
        if self.gacc is not None and call != "cpl_replay":
            plan.outputs_groups(out, ns, self.gid, self.gspec, self.gacc, r0, row=srow)
        if self.eacc is not None and call != "cpl_replay":
            plan.outputs_ens(out, ns, self.etab, self.espec, self.eacc, r0, row=srow)
        if self.recluster:
            for k in dv.OUT_FIELDS:
                self.out.tensors[k][r0:r0 + ns].index_copy_(1, order, out.tensors[k])
            plan.recluster()

    def chunks(self, lo, hi, chunk, call="step"):
        t0 = lo
        while t0 <= hi:
            ns = min(chunk or hi - lo + 1, hi - t0 + 1)
            self.launch(t0, ns, call)
            t0 += ns

    def results(self):
        self.plan.sync()
        return {k: self.out.tensors[k][:, :self.n].T.contiguous().double().cpu().numpy() for k in self.dv.OUT_FIELDS}


def run_ensemble(station_forcing: dict, member_tail: dict, B: int, settings: abi.InputSettings,
                 params: abi.InputParameters, station_local, member_local=None, parent=None, chunk: int = 0,
                 variant: int = 0, precision: int = 64, recluster: bool = False, groups=None, device: int = 0,
                 timing: dict | None = None, stats=None):
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
    device (group = parent), behind every launch: mean, spread and quantiles of Tsurf, mean storages.

    Returns a dict: ``stations[name][S][B]``, ``members[name][len(parent)][L - B]`` (row r is time index
    ``B + 1 + r``), ``failed`` = (stations, members) counts, with ``groups`` the series ``[L - B, ngroups, cols]`` and
    with ``stats`` the cells ``stats[L - B, S, cols]`` of ``ensstats.reduce_members`` (row r is time index ``B + 1 + r``).
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
    check(S, L, B, settings, sl, member_local, parent, precision, recluster, stats)
    if station_forcing["tair"].shape[1] < B:
        raise ValueError(f"run_ensemble: the stations' forcing is shorter than B = {B}")
    ml = member_locals(sl, member_local, parent)
    head = {k: np.asarray(v)[:, :B] for k, v in station_forcing.items()
            if np.asarray(v).ndim == 2 and k != "local_horizons"}
    coupled = settings.use_coupling == 1
    # one feature set for both legs, chosen as device.run_points chooses it for the replicated input
    initlen = np.array([l.InitLenI for l in sl])
    skyv = np.array([l.sky_view for l in sl])
    sky_on = bool(((skyv < 1.0) & (skyv > -0.01)).any())
    need_full = bool(initlen.max() > 1 or settings.force_tsurf == 1 or settings.use_relaxation == 1 or coupled
                     or sky_on or settings.tsurfOutputDepth >= 0
                     or any((f["depth"] >= 0).any() or ((f["tdew"] < -90.0) | (f["tdew"] > 100.0)).any()
                            for f in (head, member_tail)))
    date = tuple(int(station_forcing[k][0]) for k in ("year", "month", "day"))
    from . import device as dv
    dv.require_gpu()
    sky_st = sky_mem = None
    if sky_on:  # a member has its station's geometry and horizons
        hz = station_forcing.get("local_horizons")
        axes = ("year", "month", "day", "hour", "minute", "second")
        sky_st = {"axes": {k: np.asarray(station_forcing[k])[:B] for k in axes}, "horizons": hz}
        sky_mem = {"axes": {k: member_tail[k] for k in axes}, "horizons": None if hz is None else np.asarray(hz)[parent]}
    st = _Leg(S, 1, head, np.asarray(station_forcing["hour"])[:B], settings, params, sl, need_full, precision, variant,
              recluster, device, date, sky=sky_st)
    mem = _Leg(nmem, B + 1, member_tail, member_tail["hour"], settings, params, ml, need_full, precision, variant,
               recluster, device, date, groups, sky=sky_mem, stats=None if stats is None else (stats, parent))
    st.init()
    if coupled:
        # as device.run_points: lock-step chunks up to the last coupling-window end, the replay rounds over the block
        # of windows (to the index behind the last one, <= B), the chunks from the first window end on - then every
        # window is closed, and the members go on in lock step from where every point resumes, B + 1
        ci = np.array([l.couplingIndexI for l in sl])
        ct = np.array([l.couplingTsurf for l in sl])
        on = ~((ct < -100) | (ci < 1))
        cpl_len = int(settings.coupling_minutes * 60 / settings.DTSecs)
        cs = np.where(ci <= settings.coupling_minutes * 60 / settings.DTSecs, 1, ci - cpl_len)
        if on.any():
            ce_max, ce_min, cs_min = int(ci[on].max()), int(ci[on].min()), int(cs[on].min())
            st.chunks(1, ce_max, chunk, "step_cpl")
            st.launch(cs_min, ce_max + 1 - cs_min + 1, "cpl_replay")
            st.chunks(ce_min + 1, B, chunk, "step_cpl")
        else:
            st.chunks(1, B, chunk, "step_cpl")
        st.plan.coupling_windows_closed(True)
    else:
        st.chunks(1, B, chunk)
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
    if mem.gacc is not None:
        res["groups"] = mem.plan.groups(mem.gacc, mem.gspec)
    if mem.eacc is not None:
        res["stats"] = mem.plan.ens(mem.eacc, mem.espec)
    if ev:
        timing["fanout_ms"] = float(ev[0].elapsed_time(ev[1]))
    st.plan.close()
    mem.plan.close()
    return res
