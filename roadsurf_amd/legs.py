"""The bridge from host arrays ``[n][rows]`` (numpy, reference layout) to the device-resident API, said once.

``device.run_points`` and ``ensemble.run_ensemble`` both go through it: which feature set a run needs
(``feature_set``), how a coupled run is staged (``coupling_stages``), the host tables of sky view (``sky_tables``),
and ``Leg`` - one plan, its padded windows and per-point vectors, its launches and the reducers behind them.
The rules are numpy and import without torch or a GPU; ``Leg`` imports torch and ``device`` when it is made.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, lib

AXES = ("year", "month", "day", "hour", "minute", "second")
RELAX_FIELDS = ("tair_relax", "VZ_relax", "RH_relax")


def feature_set(settings, locals_, forcings, lean_if_possible=True):
    """(need_full, sky_on) of a run: the LEAN kernels serve it unless anything below is on.  ``forcings``: the dicts
    whose ``depth`` and ``tdew`` the run reads (the LEAN kernels skip the Tdew check and have no depth stream)."""
    skyv = np.array([l.sky_view for l in locals_])
    sky_on = bool(((skyv < 1.0) & (skyv > -0.01)).any())
    need_full = bool((not lean_if_possible) or max(l.InitLenI for l in locals_) > 1 or settings.force_tsurf == 1
                     or settings.use_relaxation == 1 or settings.use_coupling == 1 or sky_on
                     or settings.tsurfOutputDepth >= 0
                     or any((f["depth"] >= 0).any() or ((f["tdew"] < -90.0) | (f["tdew"] > 100.0)).any()
                            for f in forcings))
    return need_full, sky_on


def coupling_stages(settings, locals_, last, chunked):
    """The launches of the time indices ``1 .. last`` as (call, lo, hi), call a method of ``Plan``.  Time-chunked
    coupling: lock-step chunks up to the last coupling-window end, the replay rounds over the window block, then the
    chunks from the first window end on (points whose window ends later wait there; include/roadsurf.h,
    rs_hip_step_cpl).  Coupled and not ``chunked`` is ONE ``step`` over the series, the general coupled kernel."""
    if settings.use_coupling != 1 or not chunked:
        return [("step", 1, last)]
    ci = np.array([l.couplingIndexI for l in locals_])
    ct = np.array([l.couplingTsurf for l in locals_])
    on = ~((ct < -100) | (ci < 1))
    if not on.any():
        return [("step_cpl", 1, last)]
    cpl_len = int(settings.coupling_minutes * 60 / settings.DTSecs)
    cs = np.where(ci <= settings.coupling_minutes * 60 / settings.DTSecs, 1, ci - cpl_len)
    ce_max, ce_min, cs_min = int(ci[on].max()), int(ci[on].min()), int(cs[on].min())
    # the replay window reaches one index beyond the last window end: a point that replays has CheckValues run on
    # index couplingEndI+1 before it rewinds (Simulation.f90:59-66)
    return [("step_cpl", 1, min(ce_max, last)), ("cpl_replay", cs_min, min(ce_max + 1, last)),
            ("step_cpl", ce_min + 1, last)]


def sky_tables(axes, locals_):
    """The host tables of sky view: the sun rows [nrows, RS_SUN_COLS = 6] of the six time axes ``axes[name][nrows]``,
    and per point sky_view, sin_lat, cos_lat, lon_rad - all float64."""
    Lh = lib.load()
    ax = [np.ascontiguousarray(axes[k], np.int32) for k in AXES]
    nrows = len(ax[0])
    assert all(a.shape == (nrows,) for a in ax)
    sun = np.zeros((nrows, 6))
    Lh.rs_sun_table(nrows, *[C.c_void_p(a.ctypes.data) for a in ax], C.c_void_p(sun.ctypes.data))
    n = len(locals_)
    larr = (abi.LocalParameters * n)(*locals_)
    geo = [np.zeros(n) for _ in range(3)]
    Lh.rs_point_geometry(n, larr, *[C.c_void_p(g.ctypes.data) for g in geo])
    return (sun, np.array([l.sky_view for l in locals_]), *geo)


def pad_rows(a, stride, dtype, dev):
    """Host ``a[n][rows]`` as the device tensor ``[rows][stride]``, zeros behind column n."""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.zeros((a.shape[1], stride), dtype=dtype, device=dev)
    t[:, :a.shape[0]] = torch.from_numpy(a).to(dev).T
    return t


class Leg:
    """One plan and the rows of forcing it steps: row r of its windows is time index ``first + r``.

    ``forcing`` as ``device.run_points`` takes it: series ``[n][nrows]``, the one-dimensional ``hour``, with sky view
    the six time axes and optionally ``local_horizons`` [n][360].  ``need_full``, ``sky_on``: ``feature_set``.
    ``recluster``: ``Plan.recluster()`` behind every launch.  ``horizon_index``: point i reads column
    ``horizon_index[i]`` of ``local_horizons`` (not with ``recluster``, which derives its own from the plan order).
    The reducers run behind every launch but a replay: ``summary`` (a SummarySpec) and ``episodes`` (an EpisodeSpec)
    by absolute time index, ``groups`` (GroupSpec, ids [n]) and ``stats`` (EnsSpec, stations [n]) by row, and
    ``probs`` (ProbSpec without the deficit, stations [n]) by row and in row order, its carry reset once, and
    ``periods`` (a PeriodSpec) by absolute time index and in time order, its cells reset once."""

    def __init__(self, forcing, settings, params, local, *, need_full, tbottom_date, sky_on=False, first=1,
                 precision=64, variant=0, history_score=None, recluster=False, horizon_index=None, device=0,
                 summary=None, groups=None, episodes=None, stats=None, probs=None, periods=None):
        import torch
        from . import device as dv
        assert not (recluster and horizon_index is not None)
        self.dv, self.torch = dv, torch
        self.n, self.nrows = n, nrows = forcing["tair"].shape
        self.first, self.recluster = first, recluster
        if isinstance(local, abi.LocalParameters):
            local = [local] * n
        self.plan = plan = dv.Plan(n, settings, params, device)
        if variant:
            plan.set_variant(variant)
        if history_score is not None:
            plan.set_history_score(history_score)
        if precision == 32:  # the fp32 flavour: windows and outputs hold floats (rs_hip_set_precision)
            plan.set_precision(32)
        self.wdt = wdt = torch.float32 if precision == 32 else torch.float64
        self.dev = dev = plan.device
        self.npad = npad = plan.np_pad

        nat = {k: pad_rows(forcing[k], npad, wdt, dev) for k in ("tair", "vz", "rhz", "prec", "sw", "lw", "tsurfobs")}
        nat["tdew"] = pad_rows(forcing["tdew"], npad, wdt, dev) if need_full else None
        # no depth stream where no value of it can act (depth(i) >= 0 takes the surface temperature from the profile
        # at that depth): the kernels read a missing stream as -9999.9, and the two-wavefront flavour has the FULL
        # feature set only without one
        depth_on = need_full and bool((forcing["depth"] >= 0).any())
        nat["depth"] = pad_rows(forcing["depth"], npad, wdt, dev) if depth_on else None
        nat["precphase"] = pad_rows(forcing["precphase"], npad, torch.int32, dev)
        self.nat = nat
        self.hour = torch.from_numpy(np.ascontiguousarray(forcing["hour"], np.int32)).to(dev)

        def vec(vals, dtype):
            t = torch.zeros((npad,), dtype=dtype, device=dev)
            t[:n] = torch.from_numpy(np.ascontiguousarray(vals)).to(dtype)
            return t

        relax_on = settings.use_relaxation == 1
        coupled = settings.use_coupling == 1
        # (one tensor for every RsPointParams of the leg: Plan.point_params keeps only its latest arguments alive)
        self.tb = torch.full((npad,), float(plan.uniform_tbottom(*tbottom_date)), dtype=torch.float64, device=dev)
        self.pvec = None
        if need_full:
            self.pvec = [vec([l.InitLenI for l in local], torch.int32)]
            self.pvec += [vec([getattr(l, k) for l in local], torch.float64) if relax_on else None
                          for k in RELAX_FIELDS]
            self.pvec += [vec([l.couplingIndexI for l in local], torch.int32) if coupled else None,
                          vec([l.couplingTsurf for l in local], torch.float64) if coupled else None]
        # sky view: the two radiation streams in the plan's precision; the sun rows of the leg's indices, the points'
        # geometry and their horizons in fp64
        self.sun = self.sky = None
        if sky_on:
            nat["sw_dir"] = pad_rows(forcing["sw_dir"], npad, wdt, dev)
            nat["lw_net"] = pad_rows(forcing["lw_net"], npad, wdt, dev)
            sun, *geo = sky_tables(forcing, local)
            assert sun.shape[0] == nrows
            self.sun = torch.from_numpy(sun).to(dev)
            self.sky = {k: vec(g, torch.float64) for k, g in zip(("sky_view", "sin_lat", "cos_lat", "lon_rad"), geo)}
            if forcing.get("local_horizons") is not None:
                self.sky["horizons"] = pad_rows(forcing["local_horizons"], npad, torch.float64, dev)
                if horizon_index is not None:
                    self.sky["horizon_index"] = vec(np.asarray(horizon_index, np.int32), torch.int32)
        self.out = dv.OutputWindow.empty(nrows, npad, dev, dtype=wdt)
        if not recluster:
            self.win = self._window(nat, self.hour, self.sun, nrows)
            self.pp = self._pp(None)
        # the reducers: (name, what runs behind a launch of ns indices from t0 whose rows start at `row` of `out`,
        # what collects the result)
        self.reducers = []
        if summary is not None:
            sacc = plan.summary_reset()
            self.reducers.append(("summary", lambda out, ns, t0, row: plan.outputs_summary(
                out, ns, t0, 1, summary, sacc, row=row), lambda: plan.summary(sacc)))
        if groups is not None:
            gspec, gid = groups[0], torch.from_numpy(np.ascontiguousarray(groups[1], dtype=np.int32)).to(dev)
            assert gid.shape == (n,)
            gacc = plan.groups_reset(nrows, gspec)
            self.reducers.append(("groups", lambda out, ns, t0, row: plan.outputs_groups(
                out, ns, gid, gspec, gacc, t0 - first, row=row), lambda: plan.groups(gacc, gspec)))
        if episodes is not None:
            eacc = plan.episodes_reset(episodes)

            def finished():
                plan.episodes_finish(episodes, eacc)
                return plan.episodes(eacc)
            self.reducers.append(("episodes", lambda out, ns, t0, row: plan.outputs_episodes(
                out, ns, t0, 1, episodes, eacc, row=row), finished))
        if stats is not None:  # (a cell is written, so no reset)
            tspec = stats[0]
            table = plan.ens_table(np.ascontiguousarray(stats[1], dtype=np.int32), tspec)
            tacc = torch.empty((nrows, int(tspec.ngroups), lib.ens_cols(tspec)), dtype=torch.float64, device=dev)
            self.reducers.append(("stats", lambda out, ns, t0, row: plan.outputs_ens(
                out, ns, table, tspec, tacc, t0 - first, row=row), lambda: plan.ens(tacc, tspec)))
        if probs is not None:  # (cells are written, so no reset of them; the carry is reset once, here)
            pspec = probs[0]
            ptable = plan.ens_table(np.ascontiguousarray(probs[1], dtype=np.int32), pspec)
            pever = plan.prob_reset()
            pacc = torch.empty((nrows, int(pspec.ngroups), lib.prob_cols(pspec)), dtype=torch.float64, device=dev)
            self.reducers.append(("probs", lambda out, ns, t0, row: plan.outputs_prob(
                out, ns, ptable, pspec, pever, pacc, t0 - first, row=row), lambda: plan.prob(pacc, pspec)))
        if periods is not None:  # (the launches of a leg come in time order: what the sum of a period needs)
            wacc = plan.periods_reset(periods)
            self.reducers.append(("periods", lambda out, ns, t0, row: plan.outputs_periods(
                out, ns, t0, 1, periods, wacc, row=row), lambda: plan.periods(wacc, periods)))

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
        if call != "cpl_replay":  # (a replay rewrites rows that earlier launches wrote)
            for _, behind, _ in self.reducers:
                behind(out, ns, t0, srow)
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

    def run(self, stages, chunk=0):
        """The stages of ``coupling_stages`` in launches of ``chunk`` indices (0: a stage in one launch); a replay is
        one launch, an empty stage none."""
        for call, lo, hi in stages:
            self.chunks(lo, hi, 0 if call == "cpl_replay" else chunk, call)

    def results(self):
        self.plan.sync()
        return {k: self.out.tensors[k][:, :self.n].T.contiguous().double().cpu().numpy() for k in self.dv.OUT_FIELDS}

    def reduced(self):
        """What the reducers hold, by name (synchronises)."""
        return {name: collect() for name, _, collect in self.reducers}
