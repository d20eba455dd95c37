"""Builds one case twice through ``roadsurf_amd.device.Plan`` for tests/test_hip_padding.py (a plain module: no
fixture, no pytest setting).

The CLEAN build is what the GPU suite uses everywhere else: windows of ``np_pad`` columns, zeros behind ``n``,
``RsPointParams`` arrays of ``np_pad`` elements.  The HOSTILE build is the same case with every caller-owned array
carved out of a larger buffer: a guard band of 64 elements before and after it, windows of ``np_pad + 64`` columns,
``RsPointParams`` arrays of exactly ``n`` elements (include/roadsurf.h: ``[npoints]``) - and every element that is
not a live column ``[0, n)`` holds poison.  Behind an exact-length array the band is long enough (``np_pad - n + 64``)
that a read up to column ``np_pad - 1`` meets poison, never memory that is not the test's.  The state block is the
plan's own: it is downloaded after ``init_state``, poisoned in the columns ``>= n`` in the precision's element type
and uploaded again.  No poison is an index outside its array: a leak shows as changed bits, not as a wild address.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

import golden_helpers as gh
import oracle_helpers as oh
from roadsurf_amd import abi, device, legs, lib

GUARD = 64
SIMLEN = 241
SPK = 120
NKNOTS = (SIMLEN - 1) // SPK + 2
SIZES = (1, 63, 65, 129, 203, 257)
POISONS = ("nan", "huge", "opposite", "failing")
SEEDS = tuple(range(1, 201))  # the fixed candidate list of prepare
NL = 15
# rows of the state block (roadsurf_amd/csrc/rs_state.h)
ST_TNW1 = abi.RS_MAX_LAYERS
(ST_TNW2, ST_TSURF, ST_WAT, ST_SNOW, ST_ICE, ST_ICE2, ST_DEP) = range(ST_TNW1 + 1, ST_TNW1 + 8)
ST_FAILED = ST_TNW1 + 12
ST_BLSCORE = ST_TNW1 + 16
KNOT_FIELDS = ("tair", "tdew", "vz", "rhz", "prec", "sw", "lw", "tsurfobs", "precphase")  # rs_synth.h

# `opposite`: valid values that vote "no" in every wave-wide shortcut (snow on the road, water, ice, a frozen
# profile, precipitation with the snow phase at every index, no sun); the other members are merely valid and unlike
# the live ones
OPPOSITE = dict(tair=-5.0, tdew=-6.0, vz=8.0, rhz=95.0, prec=2.0, sw=0.0, lw=250.0, tsurfobs=-5.0, sw_dir=0.0,
                lw_net=-40.0, sun=1.0, tbottom=2.5, tair_relax=5.0, vz_relax=1.0, rh_relax=50.0, coupling_tsurf=-3.0,
                sky_view=0.5, sin_lat=math.sin(math.radians(60.0)), cos_lat=math.cos(math.radians(60.0)), lon_rad=0.4,
                horizons=20.0, out=4321.0, dst=4321.0)
SNOW_PHASE = 3  # src/Cond.f90:143-249: phase codes 3 and 6 are snow


def float_poison(cls: str, name: str) -> float:
    if cls == "nan":
        return float("nan")
    if cls == "huge":
        return float("inf")
    if cls == "failing" and name == "tair":
        return 250.0  # CheckValues would fail the lane (src/InputOutput.f90:55-66)
    return OPPOSITE[name]


def int_poison(name: str, n: int) -> int:
    """Valid in every class, and not what the live points have."""
    return {"precphase": SNOW_PHASE, "initlen": SIMLEN + 1000, "coupling_index": 100, "horizon_index": n - 1,
            "hour": 12}[name]


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def np_bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.int64 if a.itemsize == 8 else np.int32)


class Arena:
    """Every caller-owned device array of one build, each inside a buffer with guard bands."""

    def __init__(self, dev, n: int, np_pad: int, cls: str | None):
        self.dev, self.n, self.np_pad, self.cls = dev, n, np_pad, cls
        self.hostile = cls is not None
        self.items = {}  # name -> (buffer, view, role)

    def carve(self, name, shape, dtype, fill, role="in", tail=GUARD):
        numel = int(np.prod(shape))
        buf = torch.full((GUARD + numel + tail,), fill, dtype=dtype, device=self.dev)
        view = buf[GUARD:GUARD + numel].view(*shape)
        assert name not in self.items
        self.items[name] = (buf, view, role)
        return view

    def fill(self, name, dtype):
        if not self.hostile:
            return 0
        return int_poison(name, self.n) if dtype == torch.int32 else float_poison(self.cls, name)

    @property
    def stride(self):
        return self.np_pad + (GUARD if self.hostile else 0)

    def rows(self, name, a, dtype, nrows=None, key=None):
        """A window stream [rows][stride] from the host array a[n][rows] (None: nothing live yet)."""
        nrows = a.shape[1] if a is not None else nrows
        v = self.carve(key or name, (nrows, self.stride), dtype, self.fill(name, dtype))
        if a is not None:
            v[:, :self.n] = torch.from_numpy(np.ascontiguousarray(a)).to(self.dev).T.to(dtype)
        return v

    def axis(self, name, a, dtype):
        """An array shared by all points (the hour axis, the sun table): only its guard bands hold poison."""
        v = self.carve(name, a.shape, dtype, self.fill(name, dtype))
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(self.dev).to(dtype))
        return v

    def vec(self, name, live, dtype):
        """A per-point array: np_pad elements with zeros behind n, or exactly n with poison directly behind it."""
        n, npd = self.n, self.np_pad
        v = self.carve(name, (n if self.hostile else npd,), dtype, self.fill(name, dtype),
                       tail=(npd - n + GUARD) if self.hostile else GUARD)
        v[:n] = torch.from_numpy(np.ascontiguousarray(live)).to(self.dev).to(dtype)
        return v

    def table(self, name, a, dtype):
        """[k][np_pad] from a[n][k] (the horizon table)."""
        v = self.carve(name, (a.shape[1], self.np_pad), dtype, self.fill(name, dtype))
        v[:, :self.n] = torch.from_numpy(np.ascontiguousarray(a)).to(self.dev).T.to(dtype)
        return v

    def output(self, nrows, dtype, tag=""):
        # rows the simulation never saves read -9999.0 (device.OutputWindow.empty): the live columns start that way
        t = {}
        for k in device.OUT_FIELDS:
            v = self.carve("out_" + k + tag, (nrows, self.stride), dtype, self.fill("out", dtype) if self.hostile else -9999.0,
                           role="out")
            v[:, :self.n] = -9999.0
            t[k] = v
        return device.OutputWindow(nrows, self.stride, t)

    def snapshot(self):
        torch.cuda.synchronize(self.dev)
        return {k: b.clone() for k, (b, _, _) in self.items.items()}

    def touched(self, snap, exempt=()):
        """Names of the buffers in which anything but the live columns of an output changed since `snap`."""
        torch.cuda.synchronize(self.dev)
        bad = []
        for k, (b, v, role) in self.items.items():
            if k in exempt:
                continue
            cur = b.clone()
            if role in ("out", "written"):  # the live columns [0, n) of every row are the kernel's to write
                numel = v.numel()
                cur[GUARD:GUARD + numel].view(*v.shape)[..., :self.n] = snap[k][GUARD:GUARD + numel].view(*v.shape)[..., :self.n]
            elif role == "dst":  # point-major [n][7 + rows]: every row from its column 7 on
                numel = v.numel()
                cur[GUARD:GUARD + numel].view(*v.shape)[:, 7:] = snap[k][GUARD:GUARD + numel].view(*v.shape)[:, 7:]
            if not torch.equal(bits(cur), bits(snap[k])):
                where = torch.nonzero(bits(cur) != bits(snap[k])).flatten()[:4].tolist()
                bad.append((k, where))
        return bad


@dataclass(frozen=True)
class Case:
    name: str
    precision: int = 64
    variant: int = 0
    src: str = "window"      # or "knots" (rs_hip_step_knots)
    full: bool = False       # use_relaxation, an initialization phase of 60 indices with observations, a dew point
    sky: bool = False
    cpl: str | None = None   # "general" (rs_hip_step, whole series) or "chunk" (rs_hip_step_cpl + rs_hip_cpl_replay)
    depth: bool = False      # tsurfOutputDepth: the fp32 general kernel
    a32_limit: str | None = None  # ROADSURF_HIP_A32_LIMIT: 64-bit window offsets, which the two-wavefront kernels lack


def wave_points(case: Case) -> int:
    """Points that vote together: a wavefront's 64, or the 128 of the fp32 two-points-per-lane kernels."""
    one_per_lane = case.variant in (1, 2) or case.depth
    return 128 if case.precision == 32 and not one_per_lane else 64


def last_wave(n: int, wave: int):
    return ((n - 1) // wave) * wave, n


def bare_and_dry_fraction(ora, f, n, wave):
    """Share of the indices at which EVERY live point of the ragged last wave is bare and dry: all five storages
    exactly 0 and no precipitation - what a wave-wide shortcut asks."""
    a, b = last_wave(n, wave)
    bd = np.ones(SIMLEN, bool)
    for k in ("snow", "water", "ice", "deposit", "ice2"):
        bd &= (ora[k][a:b] == 0.0).all(axis=0)
    bd &= (f["prec"][a:b] == 0.0).all(axis=0)
    return float(bd.mean())


# Dozens of points of this weather are never all bare and dry at once (about a third carry something at any time).
# So the live points of the last wave get a dry first hour - no precipitation, at most 60 % humidity - and the first of
# them rain from the second hour on: the same edit of the hourly knots and of the host series.  Whether the wave then
# IS bare and dry for a quarter of the series and is not for another quarter is still the oracle's to say (prepare).
def dry_spell_host(f, n, wave):
    a, b = last_wave(n, wave)
    f["prec"][a:b, :SPK + 1] = 0.0
    f["rhz"][a:b, :SPK + 1] = np.minimum(f["rhz"][a:b, :SPK + 1], 60.0)
    f["prec"][a, SPK + 1:] = 1.0
    f["precphase"][a, SPK + 1:] = 1


def dry_spell_knots(knots, n, wave):
    a, b = last_wave(n, wave)
    knots[:2, 4, a:b] = 0.0
    knots[:2, 3, a:b] = torch.clamp(knots[:2, 3, a:b], max=60.0)
    knots[2:, 4, a] = 1.0
    knots[2:, 8, a] = 1.0


def oracle_kind(case: Case) -> str:
    """test_hip_parity's kind; with coupling the reference build in which coupling acts (tests/test_hip_coupling.py)."""
    if case.cpl:
        return "ref_cpl" if os.path.exists(oh.REF_CPL_SO) else "port"
    return "ref" if oh.have_ref() else "port"


_prepared = {}


def prepare(case: Case, n: int):
    """(seed, share, oracle outputs): the first candidate seed whose reference run OF THIS CASE'S OWN DATA leaves the
    ragged last wave bare and dry at no less than a quarter of the indices and not bare and dry at no less than a
    quarter: zero padding then lets that wave take the shortcuts and `opposite` padding forbids them.  From the
    oracle's series alone; no seed: the test fails."""
    key = _data_key(case, n)
    if key in _prepared:
        return _prepared[key]
    for seed in SEEDS:
        f, s, p, ls, _ = case_data(case, n, seed, False)
        ora, _, _ = oh.run_oracle(oracle_kind(case), f, s, p, ls)
        frac = bare_and_dry_fraction(ora, f, n, wave_points(case))
        if 0.25 <= frac <= 0.75:
            _prepared[key] = (seed, frac, ora)
            return _prepared[key]
    raise AssertionError(f"{case.name}, {n} points: no candidate seed leaves the last wave bare and dry for a quarter "
                         f"of the indices and covered or wet for another quarter")


def knot_series(n: int, seed: int, wave: int):
    """The host series of a knot-reading case: the hourly knots of the generator's host twin with the dry spell of
    dry_spell_knots, expanded by the plain numpy rule (golden_helpers.expand_knots: IEEE float64) - nothing of it
    comes from a kernel, so the oracle's input is independent of the expansion rs_hip_step_knots does itself."""
    g = oh.synth_forcing(n, (NKNOTS - 1) * SPK + 1, seed=seed)
    K = {k: np.ascontiguousarray(g[k][:, ::SPK]) for k in gh.KNOT_FIELDS}
    K["phase"] = np.ascontiguousarray(g["precphase"][:, ::SPK])
    K["tsurf0"] = g["tsurfobs"][:, 0].copy()
    a, b = last_wave(n, wave)
    K["prec"][a:b, :2] = 0.0
    K["rhz"][a:b, :2] = np.minimum(K["rhz"][a:b, :2], 60.0)
    K["prec"][a, 2:] = 1.0
    K["phase"][a, 2:] = 1
    e = gh.expand_knots(K, SIMLEN, SPK)
    f = oh.synth_forcing(n, SIMLEN, seed=seed)
    for k in ("tair", "tdew", "vz", "rhz", "prec", "sw", "lw", "tsurfobs", "precphase"):
        assert e[k].dtype == f[k].dtype and e[k].shape == f[k].shape
        f[k] = e[k]
    return f


_data = {}


def _data_key(case, n):
    return (case.src, case.full, case.sky, case.cpl is not None, case.depth, wave_points(case), n)


def case_data(case: Case, n: int, seed: int, failing: bool):
    """Host arrays, settings, parameters and per-point locals of a case - the same for both builds and the oracle."""
    key = _data_key(case, n) + (seed, failing)
    if key in _data:
        return _data[key]
    L = SIMLEN
    wave = wave_points(case)
    if case.src == "knots":
        f = knot_series(n, seed, wave)
    else:
        f = oh.synth_forcing(n, L, seed=seed)
        dry_spell_host(f, n, wave)
    rs = np.random.RandomState(seed + n)
    s = abi.default_settings(L); p = abi.default_parameters()
    bad = {}
    if failing:  # two live points fail on purpose (one where there is only one)
        bad = {0: 30} if n == 1 else {0: 30, n - 1: 130}
        for pt, idx in bad.items():
            f["tair"][pt, idx] = 250.0
    if case.sky:  # as tests/test_hip_skyview.py makes them
        f["sw"] *= 2.0
        f["sw_dir"] = np.ascontiguousarray(f["sw"] * rs.uniform(0.2, 1.2, (n, 1)))
        f["lw_net"] = np.ascontiguousarray(-40.0 - 30 * rs.rand(n, L))
        hz = np.ascontiguousarray(np.round(rs.uniform(0, 25, (n, 360)), 1)); hz[::7] = 0.0
        f["local_horizons"] = hz
        f.update(oh.time_axis(L, 30.0, (2024, 6, 20, 9, 0, 0)))  # the sun is up
    if case.full and case.src == "window":  # (the knots carry the observation of index 1 only)
        f["tsurfobs"][:, :60] = f["tair"][:, :60] - 0.5
    if case.full:
        s.use_relaxation = 1
    if case.depth:
        s.tsurfOutputDepth = 0.05
    base = None
    if case.cpl:
        s.use_coupling = 1; s.coupling_minutes = 30
        l0 = abi.default_local(); l0.InitLenI = 1
        base, _, _ = oh.run_oracle("port", f, abi.default_settings(L), p, l0)
        f["tsurfobs"][:, :] = base["tsurf"] + 0.3  # as tests/test_hip_coupling.py: observations up to the coupling index
    ls = []
    for i in range(n):
        li = abi.default_local()
        li.InitLenI = 150 if case.cpl else 60 if case.full else 1
        if case.full:
            li.tair_relax = float(f["tair"][i, 60]) + 1.5; li.VZ_relax = 3.0; li.RH_relax = 85.0
            if i % 5 == 4:
                li.tair_relax = -9999.0  # an invalid target: no relaxation for the point
        if case.cpl:
            li.couplingIndexI = 150
            li.couplingTsurf = float(base["tsurf"][i, 149] + rs.choice([0.05, 0.5, -0.5, 2.0, -2.0, 6.0]))
            if i % 9 == 8:
                li.couplingTsurf = -9999.0  # no usable observation: coupling off for the point
        if case.sky:
            li.lat = float(rs.uniform(59, 70)); li.lon = float(rs.uniform(19, 31))
            li.sky_view = float(rs.choice([0.0, 0.3, 0.75, 0.99, 1.0]))
        ls.append(li)
    _data[key] = (f, s, p, ls, bad)
    return _data[key]


def poison_state(plan, n, cls, f32):
    """The state block after init_state with its columns >= n poisoned, in the precision's own element type."""
    t = plan.state()
    v = state_view(t.numpy(), plan.np_pad, f32)
    if cls in ("nan", "huge"):
        v[:ST_BLSCORE, n:] = np.nan if cls == "nan" else np.finfo(v.dtype).max
    else:
        v[:NL, n:] = -5.0
        for row, val in ((ST_TNW1, -5.0), (ST_TNW2, -5.0), (ST_TSURF, -5.0), (ST_SNOW, 3.0), (ST_WAT, 0.5),
                         (ST_ICE, 1.0), (ST_ICE2, 0.5), (ST_DEP, 0.2),
                         (ST_BLSCORE, float(2 ** 21 - 1))):  # the largest sort key of rs_hip_recluster
            v[row, n:] = val
    plan.load_state(t)


def state_view(a: np.ndarray, np_pad: int, f32: bool) -> np.ndarray:
    """[RS_NSTATE][np_pad] in the element type of the plan (an fp32 plan keeps floats at the front of the block)."""
    if not f32:
        return a
    return a.view(np.float32).reshape(-1)[:lib.RS_NSTATE * np_pad].reshape(lib.RS_NSTATE, np_pad)


def make_knots(plan, arena: Arena, seed: int, wave: int):
    """plan.synth_knots into a carved buffer with the dry spell of the last wave; hostile: the pad columns overwritten
    on the device."""
    spec = lib.RsSynthSpec(seed, 0, SPK, 0)
    knots = arena.carve("knots", (NKNOTS, lib.RS_KNOT_FIELDS, plan.np_pad), torch.float64,
                        float_poison(arena.cls, "tair") if arena.hostile else 0.0)
    lib.check(plan.L.rs_hip_synth_knots(plan._h, C.byref(spec), C.c_void_p(knots.data_ptr()), 0, NKNOTS),
              "rs_hip_synth_knots")
    plan.sync()
    dry_spell_knots(knots, arena.n, wave)
    if arena.hostile:
        for q, name in enumerate(KNOT_FIELDS):
            knots[:, q, arena.n:] = float(SNOW_PHASE) if name == "precphase" else float_poison(arena.cls, name)
    else:
        knots[:, :, arena.n:] = 0.0
    return spec, knots


def sky_params(arena: Arena, f, ls, n):
    sun, *geo = legs.sky_tables(f, ls)
    assert sun.shape == (SIMLEN, 6)  # RS_SUN_COLS
    sky = {k: arena.vec(k, g, torch.float64) for k, g in zip(("sky_view", "sin_lat", "cos_lat", "lon_rad"), geo)}
    sky["horizons"] = arena.table("horizons", f["local_horizons"], torch.float64)
    sky["horizon_index"] = arena.vec("horizon_index", np.arange(n, dtype=np.int32), torch.int32)
    return sky, sun


def run_case(case: Case, n: int, seed: int, cls: str | None, failing: bool = False, by_point: bool = False):
    """One build of a case: cls None = clean, else the poison class of the hostile build.  Returns the live outputs
    [n][SimLen], the live columns of the state after init_state and after the run, the failure count and indices
    and, for a hostile build, what was written outside the live columns."""
    f, s, p, ls, bad = case_data(case, n, seed, failing)
    L = SIMLEN
    f32 = case.precision == 32
    plan = device.Plan(n, s, p, 0)
    if case.variant:
        plan.set_variant(case.variant)
    if f32:
        plan.set_precision(32)
    wdt = torch.float32 if f32 else torch.float64
    A = Arena(plan.device, n, plan.np_pad, cls)
    need_full = case.full or case.sky or bool(case.cpl) or case.depth
    relax = case.full
    sky = None
    spec = knots = None
    if case.src == "window":
        tens = {k: A.rows(k, f[k], wdt) for k in ("tair", "vz", "rhz", "prec", "sw", "lw", "tsurfobs")}
        tens["tdew"] = A.rows("tdew", f["tdew"], wdt) if need_full else None
        tens["depth"] = None
        tens["precphase"] = A.rows("precphase", f["precphase"], torch.int32)
        tens["hour"] = A.axis("hour", f["hour"], torch.int32)
        if case.sky:
            tens["sw_dir"] = A.rows("sw_dir", f["sw_dir"], wdt)
            tens["lw_net"] = A.rows("lw_net", f["lw_net"], wdt)
            sky, sun = sky_params(A, f, ls, n)
            tens["sun"] = A.axis("sun", sun, torch.float64)
        win = device.ForcingWindow(L, A.stride, tens)
        win0 = win
    else:
        spec, knots = make_knots(plan, A, seed, wave_points(case))
        for pt, idx in bad.items():  # the knot behind the index: the interpolated series leaves the limits before it
            knots[idx // SPK + 1, 0, pt] = 250.0
        # index 1 for the init kernel, expanded from the knots (which writes live columns only)
        t0 = {k: A.rows(k, None, wdt, nrows=1) for k in ("tair", "tdew", "vz", "rhz", "prec", "sw", "lw", "tsurfobs")}
        t0["depth"] = None
        t0["precphase"] = A.rows("precphase", None, torch.int32, nrows=1)
        t0["hour"] = A.carve("hour", (1,), torch.int32, A.fill("hour", torch.int32))
        win0 = device.ForcingWindow(1, A.stride, t0)
        plan.expand(spec, knots, win0, 1, 1)
        plan.sync()
        win = None
    tb = plan.uniform_tbottom(int(f["year"][0]), int(f["month"][0]), int(f["day"][0]))
    ppv = [A.vec("tbottom", np.full(n, tb), torch.float64)]
    ppv.append(A.vec("initlen", np.array([l.InitLenI for l in ls], np.int32), torch.int32) if need_full else None)
    for name, attr in (("tair_relax", "tair_relax"), ("vz_relax", "VZ_relax"), ("rh_relax", "RH_relax")):
        ppv.append(A.vec(name, np.array([getattr(l, attr) for l in ls]), torch.float64) if relax else None)
    ppv.append(A.vec("coupling_index", np.array([l.couplingIndexI for l in ls], np.int32), torch.int32) if case.cpl else None)
    ppv.append(A.vec("coupling_tsurf", np.array([l.couplingTsurf for l in ls]), torch.float64) if case.cpl else None)
    pp = plan.point_params(*ppv, sky)
    out = A.output(L, wdt)
    dst = None
    if by_point:  # point-major series [n][7 + SimLen] for rs_hip_outputs_by_point: exactly n rows
        dst = {k: A.carve("dst_" + k, (n, L + 7), torch.float64, float_poison(cls, "dst") if cls else -1.0, role="dst")
               for k in device.OUT_FIELDS}
    snap = A.snapshot()
    plan.init_state(win0, pp)
    state0 = state_view(plan.state().numpy(), plan.np_pad, f32)[:, :n].copy()
    if cls:
        poison_state(plan, n, cls, f32)
    if case.src == "knots":
        for t0_, ns in ((1, 120), (121, 120), (241, 1)):
            plan.step_knots(spec, knots, out, pp, t0_, ns, out_row0=0)
    elif case.cpl == "general":
        plan.step(win, out, pp, 1, L, window_row=0, out_row0=0)
    elif case.cpl == "chunk":
        for call, lo, hi in legs.coupling_stages(s, ls, L, chunked=True):  # lock-step chunks of 97, a replay whole
            t0_ = lo
            while t0_ <= hi:
                ns = hi - t0_ + 1 if call == "cpl_replay" else min(97, hi - t0_ + 1)
                getattr(plan, call)(win, out, pp, t0_, ns, window_row=t0_ - 1, out_row0=0)
                t0_ += ns
    else:
        launches = ((1, 120), (121, 120), (241, 1))  # the series ends in a launch of one index
        if case.a32_limit:
            # every launch must lose its 32-bit window offsets (rs_api.hip window_a32: forcing stride x indices, or
            # output stride x rows up to the launch's last, at or above the limit) - and the library honours a limit
            # only in [1024, 2^29): a value it ignores must not pass
            lim = int(case.a32_limit)
            assert 1024 <= lim < 2 ** 29 and os.environ.get("ROADSURF_HIP_A32_LIMIT") == case.a32_limit
            assert all(max(A.stride * ns, A.stride * (t0_ + ns - 1)) >= lim for t0_, ns in launches)
        for t0_, ns in launches:
            plan.step(win, out, pp, t0_, ns, window_row=t0_ - 1, out_row0=0)
    plan.sync()
    res = {"out": {k: out.tensors[k][:, :n].T.contiguous().cpu().numpy() for k in device.OUT_FIELDS},
           "state0": state0,
           "state": state_view(plan.state().numpy(), plan.np_pad, f32)[:, :n].copy(),
           "failed": plan.failed_count(), "first_failed": plan.first_failed_index(), "bad": bad}
    if by_point:
        plan.outputs_by_point(out, L, dst, dst_row0=7)
        plan.sync()
        res["dst"] = {k: dst[k].cpu().numpy() for k in device.OUT_FIELDS}
        res["dst_fill"] = float_poison(cls, "dst") if cls else -1.0
    res["touched"] = A.touched(snap) if cls else []
    plan.close()
    return res
