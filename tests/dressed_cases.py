"""The wavefronts of tests/storage_cases.py dressed with sky view and with coupling (a plain module: no fixture, no
pytest setting, no GPU at import) - tests/test_hip_sky_cpl_waves.py runs them on the GPU, and proves from the oracle's
outputs alone what they contain (test_the_dressings_are_what_they_claim, no GPU).

A dressing is a function of the crafted point - of its lane and its wavefront, and for the coupling observation of its
case - so it travels with the point through storage_cases.batch(mixed=True)'s permutation.  "lane" as in
storage_cases: the position in the first wavefront; the second wavefront is the first with the lanes reversed.

  sky        latitude 30 + 0.5 lane in the first wavefront (a January day, 09-15 UTC: a low sun) and -(10 + 0.5 lane)
             in the second (southern summer: a high one), longitude 20 + 2 (lane % 8), sky_view SKY_VIEWS[lane % 5]
             (1.0: no sky view for that lane), horizons 8 (lane % 4) + 3 (azimuth % 3) degrees: neighbours in a
             wavefront are in shade and in sun at the same index, some in the dark shortcut of sky_view_radiation,
             some without the branch at all
  cpl        use_coupling, a window of CPL_MINUTES, InitLenI = 1, couplingIndexI = CPL_INDEX; couplingTsurf = the
             UNCOUPLED oracle's Tsurf at that index (15 layers, the same sky dressing) + CPL_OFFSETS[lane % 8]: every
             wavefront holds points that are accepted at once, after a few replays and never (25 replays);
             lane % 16 == 15: couplingIndexI = 0, lane % 16 == 14: couplingTsurf = -9999 - coupling off for the point
  driver     the case's knots as an hourly forecast source (the one test_driver_raw_series_equals_its_oracle builds;
             with sky view also the direct short wave and the net long wave, as golden_helpers.expand_knots has them)
             and an hourly observation source over knots 0 .. DRIVER_OBS_KNOTS - 1 with tair, rhz, vz, prec and
             tsurfobs = the uncoupled driver oracle's Tsurf at those hours, the last one shifted by
             CPL_OFFSETS[lane % 8]; forecast_time = start + 4 h, use_coupling = use_relaxation = 1, outputStep = 1:
             read_input itself sets InitLenI, couplingIndexI and couplingTsurf

The references are the CPU oracle's - the reference's own Fortran where it is built (with working coupling for a
coupled run: oracle_helpers.REF_CPL_SO), the C restatement otherwise - made once per process and never written to.
"""
from __future__ import annotations

import os

import numpy as np

import knot_helpers as kh
import oracle_helpers as oh
import storage_cases as sc
from roadsurf_amd import abi

N, L, CASES = sc.N, sc.L, sc.CASES
SKY_VIEWS = (0.0, 0.3, 0.75, 0.99, 1.0)
CPL_OFFSETS = (0.0, 0.05, -0.5, 2.0, -2.0, 6.0, -6.0, 0.5)
CPL_MINUTES, CPL_INDEX = 120, 481
WINDOW = slice(CPL_INDEX - CPL_MINUTES * 2 - 1, CPL_INDEX)  # the rows of the indices 241 .. 481
SUNNY = ("melt_out", "thaw_ramp", "minus_zero")
SNOW_IN_WINDOW = ("one_snowy", "sleet_ladder", "melt_out", "frost_ladder", "rain_on_snow", "heavy_snow_one")
DRIVER_OBS_KNOTS = 5
RAW_NAMES = ("tair", "rhz", "vz", "prec", "sw", "lw")
OBS_NAMES = ("tair", "rhz", "vz", "prec")


def kind(coupled: bool) -> str:
    if coupled:
        return "ref_cpl" if os.path.exists(oh.REF_CPL_SO) else "port"
    return "ref" if oh.have_ref() else "port"


def sky_of_points():
    """(lat, lon, sky_view [N], horizons [N][360]) of a case's 128 points."""
    lane = sc.LANE
    first = np.arange(N) < 64
    lat = np.where(first, 30.0 + 0.5 * lane, -(10.0 + 0.5 * lane))
    lon = 20.0 + 2.0 * (lane % 8)
    sky_view = np.asarray(SKY_VIEWS)[lane % 5]
    hz = 8.0 * (lane % 4)[:, None] + 3.0 * (np.arange(360) % 3)[None, :]
    return lat, lon, sky_view, np.ascontiguousarray(hz)


def coupling_off(lane):
    """(couplingIndexI = 0, couplingTsurf = -9999) of the lanes"""
    return lane % 16 == 15, lane % 16 == 14


def settings(cpl: bool = False, nlayers: int = 15):
    s = abi.default_settings(L)
    s.NLayers = nlayers
    if cpl:
        s.use_coupling = 1
        s.coupling_minutes = CPL_MINUTES
    return s


def locals_of(sky: bool, base_tsurf=None):
    """The 128 LocalParameters of a case; base_tsurf [N][L]: the uncoupled rows the coupling observation is made
    from (None: no coupling)."""
    lat, lon, sky_view, _ = sky_of_points()
    no_index, no_obs = coupling_off(sc.LANE)
    out = []
    for i in range(N):
        l = sc.local()
        if sky:
            l.lat, l.lon, l.sky_view = float(lat[i]), float(lon[i]), float(sky_view[i])
        if base_tsurf is not None:
            l.couplingIndexI = 0 if no_index[i] else CPL_INDEX
            l.couplingTsurf = -9999.0 if no_obs[i] else float(base_tsurf[i, CPL_INDEX - 1] +
                                                              CPL_OFFSETS[int(sc.LANE[i]) % 8])
        out.append(l)
    return out


def forcing_of(case, sky: bool):
    f = dict(sc.references()[case][1])
    if sky:
        f["local_horizons"] = sky_of_points()[3]
    return f


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


_REFS: dict = {}


def references(sky: bool, cpl: bool, nlayers: int = 15, which: str | None = None):
    """{case: (forcing, locals, oracle outputs [N][L], first failed index [N], the oracle's mutated sw_dir [N][L])} of
    a dressing at a layer count; made once per process, the arrays read-only.  The coupling observation comes from the
    15-layer uncoupled reference of the same sky dressing, whatever ``nlayers``: it belongs to the point, not to the
    model's grid.  ``which``: the oracle, default kind(cpl)."""
    which = which or kind(cpl)
    key = (sky, cpl, nlayers, which)
    if key not in _REFS:
        if not sky and not cpl and nlayers == 15 and which == kind(False):
            plain = sc.references()
            _REFS[key] = {c: (plain[c][1], [sc.local()] * N, plain[c][2], plain[c][3], plain[c][1]["sw_dir"])
                          for c in CASES}
            return _REFS[key]
        base = references(sky, False, 15) if cpl else None
        refs = {}
        for case in CASES:
            f = forcing_of(case, sky)
            ls = locals_of(sky, base[case][2]["tsurf"] if cpl else None)
            ora, fmut, _ = oh.run_oracle(which, f, settings(cpl, nlayers), abi.default_parameters(), ls)
            _frozen(ora)
            failed = kh.first_blank(ora)
            failed.setflags(write=False)
            fmut["sw_dir"].setflags(write=False)
            refs[case] = (f, ls, ora, failed, fmut["sw_dir"])
        _REFS[key] = refs
    return _REFS[key]


def batch(sky: bool, cpl: bool, nlayers: int, mixed: bool):
    """All cases of a dressing in one batch of N * len(CASES) points, in the crafted order or under
    storage_cases.permutation(): (forcing, locals, oracle outputs, first failed index, point of every slot).  The
    oracle is per point: rows, locals and horizons are the cases', concatenated and permuted."""
    refs = references(sky, cpl, nlayers)
    slot = sc.permutation() if mixed else np.arange(N * len(CASES))
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts, axis=0)[slot])
    f0 = refs[CASES[0]][0]
    f = {k: (cat([refs[c][0][k] for c in CASES]) if (v.ndim == 2 and v.shape[0] == N) else v.copy())
         for k, v in f0.items()}
    every = [l for c in CASES for l in refs[c][1]]
    ls = [every[int(q)] for q in slot]
    ora = {k: cat([refs[c][2][k] for c in CASES]) for k in kh.OUT}
    failed = cat([refs[c][3] for c in CASES])
    return f, ls, ora, failed, slot


# ---- the driver: two sources ---------------------------------------------------------------------------------------

def driver_settings(coupled: bool):
    s = sc.settings()
    s.outputStep = 1  # every second index is kept
    if coupled:
        s.use_coupling = s.use_relaxation = 1
    return s


def driver_times():
    """(start, forecast_time) of the coupled layout; the uncoupled one takes forecast_time = start."""
    import driver_helpers as dh
    t0 = dh.START + sc.START_HOUR * 3600
    return t0, t0 + (DRIVER_OBS_KNOTS - 1) * 3600


def _forecast_source(K, sky):
    """One hourly forecast source of the knots; with sky view the two radiation streams the branch reads as well -
    the direct short wave 0.6 of the global and a net long wave of -40 W/m2, as golden_helpers.expand_knots has
    them (a point with a sky view and without them fails CheckValues at index 1)."""
    from roadsurf_amd import driver
    t0, _ = driver_times()
    if sky:
        K = dict(K, sw_dir=0.6 * K["sw"], lw_net=np.full(K["sw"].shape, -40.0))
    # (the last knot once more an hour behind the end: the reference's interpolation leaves an index ON the last raw
    # time missing)
    return driver.RawSource(t0 + 3600 * np.arange(sc.NK + 1, dtype=np.int64),
                            {k: np.ascontiguousarray(np.concatenate([K[k], K[k][:, -1:]], axis=1), np.float64)
                             for k in RAW_NAMES + (("sw_dir", "lw_net") if sky else ())}, False)


def _driver_sky():
    lat, lon, sky_view, hz = sky_of_points()
    ls = []
    for i in range(N):
        l = abi.default_local()
        l.lat, l.lon, l.sky_view = float(lat[i]), float(lon[i]), float(sky_view[i])
        ls.append(l)
    return ls * len(CASES), np.ascontiguousarray(np.tile(hz, (len(CASES), 1)))


_DRIVER: dict = {}


def driver_reference(sky: bool, coupled: bool, which: str | None = None):
    """The crafted-order driver batch of all cases and its oracle: dict(src, settings, start, forecast_time, local,
    horizons, oracle) - local and horizons None without sky view.  Made once per process."""
    import driver_helpers as dh
    from roadsurf_amd import driver
    which = which or kind(coupled)
    key = (sky, coupled, which)
    if key in _DRIVER:
        return _DRIVER[key]
    Ks = [sc.knots_of(c) for c in CASES]
    K = {k: np.ascontiguousarray(np.concatenate([q[k] for q in Ks], axis=0)) for k in RAW_NAMES}
    n = N * len(CASES)
    local, hz = _driver_sky() if sky else (None, None)
    t0, tf = driver_times()
    p = abi.default_parameters()
    src = [_forecast_source(K, sky)]
    if coupled:
        base = driver_reference(sky, False)["oracle"]
        rows = 60 * np.arange(DRIVER_OBS_KNOTS)  # hour h is index 120 h + 1, kept row 60 h
        obs = {k: np.ascontiguousarray(K[k][:, :DRIVER_OBS_KNOTS]) for k in OBS_NAMES}
        tobs = np.array(base["tsurf"][:, rows])
        tobs[:, -1] += np.asarray(CPL_OFFSETS)[np.tile(sc.LANE, len(CASES)) % 8]
        obs["tsurfobs"] = np.ascontiguousarray(tobs)
        src.append(driver.RawSource(t0 + 3600 * np.arange(DRIVER_OBS_KNOTS, dtype=np.int64), obs, True))
    else:
        tf = t0
    s = driver_settings(coupled)
    o = dh.oracle_run(which, src, s, p, t0, tf, local=local, horizons=hz)
    for k in kh.OUT + ("status", "missing_index"):
        o[k].setflags(write=False)
    assert o["tsurf"].shape == (n, (L + 1) // 2)
    _DRIVER[key] = dict(src=src, settings=s, start=t0, forecast_time=tf, local=local, horizons=hz, oracle=o)
    return _DRIVER[key]


def driver_batch(sky: bool, coupled: bool, mixed: bool):
    """driver_reference's batch in the crafted order or under storage_cases.permutation(): (sources, settings, start, forecast_time, local,
    horizons, oracle rows dict, point of every slot)."""
    from roadsurf_amd import driver
    d = driver_reference(sky, coupled)
    slot = sc.permutation() if mixed else np.arange(N * len(CASES))
    src = [driver.RawSource(x.times, {k: np.ascontiguousarray(v[slot]) for k, v in x.fields.items()},
                            x.is_observation) for x in d["src"]]
    local = None if d["local"] is None else [d["local"][int(q)] for q in slot]
    hz = None if d["horizons"] is None else np.ascontiguousarray(d["horizons"][slot])
    o = {k: np.ascontiguousarray(d["oracle"][k][slot]) for k in kh.OUT + ("status", "missing_index")}
    return src, d["settings"], d["start"], d["forecast_time"], local, hz, o, slot
