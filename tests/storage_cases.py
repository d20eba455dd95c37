"""Hand-made wavefronts for the storage, precipitation and thaw shortcuts of rs_physics_body.inc (a plain module: no
fixture, no pytest setting, no GPU at import) - tests/test_hip_storage_waves.py runs them on the GPU, and proves
from the oracle's outputs alone what they contain (test_the_cases_are_what_they_claim, no GPU).

Every case: 128 points x 6 h (721 indices) from 7 hourly knots, 120 steps per knot, settings and parameters at their
defaults, InitLenI = 1, the clock started at START_HOUR for all of them - so that cases can be concatenated into one
batch.  "lane" below is the position in the first wavefront; the second wavefront is the first with the lanes reversed
(lane l is point l and point 127 - l).  The reference is knot_helpers.expand + knot_helpers.reference: the reference's
own Fortran where it is built, the C restatement otherwise.

  one_snowy          air -5, surface -4 degrees, dark; snow (phase 3) of 1 mm/h on lane 17 in knots 1-2: one lane with
                     snow among bare ones, later ice and ice2 on that lane - born in a wavefront that had none
  freezing_rain_one  air -3, surface -2 degrees; rain (phase 1) on the same lane: the water freezes in the step it
                     falls in (`freezes` in a wavefront with no ice), the water row stays 0
  sleet_ladder       air -2 .. +2 degrees across the lanes, sleet (phase 2) of 2 mm/h in knots 1-3: snow on all lanes,
                     water on some, the surface below zero in some lanes only, rain that freezes on the cold lanes
  melt_out           snow of 0.3 + 0.01 lane mm/h in knots 0-1, the air -1 -> 5 degrees and the sun 0 -> 300 W/m2 over
                     the six hours: every storage goes through none / some / all lanes, and so does tsurf < 0
  thaw_ramp          dry at 40 % humidity, the air -4 -> +4 degrees with the lanes 0.05 K apart and the sun 0 -> 400
                     W/m2: bare throughout (the storage block is the shortcut at every step) while the upper layers
                     go all-frozen -> mixed -> all-thawed
  frost_ladder       air -2 degrees at 98 % humidity, the surface -6 .. -1 degrees across the lanes: deposit on all
                     lanes - no lane bare although every other storage is +0.0; snow on lane 17 in knot 4 turns that
                     lane's deposit into ice (Storage.f90, SnowStorage)
  odd_prec           air +2 degrees; precipitation -0.05 on lane 3 (CheckValues lets it through), -0.0 on lane 4, 1e-7
                     (under MinPrecmm) on lane 5, 0.5 mm/h with phase 7 (CalcPrecType's default arm) on lane 6, 0.5
                     mm/h with phase -9999 (from Tair and Rhz) on lane 7; the second wavefront all zero
  heavy_snow_one     -8 degrees, snow of 60 mm/h on lane 17 and 99 mm/h on lane 40: Snowmms reaches MaxSnowmms and
                     drops by its half, Icemms reaches MaxIcemms
  minus_zero         `thaw_ramp` with lane 31's air and first surface temperature -0.0 and lane 32's +0.0
  rain_on_snow       (not among the cases the shortcuts were first listed with: sleet_ladder's 2 mm/h never fills the
                     pores, so its snow is never wet)  air -1 .. +3 degrees across the lanes, snow of 0.3 mm/h in
                     knots 0-1, then rain of 10 mm/h in knots 2-4: water reaches MaxWatmms, thin snow over standing
                     water - wet snow that melts at once on the warm lanes (WetSnowMeltR) while the rain freezes as it
                     falls on the cold ones
"""
from __future__ import annotations

import numpy as np

import knot_helpers as kh
from roadsurf_amd import abi

SPK = 120
N, NK, L = 128, 7, 721
START_HOUR = 9
CASES = ("one_snowy", "freezing_rain_one", "sleet_ladder", "melt_out", "thaw_ramp", "frost_ladder", "odd_prec",
         "heavy_snow_one", "minus_zero", "rain_on_snow")
LANE = np.concatenate([np.arange(64), np.arange(64)[::-1]])
ONE, HEAVY_60, HEAVY_99 = 17, 17, 40
ODD = {"negative": 3, "minus_zero": 4, "tiny": 5, "phase7": 6, "phase_auto": 7}
MZ_NEG, MZ_POS = 31, 32
PERM_SEED = 20240110


def points_of(*lanes):
    """The points (both wavefronts) that sit on the given lanes."""
    return np.nonzero(np.isin(LANE, lanes))[0]


def local():
    l = abi.default_local(); l.InitLenI = 1
    return l


def settings():
    return abi.default_settings(L)


def knots_of(case):
    """knots [N][NK] per field (+ phase, tsurf0 [N])"""
    lane = LANE.astype(np.float64)
    col = lambda v: np.repeat(np.broadcast_to(np.asarray(v, np.float64), (N,))[:, None], NK, axis=1)
    ramp = lambda a, b: np.repeat(np.linspace(a, b, NK)[None, :], N, axis=0)
    K = {"tair": col(-5.0), "tdew": col(-8.0), "vz": col(3.0), "rhz": col(80.0), "prec": np.zeros((N, NK)),
         "sw": np.zeros((N, NK)), "lw": col(250.0), "phase": np.ones((N, NK), np.int32)}
    K["tsurf0"] = np.full(N, -4.0)
    one = LANE == ONE
    if case == "one_snowy":
        K["phase"][:] = 3
        K["prec"][one, 1:3] = 1.0
    elif case == "freezing_rain_one":
        K["tair"] = col(-3.0)
        K["tsurf0"] = np.full(N, -2.0)
        K["prec"][one, 1:3] = 1.0
    elif case == "sleet_ladder":
        K["tair"] = col(-2.0 + 4.0 * lane / 63.0)
        K["tsurf0"] = K["tair"][:, 0].copy()
        K["lw"] = col(300.0)
        K["phase"][:] = 2
        K["prec"][:, 1:4] = 2.0
    elif case == "melt_out":
        K["tair"] = ramp(-1.0, 5.0)
        K["tsurf0"] = np.full(N, -1.0)
        K["sw"] = ramp(0.0, 300.0)
        K["lw"] = col(300.0)
        K["phase"][:] = 3
        K["prec"][:, 0:2] = (0.3 + 0.01 * lane)[:, None]
    elif case in ("thaw_ramp", "minus_zero"):
        K["tair"] = ramp(-4.0, 4.0) + 0.05 * lane[:, None]
        K["tsurf0"] = K["tair"][:, 0].copy()
        K["rhz"] = col(40.0)
        K["tdew"] = col(-15.0)
        K["sw"] = ramp(0.0, 400.0)
        K["lw"] = col(300.0)
        if case == "minus_zero":
            K["tair"][LANE == MZ_NEG] = -0.0
            K["tsurf0"][LANE == MZ_NEG] = -0.0
            K["tair"][LANE == MZ_POS] = 0.0
            K["tsurf0"][LANE == MZ_POS] = 0.0
    elif case == "frost_ladder":
        K["tair"] = col(-2.0)
        K["tdew"] = col(-2.3)
        K["rhz"] = col(98.0)
        K["tsurf0"] = -6.0 + 5.0 * lane / 63.0
        K["phase"][:] = 3
        K["prec"][one, 4] = 1.0
    elif case == "odd_prec":
        K["tair"] = col(2.0)
        K["tdew"] = col(-1.0)
        K["tsurf0"] = np.full(N, 2.0)
        K["lw"] = col(300.0)
        first = np.arange(N) < 64
        K["prec"][first & (LANE == ODD["negative"])] = -0.05
        K["prec"][first & (LANE == ODD["minus_zero"])] = -0.0
        K["prec"][first & (LANE == ODD["tiny"])] = 1e-7
        K["prec"][first & (LANE == ODD["phase7"])] = 0.5
        K["phase"][first & (LANE == ODD["phase7"])] = 7
        K["prec"][first & (LANE == ODD["phase_auto"])] = 0.5
        K["phase"][first & (LANE == ODD["phase_auto"])] = -9999
    elif case == "heavy_snow_one":
        K["tair"] = col(-8.0)
        K["tdew"] = col(-11.0)
        K["tsurf0"] = np.full(N, -8.0)
        K["phase"][:] = 3
        K["prec"][LANE == HEAVY_60] = 60.0
        K["prec"][LANE == HEAVY_99] = 99.0
    elif case == "rain_on_snow":
        K["tair"] = col(-1.0 + 4.0 * lane / 63.0)
        K["tsurf0"] = K["tair"][:, 0].copy()
        K["lw"] = col(300.0)
        K["prec"][:, 0:2] = 0.3
        K["phase"][:, 0:2] = 3
        K["prec"][:, 2:5] = 10.0
    else:
        raise KeyError(case)
    return {k: np.ascontiguousarray(v) for k, v in K.items()}


def reference_of(K):
    """(knots, expanded forcing, oracle outputs [n][L], first failed index [n]) of a knot block."""
    f = kh.expand(K, L, SPK, start_hour=START_HOUR)
    ora, failed = kh.reference(f, settings(), abi.default_parameters(), local())
    return K, f, ora, failed


_REFS: dict = {}


def references():
    """{case: reference_of(knots_of(case))}, made once per process and never written to."""
    if not _REFS:
        for case in CASES:
            _REFS[case] = reference_of(knots_of(case))
            for a in (*_REFS[case][2].values(), _REFS[case][3]):  # (the oracle's rows: nobody writes to them)
                a.setflags(write=False)
    return _REFS


def permutation():
    """The fixed permutation of the concatenated batch: slot s holds point permutation()[s]."""
    return np.random.RandomState(PERM_SEED).permutation(N * len(CASES))


def batch(mixed: bool):
    """All cases in one batch of N * len(CASES) points, in the crafted order (case c owns the points c * N ..) or
    permuted by permutation(): (knots, forcing, oracle outputs, first failed index, point of every slot).  The oracle
    is per point: its rows are the cases' rows, concatenated and permuted - nothing is computed again."""
    refs = references()
    slot = permutation() if mixed else np.arange(N * len(CASES))
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts, axis=0)[slot])
    K = {k: cat([refs[c][0][k] for c in CASES]) for k in refs[CASES[0]][0]}
    f0 = refs[CASES[0]][1]
    f = {k: (cat([refs[c][1][k] for c in CASES]) if (v.ndim == 2 and v.shape[0] == N) else v.copy())
         for k, v in f0.items()}
    ora = {k: cat([refs[c][2][k] for c in CASES]) for k in kh.OUT}
    failed = cat([refs[c][3] for c in CASES])
    return K, f, ora, failed, slot


def case_of_point(point):
    return np.asarray(point) // N
