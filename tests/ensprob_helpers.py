"""What tests/test_ensprob_reference.py (CPU) and tests/test_hip_ensprob.py (GPU) share: made member series with every
edge the definition names, the conditions, the station layouts, and the non-vacuity counts on the reference case."""
from __future__ import annotations

import numpy as np

from roadsurf_amd import ensemble, ensprob

OUT = ("tsurf", "snow", "water", "ice", "deposit", "ice2")
SERIES = OUT + ("deficit",)
# few values, all exact in fp32 too, so that many of them lie exactly ON a bound: every bound below is one of them
TSURF_VALUES = np.array([-2.0, -0.5, 0.0, 0.0, 0.5, 1.5, 2.0])
STORAGE_VALUES = np.array([0.0, 0.125, 0.125, 0.75])
DEFICIT_VALUES = np.array([-1.0, -0.25, 0.0, 0.5])

W = ensprob.Condition.where
CONDITIONS = (W(tsurf=(None, 0.0)), W(ice=(0.0, None)), W(tsurf=(None, 2.0), water=(0.125, None)),
              W(deficit=(None, 0.0)), W(snow=(0.0, 0.75)), W(deposit=(0.125, None), ice2=(None, 0.75)),
              W(tsurf=(-2.0, 1.5)), W(tsurf=(None, 0.5), snow=(0.0, None), water=(None, 0.75)))
# what the issue asks of the reference case: the three conditions a forecaster would name
FORECAST_CONDITIONS = (W(tsurf=(None, 0.0)), W(ice=(0.0, None)), W(tsurf=(None, 2.0), water=(0.05, None)))


def conditions(how_many):
    """1, 3 or 8 of CONDITIONS; the eight include the one on the deficit."""
    return CONDITIONS[:how_many]


def made_series(n, nrows, seed, np_dtype=np.float64):
    """Seven series [n, nrows] in point order: values from the small sets (many exactly on a bound), some points with a
    -9999.0 tail, one point invalid everywhere, a NaN Tsurf, NaN storages under used bounds, deficits of -9999.0."""
    rs = np.random.RandomState(seed)
    d = {"tsurf": TSURF_VALUES[rs.randint(0, len(TSURF_VALUES), (n, nrows))]}
    for k in OUT[1:]:
        d[k] = STORAGE_VALUES[rs.randint(0, len(STORAGE_VALUES), (n, nrows))]
    d["deficit"] = DEFICIT_VALUES[rs.randint(0, len(DEFICIT_VALUES), (n, nrows))]
    d["deficit"][rs.rand(n, nrows) < 0.1] = -9999.0
    for p in range(0, n, 5):
        d["tsurf"][p, rs.randint(0, nrows):] = -9999.0
    if n >= 3:
        d["tsurf"][n // 2] = -9999.0
    d["tsurf"][n - 1, nrows // 2] = np.nan
    d["ice"][n - 1, 0] = np.nan
    if n >= 7:
        d["water"][n - 4, nrows - 1] = np.nan
        d["ice"][n - 3, nrows // 3] = np.nan
    return {k: np.ascontiguousarray(v.astype(np_dtype)) for k, v in d.items()}


def layouts(S, M, rs):
    """(name, ids [S * M], ngroups, max_members): the members of a station side by side; far apart, with a last station
    that has no member and room for more members than any station has; the same with ids of -1 and ids >= ngroups."""
    n = S * M
    irregular = ((np.arange(n) * 37 + 11) % S).astype(np.int32)
    outside = irregular.copy()
    outside[rs.rand(n) < 0.1] = -1
    outside[rs.rand(n) < 0.1] = S + 1 + rs.randint(0, 3)
    most = int(np.bincount(irregular).max())
    return [("parents", ensemble.parents(S, M), S, M), ("irregular", irregular, S + 1, min(64, most + 3)),
            ("ids outside", outside, S + 1, most)]


def reduce(d, gid, spec, ever=None, rows=slice(None)):
    """reduce_members_prob of the made series' rows ``rows``."""
    x = [d[k][:, rows] for k in OUT] + [d["deficit"][:, rows] if ensprob.needs_deficit(spec) else None]
    return ensprob.reduce_members_prob(*x, gid, spec, ever)


def non_vacuity(cells, spec, members):
    """Per condition: (cells with 0 < NOW < members, cells with BY_NOW > NOW)."""
    C = len(spec.conditions)
    now, by = cells[:, :, 1:1 + C], cells[:, :, 1 + C:]
    return [(int(((now[:, :, c] > 0) & (now[:, :, c] < members)).sum()), int((by[:, :, c] > now[:, :, c]).sum()))
            for c in range(C)]
