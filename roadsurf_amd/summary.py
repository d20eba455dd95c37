"""Per-point forecast summaries of the six output series: the definition, in numpy.

What a road-weather consumer derives from a point's series - the lowest surface temperature and when, whether and
when the surface first drops below a threshold and for how long, how much snow, water, ice, deposit there is at most
and for how long - as ``RS_SUM_COLS`` numbers per point.  ``reduce_series`` is the specification; the device
reducer (``rs_hip_outputs_summary``, ``rs_driver_run_summary``: include/roadsurf.h) is held to it exactly by the
tests.  Columns of a summary row::

    0        number of valid rows (a row is valid iff its Tsurf is not exactly -9999.0)
    1, 2     min Tsurf, index of it (the smallest index among equals)
    3, 4     max Tsurf, index of it (the smallest index among equals)
    5        smallest index with Tsurf < spec.tsurf_below (0 = none)
    6        number of rows with Tsurf < spec.tsurf_below
    7..11    max of snow, water, ice, deposit, ice2
    12..16   number of rows with that storage > spec.storage_above[k]

Only valid rows count; every comparison is strict; NaN compares false everywhere and still counts as a valid
row.  A point without valid rows has count 0, min +inf, max -inf, indices 0, storage maxima -inf, counts 0.
Indices are absolute 1-based time indices.
"""
from __future__ import annotations

import dataclasses

import numpy as np

RS_SUM_COLS = 17
INVALID = -9999.0  # OutputData.cpp:5-13: what rows the simulation never saved read
STORAGES = ("snow", "water", "ice", "deposit", "ice2")
(COUNT, TMIN, TMIN_INDEX, TMAX, TMAX_INDEX, FIRST_BELOW, N_BELOW) = range(7)
STORAGE_MAX, STORAGE_COUNT = 7, 12


@dataclasses.dataclass
class SummarySpec:
    """Thresholds of a summary (RsSummarySpec): Tsurf strictly below, storages strictly above."""
    tsurf_below: float = 0.0
    storage_above: tuple = (0.0, 0.0, 0.0, 0.0, 0.0)


def empty(n: int) -> np.ndarray:
    """The summary of no rows for n points."""
    a = np.zeros((n, RS_SUM_COLS))
    a[:, TMIN] = np.inf
    a[:, TMAX] = -np.inf
    a[:, STORAGE_MAX:STORAGE_MAX + 5] = -np.inf
    return a


def merge(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The summary of the rows behind ``a`` and the rows behind ``b`` together (disjoint sets of rows: a row
    that is behind both is counted twice).  Extremes tie to the smaller index, the first index below the
    threshold is the smaller of the two with 0 as "none", counts add - so the order of merging does not matter."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    r = a.copy()
    r[:, COUNT] = a[:, COUNT] + b[:, COUNT]
    lower = (b[:, TMIN] < a[:, TMIN]) | ((b[:, TMIN] == a[:, TMIN]) & (b[:, TMIN_INDEX] < a[:, TMIN_INDEX]))
    r[lower, TMIN:TMIN_INDEX + 1] = b[lower, TMIN:TMIN_INDEX + 1]
    higher = (b[:, TMAX] > a[:, TMAX]) | ((b[:, TMAX] == a[:, TMAX]) & (b[:, TMAX_INDEX] < a[:, TMAX_INDEX]))
    r[higher, TMAX:TMAX_INDEX + 1] = b[higher, TMAX:TMAX_INDEX + 1]
    fa, fb = a[:, FIRST_BELOW], b[:, FIRST_BELOW]
    r[:, FIRST_BELOW] = np.where(fa == 0, fb, np.where(fb == 0, fa, np.minimum(fa, fb)))
    r[:, N_BELOW] = a[:, N_BELOW] + b[:, N_BELOW]
    for k in range(5):
        c = STORAGE_MAX + k
        more = b[:, c] > a[:, c]
        r[more, c] = b[more, c]
        r[:, STORAGE_COUNT + k] = a[:, STORAGE_COUNT + k] + b[:, STORAGE_COUNT + k]
    return r


def _extreme(v, ok, index, lowest: bool):
    """(value, smallest index of it) over the rows `ok` of every point; NaN and the empty value itself never win."""
    none = np.inf if lowest else -np.inf
    w = np.where(ok & ~np.isnan(v), v, none)
    m = w.min(axis=1) if lowest else w.max(axis=1)
    hit = ok & (v == m[:, None]) & (m[:, None] != none)
    far = np.iinfo(np.int64).max
    idx = np.where(hit, index[None, :], far).min(axis=1)
    return m, np.where(idx == far, 0, idx).astype(np.float64)


def reduce_series(tsurf, snow, water, ice, deposit, ice2, index, spec, acc=None) -> np.ndarray:
    """Summaries float64[n, RS_SUM_COLS] of the series [n, nrows] (any float type; widened to float64, which
    is exact); ``index[r]`` is the absolute 1-based time index of row r; ``spec`` has ``tsurf_below`` and
    ``storage_above[5]``.  ``acc``: an earlier result over OTHER rows of the same points to merge into."""
    t = np.asarray(tsurf, np.float64)
    n, nrows = t.shape
    index = np.asarray(index, np.int64)
    assert index.shape == (nrows,)
    out = empty(n)
    if nrows:
        ok = t != INVALID
        out[:, COUNT] = ok.sum(axis=1)
        out[:, TMIN], out[:, TMIN_INDEX] = _extreme(t, ok, index, True)
        out[:, TMAX], out[:, TMAX_INDEX] = _extreme(t, ok, index, False)
        below = ok & (t < float(spec.tsurf_below))
        far = np.iinfo(np.int64).max
        first = np.where(below, index[None, :], far).min(axis=1)
        out[:, FIRST_BELOW] = np.where(first == far, 0, first)
        out[:, N_BELOW] = below.sum(axis=1)
        for k, s in enumerate((snow, water, ice, deposit, ice2)):
            s = np.asarray(s, np.float64)
            assert s.shape == t.shape
            out[:, STORAGE_MAX + k] = np.where(ok & ~np.isnan(s), s, -np.inf).max(axis=1)
            out[:, STORAGE_COUNT + k] = (ok & (s > float(spec.storage_above[k]))).sum(axis=1)
    return out if acc is None else merge(acc, out)
