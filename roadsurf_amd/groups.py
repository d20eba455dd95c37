"""Per-group time series of the six output series: the definition, in numpy.

The other axis of reduction beside ``summary.py``: per kept row, over a set of points.  Every point has a group id
(``group[n]``, int32, point order; an id outside ``[0, ngroups)`` belongs to no group and is ignored) - a district of
a road network, or the station whose ensemble members the points are - and for every row r and group g there is one
cell of ``cols(spec)`` numbers.  ``reduce_groups`` is the specification; the device reducer
(``rs_hip_outputs_groups``, ``rs_driver_run_groups``: include/roadsurf.h) is held to it exactly by the tests.
Columns of a cell::

    0        number of valid points of g at row r (valid iff Tsurf is not exactly -9999.0; only these count below)
    1, 2     min Tsurf, max Tsurf            (+inf / -inf when there is none; a NaN never wins)
    3        number of points with Tsurf < spec.thresholds.tsurf_below
    4..8     number of points with snow, water, ice, deposit, ice2 > spec.thresholds.storage_above[k]
    9..13    max of snow, water, ice, deposit, ice2   (-inf when none; a NaN never wins)
    14..     optional histogram of Tsurf over spec.edges (strictly increasing, at most RS_GRP_MAX_EDGES): nedges + 1
             bins, a valid non-NaN Tsurf falls into bin j = number of edges <= Tsurf (a value equal to an edge lies in
             the upper bin, a NaN in no bin).  No edges: no bins.

Every comparison is strict; NaN compares false everywhere and still counts in column 0.  There are no sums and no
means, on purpose: every column is a count (exact in float64), a minimum or a maximum, so the merge of two cells is
exact, commutative and associative, and the result does not depend on the order in which points, launches, tiles or
devices contribute.  Medians and percentiles come from the histogram.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import summary

RS_GRP_COLS = 14
RS_GRP_MAX_EDGES = 31
INVALID = summary.INVALID
(COUNT, TMIN, TMAX, N_BELOW) = range(4)
STORAGE_COUNT, STORAGE_MAX, BINS = 4, 9, 14


@dataclasses.dataclass
class GroupSpec:
    """RsGroupSpec: the thresholds of a summary.SummarySpec, the number of groups and the histogram's edges."""
    thresholds: summary.SummarySpec = dataclasses.field(default_factory=summary.SummarySpec)
    ngroups: int = 1
    edges: tuple = ()


def _checked(spec) -> np.ndarray:
    edges = np.asarray(spec.edges, np.float64).reshape(-1)
    if int(spec.ngroups) < 1:
        raise ValueError("ngroups: at least one group")
    if len(edges) > RS_GRP_MAX_EDGES:
        raise ValueError(f"edges: at most {RS_GRP_MAX_EDGES}")
    if np.isnan(edges).any() or not (np.diff(edges) > 0).all():
        raise ValueError("edges: strictly increasing")
    return edges


def cols(spec) -> int:
    """Numbers per cell: RS_GRP_COLS, and nedges + 1 bins where there are edges."""
    nedges = len(_checked(spec))
    return RS_GRP_COLS + (nedges + 1 if nedges else 0)


def empty(nrows: int, spec) -> np.ndarray:
    """The cells of no points: [nrows, ngroups, cols]."""
    a = np.zeros((nrows, int(spec.ngroups), cols(spec)))
    a[:, :, TMIN] = np.inf
    a[:, :, TMAX] = -np.inf
    a[:, :, STORAGE_MAX:STORAGE_MAX + 5] = -np.inf
    return a


def merge(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The cells of the points behind ``a`` and the points behind ``b`` together (a point behind both is counted
    twice): counts add, extremes are the extremes of the two."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape
    r = a + b                                   # the counts (and the bins); the rest is overwritten
    r[..., TMIN] = np.minimum(a[..., TMIN], b[..., TMIN])          # (cells never hold a NaN)
    r[..., TMAX] = np.maximum(a[..., TMAX], b[..., TMAX])
    s = slice(STORAGE_MAX, STORAGE_MAX + 5)
    r[..., s] = np.maximum(a[..., s], b[..., s])
    return r


def reduce_groups(tsurf, snow, water, ice, deposit, ice2, group, spec, acc=None) -> np.ndarray:
    """Cells float64[nrows, ngroups, cols] of the series [n, nrows] (any float type; widened to float64, which is
    exact) of the points whose groups are ``group[n]``.  ``acc``: an earlier result over OTHER points (or other
    launches' rows, laid side by side by the caller) to merge into."""
    t = np.asarray(tsurf, np.float64)
    n, nrows = t.shape
    group = np.asarray(group, np.int64)
    assert group.shape == (n,)
    edges = _checked(spec)
    th = spec.thresholds
    out = empty(nrows, spec)
    st = [np.asarray(s, np.float64) for s in (snow, water, ice, deposit, ice2)]
    for s in st:
        assert s.shape == t.shape
    keep = (group >= 0) & (group < int(spec.ngroups))
    if keep.any() and nrows:
        t, st, g = t[keep], [s[keep] for s in st], group[keep]
        at = (np.broadcast_to(np.arange(nrows)[None, :], t.shape), np.broadcast_to(g[:, None], t.shape))
        ok = t != INVALID
        live = ok & ~np.isnan(t)

        def count(col, mask):
            np.add.at(out[:, :, col], at, mask.astype(np.float64))
        count(COUNT, ok)
        np.minimum.at(out[:, :, TMIN], at, np.where(live, t, np.inf))
        np.maximum.at(out[:, :, TMAX], at, np.where(live, t, -np.inf))
        count(N_BELOW, ok & (t < float(th.tsurf_below)))
        for k, s in enumerate(st):
            count(STORAGE_COUNT + k, ok & (s > float(th.storage_above[k])))
            np.maximum.at(out[:, :, STORAGE_MAX + k], at, np.where(ok & ~np.isnan(s), s, -np.inf))
        if len(edges):
            j = np.searchsorted(edges, t, side="right")      # the number of edges <= Tsurf
            for b in range(len(edges) + 1):
                count(BINS + b, live & (j == b))
    return out if acc is None else merge(acc, out)
