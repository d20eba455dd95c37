"""Per-point aggregates of the six output series over output periods: the definition, in numpy.

The model steps every 30 s; a consumer keeps a row an hour.  A kept row is a sample: it does not show how cold the
surface got within the hour, nor whether there was ice at any time in it.  A ``PeriodSpec`` cuts the time axis into
``nperiods`` periods of ``length`` indices - period ``w`` holds the absolute 1-based time indices
``first_index + w*length .. first_index + (w+1)*length - 1`` - and every point gets ``RS_PER_COLS`` numbers per
period, the aggregate of EVERY time step in it.  Rows outside ``[first_index, first_index + length*nperiods)`` belong
to no period and are ignored.

    With ``first_index = 2`` and ``length = step`` (the driver keeps the indices ``1, 1 + step, 1 + 2*step, ...``
    as its rows 0, 1, 2, ...), period ``w`` holds the indices ``2 + w*step .. 1 + (w+1)*step`` and so ENDS at the
    driver's kept row ``w + 1``: column 5 of period ``w`` is that kept row, columns 1 and 2 what happened since
    the kept row before it.

``reduce_series`` is the specification; the device reducer (``rs_hip_outputs_periods``: include/roadsurf.h) is held
to it bit for bit by the tests.  Columns of a cell::

    0        number of valid rows (a row is valid iff its Tsurf is not exactly -9999.0, as in summary.py)
    1, 2     min Tsurf, max Tsurf (+inf / -inf when there is no valid row)
    3        sum of Tsurf over the valid rows in ascending time index, ((x0 + x1) + x2) + ..., every addition rounded
             on its own (0.0 when there is none); ``mean`` is the one division by column 0
    4        number of rows with Tsurf < spec.tsurf_below
    5, 6     Tsurf of the valid row with the largest time index, and that index (-9999.0 and 0 when there is none):
             the sample, which beside min and max shows what sampling missed
    7..11    max of snow, water, ice, deposit, ice2 (-inf when there is none)
    12..16   number of rows with that storage > spec.storage_above[k]

Only valid rows count; every comparison is strict; NaN compares false everywhere and still counts as a valid row:
through a NaN row column 3 becomes NaN and column 5 may be NaN (compare with ``equal_nan=True``).

The feed contract.  Every column except 3 is independent of the order in which rows are fed (column 6 decides column
5).  Column 3 equals the definition when each period's rows are fed in ascending time order, each once, cut into
calls (``acc=``) anywhere.  Feeding out of order gives the sum in the order fed, feeding a row twice counts it twice:
documented, not detected - the contract of BY_NOW in ensprob.py.
"""
from __future__ import annotations

import dataclasses

import numpy as np

RS_PER_COLS = 17
INVALID = -9999.0  # OutputData.cpp:5-13: what rows the simulation never saved read
STORAGES = ("snow", "water", "ice", "deposit", "ice2")
(COUNT, TMIN, TMAX, TSUM, N_BELOW, LAST, LAST_INDEX) = range(7)
STORAGE_MAX, STORAGE_COUNT = 7, 12
INT32_MAX = 2**31 - 1


@dataclasses.dataclass
class PeriodSpec:
    """RsPeriodSpec: period w holds the time indices first_index + w*length .. first_index + (w+1)*length - 1,
    0 <= w < nperiods; the thresholds are those of summary.SummarySpec (Tsurf strictly below, storages strictly
    above)."""
    first_index: int
    length: int
    nperiods: int
    tsurf_below: float = 0.0
    storage_above: tuple = (0.0, 0.0, 0.0, 0.0, 0.0)


def check_spec(spec) -> None:
    """Raises ValueError for a spec the library refuses (rs_hip_period_check < 0)."""
    if int(spec.first_index) < 1:
        raise ValueError("first_index: a 1-based time index, at least 1")
    if int(spec.length) < 1:
        raise ValueError("length: at least one index per period")
    if int(spec.nperiods) < 1:
        raise ValueError("nperiods: at least one period")
    if int(spec.length) * int(spec.nperiods) > INT32_MAX:
        raise ValueError("length * nperiods: at most 2**31 - 1")
    above = np.asarray(spec.storage_above, np.float64)
    if above.shape != (5,):
        raise ValueError("storage_above: five thresholds (snow, water, ice, deposit, ice2)")
    if not (np.isfinite(float(spec.tsurf_below)) and np.isfinite(above).all()):
        raise ValueError("tsurf_below, storage_above: finite thresholds")


def period_of(index, spec) -> np.ndarray:
    """The period of every time index (int64, any shape), -1 where it belongs to none."""
    off = np.asarray(index, np.int64) - int(spec.first_index)
    inside = (off >= 0) & (off < int(spec.length) * int(spec.nperiods))
    return np.where(inside, off // int(spec.length), -1)


def empty(n: int, spec) -> np.ndarray:
    """The cells of no rows for n points: float64 [n, nperiods, RS_PER_COLS]."""
    check_spec(spec)
    a = np.zeros((n, int(spec.nperiods), RS_PER_COLS))
    a[..., TMIN] = np.inf
    a[..., TMAX] = -np.inf
    a[..., LAST] = INVALID
    a[..., STORAGE_MAX:STORAGE_MAX + 5] = -np.inf
    return a


def reduce_series(tsurf, snow, water, ice, deposit, ice2, index, spec, acc=None) -> np.ndarray:
    """Cells float64 [n, nperiods, RS_PER_COLS] of the series [n, nrows] (any float type; widened to float64, which
    is exact); ``index[r]`` is the absolute 1-based time index of row r; ``spec``: a PeriodSpec.  ``acc``: an earlier
    result over EARLIER rows of the same points, which these rows continue (it is not changed).  The rows are
    taken one by one in the order given - that is the order of the additions of column 3."""
    check_spec(spec)
    t = np.asarray(tsurf, np.float64)
    n, nrows = t.shape
    sto = [np.asarray(s, np.float64) for s in (snow, water, ice, deposit, ice2)]
    assert all(s.shape == t.shape for s in sto)
    index = np.asarray(index, np.int64)
    assert index.shape == (nrows,)
    out = empty(n, spec) if acc is None else np.array(acc, np.float64)
    assert out.shape == (n, int(spec.nperiods), RS_PER_COLS)
    below, above = float(spec.tsurf_below), [float(x) for x in spec.storage_above]
    period = period_of(index, spec)
    for r in range(nrows):
        w = int(period[r])
        if w < 0:
            continue
        cell = out[:, w, :]                      # (a view: [n, RS_PER_COLS])
        x = t[:, r]
        ok = x != INVALID
        first = ok & (cell[:, COUNT] == 0)       # the first valid row IS the sum, not 0.0 + it
        with np.errstate(invalid="ignore"):
            cell[:, TSUM] = np.where(first, x, np.where(ok, cell[:, TSUM] + x, cell[:, TSUM]))
        cell[:, COUNT] += ok
        cell[:, TMIN] = np.where(ok & (x < cell[:, TMIN]), x, cell[:, TMIN])
        cell[:, TMAX] = np.where(ok & (x > cell[:, TMAX]), x, cell[:, TMAX])
        cell[:, N_BELOW] += ok & (x < below)
        later = ok & (float(index[r]) > cell[:, LAST_INDEX])
        cell[:, LAST] = np.where(later, x, cell[:, LAST])
        cell[:, LAST_INDEX] = np.where(later, float(index[r]), cell[:, LAST_INDEX])
        for k, s in enumerate(sto):
            y = s[:, r]
            c = STORAGE_MAX + k
            cell[:, c] = np.where(ok & (y > cell[:, c]), y, cell[:, c])
            cell[:, STORAGE_COUNT + k] += ok & (y > above[k])
    return out


def mean(cells) -> np.ndarray:
    """Mean Tsurf of every cell, column 3 over column 0: float64 [...], NaN where a period has no valid row."""
    cells = np.asarray(cells, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cells[..., COUNT] > 0, cells[..., TSUM] / cells[..., COUNT], np.nan)
