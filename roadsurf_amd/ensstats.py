"""Per-station ensemble statistics of the six output series: the definition, in numpy.

What an ensemble consumer wants per station and row: the mean, the spread and a few percentiles of the members'
surface temperature, and the mean storages.  ``groups.py`` cannot give them - its columns are counts and extremes, so
that the device may use atomics - and a sum equals a definition bit for bit only if the members of a station are
visited in ONE fixed order and every operation is rounded on its own.  The order is ``member_table``: per station its
members in ascending point index.  ``reduce_members`` is the specification; the device reducer
(``rs_hip_outputs_ens``: include/roadsurf.h) is held to it exactly by the tests.  Columns of a cell::

    0        number of VALID members (valid iff Tsurf is not exactly -9999.0)
    1        k, the number of USED members (valid, and Tsurf not NaN); x_0 .. x_{k-1} their Tsurf in table order
    2        mean Tsurf  (((x_0 + x_1) + x_2) + ...) / k
    3        spread      sqrt(((d_0*d_0 + d_1*d_1) + ...) / k),  d_j = x_j - mean   (population form)
    4..8     mean of snow, water, ice, deposit, ice2 over the USED members, summed the same way; a NaN storage of a
             used member makes that one mean NaN and nothing else
    9 + j    quantile q_j of the used Tsurf sorted ascending to y: h = q_j * (k - 1), lo = floor(h),
             hi = min(lo + 1, k - 1), t = h - lo, the value y[lo] + t * (y[hi] - y[lo])

Every operation is one float64 operation, rounded on its own.  With k = 0 the columns 2 and above are -9999.0.  The
sums are explicit loops over the member position, vectorised over stations and rows; numpy's own mean, std and
quantile are not used: their summation order and interpolation are no contract.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import summary

RS_ENS_MAX_MEMBERS = 64
RS_ENS_MAX_QUANT = 8
RS_ENS_COLS = 9
INVALID = summary.INVALID
(N_VALID, N_USED, MEAN, SPREAD) = range(4)
STORAGE_MEAN, QUANT = 4, 9


@dataclasses.dataclass
class EnsSpec:
    """RsEnsSpec: the number of stations, the most members a station may have, and the quantiles of Tsurf."""
    ngroups: int = 1
    max_members: int = RS_ENS_MAX_MEMBERS
    quantiles: tuple = ()


def _checked(spec) -> np.ndarray:
    q = np.asarray(spec.quantiles, np.float64).reshape(-1)
    if int(spec.ngroups) < 1:
        raise ValueError("ngroups: at least one station")
    if not 1 <= int(spec.max_members) <= RS_ENS_MAX_MEMBERS:
        raise ValueError(f"max_members: 1 .. {RS_ENS_MAX_MEMBERS}")
    if len(q) > RS_ENS_MAX_QUANT:
        raise ValueError(f"quantiles: at most {RS_ENS_MAX_QUANT}")
    if np.isnan(q).any() or (q < 0).any() or (q > 1).any() or not (np.diff(q) > 0).all():
        raise ValueError("quantiles: in [0, 1], strictly increasing")
    return q


def cols(spec) -> int:
    """Numbers per cell: RS_ENS_COLS and one per quantile."""
    return RS_ENS_COLS + len(_checked(spec))


def table_ints(npoints: int, spec) -> int:
    _checked(spec)
    return int(spec.ngroups) + 1 + int(npoints)


def member_table(group, spec) -> np.ndarray:
    """int32 [ngroups + 1 + n]: ``start[0 .. ngroups]``, then the members of station 0, of station 1, ... - each
    station's in ascending point index -, the unused tail -1.  Station g's members are the entries ``start[g] ..
    start[g + 1] - 1`` of the list behind the starts.  ``group``: int32 [n] in point order, an id outside
    ``[0, ngroups)`` belongs to no station.  ValueError, naming the first such station, where one has more than
    ``max_members`` members."""
    _checked(spec)
    group = np.asarray(group, np.int64).reshape(-1)
    ng, n = int(spec.ngroups), len(group)
    keep = (group >= 0) & (group < ng)
    count = np.bincount(group[keep], minlength=ng)
    over = np.nonzero(count > int(spec.max_members))[0]
    if len(over):
        g = int(over[0])
        raise ValueError(f"member_table: station {g} has {int(count[g])} members, more than max_members = "
                         f"{int(spec.max_members)}")
    table = np.full(ng + 1 + n, -1, np.int32)
    table[0] = 0
    table[1:ng + 1] = np.cumsum(count)
    points = np.nonzero(keep)[0]
    members = points[np.argsort(group[points], kind="stable")]     # by station, ascending point index within one
    table[ng + 1:ng + 1 + len(members)] = members
    return table


def empty(nrows: int, spec) -> np.ndarray:
    """The cells of no members: [nrows, ngroups, cols]."""
    a = np.full((nrows, int(spec.ngroups), cols(spec)), INVALID)
    a[:, :, :MEAN] = 0.0
    return a


def _ordered_sum(v, k):
    """(((v_0 + v_1) + v_2) + ...) over the first k[...] positions of axis 0, one rounded addition at a time."""
    s = v[0].copy()
    for j in range(1, v.shape[0]):
        s = np.where(j < k, s + v[j], s)
    return s


def reduce_members(tsurf, snow, water, ice, deposit, ice2, group, spec) -> np.ndarray:
    """Cells float64 [nrows, ngroups, cols] of the series [n, nrows] (any float type; widened to float64, which is
    exact) of the points whose stations are ``group[n]``."""
    quant = _checked(spec)
    t = np.asarray(tsurf, np.float64)
    n, nrows = t.shape
    st = [np.asarray(s, np.float64) for s in (snow, water, ice, deposit, ice2)]
    for s in st:
        assert s.shape == t.shape
    ng = int(spec.ngroups)
    table = member_table(group, spec)
    start, members = table[:ng + 1].astype(np.int64), table[ng + 1:].astype(np.int64)
    count = np.diff(start)
    out = empty(nrows, spec)
    width = int(count.max()) if ng else 0
    if width == 0 or nrows == 0:
        return out
    # member position j of station g: its point, or none
    pos = np.arange(width)[:, None]                                  # [width, 1]
    there = pos < count[None, :]                                     # [width, ng]
    point = np.where(there, members[np.minimum(start[:-1][None, :] + pos, max(n - 1, 0))], 0)
    T = np.where(there[:, :, None], t[point], INVALID)               # [width, ng, nrows]
    valid = T != INVALID
    used = valid & ~np.isnan(T)
    k = used.sum(axis=0)                                             # [ng, nrows]
    rank = np.cumsum(used, axis=0) - 1                               # where a used member lands among the used

    def compact(V):
        """the used members' values to the front, in table order; what is behind them is never read"""
        X = np.zeros_like(V)
        gi, ri = np.meshgrid(np.arange(ng), np.arange(nrows), indexing="ij")
        for j in range(width):
            u = used[j]
            X[rank[j][u], gi[u], ri[u]] = V[j][u]
        return X

    some = k > 0
    kd = np.where(some, k, 1).astype(np.float64)
    X = compact(T)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = _ordered_sum(X, k) / kd
        D = X - mean[None]
        spread = np.sqrt(_ordered_sum(D * D, k) / kd)
        cells = [valid.sum(axis=0).astype(np.float64), k.astype(np.float64), mean, spread]
        for s in st:
            S = compact(np.where(there[:, :, None], s[point], 0.0))
            cells.append(_ordered_sum(S, k) / kd)
        if len(quant):
            Y = np.sort(np.where(pos[:, :, None] < k[None], X, np.inf), axis=0)   # (the used values hold no NaN)
            km1 = np.where(some, k - 1, 0)
            for q in quant:
                h = q * km1.astype(np.float64)
                lo = np.floor(h).astype(np.int64)
                hi = np.minimum(lo + 1, km1)
                tt = h - lo.astype(np.float64)
                ylo = np.take_along_axis(Y, lo[None], axis=0)[0]
                yhi = np.take_along_axis(Y, hi[None], axis=0)[0]
                cells.append(ylo + tt * (yhi - ylo))
    for c, v in enumerate(cells):
        out[:, :, c] = (v if c < MEAN else np.where(some, v, INVALID)).T
    return out
