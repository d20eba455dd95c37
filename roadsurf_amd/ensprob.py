"""Per-station probabilities of a road condition over the ensemble members: the definition, in numpy.

The number a road-weather ensemble is run for is the share of a station's members on which a condition holds -
"Tsurf below 0 and water on the road", "ice present", "dew-point deficit below 0" (hoar frost) - and whether it has
occurred by a given hour: the monotone curve a forecaster reads, "probability of ice by 06:00".  A CONDITION is the
condition of the per-point episodes (roadsurf_amd/episodes.py): a conjunction of strict bounds on the six outputs and
the dew-point deficit, and a row of a member HOLDS under it by ``episodes.holds`` - its Tsurf is not exactly -9999.0,
every used variable k passes ``above[k] < x < below[k]`` (a NaN compares false) and, if the deficit is used, the
deficit is not exactly -9999.0.  ``reduce_members_prob`` is the specification; the device reducer
(``rs_hip_outputs_prob``: include/roadsurf.h) is held to it exactly by the tests.

A station's members are given by ``ensstats.member_table``: an id outside ``[0, ngroups)`` belongs to no station.
The cell of station g and row r has ``cols = 1 + 2 * C`` float64 columns for C conditions::

    0            the number of VALID members at r (Tsurf not exactly -9999.0)
    1 + c        NOW: the number of members whose row r holds under condition c
    1 + C + c    BY_NOW: the number of members that are valid at r and for which condition c has held at r or at any
                 row fed earlier since the carry was reset

The test of validity at r keeps every count at or below column 0: a member that failed after the condition held leaves
numerator and denominator together.  Every cell is a count; ``probabilities`` divides.

The carry is one int32 per point, in POINT order: bit c set means that condition c has held at a fed row of the point.
An invalid row sets nothing.  Columns 0 and NOW do not depend on the order of feeding; BY_NOW does: rows fed in time
order and cut anywhere give the cells of one call, rows fed out of order give the curve of the order fed (documented,
not detected).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import ensstats, episodes

RS_PROB_MAX_CONDS = 8
RS_ENS_MAX_MEMBERS = ensstats.RS_ENS_MAX_MEMBERS
RS_EPI_VARS = episodes.RS_EPI_VARS
VARS = episodes.VARS
INVALID = episodes.INVALID
N_VALID, NOW = 0, 1


@dataclasses.dataclass
class Condition:
    """RsProbCond, the condition fields of episodes.EpisodeSpec: bit k of ``use`` tests variable k of ``VARS``
    against ``above[k] < x < below[k]``, both strict."""
    use: int = 1
    above: tuple = (-np.inf,) * RS_EPI_VARS
    below: tuple = (np.inf,) * RS_EPI_VARS

    @classmethod
    def where(cls, **bounds) -> "Condition":
        """``where(tsurf=(None, 0.0), water=(0.05, None))``: name -> (above, below), None = no bound."""
        e = episodes.EpisodeSpec.where(**bounds)
        return cls(e.use, e.above, e.below)


@dataclasses.dataclass
class ProbSpec:
    """RsProbSpec: the number of stations, the most members a station may have, and 1 .. RS_PROB_MAX_CONDS
    conditions."""
    ngroups: int = 1
    max_members: int = RS_ENS_MAX_MEMBERS
    conditions: tuple = ()


def check_spec(spec) -> None:
    """Raises ValueError for a spec the library refuses (rs_hip_prob_cols < 0)."""
    if int(spec.ngroups) < 1:
        raise ValueError("ngroups: at least one station")
    if not 1 <= int(spec.max_members) <= RS_ENS_MAX_MEMBERS:
        raise ValueError(f"max_members: 1 .. {RS_ENS_MAX_MEMBERS}")
    if not 1 <= len(spec.conditions) <= RS_PROB_MAX_CONDS:
        raise ValueError(f"conditions: 1 .. {RS_PROB_MAX_CONDS}")
    for c, cond in enumerate(spec.conditions):
        use = int(cond.use)
        if use <= 0 or use >> RS_EPI_VARS:
            raise ValueError(f"condition {c}: use: at least one of the bits 0..6, none above")
        if len(cond.above) != RS_EPI_VARS or len(cond.below) != RS_EPI_VARS:
            raise ValueError(f"condition {c}: above, below: seven bounds")
        if np.isnan(np.asarray(cond.above, np.float64)).any() or np.isnan(np.asarray(cond.below, np.float64)).any():
            raise ValueError(f"condition {c}: a bound is NaN")


def cols(spec) -> int:
    """Numbers per cell: the valid members, then NOW and BY_NOW per condition."""
    check_spec(spec)
    return 1 + 2 * len(spec.conditions)


def needs_deficit(spec) -> bool:
    """Whether the deficit rows must be given: some condition tests it."""
    check_spec(spec)
    return any(int(c.use) >> episodes.DEFICIT & 1 for c in spec.conditions)


def table_spec(spec) -> ensstats.EnsSpec:
    """The spec ``ensstats.member_table`` takes for the same stations: one table serves both reducers."""
    return ensstats.EnsSpec(int(spec.ngroups), int(spec.max_members))


def empty(nrows: int, spec) -> np.ndarray:
    """The cells of no members: zeros [nrows, ngroups, cols]."""
    return np.zeros((int(nrows), int(spec.ngroups), cols(spec)))


def reduce_members_prob(tsurf, snow, water, ice, deposit, ice2, deficit, group, spec, ever=None):
    """(cells float64 [nrows, ngroups, cols], carry int32 [n]) of the series [n, nrows] (any float type; widened to
    float64, which is exact) of the points whose stations are ``group[n]``.  ``deficit``: None where
    ``needs_deficit`` is false.  ``ever``: the carry int32 [n] of the rows fed before (None: none were); it is not
    changed, the carry behind these rows is returned."""
    C = len(spec.conditions)
    ncols = cols(spec)
    if needs_deficit(spec) and deficit is None:
        raise ValueError("this spec needs the deficit rows")
    series = [None if s is None else np.asarray(s, np.float64) for s in (tsurf, snow, water, ice, deposit, ice2, deficit)]
    t = series[0]
    n, nrows = t.shape
    assert all(s is None or s.shape == t.shape for s in series)
    group = np.asarray(group, np.int64).reshape(-1)
    assert group.shape == (n,)
    ng = int(spec.ngroups)
    ensstats.member_table(group, table_spec(spec))                    # (a station over max_members is refused)
    ever = np.zeros(n, np.int32) if ever is None else np.array(ever, np.int32).reshape(-1)
    assert ever.shape == (n,)
    member = (group >= 0) & (group < ng)
    gid = group[member]

    def per_station(mat):
        out = np.zeros((ng, nrows))
        np.add.at(out, gid, mat[member].astype(np.float64))
        return out.T

    valid = t != INVALID
    cells = np.zeros((nrows, ng, ncols))
    cells[:, :, N_VALID] = per_station(valid)
    for c, cond in enumerate(spec.conditions):
        h = episodes.holds(series, cond)                              # [n, nrows]
        held = (ever >> c & 1).astype(bool)[:, None] | (np.cumsum(h, axis=1) > 0)
        cells[:, :, NOW + c] = per_station(h)
        cells[:, :, NOW + C + c] = per_station(valid & held)
        if nrows:
            ever = ever | (held[:, -1].astype(np.int32) << c)
    return cells, ever


def probabilities(cells) -> np.ndarray:
    """The counts over column 0: float64 [..., cols - 1], NaN where no member is valid."""
    cells = np.asarray(cells, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cells[..., :1] > 0, cells[..., 1:] / cells[..., :1], np.nan)
