"""CPU: the definition of the per-group time series (roadsurf_amd/groups.py, reduce_groups) on hand-written rows
with known answers, and its merge rule: disjoint sets of points merged in any order give what one call gives.  The
device reducer is held to this definition by tests/test_hip_groups.py."""
import itertools

import numpy as np
import pytest

from roadsurf_amd import groups, summary

INF = np.inf
M = -9999.0
NAN = np.nan


def test_known_answers():
    th = summary.SummarySpec(tsurf_below=0.0, storage_above=(0.5, 0.0, 0.1, 0.0, 0.0))
    spec = groups.GroupSpec(th, ngroups=4, edges=(-1.0, 0.0, 2.0))
    assert groups.cols(spec) == groups.RS_GRP_COLS + 4 == 18
    #            row 0   row 1   row 2
    t = np.array([[-2.0, 0.0, 2.0],     # point 0, group 0: ties the minimum of point 1; equal to the threshold; to an edge
                  [-2.0, 3.0, 3.0],     # point 1, group 0: ... and the maximum of point 2 at row 1
                  [1.0, 3.0, NAN],      # point 2, group 0: a NaN Tsurf counts as valid and wins nothing
                  [5.0, -1.0, M],       # point 3, group 2: a failed point with a -9999.0 tail; -1.0 is an edge
                  [M, M, M],            # point 4, group 2: a rejected point
                  [7.0, 7.0, 7.0],      # point 5, id -1: no group
                  [8.0, 8.0, 8.0],      # point 6, id 4 = ngroups: no group
                  [-3.0, -3.0, -3.0]])  # point 7, group 3
    gid = np.array([0, 0, 0, 2, 2, -1, 4, 3], np.int32)   # group 1 is empty
    snow = np.array([[0.5, 0.6, 0.7], [0.5, NAN, 0.0], [0.0, 0.0, 0.0], [0.9, 0.0, 9.0], [9.0, 9.0, 9.0],
                     [9.0, 9.0, 9.0], [9.0, 9.0, 9.0], [0.0, 0.0, 0.0]])   # a NaN storage; storages behind -9999.0
    ice = np.array([[0.1, 0.2, 0.0], [0.0, 0.3, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0],
                    [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    z = np.zeros_like(t)
    got = groups.reduce_groups(t, snow, z, ice, z, z, gid, spec)
    assert got.shape == (3, 4, 18) and got.dtype == np.float64
    none = [0, INF, -INF, 0, 0, 0, 0, 0, 0, -INF, -INF, -INF, -INF, -INF, 0, 0, 0, 0]
    want = np.array([
        # n  min   max  below | counts snow water ice dep ice2 | max snow water ice dep ice2 | bins <-1, [-1,0), [0,2), >=2
        [[3, -2.0, 1.0, 2, 0, 0, 0, 0, 0, 0.5, 0.0, 0.1, 0.0, 0.0, 2, 0, 1, 0],
         none,
         [1, 5.0, 5.0, 0, 1, 0, 0, 0, 0, 0.9, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 1],
         [1, -3.0, -3.0, 1, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 1, 0, 0, 0]],
        [[3, 0.0, 3.0, 0, 1, 0, 2, 0, 0, 0.6, 0.0, 0.3, 0.0, 0.0, 0, 0, 1, 2],
         none,
         [1, -1.0, -1.0, 1, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 1, 0, 0],
         [1, -3.0, -3.0, 1, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 1, 0, 0, 0]],
        [[3, 2.0, 3.0, 0, 1, 0, 0, 0, 0, 0.7, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 2],
         none,
         none,
         [1, -3.0, -3.0, 1, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 1, 0, 0, 0]],
    ], np.float64)
    assert np.array_equal(got, want), np.argwhere(got != want)
    assert np.array_equal(groups.empty(1, spec)[0, 0], np.array(none, np.float64))
    # no edges: no bins, the other columns unchanged
    plain = groups.GroupSpec(th, ngroups=4)
    assert groups.cols(plain) == groups.RS_GRP_COLS
    assert np.array_equal(groups.reduce_groups(t, snow, z, ice, z, z, gid, plain), want[:, :, :groups.RS_GRP_COLS])


def test_bad_specs_are_refused():
    th = summary.SummarySpec()
    for bad in (groups.GroupSpec(th, 0), groups.GroupSpec(th, 2, tuple(range(32))), groups.GroupSpec(th, 2, (1.0, 1.0)),
                groups.GroupSpec(th, 2, (2.0, 1.0))):
        with pytest.raises(ValueError):
            groups.cols(bad)
    assert groups.cols(groups.GroupSpec(th, 2, tuple(range(31)))) == groups.RS_GRP_COLS + 32


def test_float32_series_widen_exactly():
    th = summary.SummarySpec(tsurf_below=np.float32(0.1), storage_above=(0.0,) * 5)  # the float's value as a double
    spec = groups.GroupSpec(th, 1, edges=(float(np.float32(0.2)),))
    t = np.array([[0.1], [0.2], [-9999.0]], np.float32)
    got = groups.reduce_groups(t, *[np.zeros((3, 1), np.float32)] * 5, np.zeros(3, np.int32), spec)
    assert got[0, 0, groups.COUNT] == 2 and got[0, 0, groups.N_BELOW] == 0
    assert got[0, 0, groups.TMIN] == float(np.float32(0.1)) != 0.1
    assert got[0, 0, groups.TMAX] == float(np.float32(0.2)) != 0.2
    assert list(got[0, 0, groups.BINS:]) == [1, 1]           # the float 0.2 equals the edge: the upper bin


def _made(n, nrows, seed):
    rs = np.random.RandomState(seed)
    vals = np.array([-2.0, -0.5, 0.0, 0.0, 0.5, 1.5])  # few values: ties and exact threshold and edge hits everywhere
    t = vals[rs.randint(0, len(vals), (n, nrows))]
    st = [np.array([0.0, 0.1, 0.1, 0.7])[rs.randint(0, 4, (n, nrows))] for _ in range(5)]
    for p in range(0, n, 5):
        t[p, rs.randint(0, nrows):] = M
    t[3] = M
    t[4, 11] = NAN
    st[1][6, 2] = NAN
    gid = rs.randint(-1, 6, n).astype(np.int32)          # -1 and 5 = ngroups among them
    gid[3] = gid[4] = 2                                  # the rejected point and the NaN are in a group
    return t, st, gid


def test_disjoint_point_sets_merge_in_any_order():
    n, nrows = 60, 13
    t, st, gid = _made(n, nrows, 5)
    spec = groups.GroupSpec(summary.SummarySpec(0.0, (0.1, 0.0, 0.1, 0.5, 0.1)), 5, edges=(-0.5, 0.0, 1.0))
    whole = groups.reduce_groups(t, *st, gid, spec)
    assert (gid == -1).any() and (gid == 5).any() and (whole[:, :, groups.N_BELOW] > 0).any()
    rs = np.random.RandomState(9)
    part = rs.randint(0, 3, n)
    for perm in itertools.permutations(range(3)):
        acc = None
        for k in perm:
            m = part == k
            acc = groups.reduce_groups(t[m], *[s[m] for s in st], gid[m], spec, acc=acc)
        assert np.array_equal(acc, whole), perm
    # no points at all: the empty cells, and merging them changes nothing
    none = groups.reduce_groups(t[:0], *[s[:0] for s in st], gid[:0], spec)
    assert np.array_equal(none, groups.empty(nrows, spec))
    assert np.array_equal(groups.merge(whole, none), whole) and np.array_equal(groups.merge(none, whole), whole)
    # a point fed twice is counted twice: documented, not detected
    twice = groups.reduce_groups(t, *st, gid, spec, acc=whole)
    counts = [groups.COUNT, groups.N_BELOW] + list(range(groups.STORAGE_COUNT, groups.STORAGE_COUNT + 5)) + \
        list(range(groups.BINS, groups.cols(spec)))
    extremes = [groups.TMIN, groups.TMAX] + list(range(groups.STORAGE_MAX, groups.STORAGE_MAX + 5))
    assert np.array_equal(twice[:, :, counts], 2 * whole[:, :, counts])
    assert np.array_equal(twice[:, :, extremes], whole[:, :, extremes])


def test_histogram_counts_every_valid_number_once():
    n, nrows = 60, 13
    t, st, gid = _made(n, nrows, 17)
    spec = groups.GroupSpec(summary.SummarySpec(), 5, edges=(-2.0, -0.5, 0.25, 1.5))
    got = groups.reduce_groups(t, *st, gid, spec)
    for g in range(5):
        m = gid == g
        valid = (t[m] != M).sum(axis=0)
        nans = np.isnan(t[m]).sum(axis=0)
        assert np.array_equal(got[:, g, groups.COUNT], valid)
        assert np.array_equal(got[:, g, groups.BINS:].sum(axis=1), valid - nans)
