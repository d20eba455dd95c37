"""CPU: the definition of the per-point forecast summaries (roadsurf_amd/summary.py, reduce_series) on hand-written
rows with known answers, and its merge rule: disjoint row ranges fed in any order give what one call gives.  The
device reducer is held to this definition by tests/test_hip_summary.py."""
import itertools

import numpy as np

from roadsurf_amd import summary

INF = np.inf
M = -9999.0


def _series(t, snow=None, water=None, ice=None, deposit=None, ice2=None):
    t = np.asarray(t, np.float64)
    z = np.zeros_like(t)
    return [t] + [z if s is None else np.asarray(s, np.float64) for s in (snow, water, ice, deposit, ice2)]


def test_known_answers():
    spec = summary.SummarySpec(tsurf_below=0.0, storage_above=(0.5, 0.0, 0.1, 0.0, 0.0))
    index = np.array([7, 127, 247, 367, 487])
    t = [[1.0, -2.0, 3.0, -2.0, 3.0],      # equal minima at 127 and 367, equal maxima at 247 and 487
         [0.0, 0.0, 0.0, 0.0, 0.0],        # equal to the threshold everywhere: never below
         [2.0, -1.0, M, M, M],             # a failed point: two saved rows, then the -9999.0 tail
         [M, M, M, M, M],                  # a rejected point
         [np.nan, -3.0, 4.0, np.nan, M]]   # NaN: a valid row that wins nothing
    snow = [[0.5, 0.6, 0.5, 0.7, 0.0],     # equal to its threshold three times: two rows above
            [0.0] * 5,
            [0.0, 0.9, 5.0, 5.0, 5.0],     # storages behind the last saved row do not count
            [9.0] * 5,
            [np.nan, 1.0, 0.2, 0.6, 7.0]]
    ice = [[0.0, 0.1, 0.2, 0.1, 0.3], [0.0] * 5, [0.3, 0.0, 1.0, 1.0, 1.0], [1.0] * 5, [0.0] * 5]
    got = summary.reduce_series(*_series(t, snow=snow, ice=ice), index, spec)
    assert got.shape == (5, summary.RS_SUM_COLS) and got.dtype == np.float64
    want = np.array([
        # n  min  at   max  at  first nbelow  max snow water ice dep ice2   counts
        [5, -2.0, 127, 3.0, 247, 127, 2, 0.7, 0.0, 0.3, 0.0, 0.0, 2, 0, 2, 0, 0],
        [5, 0.0, 7, 0.0, 7, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0],
        [2, -1.0, 127, 2.0, 7, 127, 1, 0.9, 0.0, 0.3, 0.0, 0.0, 1, 0, 1, 0, 0],
        [0, INF, 0, -INF, 0, 0, 0, -INF, -INF, -INF, -INF, -INF, 0, 0, 0, 0, 0],
        [4, -3.0, 127, 4.0, 247, 127, 1, 1.0, 0.0, 0.0, 0.0, 0.0, 2, 0, 0, 0, 0],
    ])
    assert np.array_equal(got, want), np.argwhere(got != want)
    assert np.array_equal(summary.empty(1)[0], want[3])


def test_float32_series_widen_exactly():
    spec = summary.SummarySpec(tsurf_below=np.float32(0.1), storage_above=(0.0,) * 5)  # the float's value as a double
    t = np.array([[0.1, 0.2, -9999.0]], np.float32)
    got = summary.reduce_series(t, *[np.zeros((1, 3), np.float32)] * 5, np.array([1, 2, 3]), spec)
    assert got[0, summary.COUNT] == 2 and got[0, summary.N_BELOW] == 0
    assert got[0, summary.TMIN] == float(np.float32(0.1)) != 0.1


def test_disjoint_row_ranges_merge_in_any_order():
    rs = np.random.RandomState(5)
    n, nrows = 40, 37
    vals = np.array([-2.0, -0.5, 0.0, 0.0, 0.5, 1.5])  # few values: ties and exact threshold hits everywhere
    t = vals[rs.randint(0, len(vals), (n, nrows))]
    st = [np.array([0.0, 0.1, 0.1, 0.7])[rs.randint(0, 4, (n, nrows))] for _ in range(5)]
    for p in range(0, n, 5):
        t[p, rs.randint(0, nrows):] = M
    t[3] = M
    t[4, 11] = np.nan
    index = 7 + 120 * np.arange(nrows)
    spec = summary.SummarySpec(0.0, (0.1, 0.0, 0.1, 0.5, 0.1))
    whole = summary.reduce_series(t, *st, index, spec)
    assert whole[3, 0] == 0 and (whole[:, summary.FIRST_BELOW] > 0).any() and (whole[:, summary.FIRST_BELOW] == 0).any()
    cuts = [(0, 9), (9, 10), (10, nrows)]
    for perm in itertools.permutations(range(3)):
        acc = None
        for k in perm:
            a, b = cuts[k]
            acc = summary.reduce_series(t[:, a:b], *[s[:, a:b] for s in st], index[a:b], spec, acc=acc)
        assert np.array_equal(acc, whole), perm
    # no rows at all: the empty summary, and merging it changes nothing
    none = summary.reduce_series(t[:, :0], *[s[:, :0] for s in st], index[:0], spec)
    assert np.array_equal(none, summary.empty(n))
    assert np.array_equal(summary.merge(whole, none), whole) and np.array_equal(summary.merge(none, whole), whole)
    # a row fed twice is counted twice: documented, not detected
    twice = summary.reduce_series(t, *st, index, spec, acc=whole)
    assert np.array_equal(twice[:, summary.COUNT], 2 * whole[:, summary.COUNT])
    assert np.array_equal(twice[:, 1:6], whole[:, 1:6])
