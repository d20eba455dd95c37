"""CPU: the definition of the per-point threshold episodes (roadsurf_amd/episodes.py) against a plain per-point loop
over the reference's own fixtures and over made series, the order-dependent properties of the automaton (split
feeding, index jumps, min_rows over a cut, finish), every refusal of a spec - in numpy and in the library, whose
rs_hip_episode_cols needs no device - and the ctypes binding of RsEpisodeSpec against the C header."""
import ctypes as C
import dataclasses
import math
import os
import subprocess

import numpy as np
import pytest

from roadsurf_amd import episodes, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = ("tsurf", "snow", "water", "ice", "deposit", "ice2")
INF = math.inf


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _brute(series, index0, index_step, spec):
    """Whole series by a plain loop that knows nothing of accumulators: mark the rows that hold, cut them into
    maximal runs, drop the short ones, describe the others."""
    x = [None if s is None else np.asarray(s, np.float64) for s in series]
    x += [None] * (7 - len(x))
    n, nrows = x[0].shape
    K = spec.max_episodes
    acc = np.zeros((n, 10 + 6 * K))
    for p in range(n):
        runs, cur = [], []
        for r in range(nrows):
            ok = float(x[0][p, r]) != -9999.0
            for k in range(7):
                if spec.use >> k & 1:
                    v = float(x[k][p, r])
                    ok = ok and spec.above[k] < v and v < spec.below[k]
            if spec.use >> 6 & 1:
                ok = ok and float(x[6][p, r]) != -9999.0
            if ok:
                cur.append(r)
            elif cur:
                runs.append(cur)
                cur = []
        if cur:
            runs.append(cur)
        runs = [q for q in runs if len(q) >= spec.min_rows]
        acc[p, 0] = len(runs)
        acc[p, 1] = sum(len(q) for q in runs)
        acc[p, 2] = max([len(q) for q in runs], default=0)
        recs = [(0.0, 0.0, 0.0, INF, 0.0, -INF)] * (K + 1)  # [0]: the open run of a finished accumulator
        for j, q in enumerate(runs[:K]):
            tmin, tmin_i, peak = INF, 0.0, -INF
            for r in q:
                t, pk = float(x[0][p, r]), float(x[spec.peak][p, r])
                if t < tmin:
                    tmin, tmin_i = t, float(index0 + r * index_step)
                if pk > peak:
                    peak = pk
            recs[j + 1] = (float(index0 + q[0] * index_step), float(index0 + q[-1] * index_step), float(len(q)), tmin,
                           tmin_i, peak)
        acc[p, 4:] = np.asarray(recs).ravel()
    return acc


def _reduce(series, index0, index_step, spec):
    s = list(series) + [None] * (7 - len(series))
    return episodes.reduce_series(*s, index0, index_step, spec)


def test_the_operational_fixture_against_brute_force():
    """The reference's operational run, 401 stations x 32 kept rows, Tsurf < 0: for more than half of the stations
    the surface is below freezing in several separate intervals."""
    z = np.load(os.path.join(GOLDEN, "e2e_operational.npz"))
    index0, step = 19, 40   # the fixture keeps 32 selected rows: consecutive rows here, at made indices
    spec = episodes.EpisodeSpec.where(tsurf=(None, 0.0), peak="water")
    for kind in ("files", "sky"):
        series = [z[f"{kind}_{k}"] for k in OUT]
        got = _reduce(series, index0, step, spec)
        assert _same_bits(got, _brute(series, index0, step, spec)), kind
        n_epi = got[:, episodes.COMMITTED].astype(int)
        assert (n_epi == 0).any() and (n_epi == 1).any() and (n_epi >= 3).any()
        invalid = (series[0] == -9999.0).all(axis=1)
        assert _same_bits(got[invalid], episodes.empty(int(invalid.sum()), spec))
        if kind == "files":
            assert np.bincount(n_epi, minlength=5).tolist() == [58, 115, 88, 68, 72]
            assert int(invalid.sum()) == 13
        two = dataclasses.replace(spec, max_episodes=2)
        got2 = _reduce(series, index0, step, two)
        assert _same_bits(got2, _brute(series, index0, step, two))
        assert int((got2[:, episodes.COMMITTED] > 2).sum()) >= 100
        assert _same_bits(got2[:, :22], got[:, :22])  # what is kept of the first two does not depend on K
        count, rec = episodes.decode(got2, two)
        assert count.max() == 2 and (rec["rows"][count == 2] > 0).all() and (rec["rows"][count == 0] == 0).all()
        assert (rec["last"] - rec["first"] == (rec["rows"] - 1) * step)[rec["rows"] > 0].all()


def test_the_scenarios_fixture_against_brute_force():
    z = np.load(os.path.join(GOLDEN, "e2e_scenarios.npz"))
    series = [z[f"out_{k}"] for k in OUT]
    index = z["out_index"]
    step = int(index[1] - index[0])
    assert (np.diff(index) == step).all()
    for min_rows in (1, 3):
        spec = episodes.EpisodeSpec.where(ice=(0.0, None), peak="ice", min_rows=min_rows)
        got = _reduce(series, int(index[0]) + 1, step, spec)   # (the fixture's indices are 0-based)
        assert _same_bits(got, _brute(series, int(index[0]) + 1, step, spec))
    assert (got[:, episodes.COMMITTED] > 0).any() and (got[:, episodes.COMMITTED] == 0).any()


def _made(n=23, nrows=41, seed=4):
    """Few values, exactly on the bounds among them; NaN in used and unused variables; -9999.0 rows in the middle;
    deficits that are -9999.0."""
    rs = np.random.RandomState(seed)
    t = np.array([-2.0, -0.5, 0.0, 0.0, 0.5, -1.0])[rs.randint(0, 6, (n, nrows))]
    s = [np.array([0.0, 0.05, 0.125, 0.75])[rs.randint(0, 4, (n, nrows))] for _ in range(5)]
    d = np.array([-1.5, -0.25, 0.0, 0.25, -9999.0])[rs.randint(0, 5, (n, nrows))]
    t[rs.rand(n, nrows) < 0.05] = -9999.0
    t[3, 10:14] = -9999.0
    t[rs.rand(n, nrows) < 0.03] = np.nan
    t[5] = -9999.0
    s[1][rs.rand(n, nrows) < 0.05] = np.nan   # water
    s[4][rs.rand(n, nrows) < 0.05] = np.nan   # ice2
    d[rs.rand(n, nrows) < 0.03] = np.nan
    t[7] = -1.0                                # one run over everything
    s[1][7] = 0.125
    d[7] = -0.25
    return [t] + s + [d]


MADE_SPECS = [
    episodes.EpisodeSpec.where(tsurf=(None, 0.0)),
    episodes.EpisodeSpec.where(tsurf=(None, 0.0), water=(0.05, None), peak="water", max_episodes=3),
    episodes.EpisodeSpec.where(tsurf=(None, 0.0), deficit=(None, 0.0), peak="deficit", min_rows=2),
    episodes.EpisodeSpec.where(snow=(0.05, 0.75), peak="deficit", max_episodes=1),  # Tsurf unused: a NaN Tsurf row holds
    episodes.EpisodeSpec.where(tsurf=(-2.0, 0.5), ice2=(-INF, INF), peak="ice2", min_rows=3, max_episodes=8),
    episodes.EpisodeSpec.where(deficit=(-0.25, None), peak="tsurf"),
]


@pytest.mark.parametrize("k", range(len(MADE_SPECS)))
def test_made_series_against_brute_force(k):
    spec, series = MADE_SPECS[k], _made()
    got = _reduce(series, 7, 3, spec)
    assert _same_bits(got, _brute(series, 7, 3, spec))
    assert (got[:, 0] >= 2).any() and (got[:, 0] == 0).any()
    assert _same_bits(got[5], episodes.empty(1, spec)[0])
    # float32 series are widened exactly
    s32 = [a.astype(np.float32) for a in series]
    assert _same_bits(_reduce(s32, 7, 3, spec), _reduce([a.astype(np.float64) for a in s32], 7, 3, spec))


def test_values_exactly_on_a_bound_and_special_values():
    spec = episodes.EpisodeSpec.where(tsurf=(-1.0, 0.0), peak="snow")
    t = np.array([[-1.0, np.nextafter(-1.0, 0.0), -0.5, np.nextafter(0.0, -1.0), 0.0, -0.0, np.nan, -0.5, -9999.0, -0.5]])
    snow = np.array([[9.0, 1.0, np.nan, -9999.0, 9.0, 9.0, 9.0, np.nan, 9.0, -INF]])
    zero = np.zeros_like(t)
    got = _reduce([t, snow, zero, zero, zero, zero], 1, 1, spec)
    count, rec = episodes.decode(got, spec)
    assert count[0] == 3 and got[0, :4].tolist() == [3.0, 5.0, 3.0, 0.0]
    # rows 1..3 (indices 2..4): the bounds themselves are outside; a NaN peak never wins, -9999.0 is a number here
    assert rec[0, 0].tolist() == (2, 4, 3, np.nextafter(-1.0, 0.0), 2, 1.0)
    assert rec[0, 1].tolist() == (8, 8, 1, -0.5, 8, -INF)   # its only peak value is NaN
    assert rec[0, 2].tolist() == (10, 10, 1, -0.5, 10, -INF)
    # equal minima: the smallest index
    t2 = np.array([[-0.5, -0.75, -0.75, -0.5]])
    z2 = np.zeros_like(t2)
    assert episodes.decode(_reduce([t2, z2, z2, z2, z2, z2], 5, 5, spec), spec)[1][0, 0]["tsurf_min_index"] == 10
    # the deficit -9999.0 fails a used deficit even inside the bounds, and is a number for an unused peak
    d = np.array([[-9999.0, -9999.0, 0.5, -9999.0]])
    wide = episodes.EpisodeSpec.where(deficit=(-INF, INF))
    assert _reduce([t2, z2, z2, z2, z2, z2, d], 1, 1, wide)[0, :3].tolist() == [1.0, 1.0, 1.0]
    pk = episodes.EpisodeSpec.where(tsurf=(None, 0.0), peak="deficit")
    assert _reduce([t2, z2, z2, z2, z2, z2, d[:, [0, 1, 1, 3]]], 1, 1, pk)[0, 10 + episodes.PEAK] == -9999.0


@pytest.mark.parametrize("k", [1, 2, 4])
def test_split_feeding_gives_the_same_accumulator(k):
    spec, series = MADE_SPECS[k], _made()
    n, nrows = series[0].shape
    whole = episodes.feed(episodes.empty(n, spec), series, 7, 3, spec)
    assert (whole[:, episodes.OPEN + episodes.ROWS] > 0).any()   # unfinished: open runs are compared too
    one = episodes.empty(n, spec)
    for r in range(nrows):
        episodes.feed(one, [a[:, r:r + 1] for a in series], 7 + 3 * r, 3, spec)
    assert _same_bits(one, whole)
    for cut in range(nrows + 1):
        acc = episodes.empty(n, spec)
        for lo, hi in ((0, cut), (cut, nrows)):
            if hi > lo:
                episodes.feed(acc, [a[:, lo:hi] for a in series], 7 + 3 * lo, 3, spec)
        assert _same_bits(acc, whole), cut
    assert _same_bits(episodes.finish(one, spec), _reduce(series, 7, 3, spec))


def test_an_unexpected_index_closes_the_open_run():
    spec = episodes.EpisodeSpec.where(tsurf=(None, 0.0))
    t = np.full((1, 6), -1.0)
    z = np.zeros_like(t)
    s = [t, z, z, z, z, z]
    acc = episodes.empty(1, spec)
    episodes.feed(acc, [a[:, :3] for a in s], 1, 2, spec)
    assert acc[0, :4].tolist() == [0.0, 0.0, 0.0, 7.0] and acc[0, 4:7].tolist() == [1.0, 5.0, 3.0]
    episodes.feed(acc, [a[:, 3:] for a in s], 9, 2, spec)   # 9, not 7: a gap
    episodes.finish(acc, spec)
    count, rec = episodes.decode(acc, spec)
    assert count[0] == 2 and rec[0, 0].tolist()[:3] == (1, 5, 3) and rec[0, 1].tolist()[:3] == (9, 13, 3)
    # ... and the expected index continues it
    acc = episodes.empty(1, spec)
    episodes.feed(acc, [a[:, :3] for a in s], 1, 2, spec)
    episodes.feed(acc, [a[:, 3:] for a in s], 7, 2, spec)
    assert episodes.decode(episodes.finish(acc, spec), spec)[1][0, 0].tolist()[:3] == (1, 11, 6)
    # another step size is another index too; an index that goes back as well
    acc = episodes.empty(1, spec)
    episodes.feed(acc, [a[:, :3] for a in s], 1, 2, spec)
    episodes.feed(acc, [a[:, 3:] for a in s], 3, 2, spec)
    assert episodes.finish(acc, spec)[0, :3].tolist() == [2.0, 6.0, 3.0]
    with pytest.raises(ValueError):
        episodes.feed(acc, s, 0, 1, spec)
    with pytest.raises(ValueError):
        episodes.feed(acc, s, 1, 0, spec)


def test_min_rows_drops_short_runs_also_over_a_cut():
    spec = episodes.EpisodeSpec.where(tsurf=(None, 0.0), min_rows=3)
    #                 a run of 2   a run of 3 over the cut      a run of 1
    t = np.array([[-1.0, -1.0, 1.0, -1.0, -2.0, -1.0, 1.0, -1.0]])
    z = np.zeros_like(t)
    s = [t, z, z, z, z, z]
    acc = episodes.empty(1, spec)
    episodes.feed(acc, [a[:, :5] for a in s], 1, 1, spec)
    assert acc[0, 0] == 0.0 and acc[0, episodes.OPEN + episodes.ROWS] == 2.0   # too short alone
    episodes.feed(acc, [a[:, 5:] for a in s], 6, 1, spec)
    episodes.finish(acc, spec)
    assert acc[0, :4].tolist() == [1.0, 3.0, 3.0, 0.0]
    assert episodes.decode(acc, spec)[1][0, 0].tolist() == (4, 6, 3, -2.0, 5, -1.0)   # the peak variable is Tsurf itself
    assert _same_bits(acc, _reduce(s, 1, 1, spec)) and _same_bits(acc, _brute(s, 1, 1, spec))
    # fed apart with a gap the halves are two short runs
    acc = episodes.empty(1, spec)
    episodes.feed(acc, [a[:, :5] for a in s], 1, 1, spec)
    episodes.feed(acc, [a[:, 5:] for a in s], 16, 1, spec)
    assert _same_bits(episodes.finish(acc, spec), episodes.empty(1, spec))


def test_finish_is_idempotent():
    spec, series = MADE_SPECS[1], _made()
    acc = episodes.feed(episodes.empty(series[0].shape[0], spec), series, 1, 1, spec)
    once = episodes.finish(acc.copy(), spec)
    assert not _same_bits(once, acc)
    assert _same_bits(episodes.finish(once.copy(), spec), once)
    assert (once[:, episodes.EXPECT] == 0).all() and _same_bits(once[:, 4:10], episodes.empty(len(once), spec)[:, 4:10])
    assert _same_bits(episodes.reset(once, spec), episodes.empty(len(once), spec))


GOOD = dict(use=0b1000001, above=(-INF,) * 7, below=(0.0,) + (INF,) * 6, peak=6, min_rows=1, max_episodes=8)
REFUSED = [
    dict(use=0), dict(use=1 << 7), dict(use=0x81), dict(use=-1),
    dict(above=(np.nan,) + (-INF,) * 6), dict(below=(INF,) * 6 + (np.nan,)), dict(above=(-INF,) * 3 + (np.nan,) + (-INF,) * 3),
    dict(peak=-1), dict(peak=7), dict(min_rows=0), dict(min_rows=-3), dict(max_episodes=0), dict(max_episodes=9),
]


@pytest.mark.parametrize("bad", REFUSED)
def test_every_refusal_of_a_spec(bad, hip_lib):
    good = episodes.EpisodeSpec(**GOOD)
    episodes.check_spec(good)
    assert episodes.cols(good) == 58 == lib.episode_cols(good)
    assert hip_lib.rs_hip_episode_cols(C.byref(lib.episode_spec(good))) == 58
    spec = episodes.EpisodeSpec(**dict(GOOD, **bad))
    with pytest.raises(ValueError):
        episodes.check_spec(spec)
    with pytest.raises(ValueError):
        episodes.empty(1, spec)
    assert hip_lib.rs_hip_episode_cols(C.byref(lib.episode_spec(spec))) < 0
    with pytest.raises(RuntimeError):
        lib.episode_cols(spec)
    assert hip_lib.rs_hip_episode_cols(None) < 0


def test_cols_and_the_deficit_rule():
    for K in range(1, 9):
        spec = episodes.EpisodeSpec(**dict(GOOD, max_episodes=K))
        assert episodes.cols(spec) == 10 + 6 * K == lib.episode_cols(spec)
    assert episodes.needs_deficit(episodes.EpisodeSpec(**GOOD))
    assert episodes.needs_deficit(episodes.EpisodeSpec.where(tsurf=(None, 0.0), peak="deficit"))
    assert not episodes.needs_deficit(episodes.EpisodeSpec.where(tsurf=(None, 0.0), peak="ice2"))
    with pytest.raises(ValueError):
        t = np.zeros((1, 2))
        _reduce([t] * 6, 1, 1, episodes.EpisodeSpec(**GOOD))


def test_struct_layout_against_the_header(tmp_path):
    """sizeof / offsetof of RsEpisodeSpec as a C compiler sees include/roadsurf.h = the ctypes binding's"""
    src = tmp_path / "episode_layout.c"
    members = ("use", "peak", "min_rows", "max_episodes", "above", "below")
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n"
        f'#include "{ROOT}/include/roadsurf.h"\n'
        "int main(void) {\n"
        '  printf("%zu %d %d %d %d", sizeof(RsEpisodeSpec), RS_EPI_VARS, RS_EPI_MAX, RS_EPI_HEAD, RS_EPI_REC);\n'
        + "".join(f'  printf(" %zu", offsetof(RsEpisodeSpec, {m}));\n' for m in members)
        + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "episode_layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = lib.RsEpisodeSpec
    assert out[0] == C.sizeof(S) == 16 + 2 * 7 * 8
    assert out[1:5] == [episodes.RS_EPI_VARS, episodes.RS_EPI_MAX, episodes.RS_EPI_HEAD, episodes.RS_EPI_REC]
    assert out[1:5] == [lib.RS_EPI_VARS, lib.RS_EPI_MAX, lib.RS_EPI_HEAD, lib.RS_EPI_REC]
    assert out[5:] == [getattr(S, m).offset for m in members]
