"""CPU: the definition of the per-station probabilities of a condition over the ensemble members
(roadsurf_amd/ensprob.py) - against a plain triple loop written here, against the definitions the project already has
where they say the same thing, under cuts and re-orderings of the feed, and on the reference's own ensemble, where the
conditions a forecaster names must really split the members.  Every cell is a count: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import ensemble_helpers as eh
import ensprob_helpers as ph
from roadsurf_amd import ensemble, ensprob, episodes, groups, lib, summary

OUT = ph.OUT
NROWS = 33


def _holds(x, cond):
    """One row of one member, Python floats: the rule of episodes.holds said again, plainly."""
    if x[0] == -9999.0:
        return False
    for k in range(7):
        if cond.use >> k & 1 and not (cond.above[k] < x[k] and x[k] < cond.below[k]):   # (a NaN compares false)
            return False
    return not (cond.use >> 6 & 1 and x[6] == -9999.0)


def _loop_reference(d, group, spec, ever=None):
    """Cells and carry by a plain triple loop over stations, members and rows."""
    n, nrows = d["tsurf"].shape
    C_ = len(spec.conditions)
    cells = np.zeros((nrows, spec.ngroups, 1 + 2 * C_))
    ever = np.zeros(n, np.int32) if ever is None else ever.copy()
    for g in range(-1, spec.ngroups):                 # (-1: the points of no station, whose carry moves all the same)
        members = [p for p in range(n) if (group[p] == g if g >= 0 else not 0 <= group[p] < spec.ngroups)]
        for p in members:
            for r in range(nrows):
                x = [float(d[k][p, r]) for k in ph.SERIES]
                valid = x[0] != -9999.0
                if g >= 0 and valid:
                    cells[r, g, 0] += 1
                for c, cond in enumerate(spec.conditions):
                    if _holds(x, cond):
                        ever[p] |= 1 << c
                        if g >= 0:
                            cells[r, g, 1 + c] += 1
                    if g >= 0 and valid and ever[p] >> c & 1:
                        cells[r, g, 1 + C_ + c] += 1
    return cells, ever


@pytest.mark.parametrize("S,M", [(13, 5), (3, 64)], ids=["13x5", "3x64"])
def test_reduce_members_prob_equals_a_plain_triple_loop(S, M):
    n = S * M
    d = ph.made_series(n, NROWS, 7 * n)
    # what the series are there for
    assert (d["tsurf"] == 0.0).any() and (d["water"] == 0.125).any() and (d["tsurf"] == 2.0).any()   # on a bound
    assert np.isnan(d["tsurf"]).sum() == 1 and np.isnan(d["ice"]).any() and np.isnan(d["water"]).any()
    assert (d["tsurf"][n // 2] == -9999.0).all() and (d["tsurf"][0, -1] == -9999.0) and (d["deficit"] == -9999.0).any()
    for name, gid, ng, mm in ph.layouts(S, M, np.random.RandomState(n)):
        for nc in (1, 3, 8):
            spec = ensprob.ProbSpec(ng, mm, ph.conditions(nc))
            assert ensprob.cols(spec) == 1 + 2 * nc and ensprob.needs_deficit(spec) == (nc == 8)
            got, ever = ph.reduce(d, gid, spec)
            want, want_ever = _loop_reference(d, gid, spec)
            assert got.shape == (NROWS, ng, 1 + 2 * nc) and got.dtype == np.float64 and ever.dtype == np.int32
            assert np.array_equal(got, want), (name, nc, np.argwhere(got != want)[:5])
            assert np.array_equal(ever, want_ever), (name, nc)
            assert (got[:, :, 1:] <= got[:, :, :1]).all()                       # every count at or below column 0
            assert (got[:, :, 1 + nc:] >= got[:, :, 1:1 + nc]).all()        # held now is held by now
            if name != "parents":
                assert (got[:, ng - 1] == 0).all()                              # the station without members
            if name == "ids outside":
                assert ((gid < 0) | (gid >= ng)).sum() > 0
    # strictness: a value on the bound does not pass, and the NaN Tsurf is valid and holds under nothing
    one = ensprob.ProbSpec(n, 1, ph.conditions(1))
    got, _ = ph.reduce(d, np.arange(n), one)
    assert np.array_equal(got[:, :, 1].T, (d["tsurf"] < 0.0) & (d["tsurf"] != -9999.0))
    assert got[NROWS // 2, n - 1, 0] == 1 and got[NROWS // 2, n - 1, 1] == 0
    # fp32 series are widened exactly
    d32 = ph.made_series(n, NROWS, 7 * n, np.float32)
    spec = ensprob.ProbSpec(S, M, ph.conditions(8))
    a, ea = ph.reduce(d32, ensemble.parents(S, M), spec)
    b, eb = ph.reduce({k: v.astype(np.float64) for k, v in d32.items()}, ensemble.parents(S, M), spec)
    assert np.array_equal(a, b) and np.array_equal(ea, eb)


def test_a_cut_feed_equals_one_feed_and_a_reversed_one_does_not():
    S, M = 13, 5
    d = ph.made_series(S * M, NROWS, 3)
    gid = ensemble.parents(S, M)
    spec = ensprob.ProbSpec(S, M, ph.conditions(8))
    whole, ever = ph.reduce(d, gid, spec)
    parts, carry = [], None
    for lo, hi in ((0, 8), (8, 9), (9, NROWS)):
        cells, carry = ph.reduce(d, gid, spec, carry, slice(lo, hi))
        parts.append(cells)
    assert np.array_equal(np.concatenate(parts), whole) and np.array_equal(carry, ever)
    # the given carry is not changed, and an empty feed changes nothing
    before = ever.copy()
    cells, again = ph.reduce(d, gid, spec, ever, slice(0, 0))
    assert cells.shape == (0, S, 17) and np.array_equal(again, before) and np.array_equal(ever, before)
    # the same rows in reverse order: columns 0 and NOW are the rows' own, BY_NOW is the curve of the order fed
    back, back_ever = ph.reduce({k: v[:, ::-1] for k, v in d.items()}, gid, spec)
    assert np.array_equal(back[::-1, :, :9], whole[:, :, :9])
    assert not np.array_equal(back[::-1, :, 9:], whole[:, :, 9:])
    assert np.array_equal(back_ever, ever)                  # (what has held at some row does not depend on the order)
    # BY_NOW is monotone per member: with every member a station of its own, it never falls while the member is valid
    per, _ = ph.reduce(d, np.arange(S * M), ensprob.ProbSpec(S * M, 1, ph.conditions(8)))
    stay = np.flatnonzero((d["tsurf"] != -9999.0).all(axis=1))
    assert len(stay) > S and (np.diff(per[:, stay, 9:], axis=0) >= 0).all() and per[:, stay, 9:].any()
    assert np.array_equal(ensprob.empty(4, spec), np.zeros((4, S, 17)))


def test_now_is_the_group_series_and_the_episodes_rule():
    S, M = 13, 5
    n = S * M
    d = ph.made_series(n, NROWS, 11)
    name, gid, ng, mm = ph.layouts(S, M, np.random.RandomState(1))[2]
    for x in (0.0, 0.5, -1.0):
        spec = ensprob.ProbSpec(ng, mm, (ensprob.Condition.where(tsurf=(None, x)),))
        got, _ = ph.reduce(d, gid, spec)
        grp = groups.reduce_groups(*[d[k] for k in OUT], gid, groups.GroupSpec(summary.SummarySpec(tsurf_below=x), ng))
        assert np.array_equal(got[:, :, 0], grp[:, :, groups.COUNT])
        assert np.array_equal(got[:, :, 1], grp[:, :, groups.N_BELOW]) and got[:, :, 1].any()
    spec = ensprob.ProbSpec(ng, mm, ph.conditions(8))
    got, _ = ph.reduce(d, gid, spec)
    for c, cond in enumerate(spec.conditions):
        h = episodes.holds([d[k] for k in ph.SERIES], cond)
        want = np.stack([h[gid == g].sum(axis=0) for g in range(ng)], axis=1)
        assert np.array_equal(got[:, :, 1 + c], want) and want.any(), c
    # Condition.where is EpisodeSpec.where without what an episode keeps
    e = episodes.EpisodeSpec.where(tsurf=(None, 0.0), water=(0.05, None))
    w = ensprob.Condition.where(tsurf=(None, 0.0), water=(0.05, None))
    assert (w.use, w.above, w.below) == (e.use, e.above, e.below) == (5, w.above, w.below)
    # the probabilities: counts over column 0, NaN where no member is valid
    pr = ensprob.probabilities(got)
    assert pr.shape == got.shape[:2] + (16,)
    some = got[:, :, 0] > 0
    assert (~some).any() and np.isnan(pr[~some]).all() and not np.isnan(pr[some]).any()
    assert np.array_equal(pr[some], got[some][:, 1:] / got[some][:, :1]) and pr[some].max() <= 1.0


def test_the_forecast_conditions_split_the_members_of_the_reference_case():
    """The reference's own ensemble (70 stations x 5 members, 288 forecast rows): the three conditions must give
    mixed cells - some members under the condition, not all - and cells where BY_NOW is above NOW, or the comparison
    of the device against this definition (tests/test_hip_ensprob.py) would hold trivially."""
    c = eh.lean_case()
    o = eh.lean_oracle()
    rows = slice(c["B"], c["L"])
    spec = ensprob.ProbSpec(c["S"], c["M"], ph.FORECAST_CONDITIONS)
    cells, ever = ensprob.reduce_members_prob(*[o[k][:, rows] for k in OUT], None, c["parent"], spec)
    assert cells.shape == (288, 70, 7) and cells[:, :, 0].min() == 5
    for mixed, later in ph.non_vacuity(cells, spec, c["M"]):
        assert mixed >= 1000 and later >= 100, (mixed, later)
    assert (np.diff(cells[:, :, 4:], axis=0) >= 0).all()                 # nobody fails here: the curves are monotone
    assert np.array_equal(cells[-1, :, 4:], np.stack([[(ever[c["parent"] == g] >> k & 1).sum() for k in range(3)]
                                                      for g in range(70)]))


def test_every_bad_spec_is_refused_here_and_by_the_library():
    L = lib.load()
    assert hasattr(L, "rs_hip_prob_cols")                    # (missing: a failure, not a skip)
    assert {"rs_hip_prob_cols", "rs_hip_prob_needs_deficit", "rs_hip_prob_spec_bytes", "rs_hip_prob_work_ints",
            "rs_hip_prob_reset", "rs_hip_outputs_prob"} <= set(lib.EXPORTS)
    assert L.rs_hip_prob_spec_bytes() == C.sizeof(lib.RsProbSpec) == 16 + 8 * (8 + 14 * 8)
    assert (lib.RS_PROB_MAX_CONDS, ensprob.RS_PROB_MAX_CONDS, ensprob.RS_ENS_MAX_MEMBERS) == (8, 8, 64)
    assert L.rs_hip_prob_work_ints(None, 5) < 0
    ok = ph.conditions(3)
    for spec in (ensprob.ProbSpec(1, 1, ok[:1]), ensprob.ProbSpec(50000, 64, ph.conditions(8)),
                 ensprob.ProbSpec(70, 5, ok)):
        n = len(spec.conditions)
        assert lib.prob_cols(spec) == ensprob.cols(spec) == 1 + 2 * n
        assert L.rs_hip_prob_needs_deficit(C.byref(lib.prob_spec(spec))) == int(ensprob.needs_deficit(spec)) == (n == 8)
    Cn = ensprob.Condition
    nan = float("nan")
    bad = [ensprob.ProbSpec(0, 5, ok), ensprob.ProbSpec(-2, 5, ok), ensprob.ProbSpec(3, 0, ok),
           ensprob.ProbSpec(3, 65, ok), ensprob.ProbSpec(3, 5, ()), ensprob.ProbSpec(3, 5, ph.CONDITIONS + ok[:1]),
           ensprob.ProbSpec(3, 5, (Cn(0),)), ensprob.ProbSpec(3, 5, (Cn(-1),)), ensprob.ProbSpec(3, 5, (Cn(128),)),
           ensprob.ProbSpec(3, 5, ok[:2] + (Cn(1 << 7 | 1),)),
           ensprob.ProbSpec(3, 5, (Cn(1, (nan,) + (-np.inf,) * 6),)),
           ensprob.ProbSpec(3, 5, (ok[0], Cn(2, below=(np.inf,) * 6 + (nan,))))]
    for spec in bad:
        for f in (ensprob.check_spec, ensprob.cols, ensprob.needs_deficit, lambda s: ensprob.empty(3, s)):
            with pytest.raises(ValueError):
                f(spec)
        sp = lib.prob_spec(spec)
        assert L.rs_hip_prob_cols(C.byref(sp)) < 0 and L.rs_hip_prob_needs_deficit(C.byref(sp)) < 0, spec
        with pytest.raises(RuntimeError, match="bad spec"):
            lib.prob_cols(spec)
    assert L.rs_hip_prob_cols(None) < 0
    with pytest.raises(ValueError, match="seven bounds"):
        ensprob.check_spec(ensprob.ProbSpec(3, 5, (Cn(1, (0.0,) * 6),)))
    d = ph.made_series(10, 4, 1)
    with pytest.raises(ValueError, match="needs the deficit"):
        ensprob.reduce_members_prob(*[d[k] for k in OUT], None, np.zeros(10, np.int32),
                                    ensprob.ProbSpec(1, 64, ph.conditions(8)))
    with pytest.raises(ValueError, match="station 0 has 10 members"):
        ph.reduce(d, np.zeros(10, np.int32), ensprob.ProbSpec(1, 9, ok))


def test_runner_refuses_probs_before_any_device_work():
    c = eh.lean_case()
    args = (c["S"], c["L"], c["B"], c["settings"], [c["local"]] * c["S"], None)
    ok = ph.FORECAST_CONDITIONS
    ensemble.check(*args, c["parent"], probs=ensprob.ProbSpec(c["S"], c["M"], ok))
    with pytest.raises(ValueError, match="ngroups"):
        ensemble.check(*args, c["parent"], probs=ensprob.ProbSpec(c["S"] + 1, c["M"], ok))
    with pytest.raises(ValueError, match=f"station 0 has {c['M']} members, more than max_members = {c['M'] - 1}"):
        ensemble.check(*args, c["parent"], probs=ensprob.ProbSpec(c["S"], c["M"] - 1, ok))
    with pytest.raises(ValueError, match="deficit"):
        ensemble.check(*args, c["parent"], probs=ensprob.ProbSpec(c["S"], c["M"], ph.conditions(8)))
    with pytest.raises(ValueError, match="conditions: 1 .. 8"):
        ensemble.check(*args, c["parent"], probs=ensprob.ProbSpec(c["S"], c["M"], ()))
    crowded = c["parent"].copy()
    crowded[-1] = 4                          # station 4 gets a sixth member
    with pytest.raises(ValueError, match="station 4 has 6 members"):
        ensemble.check(*args, crowded, probs=ensprob.ProbSpec(c["S"], c["M"], ok))
    # ... and run_ensemble gets there before it asks for a device
    run = lambda **kw: ensemble.run_ensemble(c["stations"], c["tails"], c["B"], c["settings"], c["params"],  # noqa: E731
                                             c["local"], **kw)
    with pytest.raises(ValueError, match="station 4 has 6 members"):
        run(parent=crowded, probs=ensprob.ProbSpec(c["S"], c["M"], ok))
    with pytest.raises(ValueError, match="ngroups"):
        run(parent=c["parent"], probs=ensprob.ProbSpec(1, 64, ok))
    with pytest.raises(ValueError, match="deficit"):
        run(parent=c["parent"], probs=ensprob.ProbSpec(c["S"], c["M"], ph.conditions(8)))
