"""The knot-reading two-wavefront step kernels carry their time bookkeeping from index to index - the knot
interval and the position in it, the hour of the interval and its day/night verdict, the output row - and take
one division per launch.  A carried counter goes wrong at a launch's first index, where an interval ends, at
midnight and where night begins or ends: every case here runs one block of caller-made knots twice over the same
launches, through rs_hip_step_knots and through rs_hip_expand_forcing_ordered + rs_hip_step - whose windows come from
expand_kernel with an hour row made on the host, index by index, by rs_sy_hour - and asks for the same bits.  One
case is held to the CPU reference as well.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import golden_helpers as gh
import knot_helpers as kh
import oracle_helpers as oh
from roadsurf_amd import abi, synth

pytestmark = pytest.mark.gpu
OUT = oh.F64_OUT
N = 70  # one full wavefront and six lanes
NIGHT_ON, NIGHT_OFF = 19, 4  # abi.default_parameters(): the hours forcing_prep compares with

# steps per knot -> (knot intervals, launch lists).  SimLen = intervals * spk + 1: the last index is a knot of its own.
# Fifty (twenty-six) hours from any start hour cross midnight, NightOn and NightOff.
CASES = {
    1: (50, [[1, 1, 2, 5, 1, 13, 7, 1, 19, 1], [51], [3] * 17]),
    7: (50, [[1, 6, 7, 8, 13, 1, 20, 6, 1, 1, 1, 40, 100, 145, 1], [351], [7] * 50 + [1], [6] * 58 + [3]]),
    120: (26, [[120, 1, 1, 117, 1, 121, 119, 60, 60, 240, 7, 600, 1, 239, 1, 1200, 232, 1], [3121]]),
}


def _launch_starts(chunks, L):
    t0, starts = 1, []
    for c in chunks:
        if t0 > L:
            break
        starts.append((t0, min(c, L - t0 + 1)))
        t0 += c
    assert t0 == L + 1, (chunks, t0)  # the lists are written to end on SimLen
    return starts


def test_the_launch_lists_hold_the_starts_they_are_meant_to():
    """Every steps-per-knot has a list that starts launches on a knot, one index behind one and
    one index before one, that holds single-index launches - one of them the last index - and ends on SimLen."""
    for spk, (nk, lists) in CASES.items():
        L = nk * spk + 1
        st = _launch_starts(lists[0], L)
        res = {(t0 - 1) % spk for t0, _ in st}
        assert {0, 1 % spk, (spk - 1) % spk} <= res, (spk, res)
        assert any(ns == 1 for _, ns in st) and st[-1] == (L, 1)
        if spk > 1:  # a single-index launch on a knot, one behind it and one before it
            assert {0, 1, spk - 1} <= {(t0 - 1) % spk for t0, ns in st if ns == 1}, spk
        for other in lists[1:]:
            _launch_starts(other, L)
    p = abi.default_parameters()
    assert (p.NightOn, p.NightOff) == (NIGHT_ON, NIGHT_OFF)
    for start in (0, 5, 23):
        for spk, (nk, _) in CASES.items():
            hours = (np.arange(nk + 1) + start) % 24
            d = np.diff((hours >= NIGHT_ON) | (hours <= NIGHT_OFF))
            assert 0 in hours[1:] and NIGHT_ON in hours and NIGHT_OFF + 1 in hours and d.any()


@functools.lru_cache(None)
def _knots(spk, start_hour):
    """Generator weather at the knots, as tests/test_hip_knots.py draws its base block."""
    nk = CASES[spk][0] + 1
    f = synth.synth_forcing(N, (nk - 1) * spk + 1, seed=20240110 + spk, steps_per_knot=spk, start_hour=start_hour)
    K = {k: np.ascontiguousarray(f[k][:, ::spk]) for k in gh.KNOT_FIELDS}
    K["phase"] = np.ascontiguousarray(f["precphase"][:, ::spk])
    K["tsurf0"] = f["tsurfobs"][:, 0].copy()
    return K


def _settings(full, L):
    s = abi.default_settings(L, 30.0)
    if full:
        s.use_relaxation = 1
    return s


def _locals(K, full, spk):
    """FULL: relaxation behind an initialization phase that ends on index 1, one behind a knot, on a knot, or
    deep in the series; one target in five invalid."""
    ls = []
    for i in range(N):
        li = abi.default_local(); li.InitLenI = 1
        if full:
            li.InitLenI = (1, spk + 2, 3 * spk + 1, 11 * spk + 5)[i % 4]
            li.tair_relax = float(K["tair"][i, 1]) + 1.5
            li.VZ_relax = 3.0; li.RH_relax = 85.0
            if i % 5 == 4:
                li.tair_relax = -9999.0
        ls.append(li)
    return ls


def _same(a, b, what):
    assert a["failed"] == b["failed"], what
    assert np.array_equal(a["first_failed"], b["first_failed"]), what
    for k in OUT:
        bad = [int(i) for i in range(N) if not kh.same_bits(a["out"][k][i], b["out"][k][i])]
        if bad:
            i = bad[0]
            at = int(np.flatnonzero(a["out"][k][i].view(np.int64 if a["out"][k].itemsize == 8 else np.int32)
                                    != b["out"][k][i].view(np.int64 if b["out"][k].itemsize == 8 else np.int32))[0])
            raise AssertionError((what, k, bad, f"point {i} differs first at index {at + 1}",
                                  a["out"][k][i, at], b["out"][k][i, at]))


def _both(spk, start_hour, full, precision, chunks, order="natural"):
    K = _knots(spk, start_hour)
    L = CASES[spk][0] * spk + 1
    s, p, ls = _settings(full, L), abi.default_parameters(), _locals(K, full, spk)
    kw = dict(precision=precision, chunks=chunks, order=order, start_hour=start_hour, spk=spk)
    return kh.run_knots(K, s, p, ls, source="knots", **kw), kh.run_knots(K, s, p, ls, source="window", **kw)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("full", [False, True], ids=["lean", "full"])
@pytest.mark.parametrize("start_hour", [0, 5, 23])
@pytest.mark.parametrize("spk", [1, 7, 120])
def test_carried_bookkeeping_equals_the_expanded_windows(spk, start_hour, full, precision):
    """All six outputs of every point at every index, and the failed indices, bit for bit (fp32 too: both sources
    run the same fp32 arithmetic), over every launch list of the steps-per-knot."""
    for chunks in CASES[spk][1]:
        a, b = _both(spk, start_hour, full, precision, list(chunks))
        assert np.isfinite(a["out"]["tsurf"]).all()
        _same(a, b, (spk, start_hour, full, precision, chunks[:8]))


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("full", [False, True], ids=["lean", "full"])
def test_carried_bookkeeping_under_the_forecast_order(full, precision):
    """Launches of sixty indices with a re-sort between them: the knot columns are gathered through the order row."""
    a, b = _both(120, 23, full, precision, 60, order="forecast")
    assert a["moved"] > 0 and all(np.array_equal(x, y) for x, y in zip(a["orders"], b["orders"]))
    _same(a, b, ("forecast", full, precision))


def test_carried_bookkeeping_equals_the_reference():
    """Seven indices per knot from 23:00, fp64, LEAN, against the CPU reference on the numpy expansion of the same
    knots: no point fails there (351 indices of generator weather)."""
    spk, start_hour = 7, 23
    K = _knots(spk, start_hour)
    L = CASES[spk][0] * spk + 1
    s, p, ls = _settings(False, L), abi.default_parameters(), _locals(K, False, spk)
    f = kh.expand(K, L, spk, start_hour)
    assert int(f["hour"][0]) == 23 and int(f["hour"][spk]) == 0 and int(f["hour"][spk - 1]) == 23
    ora, ora_failed = kh.reference(f, s, p, ls)
    assert not ora_failed.any()
    res = kh.run_knots(K, s, p, ls, chunks=list(CASES[spk][1][0]), order="natural", start_hour=start_hour, spk=spk)
    assert res["failed"] == 0 and not res["first_failed"].any()
    for k in OUT:
        bad = [int(i) for i in range(N) if not kh.same_bits(res["out"][k][i], ora[k][i])]
        assert not bad, (k, bad)


def _decimated_knots_run(K, settings, params, local, *, precision, chunks, start_hour, spk, decimate):
    """The LEAN block through rs_hip_step_knots, natural order, with every `decimate`-th index written: launch t0
    writes from row ceil((t0 - 1) / decimate) of the series (device.Plan.step_knots' default).  Returns
    out [n][rows of the series] per field, NaN where no launch wrote."""
    import torch
    from roadsurf_amd import device, lib

    n, L = K["tair"].shape[0], int(settings.SimLen)
    f32 = precision == 32
    wdt = torch.float32 if f32 else torch.float64
    plan = device.Plan(n, settings, params, 0)
    plan.set_variant(kh.DUO)
    if f32:
        plan.set_precision(32)
    plan.set_history_score(False)
    dev, npad = plan.device, plan.np_pad
    try:
        knots = torch.from_numpy(kh.knot_block(K, npad)).to(dev)
        spec = lib.RsSynthSpec(0, 0, spk, start_hour)
        f1 = kh.expand(K, 1, spk, start_hour)
        win0 = device.ForcingWindow.empty(1, npad, dev, optional=("tdew", "tsurfobs"), dtype=wdt)
        for name, t in win0.tensors.items():
            if t is None or name == "hour":
                continue
            t.zero_()
            t[0, :n] = torch.from_numpy(np.ascontiguousarray(f1[name][:, 0])).to(dev).to(t.dtype)
        win0.tensors["hour"][0] = int(f1["hour"][0])
        pp = plan.point_params(plan.uniform_tbottom(*kh.start_of(start_hour)[:3]))
        plan.reset_order()
        plan.init_state(win0, pp)
        nrows = (L - 1) // decimate + 1
        got = {k: np.full((n, nrows), np.nan, np.float32 if f32 else np.float64) for k in OUT}
        out = device.OutputWindow.empty(max(chunks) // decimate + 2, npad, dev, decimate=decimate, dtype=wdt)
        for t0, ns in _launch_starts(chunks, L):
            for t in out.tensors.values():
                t.fill_(float("nan"))
            plan.step_knots(spec, knots, out, pp, t0, ns)
            plan.sync()
            row0 = (t0 - 1 + decimate - 1) // decimate
            kept = [i for i in range(t0, t0 + ns) if (i - 1) % decimate == 0]
            for k in OUT:
                rows = out.tensors[k][:, :n].cpu().numpy()
                for i in kept:
                    got[k][:, (i - 1) // decimate] = rows[(i - 1) // decimate - row0]
                written = ~np.isnan(rows).all(axis=1)
                assert int(written.sum()) == len(kept), (k, t0, ns, written.nonzero())  # no row beside the kept ones
        return got, plan.failed_count()
    finally:
        plan.close()


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("decimate", [2, 5])
def test_carried_output_row_with_decimation_and_unaligned_launches(decimate, precision):
    """Every second / fifth index kept, seven indices per knot, launches that start on a kept index, one behind it and
    anywhere between two (single-index launches that write nothing among them): the kept rows are the rows of the
    undecimated run through the forcing windows, and no launch writes another row."""
    spk, start_hour = 7, 23
    chunks = list(CASES[spk][1][0])
    starts = {(t0 - 1) % decimate for t0, _ in _launch_starts(chunks, CASES[spk][0] * spk + 1)}
    assert starts == set(range(decimate))
    K = _knots(spk, start_hour)
    L = CASES[spk][0] * spk + 1
    s, p, l = _settings(False, L), abi.default_parameters(), _locals(K, False, spk)[0]
    want = kh.run_knots(K, s, p, l, precision=precision, chunks=chunks, order="natural", start_hour=start_hour, spk=spk,
                        source="window")
    got, failed = _decimated_knots_run(K, s, p, l, precision=precision, chunks=chunks, start_hour=start_hour, spk=spk,
                                       decimate=decimate)
    assert failed == want["failed"] == 0
    for k in OUT:
        assert kh.same_bits(got[k], np.ascontiguousarray(want["out"][k][:, ::decimate])), (k, decimate, precision)
