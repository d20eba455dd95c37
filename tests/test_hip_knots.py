"""GPU: the knot-reading kernels - step_kernel_duo<*, SRC_KNOTS>, step_kernel_f32duo<X2_KNOTS>, expand_kernel and
expand_kernel_f32 - on knots a CALLER made (include/roadsurf.h: the knot buffers are the caller's), against the plain
numpy rule `k0 + (r * (k1 - k0)) / spk` (golden_helpers.expand_knots) and the CPU checker run on its series.

fp64 comparisons are bit equality (knot_helpers.same_bits); the only cases with nan_equal=True are the ones that
hold a NaN on purpose and say so.  Nothing else has a tolerance.  The index-1 window of every run is the numpy
expansion's first row: no kernel under test produces an input of the reference or of another kernel under test.
"""
import functools
import types

import numpy as np
import pytest

import golden_helpers as gh
import knot_helpers as kh
import oracle_helpers as oh
from roadsurf_amd import abi, synth

pytestmark = pytest.mark.gpu
SPK = 120
N, NK, L, START = 130, 7, 721, 17  # two full wavefronts and a ragged one; 17:00 - 23:00, the day/night switch inside
OUT = oh.F64_OUT
F4 = kh.F4


def _lean_local():
    l = abi.default_local(); l.InitLenI = 1
    return l


# ---- (a) the golden fixtures through the headline kernels ------------------------------------------------------

@functools.lru_cache(None)
def _scenarios():
    z = gh.load("e2e_scenarios.npz")
    return z, {k[5:]: z[k] for k in z.files if k.startswith("knot_")}


@pytest.mark.parametrize("chunk", [60, 240, 7])
@pytest.mark.parametrize("order", ["natural", "forecast"])
def test_golden_scenarios_through_the_knot_reading_kernel(order, chunk):
    """e2e_scenarios.npz - the REFERENCE's own recorded answers, every precipitation phase, one failing point -
    through rs_hip_step_knots: 8 points, 50 knots, 5761 indices."""
    z, K = _scenarios()
    Ls = 48 * SPK + 1
    assert K["tair"].shape == (8, 50)
    res = kh.run_knots(K, abi.default_settings(Ls), abi.default_parameters(), _lean_local(), chunks=chunk, order=order)
    assert res["failed"] == 1
    idx = z["out_index"]
    for k in OUT:
        assert kh.same_bits(res["out"][k][:, idx], z[f"out_{k}"]), k
    f = kh.expand(K, Ls, SPK)
    assert np.array_equal(res["first_failed"], kh.predict_failure(f, False))
    assert int((res["first_failed"] > 0).sum()) == 1


@pytest.mark.parametrize("order", ["natural", "forecast"])
@pytest.mark.parametrize("case", ["relax", "force"])
def test_golden_feature_knots_through_the_full_knot_reading_kernel(case, order):
    """e2e_features.npz's knots through the FULL knot instances.  The knots carry the observation of index 1 only,
    so the oracle's input has TsurfObs missing behind index 1 too and the comparison is with a FRESH oracle run of
    that input (the stored relax_* / force_* rows were made with 360 observed indices)."""
    z = gh.load("e2e_features.npz")
    K = {k[5:]: z[k] for k in z.files if k.startswith("knot_")}
    Lf = 12 * SPK + 1
    f = kh.expand(K, Lf, SPK)
    assert (f["tsurfobs"][:, 1:] == -9999.9).all() and (f["tsurfobs"][:, 0] > -100).all()
    s = abi.default_settings(Lf)
    if case == "relax":
        s.use_relaxation = 1
    else:
        s.force_tsurf = 1
    p = abi.default_parameters()
    ls = []
    for i in range(6):
        li = abi.default_local(); li.InitLenI = 360
        li.tair_relax = float(z["tair_relax"][i]); li.VZ_relax = 3.0; li.RH_relax = 85.0
        ls.append(li)
    ora, ora_failed = kh.reference(f, s, p, ls)
    res = kh.run_knots(K, s, p, ls, chunks=97, order=order)
    assert np.array_equal(res["first_failed"], ora_failed)
    for k in OUT:
        assert kh.same_bits(res["out"][k], ora[k]), (case, k)


# ---- (c) the crafted atlas ---------------------------------------------------------------------------------------

def _base_knots(n=N, nk=NK, spk=SPK, start=START, seed=20240110):
    f = synth.synth_forcing(n, (nk - 1) * spk + 1, seed=seed, steps_per_knot=spk, start_hour=start)
    K = {k: np.ascontiguousarray(f[k][:, ::spk]) for k in gh.KNOT_FIELDS}
    K["phase"] = np.ascontiguousarray(f["precphase"][:, ::spk])
    K["tsurf0"] = f["tsurfobs"][:, 0].copy()
    return K


# (variable, side): the sixteen bounds of CheckValues' forcing tests; Tdew's two count with the FULL set only
BOUNDS = [(v, side) for v in ("tair", "vz", "rhz", "prec", "sw", "lw", "tdew") for side in (0, 1)]
NAN_POINT = 100


@functools.lru_cache(None)
def _atlas(full=True):
    """(K, edited): the block and, per edge, the points that own it.  Every other point keeps generator weather.
    The LEAN feature set does not read the knots' dew point (include/roadsurf.h: no CheckValues test of it, where the
    reference always has one), so the LEAN block leaves Tdew's two crossings out: fourteen bounds there, sixteen in
    FULL."""
    K = _base_knots()
    E = {}

    def own(name, *pts):
        for p in pts:
            assert all(p not in v for v in E.values()), (name, p)
        E[name] = pts

    sgn = lambda side: 1.0 if side else -1.0
    # crossings strictly inside an interval: knot j inside the limit, knot j + 1 beyond it
    for q, (v, side) in enumerate(BOUNDS):
        p, j = 2 + q, 1 + q % 4
        lim = kh.LIMITS[v][side]
        if v == "tdew" and not full:
            continue
        K[v][p, j] = lim - sgn(side) * (0.9 + 0.1 * q)
        K[v][p, j + 1] = lim + sgn(side) * (2.9 - 0.05 * q)
        own(f"cross_{v}_{side}", p)
    # ON the limit (the tests are strict: no failure), at a knot between knots further inside
    K["tair"][20, 2:5] = [95.0, 100.0, 95.0]
    K["prec"][21, 2:5] = [0.0, F4(-0.1), 0.0]
    own("on_limit", 20, 21)
    # the next double beyond it: fails at the knot's own index and nowhere before
    K["tair"][22, 2:5] = [95.0, np.nextafter(100.0, np.inf), 95.0]
    K["lw"][23, 2] = np.nextafter(F4(-0.1), -np.inf)
    own("beyond_limit", 22, 23)
    K["rhz"][24, 0] = 125.0
    own("fails_at_1", 24)
    K["tair"][25, 5:7] = [90.0, 90.0 + 10.12]  # 119/120 of the step is beyond 100, 118/120 is not
    own("fails_at_last_checked", 25)
    K["tair"][26, 5:7] = [90.0, 100.05]  # only index SimLen is beyond 100: not checked
    own("offends_at_simlen_only", 26)
    K["vz"][27, 0] = -1.5  # index 1 is lifted to 0.4 before the test; index 2 is not
    own("vz_floor", 27)
    # flat, falling, zeros of either sign, subnormal steps
    for v in gh.KNOT_FIELDS:
        K[v][30, :] = K[v][30, 0]
    K["phase"][30, :] = K["phase"][30, 0]
    own("flat", 30)
    j = np.arange(NK)
    K["tair"][31] = 5.0 - j; K["tdew"][31] = 3.0 - j; K["vz"][31] = 6.0 - 0.5 * j; K["rhz"][31] = 90.0 - 5 * j
    K["prec"][31] = 1.2 - 0.2 * j; K["sw"][31] = 300.0 - 50 * j; K["lw"][31] = 320.0 - 10 * j; K["phase"][31] = 1
    own("falling", 31)
    K["tair"][32] = [1.0, -0.0, -1.0, -0.0, 1.0, -0.0, -0.0]
    K["prec"][33] = [0.3, -0.0, -0.0, 0.4, -0.0, 0.0, -0.0]
    K["vz"][34] = [1.0, -0.0, 0.5, -0.0, -0.0, 1.0, -0.0]
    own("negative_zero", 32, 33, 34)
    K["prec"][35] = [0.0, 5e-324, 0.0, 5e-324, 0.0, 0.0, 5e-324]; K["phase"][35] = 1
    K["tair"][36] = [0.0, 1e-310, 0.0, 1e-310, 1e-310, 0.0, 0.0]
    own("subnormal", 35, 36)
    # every phase code at successive knots of a wet point, precipitation on one side of a knot only
    K["phase"][37] = [-9999, 0, 1, 2, 3, 4, 5]; K["prec"][37] = [1.5, 0.0, 1.5, 0.0, 1.5, 0.0, 1.5]
    K["phase"][38] = [6, 5, 4, 3, 2, 1, -9999]; K["prec"][38] = [0.0, 2.0, 0.0, 2.0, 0.0, 2.0, 0.0]
    for p in (37, 38):
        K["tair"][p] = [0.6, -0.4, 0.3, -0.6, 0.2, -0.2, 0.5]; K["tdew"][p] = K["tair"][p] - 0.3; K["rhz"][p] = 97.0
    own("phases", 37, 38)
    # calm air with a surface 40 K off the air; humidity on its limits
    K["vz"][40] = 0.0; K["tair"][40] = -10.0; K["tdew"][40] = -12.0; K["tsurf0"][40] = 30.0
    K["vz"][41] = 0.0; K["tair"][41] = 10.0; K["tdew"][41] = 8.0; K["tsurf0"][41] = -30.0
    K["rhz"][42] = 0.0
    K["rhz"][43] = 120.0
    own("calm_and_humidity", 40, 41, 42, 43)
    # non-finite and huge knots, in the second wavefront
    K["tair"][64, 3] = np.inf
    K["prec"][70, 2] = -np.inf
    K["tair"][80, 4] = 1e307
    own("nonfinite", 64, 70, 80)
    K["tair"][NAN_POINT, 3] = np.nan
    own("nan", NAN_POINT)
    return K, E


def _settings(full, simlen=L, dtsecs=30.0):
    s = abi.default_settings(simlen, dtsecs)
    if full:
        s.use_relaxation = 1
    return s


def _locals(K, full):
    """FULL: per-point InitLenI in {1, 120, 121, 500}, relaxation with one target in five invalid."""
    ls = []
    for i in range(K["tair"].shape[0]):
        li = abi.default_local(); li.InitLenI = 1
        if full:
            li.InitLenI = (1, 120, 121, 500)[i % 4]
            t = float(K["tair"][i, 1])
            li.tair_relax = (t if np.isfinite(t) and abs(t) < 60 else 0.0) + 1.5
            li.VZ_relax = 3.0; li.RH_relax = 85.0
            # an invalid target: no relaxation for the point - one in five, and the points that own a limit
            # (relaxation edits the forcing in place: the failing index would no longer be the numpy series')
            if i % 5 == 4 or 2 <= i <= 27 or i in (64, 70, 80):
                li.tair_relax = -9999.0
        ls.append(li)
    return ls


@functools.lru_cache(None)
def _atlas_reference(full):
    """(numpy series, predicted failing index, oracle outputs, oracle's failing index) of the atlas; the oracle's and
    the prediction must agree before anything runs on the device."""
    K, E = _atlas(full)
    f = kh.expand(K, L, SPK, START)
    assert int(f["hour"][0]) == START and 19 in f["hour"] and int(f["hour"][-1]) == 23  # NightOn = 19 falls inside
    want = kh.predict_failure(f, full)
    ora, ora_failed = kh.reference(f, _settings(full), abi.default_parameters(), _locals(K, full))
    clean = np.array([i for i in range(N) if i != NAN_POINT])  # (a NaN fails no test: the reference runs on with it)
    assert np.array_equal(ora_failed[clean], want[clean]), (ora_failed[clean] - want[clean]).nonzero()
    # the edges are where they were meant to be
    for q, (v, side) in enumerate(BOUNDS):
        i = int(want[2 + q])
        if v == "tdew" and not full:
            assert i == 0
        else:
            assert i > 1 and (i - 1) % SPK != 0 and (i - 1) // SPK == 1 + q % 4, (v, side, i)
    assert want[20] == 0 and want[21] == 0 and want[22] == 3 * SPK + 1 and want[23] == 2 * SPK + 1
    assert want[24] == 1 and want[25] == L - 1 and want[26] == 0 and want[27] == 2
    assert want[64] == 2 * SPK + 2 and want[70] == SPK + 2 and want[80] == 3 * SPK + 2
    for name in ("flat", "falling", "negative_zero", "subnormal", "phases", "calm_and_humidity"):
        assert all(want[p] == 0 for p in E[name]), name
    return f, want, ora, ora_failed


@functools.lru_cache(None)
def _clean_run(full, precision=64):
    """The block WITHOUT the edits, natural order: what every untouched point must keep."""
    K = _base_knots()
    res = kh.run_knots(K, _settings(full), abi.default_parameters(), _locals(_atlas()[0], full), precision=precision,
                       chunks=97, order="natural", start_hour=START)
    assert res["failed"] == 0
    return res


def _check_against_reference(res, want, ora, skip=(), nonfinite=()):
    """nonfinite: points whose forcing is infinite or beyond 1e300 at the index that fails them - the failing
    index's own row is computed from it and holds NaN in places: those points compare with nan_equal=True."""
    n, Ls = ora["tsurf"].shape
    pts = np.array([i for i in range(n) if i not in skip])
    assert np.array_equal(res["first_failed"][pts], want[pts]), \
        [(int(i), int(res["first_failed"][i]), int(want[i])) for i in pts if res["first_failed"][i] != want[i]]
    assert res["failed"] == int((want[pts] > 0).sum()) + sum(int(res["first_failed"][i] > 0) for i in skip)
    for k in OUT:
        bad = [int(i) for i in pts if not kh.same_bits(res["out"][k][i], ora[k][i], nan_equal=int(i) in nonfinite)]
        assert not bad, (k, bad, [(res["out"][k][i, want[i] - 1], ora[k][i, want[i] - 1]) for i in bad if want[i]])
    for i in pts:  # (already implied by the oracle's rows; said once more in the words of the contract)
        if want[i]:
            assert all((res["out"][k][i, want[i]:] == -9999.0).all() for k in OUT)
            assert all(res["out"][k][i, want[i] - 1] != -9999.0 for k in OUT)


# rs_hip_step_knots has a DOMAIN (include/roadsurf.h): spk <= 128, finite knots, successive knots equal or
# 2^-1015 <= |k1 - k0| < 2^1017.  These points of the atlas are outside it; the expansion kernels are held to the
# rule on them (test_expansion_kernels_equal_the_numpy_rule), the step kernel in strict expected failures below.
OUTSIDE = (64, 70, NAN_POINT)


@functools.lru_cache(None)
def _atlas_run(full, order):
    K, _ = _atlas(full)
    return kh.run_knots(K, _settings(full), abi.default_parameters(), _locals(K, full), chunks=97, order=order,
                        start_hour=START)


@pytest.mark.parametrize("order", ["natural", "forecast"])
@pytest.mark.parametrize("full", [False, True], ids=["lean", "full"])
def test_atlas_of_crafted_knots_equals_the_reference(full, order):
    """Each point or small group owns one edge (_atlas); launches of 97 indices.  Every point inside the call's
    domain: the failing index predicted from the numpy series, every row the oracle's bits (the failing index's own
    row included, -9999.0 behind it).  The 1e307 knot (point 80) is beyond the band on paper, but its first value
    behind the knot (r = 1: 8.3e304) is finite and fails the point where the reference does; its failing row is
    computed from that value and compares with nan_equal=True.  The three points OUTSIDE the domain are left to
    test_step_kernel_outside_its_knot_domain; here their neighbours and every other untouched point must keep the
    bits of the run without the edits, and with order="forecast" every order row is still a permutation.

    What the GPU said of the three predictions of the host emulation, on the code before the expansion kernels had
    their IEEE path (same tests, old library):
      inf knots: CONFIRMED - points 64 (+inf Tair) and 70 (-inf Prec) were never failed (first failed index 0 where
        the reference has 242 and 122) and the expanded windows held NaN from the knot's own index on;
      1e307 knot: NOT confirmed for the step kernel - the point was failed at the reference's index 362, because
        r = 1 gives a finite value beyond the limit long before r * dv overflows (r >= 18);
      subnormal steps: CONFIRMED in the expanded window (Tair 0.0 -> 1e-310, point 36, differed inside the interval);
        the model's outputs do not see it;
      -0.0 knots: CONFIRMED in the expanded window (VZ of point 34 differed in bits where the values compared equal);
        the model's outputs do not see it."""
    K, E = _atlas(full)
    f, want, ora, _ = _atlas_reference(full)
    res = _atlas_run(full, order)
    for c, row in enumerate(res["orders"]):
        assert np.array_equal(np.sort(row), np.arange(N)), f"launch {c}: the order row is no permutation"
    assert len(res["orders"]) == 8
    if order == "forecast":
        assert res["moved"] > 0
    _check_against_reference(res, want, ora, skip=OUTSIDE, nonfinite=(80,))
    edited = sorted(p for v in _atlas(True)[1].values() for p in v)
    untouched = np.array([i for i in range(N) if i not in edited])
    assert len(untouched) >= 80 and {63, 65, 69, 71, 99, 101, 128, 129} <= set(untouched.tolist())
    clean = _clean_run(full)
    for k in OUT:
        assert kh.same_bits(res["out"][k][untouched], clean["out"][k][untouched]), k


def _sixty():
    """spk = 60 with DTSecs = 60: 4 knots from 22:00 (the 23 -> 0 wrap of the hour, which six hours from 17:00 do
    not reach, falls inside)."""
    spk, nk, start = 60, 4, 22
    Ls = (nk - 1) * spk + 1
    K = _base_knots(nk=nk, spk=spk, start=start)
    K["tair"][3, 1:3] = [99.0, 102.5]
    K["lw"][5, 2] = F4(-0.1)
    K["tair"][32, :] = [1.0, -0.0, -1.0, -0.0]
    K["prec"][35, :] = [0.0, 5e-324, 0.0, 5e-324]; K["phase"][35] = 1
    K["tair"][36, :] = [0.0, 1e-310, 0.0, 0.0]
    K["tair"][64, 2] = np.inf
    K["prec"][70, 1] = -np.inf
    return K, spk, Ls, start


@functools.lru_cache(None)
def _sixty_run():
    K, spk, Ls, start = _sixty()
    s, p = _settings(False, Ls, 60.0), abi.default_parameters(60.0)
    f = kh.expand(K, Ls, spk, start)
    assert f["minute"][1] == 1 and f["second"][1] == 0 and f["hour"].tolist()[::spk] == [22, 23, 0, 1]
    want = kh.predict_failure(f, False)
    assert want[3] > spk + 1 and want[5] == 0 and want[64] == spk + 2 and want[70] == 2 and (want > 0).sum() == 3
    ora, ora_failed = kh.reference(f, s, p, _lean_local())
    assert np.array_equal(ora_failed, want)
    res = kh.run_knots(K, s, p, _lean_local(), chunks=97, order="natural", start_hour=start, spk=spk)
    return res, want, ora


def test_atlas_at_sixty_indices_per_knot():
    """spk = 60 with DTSecs = 60 (r_spk = 1/60, the other uniform reciprocal in use): LEAN, natural order; the two
    infinite knots are outside the call's domain (test_step_kernel_outside_its_knot_domain)."""
    res, want, ora = _sixty_run()
    _check_against_reference(res, want, ora, skip=(64, 70))


@pytest.mark.xfail(strict=True, reason="outside rs_hip_step_knots' domain (include/roadsurf.h): knot_forcing divides "
                   "by the reciprocal of the span without a test - an infinite or NaN knot turns the intervals around "
                   "it into NaN, the knot's own index included, and a NaN passes CheckValues, so the point is not "
                   "failed where the reference fails it; the guard cost the headline 1.9 % "
                   "(profiles/knot_domain_guard.txt)")
@pytest.mark.parametrize("block,point", [("atlas", 64), ("atlas", 70), ("atlas", NAN_POINT), ("sixty", 64), ("sixty", 70)])
def test_step_kernel_outside_its_knot_domain(block, point):
    """What the rule asks of the three out-of-domain points: +inf in a later Tair knot and -inf in a Prec knot fail
    the point at the first index whose expanded value is infinite, with the reference's rows up to it; a NaN Tair
    knot leaves the knot before it and everything up to it untouched (nan_equal=True: these cases hold NaN and
    infinities on purpose)."""
    if block == "atlas":
        res = _atlas_run(False, "natural")
        _, want, ora, _ = _atlas_reference(False)
    else:
        res, want, ora = _sixty_run()
    assert res["first_failed"][point] == want[point]
    for k in OUT:
        assert kh.same_bits(res["out"][k][point], ora[k][point], nan_equal=True), k


# ---- (b) the expansion kernels against the numpy rule -------------------------------------------------------------

WINDOWS = ((2 * SPK + 1, 130), (2 * SPK, 130), (2 * SPK + 2, 130), (L, 1))  # on a knot, one before, one after, the last


@pytest.mark.parametrize("n", [1, 65, 130])
@pytest.mark.parametrize("precision", [64, 32])
def test_expansion_kernels_equal_the_numpy_rule(precision, n):
    """rs_hip_expand_forcing and rs_hip_expand_forcing_ordered (the latter behind a forecast re-sort) on the first n
    points of the atlas.  fp64: bits - nan_equal=True for the three points whose knots make a NaN on purpose
    (inf - inf behind an infinite knot, the NaN knot), strict bit equality for every other.  fp32: np.float32 of one fused multiply-add (knot_helpers.lerp_f32, evaluated in float64); an element
    that differs is evaluated again with exact rationals before it counts (double rounding)."""
    import torch
    from roadsurf_amd import device, lib, workload
    Kall, _ = _atlas()
    K = {k: v[:n].copy() for k, v in Kall.items()}
    f = kh.expand(K, L, SPK, START)
    f32 = precision == 32
    wdt = torch.float32 if f32 else torch.float64
    e32 = kh.expand_f32(K, L, SPK) if f32 else None
    plan = device.Plan(n, _settings(True), abi.default_parameters(), 0)
    plan.set_variant(kh.DUO)
    if f32:
        plan.set_precision(32)
    dev, npad = plan.device, plan.np_pad
    knots = torch.from_numpy(kh.knot_block(K, npad)).to(dev)
    spec = lib.RsSynthSpec(0, 0, SPK, START)
    wrong = []
    # nan_equal=True only for the points whose knots make a NaN (inf - inf behind an infinite knot, the NaN knot)
    nanrows = np.array([i for i in OUTSIDE if i < n], np.int64)
    plain = np.array([i for i in range(n) if i not in OUTSIDE], np.int64)
    it = {8: np.int64, 4: np.int32}

    def check(tag, win, t0, ns, row):
        sl = slice(t0 - 1, t0 - 1 + ns)
        for name in gh.KNOT_FIELDS + ("tsurfobs", "precphase"):
            got = win.tensors[name][:ns, :n].cpu().numpy().T
            back = np.empty_like(got); back[row] = got
            if name == "precphase" or not f32:
                for rows, nan_equal in ((plain, False), (nanrows, True)):
                    if len(rows) and not kh.same_bits(back[rows], f[name][rows, sl], nan_equal=nan_equal):
                        d = back[rows].view(it[back.itemsize]) != f[name][rows, sl].view(it[back.itemsize])
                        wrong.append((tag, t0, name, [(int(rows[i]), int(j)) for i, j in np.argwhere(d)[:3]]))
                continue
            if name == "tsurfobs":
                exp = f[name][:, sl].astype(np.float32)
            else:
                exp = e32[name][0][:, sl]
            bad = np.argwhere(~((back.view(np.int32) == exp.view(np.int32)) | (np.isnan(back) & np.isnan(exp))))
            for i, j in bad:
                _, k0, k1, r = e32[name]
                exact = kh.lerp_f32_exact(k0[i, sl][j], k1[i, sl][j], int(r[sl][j]), SPK)
                if exact.view(np.int32) != back[i, j].view(np.int32):
                    wrong.append((tag, t0, name, int(i), int(j), float(back[i, j]), float(exact)))
        hours = win.tensors["hour"][:ns].cpu().numpy()
        if not np.array_equal(hours, f["hour"][sl]):
            wrong.append((tag, t0, "hour"))

    def window():
        w = device.ForcingWindow.empty(130, npad, dev, optional=("tdew", "tsurfobs"), dtype=wdt)
        for name, t in w.tensors.items():
            if t is not None:
                t.fill_(7)  # no value of the series: a row the kernel skips shows
        return w

    try:
        ident = np.arange(n)
        for t0, ns in WINDOWS:
            w = window()
            plan.expand_range(spec, knots, 0, NK, w, t0, ns)
            plan.sync()
            check("expand_forcing", w, t0, ns, ident)
        # ... and in slot order behind a re-sort made from this block's own knot rows
        w0 = window()
        plan.reset_order()
        plan.expand_ordered(spec, knots, w0, 1, 1)
        plan.sync()
        check("ordered, identity", w0, 1, 1, ident)
        pp = plan.point_params(plan.uniform_tbottom(2024, 1, 10))
        plan.init_state(w0, pp)
        sorter = types.SimpleNamespace(
            plan=plan, simlen=L, resort=True, forecast=True, chunk=130, spec=spec, knots=knots, precip_bit=True,
            previews_in_window=True, forecast_alpha=0.5, forecast_mode=workload.DEFAULT_FORECAST_MODE)
        workload.SyntheticRun._resort(sorter, 2 * SPK + 2)
        plan.sync()
        row = plan.order().cpu().numpy()[:n].astype(np.int64)
        assert np.array_equal(np.sort(row), ident)
        assert n < 65 or (row != ident).any()
        for t0, ns in WINDOWS:
            w = window()
            plan.expand_ordered(spec, knots, w, t0, ns)
            plan.sync()
            check("expand_forcing_ordered", w, t0, ns, row)
    finally:
        plan.close()
    assert not wrong, wrong[:12]


def test_expansion_with_a_span_beyond_128():
    """steps_per_knot = 360 (DTSecs = 10): r reaches 359, so r * dv overflows for |dv| from 2^1024 / 359 on, inside
    the band derived for spans up to 2^7 - expand_kernel divides the IEEE way for every interval of such a span."""
    import torch
    from roadsurf_amd import device, lib
    spk, nk, n = 360, 3, 65
    Ls = (nk - 1) * spk + 1
    K = _base_knots(n=n, nk=nk, spk=spk)
    K["tair"][3, 1] = 6e305          # 359 * 6e305 is infinite, 128 * 6e305 is not
    K["tair"][5] = [0.0, 2.0 ** -1016 * 3, 0.0]  # a quotient that is subnormal only for a span beyond 128
    K["lw"][7] = [-0.0, 1.0, -0.0]
    K["prec"][9, 2] = np.inf
    f = kh.expand(K, Ls, spk, START)
    assert np.isinf(f["tair"][3, spk - 1]) and np.isfinite(f["tair"][3, 100])
    plan = device.Plan(n, _settings(False, Ls, 10.0), abi.default_parameters(10.0), 0)
    try:
        knots = torch.from_numpy(kh.knot_block(K, plan.np_pad)).to(plan.device)
        spec = lib.RsSynthSpec(0, 0, spk, START)
        for t0, ns in ((1, 400), (spk, 3), (Ls, 1)):
            w = device.ForcingWindow.empty(400, plan.np_pad, plan.device, optional=("tdew", "tsurfobs"))
            plan.expand_range(spec, knots, 0, nk, w, t0, ns)
            plan.sync()
            for name in gh.KNOT_FIELDS + ("precphase",):
                got = w.tensors[name][:ns, :n].cpu().numpy().T
                rows = np.array([i for i in range(n) if not (name == "prec" and i == 9)])
                assert kh.same_bits(got[rows], f[name][rows, t0 - 1:t0 - 1 + ns]), (t0, name)
            got = w.tensors["prec"][:ns, 9].cpu().numpy()  # nan_equal=True: inf - inf behind the infinite knot
            assert kh.same_bits(got, f["prec"][9, t0 - 1:t0 - 1 + ns], nan_equal=True), t0
    finally:
        plan.close()


# ---- (d) the fp32 knot kernel's interval shortcut -----------------------------------------------------------------

def _f32_safe(K, lo, hi, full):
    """knots_safe of rs_kernels_f32.hip for the points [lo, hi): every knot end of every interval keeps 0.01, in
    single precision, to the limits written there as literals."""
    m = np.float32(0.01)
    lims = {"tair": (-90.0, 100.0), "vz": (-1.0, 100.0), "rhz": (-0.1, 120.0), "prec": (-0.1, 500.0),
            "sw": (-0.1, 4000.0), "lw": (-0.1, 1000.0), "tdew": (-90.0, 100.0)}
    ok = np.ones(NK - 1, bool)
    for v, (a, b) in lims.items():
        if v == "tdew" and not full:
            continue
        v0 = K[v][lo:hi, :-1].astype(np.float32)
        v1 = v0 + (K[v][lo:hi, 1:] - K[v][lo:hi, :-1]).astype(np.float32)
        for e in (v0, v1):
            ok &= ((e > np.float32(a) + m) & (e < np.float32(b) - m)).all(axis=0)
    return ok


@functools.lru_cache(None)
def _f32_atlas(full):
    """Per bound three EVEN points of the first workgroup (their lane partners, the odd points, stay untouched):
    a knot end 0.02 inside the limit (the shortcut holds), one 0.005 inside (within the margin: index by index, no
    failure) and a crossing.  SW's upper bound takes 0.05 and 0.005: a float32 ulp at 4000 is 2.4e-4."""
    K = _base_knots()
    roles = {}
    sgn = lambda side: 1.0 if side else -1.0
    p = 0
    for q, (v, side) in enumerate(BOUNDS):
        if v == "tdew" and not full:
            continue
        lim = kh.LIMITS[v][side]
        inside = 0.05 if (v, side) == ("sw", 1) else 0.02
        j = 1 + q % 4
        K[v][p, j] = lim - sgn(side) * inside; roles[p] = ("safe", v, side); p += 2
        K[v][p, j] = lim - sgn(side) * 0.005; roles[p] = ("margin", v, side); p += 2
        # a step of 0.04 per index with the limit half way between two indices: 0.02 of clearance on either side
        A = 0.04 * (25.5 + q)
        K[v][p, j] = lim - sgn(side) * A; K[v][p, j + 1] = lim + sgn(side) * (4.8 - A)
        roles[p] = ("cross", v, side); p += 2
    assert p <= 128
    return K, roles


@pytest.mark.parametrize("full", [False, True], ids=["lean", "full"])
def test_fp32_interval_shortcut_fails_the_same_indices_and_keeps_the_neighbours(full):
    K, roles = _f32_atlas(full)
    f = kh.expand(K, L, SPK, START)
    want = kh.predict_failure(f, full)
    # on the CPU, before any launch: a crossing clears its limit by 1e-2 at the failing index and stays 1e-2 inside
    # at the index before - float32 rounding of the forcing (at most 2.4e-4) cannot move the index; nothing else fails
    for p, (role, v, side) in roles.items():
        if role != "cross":
            assert want[p] == 0, (p, role, v, side)
            continue
        i = int(want[p]); lim = kh.LIMITS[v][side]
        assert i > 2 and (i - 1) % SPK != 0
        s = 1.0 if side else -1.0
        assert s * (f[v][p, i - 1] - lim) >= 1e-2 and s * (lim - f[v][p, i - 2]) >= 1e-2, (p, v, side)
    assert all(want[i] == 0 for i in range(N) if i not in roles)
    base = _base_knots()
    assert _f32_safe(base, 0, 128, full).all()  # the clean block takes the shortcut in every interval of workgroup 0
    safe_pts = [p for p, r in roles.items() if r[0] == "safe"]
    Ks = {k: v.copy() for k, v in base.items()}
    for p in safe_pts:
        v = roles[p][1]; Ks[v][p] = K[v][p]
    assert _f32_safe(Ks, 0, 128, full).all()  # ... and 0.02 (SW: 0.05) inside still does
    for p, (role, v, side) in roles.items():
        if role == "margin":
            Km = {k: a.copy() for k, a in base.items()}; Km[v][p] = K[v][p]
            assert not _f32_safe(Km, 0, 128, full).all(), (p, v, side)  # ... and 0.005 inside does not

    s, prm, ls = _settings(full), abi.default_parameters(), _locals(_atlas()[0], full)
    res = kh.run_knots(K, s, prm, ls, precision=32, chunks=97, order="natural", start_hour=START)
    assert np.array_equal(res["first_failed"], want), \
        [(int(i), roles.get(int(i)), int(res["first_failed"][i]), int(want[i])) for i in np.nonzero(res["first_failed"] != want)[0]]
    assert res["failed"] == int((want > 0).sum())
    for i in np.nonzero(want)[0]:
        assert all((res["out"][k][i, want[i]:] == -9999.0).all() for k in OUT)
        assert all(res["out"][k][i, want[i] - 1] != -9999.0 for k in OUT)
    clean = _clean_run(full, 32)
    untouched = np.array([i for i in range(N) if i not in roles])
    assert all((p + 1) in untouched for p in roles)  # every lane partner
    for k in OUT:
        assert kh.same_bits(res["out"][k][untouched], clean["out"][k][untouched]), k
    # the knot launch and the fp32 window launch of the same block hand the model the same bits
    win = kh.run_knots(K, s, prm, ls, precision=32, chunks=97, order="natural", start_hour=START, source="window")
    assert np.array_equal(win["first_failed"], want)
    for k in OUT:
        assert kh.same_bits(res["out"][k], win["out"][k]), k
    # the points whose shortcut holds went through it unharmed: a safe edit run ALONE keeps the workgroup's shortcut
    alone = kh.run_knots(Ks, s, prm, ls, precision=32, chunks=97, order="natural", start_hour=START)
    assert alone["failed"] == 0
    for k in OUT:
        assert kh.same_bits(alone["out"][k][untouched], clean["out"][k][untouched]), k
        assert kh.same_bits(alone["out"][k][safe_pts], res["out"][k][safe_pts]), k


def test_fp32_one_unsafe_point_leaves_the_other_127_their_bits():
    """One workgroup in which exactly one point is unsafe (a knot end 0.005 inside Tair's upper limit): the other
    127 - and the ragged second workgroup - keep the bits they have when every point is safe."""
    base = _base_knots()
    assert _f32_safe(base, 0, 128, False).all()
    K = {k: v.copy() for k, v in base.items()}
    K["tair"][77, 3] = 100.0 - 0.005
    assert not _f32_safe(K, 0, 128, False)[2:4].any() and _f32_safe(K, 0, 128, False)[[0, 1, 4, 5]].all()
    assert kh.predict_failure(kh.expand(K, L, SPK, START), False).max() == 0
    s, prm, ls = _settings(False), abi.default_parameters(), _locals(base, False)
    res = kh.run_knots(K, s, prm, ls, precision=32, chunks=97, order="natural", start_hour=START)
    clean = _clean_run(False, 32)
    assert res["failed"] == 0
    others = np.array([i for i in range(N) if i != 77])
    for k in OUT:
        assert kh.same_bits(res["out"][k][others], clean["out"][k][others]), k
    assert not kh.same_bits(res["out"]["tsurf"][77], clean["out"]["tsurf"][77])  # (its weather did change)
