"""GPU: the wave-uniform shortcuts of rs_physics_body.inc - the bare road's storage block, `snow_here`, `ice_here`, the
dry index, the per-layer frozen / mixed / thawed split, CalcLE's dead tail - and sky_view_radiation's own dark
shortcut, in the step-kernel instances WITH sky view and WITH coupling, on the hand-made wavefronts of
tests/storage_cases.py dressed by tests/dressed_cases.py.  tests/test_hip_storage_waves.py holds the instances
without either; these compile the same physics text with other template arguments, register budgets and wave
compositions: shade and sun at the same index within a wavefront, a time index per lane, wavefronts made of
whichever points are parked, and replays that rewind a point's storages and take every wave-uniform decision a second
time among other neighbours.

The partner is the CPU oracle (the reference's own Fortran where it is built - with working coupling for a coupled
run -, the C restatement otherwise): all six outputs at every index and the first failed index, bit for bit, on two
batches of 1 280 points per flavour - the crafted order, in which every wavefront is one case, and the fixed
permutation of storage_cases, in which every wavefront mixes at least five.  A difference names its case and lane.
By tests/test_step_selection.py (rows "the dressed wavefronts") the flavours take

  sky, whole and chunks of 60, with / without the history score   step_kernel_duo<15, true / false, 0, true, true,
                                                                  false, false>  (DUO_SKY_SCORE, DUO_SKY)
  sky, 64-bit window offsets (ROADSURF_HIP_A32_LIMIT lowered)     step_kernel_sky_h<4>  (SKY_HYBRID)
  sky, 12 layers                                                  step_kernel_sky<false>  (SKY_LDS)
  sky, driver.run, natural and plan order                         step_kernel_duo<15, true, 2, true, true, false,
                                                                  false>  (DUO_RAW_SKY_SCORE)
  coupling, whole series                                          step_kernel_coupled<false>  (COUPLED)
  coupling, chunks of 60, replay lockstep / lockstep-collapsed    step_kernel_cpl_h<3, false>, step_kernel_cpl_replay_h
                                                                  <3, false>  (CPL_HYBRID, CPL_REPLAY_HYBRID)
  coupling, chunks of 60, replay general                          step_kernel_cpl_h<3, false>, step_kernel_coupled
                                                                  <false> over the list  (CPL_HYBRID, COUPLED)
  the same at 12 layers                                           step_kernel_cpl<false>, step_kernel_cpl_replay<false>
                                                                  (CPL_LDS, CPL_REPLAY_LDS), step_kernel_coupled<false>
  coupling + sky, chunks of 60, 15 layers                         step_kernel_cpl_h<3, true>, step_kernel_cpl_replay_h
                                                                  <3, true>  (CPL_HYBRID_SKY, CPL_REPLAY_HYBRID_SKY)
  coupling + sky, chunks of 60, 12 layers                         step_kernel_cpl<true>, step_kernel_cpl_replay<true>
                                                                  (CPL_LDS_SKY, CPL_REPLAY_LDS_SKY)
  coupling, driver.run (two sources)                              step_kernel_duo<15, true, 2, true, false, true,
                                                                  false> and <..., true, true>  (DUO_RAW_CPL,
                                                                  DUO_RAW_REPLAY)
  coupling + sky, driver.run                                      step_kernel_duo<15, true, 2, true, true, true, false>
                                                                  (DUO_RAW_CPL_SKY; the replay rounds read a forcing
                                                                  window: step_kernel_cpl_replay_h<3, true>)
  fp32 sky, whole and chunks, with / without the history score    step_kernel_f32duo<0, true / false, true, true>
                                                                  (F32_DUO_SKY_SCORE, F32_DUO_SKY)
  fp32 coupling, whole series                                     step_kernel_f32_coupled  (F32_COUPLED)

test_the_dressings_are_what_they_claim needs no GPU: from the oracle alone the dressed cases must contain the
situations they are made for - shade next to sun, snow on some lanes of a wavefront inside the coupling window, a replay
that rewound a storage - and nobody fails.

fp32 has no bit-exact partner and no lock-step coupling (a chunked fp32 coupled run stays refused): the crafted and the
mixed batch must give every point the same bits, no NaN, every storage within its limit, and the points that ever carry
snow or ice are the fp64 oracle's.  |fp32 - fp64| is printed per case, not asserted.  profiles/sky_cpl_waves.txt keeps
one run's lines."""
import numpy as np
import pytest

import dressed_cases as dc
import knot_helpers as kh
import storage_cases as sc
from roadsurf_amd import abi
from test_hip_storage_waves import _differing, carriers, f32_distribution, nsa

N, L = sc.N, sc.L
OUT = kh.OUT
STORAGES = ("snow", "water", "ice", "deposit", "ice2")
CHUNK = kh.FLAVOUR_CHUNK
NCASES = len(sc.CASES)


# ---- what the dressings contain, by the oracle (no GPU) ------------------------------------------------------------

def _clean(case, what, ora, failed):
    assert not failed.any(), (what, case)
    for k in OUT:
        assert np.isfinite(ora[k]).all() and (ora[k] > -100.0).all(), (what, case, k)


def test_the_sky_dressing_is_what_it_claims():
    plain = dc.references(False, False)
    for nl in (15, 12):
        refs = dc.references(True, False, nl)
        for case in sc.CASES:
            f, ls, ora, failed, sw_dir = refs[case]
            _clean(case, f"sky, {nl} layers", ora, failed)
            rows = []
            for w in range(2):
                lanes = slice(64 * w, 64 * w + 64)
                shade = (sw_dir[lanes] == 0) & (f["sw_dir"][lanes] > 0)  # the direct short wave zeroed by a horizon
                sun = sw_dir[lanes] > 0
                rows.append(int((shade.any(axis=0) & sun.any(axis=0)).sum()))
            line = f"sky, {nl} layers: {case}: rows with lanes shaded next to lanes in sun: wavefront 0 {rows[0]}, 1 {rows[1]}"
            if nl == 15:
                moved = float(np.abs(ora["tsurf"] - plain[case][2]["tsurf"]).max())
                line += f"; Tsurf moves by up to {moved:.3f} K against the plain run"
                assert moved >= 0.5, case
            print(line)
            if case in dc.SUNNY:
                assert rows[0] >= 100 and rows[1] >= 30, (case, rows)


def test_the_coupling_dressing_is_what_it_claims():
    rewound = []
    for sky in (False, True):
        for nl in (15, 12):
            what = f"coupling{' + sky' if sky else ''}, {nl} layers"
            base = dc.references(sky, False, nl)
            refs = dc.references(sky, True, nl)
            port = dc.references(sky, True, nl, which="port") if dc.kind(True) != "port" else None
            for case in sc.CASES:
                f, ls, ora, failed, _ = refs[case]
                _clean(case, what, ora, failed)
                if port is not None:
                    assert all(kh.same_bits(ora[k], port[case][2][k]) for k in OUT), (what, case)
                moved = int((np.abs(ora["tsurf"] - base[case][2]["tsurf"]).max(axis=1) > 1e-3).sum())
                o = {k: v[:64, dc.WINDOW] for k, v in ora.items()}
                snow, cold = nsa(o["snow"] > 0), nsa(o["tsurf"] < 0)
                b = base[case][2]
                differs = np.logical_or.reduce([(ora[k][:, dc.WINDOW] != b[k][:, dc.WINDOW]).any(axis=1)
                                                for k in ("snow", "ice")])
                print(f"{what}: {case}: {moved} of {N} points move by more than 1e-3 K; window rows of the first "
                      f"wavefront with (no / some / all) lanes: snow {snow}, tsurf < 0 {cold}; points whose snow or ice "
                      f"in the window differs from the uncoupled run: {int(differs.sum())}"
                      + ("" if port is None else "; ref_cpl == port"))
                assert moved >= 64, (what, case)
                if case in dc.SNOW_IN_WINDOW:
                    assert snow[1] >= 100, (what, case, snow)
                if differs.any():
                    rewound.append((what, case))
    assert rewound  # a replay really rewound a storage
    assert any(w == "coupling, 15 layers" for w, _ in rewound)


def test_the_dressings_travel_with_their_points():
    slot = sc.permutation()
    per_wave = [len(set(sc.case_of_point(slot[b:b + 64]).tolist())) for b in range(0, len(slot), 64)]
    print(f"cases per wavefront of the mixed batch: {min(per_wave)} .. {max(per_wave)}")
    assert min(per_wave) >= 5
    f, ls, ora, failed, slot = dc.batch(True, True, 15, mixed=True)
    refs = dc.references(True, True, 15)
    assert f["tair"].shape == (N * NCASES, L) and f["local_horizons"].shape == (N * NCASES, 360) and len(ls) == N * NCASES
    for s in (0, 77, 640, len(slot) - 1):
        c, i = divmod(int(slot[s]), N)
        fc, lc, oc, _, _ = refs[sc.CASES[c]]
        assert kh.same_bits(ora["tsurf"][s], oc["tsurf"][i]) and kh.same_bits(f["prec"][s], fc["prec"][i])
        assert kh.same_bits(f["local_horizons"][s], fc["local_horizons"][i])
        for name in ("lat", "lon", "sky_view", "couplingIndexI", "couplingTsurf", "InitLenI"):
            assert getattr(ls[s], name) == getattr(lc[i], name), (s, name)
    # the lanes whose coupling is off are off, the others carry the observation
    no_index, no_obs = dc.coupling_off(sc.LANE[slot % N])
    assert all((ls[s].couplingIndexI == 0) == bool(no_index[s]) for s in range(len(slot)))
    assert all((ls[s].couplingTsurf == -9999.0) == bool(no_obs[s]) for s in range(len(slot)))


def test_the_driver_dressing_is_what_it_claims():
    for sky in (False, True):
        what = f"driver, coupling{' + sky' if sky else ''}"
        base = dc.driver_reference(sky, False)["oracle"]
        d = dc.driver_reference(sky, True)
        o = d["oracle"]
        port = dc.driver_reference(sky, True, which="port")["oracle"] if dc.kind(True) != "port" else None
        n = N * NCASES
        assert not base["status"].any() and not o["status"].any()  # every case is accepted by the reference
        assert (o["missing_index"] == base["missing_index"]).all()
        il = np.array([o["local"][q].InitLenI for q in range(n)])
        ci = np.array([o["local"][q].couplingIndexI for q in range(n)])
        assert (il == 480).all() and (ci == 479).all()
        cpl_len = int(d["settings"].coupling_minutes * 60 / d["settings"].DTSecs)
        window = slice((479 - cpl_len) // 2, 479 // 2 + 1)  # kept rows (every second index) of the coupling window
        for c, case in enumerate(sc.CASES):
            r = slice(c * N, (c + 1) * N)
            for k in OUT:
                assert np.isfinite(o[k][r]).all() and (o[k][r] > -100.0).all(), (what, case, k)
                if port is not None:
                    assert kh.same_bits(o[k][r], port[k][r]), (what, case, k)
            moved = int((np.abs(o["tsurf"][r] - base["tsurf"][r]).max(axis=1) > 1e-3).sum())
            some = {k: nsa(o[k][r][:64, window] > 0)[1] for k in STORAGES}
            print(f"{what}: {case}: accepted, InitLenI 480, couplingIndexI 479, {moved} of {N} points move; kept window "
                  f"rows ({window.stop - window.start}) of the first wavefront with a storage on some but not all "
                  f"lanes: {some}")
            assert moved == N, (what, case)
            if case in dc.SNOW_IN_WINDOW:
                assert max(some.values()) >= 100, (what, case, some)
        if sky:  # the sky view acts in the driver's runs too
            acts = float(np.abs(dc.driver_reference(False, False)["oracle"]["tsurf"] - base["tsurf"]).max())
            print(f"driver, sky: Tsurf moves by up to {acts:.3f} K against the run without sky view")
            assert acts >= 0.5


# ---- fp64: every flavour against the oracle, two batches each ----------------------------------------------------

def _set_replay_mode(monkeypatch, replay):
    """As tests/test_hip_coupling.py sets them: general / lockstep - the kernel of the replay rounds;
    lockstep-collapsed: every listed point runs all its replays in the first round's launch."""
    kind, _, how = replay.partition("-")
    monkeypatch.setenv("ROADSURF_HIP_CPL_REPLAY", kind)
    if how:
        monkeypatch.setenv("ROADSURF_HIP_CPL_COLLAPSE", "1" if how == "collapsed" else "0")


REPLAYS = ("lockstep", "lockstep-collapsed", "general")
# (id, sky, coupling, layers, chunk, history score, A32 limit, replay mode)
POINT_FLAVOURS = (
    [(f"sky_{'chunks' if chunk else 'whole'}_{'score' if score else 'noscore'}", True, False, 15, chunk, score, None, None)
     for chunk in (0, CHUNK) for score in (True, False)]
    # 1 280 columns x 60 rows = 76 800 elements per stream and launch: over the limit whole and in chunks
    + [(f"sky_a64_{'chunks' if chunk else 'whole'}", True, False, 15, chunk, None, "50000", None) for chunk in (0, CHUNK)]
    + [(f"sky_12layers_{'chunks' if chunk else 'whole'}", True, False, 12, chunk, None, None, None) for chunk in (0, CHUNK)]
    + [("cpl_whole", False, True, 15, 0, None, None, None)]
    + [(f"cpl_chunks_{replay}", False, True, 15, CHUNK, None, None, replay) for replay in REPLAYS]
    + [(f"cpl_12layers_chunks_{replay}", False, True, 12, CHUNK, None, None, replay) for replay in REPLAYS]
    + [(f"cpl_sky_{nl}layers_chunks_{replay}", True, True, nl, CHUNK, None, None, replay) for nl in (15, 12)
       for replay in REPLAYS])


def _named(bad):
    return {k: [(sc.CASES[q // N], q % N) for q in v] for k, v in bad.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["crafted", "mixed"])
@pytest.mark.parametrize("fl", POINT_FLAVOURS, ids=lambda fl: fl[0])
def test_dressed_batch_equals_the_oracle(fl, mixed, monkeypatch):
    from roadsurf_amd import device
    name, sky, cpl, nl, chunk, score, a32_limit, replay = fl
    if a32_limit:
        monkeypatch.setenv("ROADSURF_HIP_A32_LIMIT", a32_limit)
    if replay:
        _set_replay_mode(monkeypatch, replay)
    f, ls, ora, failed, slot = dc.batch(sky, cpl, nl, mixed)
    got, nfail = device.run_points(f, dc.settings(cpl, nl), abi.default_parameters(), ls, chunk=chunk,
                                   history_score=score, device=0)
    got = {k: got[k] for k in OUT}
    bad = _differing(got, ora, f"{name}: {'mixed' if mixed else 'crafted'} batch", points=slot)
    first_failed = kh.first_blank(got)
    assert nfail == int((first_failed > 0).sum()) and np.array_equal(first_failed, failed)
    assert not bad, (name, _named(bad))


DRIVER_FLAVOURS = [("driver_sky_natural", True, False, "0"), ("driver_sky_plan_order", True, False, "1"),
                   ("driver_cpl", False, True, "1"), ("driver_cpl_sky", True, True, "1")]


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["crafted", "mixed"])
@pytest.mark.parametrize("fl", DRIVER_FLAVOURS, ids=lambda fl: fl[0])
def test_dressed_driver_batch_equals_its_oracle(fl, mixed, monkeypatch):
    from roadsurf_amd import driver, lib
    name, sky, coupled, cluster = fl
    monkeypatch.setenv("ROADSURF_HIP_CLUSTER", cluster)
    src, s, t0, tf, local, hz, o, slot = dc.driver_batch(sky, coupled, mixed)
    g = driver.run(src, s, abi.default_parameters(), t0, tf, local=local, horizons=hz, device=0)
    assert lib.load().rs_driver_last_raw_launches() > 0  # the raw-series instances, not the windows
    assert g["step"] == 2 and g["tsurf"].shape == (N * NCASES, (L + 1) // 2)
    assert np.array_equal(g["status"], o["status"]) and not o["status"].any()
    assert np.array_equal(g["missing_index"], o["missing_index"])
    bad = _differing({k: g[k] for k in OUT}, {k: o[k] for k in OUT}, f"{name}: {'mixed' if mixed else 'crafted'} batch",
                     points=slot)
    assert not bad, (name, _named(bad))


# ---- fp32: lane logic, limits, who carries snow and ice ------------------------------------------------------------

F32_FLAVOURS = ([(f"f32_sky_{'chunks' if chunk else 'whole'}_{'score' if score else 'noscore'}", True, False, chunk, score)
                 for chunk, score in ((0, True), (CHUNK, True), (0, False), (CHUNK, False))]
                + [("f32_cpl_whole", False, True, 0, None)])


@pytest.mark.gpu
@pytest.mark.parametrize("fl", F32_FLAVOURS, ids=lambda fl: fl[0])
def test_fp32_dressed_wave_logic_is_lane_logic(fl):
    from roadsurf_amd import device
    name, sky, cpl, chunk, score = fl
    p = abi.default_parameters()
    fc, lc, ora, _, _ = dc.batch(sky, cpl, 15, mixed=False)
    fm, lm, _, _, slot = dc.batch(sky, cpl, 15, mixed=True)
    run = lambda f, ls: device.run_points(f, dc.settings(cpl), p, ls, chunk=chunk, history_score=score, precision=32,
                                          device=0)
    crafted, nfail_c = run(fc, lc)
    mixed, nfail_m = run(fm, lm)
    assert nfail_c == 0 and nfail_m == 0
    for k in OUT:
        a, b = np.ascontiguousarray(crafted[k][slot]), np.ascontiguousarray(mixed[k])
        ndiff = int((a.view(np.int64) != b.view(np.int64)).sum())
        print(f"{name}: {k}: {ndiff} of {a.size} values differ between the crafted and the mixed order")
        assert not np.isnan(a).any() and ndiff == 0, k
    for k, hi in (("snow", p.MaxSnowmms), ("water", p.MaxWatmms), ("ice", p.MaxIcemms), ("deposit", p.MaxDepmms),
                  ("ice2", p.MaxIcemms)):
        lo_, hi_ = float(crafted[k].min()), float(crafted[k].max())
        print(f"{name}: {k}: {lo_} .. {hi_} (limit {hi})")
        assert lo_ >= 0.0 and hi_ <= hi * (1 + 1e-6), (k, lo_, hi_)
    for case in ("one_snowy", "freezing_rain_one", "heavy_snow_one"):
        rows = slice(sc.CASES.index(case) * N, (sc.CASES.index(case) + 1) * N)
        icy = lambda o: carriers(o["snow"][rows]) | carriers(o["ice"][rows]) | carriers(o["ice2"][rows])
        print(f"{name}: {case}: snow or ice on points {sorted(icy(crafted))}, by the oracle {sorted(icy(ora))}")
        assert icy(crafted) == icy(ora), case
    for line in f32_distribution(crafted, ora):
        print(f"{name}: |fp32 - fp64| {line}")


@pytest.mark.gpu
def test_fp32_chunked_coupling_stays_refused():
    from roadsurf_amd import device
    f, ls, _, _, _ = dc.references(False, True)["one_snowy"]
    with pytest.raises(RuntimeError, match="time-chunked coupling needs the fp64 flavour"):
        device.run_points(f, dc.settings(True), abi.default_parameters(), ls, chunk=CHUNK, precision=32, device=0)
