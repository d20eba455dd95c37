"""GPU: the shortcuts rs_physics_body.inc takes when all 64 lanes of a wavefront agree on a storage, on the
precipitation or on a layer's frost - the bare road's storage block (RS_BARE_FAST), `snow_here`, `ice_here`, the dry
index (RS_PREC_FAST), the per-layer frozen / mixed / thawed split - and the fp32 two-points-per-lane kernel's own wave
logic, on the wavefronts of tests/storage_cases.py: made by hand so that the reference decides against a mix the
kernel could get wrong.

The partner is the CPU oracle (the reference's own Fortran where it is built, the C restatement otherwise), all six
outputs at every index and the first failed index, bit for bit, through every flavour of knot_helpers.FLAVOURS.  By
tests/test_step_selection.py these shapes (15 layers, 32-bit window offsets, under 65 536 points) take
(template arguments behind the feature set - sky view, coupling, replay - are all false and left out)
  knots, window            step_kernel_duo<15, false, 1, false> and <15, false, 0, false> (run_knots leaves no score)
  variant 1  lean / full   step_kernel_reg<15, false, true, true> / <15, true, true, true>
  variant 2  lean / full   step_kernel_lds<false, false> / <true, false>
  variant 3  lean / full   step_kernel_duo<15, true, 0, false> / <15, true, 0, true>
  variant 4  lean / full   step_kernel_reg<15, false, true, true> (HYBRID has no LEAN instance) / step_kernel_hybrid
                           <true, true>
  fp32                     step_kernel_f32duo<1, false, false, false> (knots), <0, false, false, false> (window),
                           <0, true, false, false> and <0, true, true, false> (run_points lean and full)
  driver.run               step_kernel_duo<15, true, 2, true>: the raw-series instance, the same physics text
each once per case (128 points: the two crafted wavefronts) and once with all cases in one batch of 1 280 points
under a fixed permutation, so that every wavefront mixes lanes of different cases; the oracle is per point, its rows
are permuted with the points.

test_the_cases_are_what_they_claim needs no GPU: from the oracle's outputs alone every case must contain the
situation it is named for.

fp32 has no bit-exact partner: the crafted and the mixed batch must give every point the same bits (its wave logic is
lane logic), every storage stays within its limits, and the points that ever carry snow or ice are the oracle's.  The
distribution of |fp32 - fp64| is printed per case, not asserted (profiles/storage_waves_f32.txt keeps one run's lines).

The driver: the same knots as one hourly forecast source through driver.run.  The driver hands the model what the
reference's driver would - PrecPhase -9999 (the phase is read from Tair and Rhz), no observed surface temperature, the
sky-view radiation streams missing - not what knot_helpers.expand gives, so the partner there is
driver_helpers.oracle_run at the kept rows and the cases' names describe the forcing, not necessarily the outcome."""
import numpy as np
import pytest

import knot_helpers as kh
import storage_cases as sc
from roadsurf_amd import abi

N, L = sc.N, sc.L
OUT = kh.OUT
STORAGES = ("snow", "water", "ice", "deposit", "ice2")


@pytest.fixture(scope="module")
def refs():
    return sc.references()


@pytest.fixture(scope="module")
def batches(refs):
    return {mixed: sc.batch(mixed) for mixed in (False, True)}


# ---- what the cases contain, by the oracle (no GPU) ----------------------------------------------------------------

def nsa(m):
    """(none, some, all): the number of rows of m [lanes][rows] in which no, some but not all, and all lanes hold."""
    a, s = m.all(axis=0), m.any(axis=0)
    return int((~s).sum()), int((s & ~a).sum()), int(a.sum())


def carriers(a):
    """the points whose row of `a` is ever > 0"""
    return set(np.nonzero((a > 0).any(axis=1))[0].tolist())


def is_pos_zero(a):
    return (a == 0.0) & ~np.signbit(a)


def born(o, had_snow):
    """Rows r >= 1 in which ice > 0 appears in a wavefront whose every lane had ice = ice2 = +0.0 in row r - 1, on a
    lane that had snow (had_snow) or none in that row."""
    rows = []
    for r in range(1, o["ice"].shape[1]):
        if not (is_pos_zero(o["ice"][:, r - 1]) & is_pos_zero(o["ice2"][:, r - 1])).all():
            continue
        new = o["ice"][:, r] > 0
        if new.any() and ((o["snow"][new, r - 1] > 0) == had_snow).all():
            rows.append(r)
    return rows


def test_the_cases_are_what_they_claim(refs):
    p = abi.default_parameters()
    everyone = set(range(N))
    for case in sc.CASES:
        K, f, ora, failed = refs[case]
        assert not failed.any(), case                                                          # (e)
        for k in OUT:
            assert np.isfinite(ora[k]).all() and (ora[k] > -100.0).all(), (case, k)
        for w in range(2):
            o = {k: v[64 * w:64 * w + 64] for k, v in ora.items()}
            cold = nsa(o["tsurf"] < 0)
            bare = nsa(np.logical_and.reduce([is_pos_zero(o[k]) for k in STORAGES]))
            ice = (o["ice"] > 0) | (o["ice2"] > 0)
            print(f"{case}: wavefront {w}: rows with (no / some / all) lanes: " +
                  "; ".join(f"{k} {nsa(o[k] > 0)}" for k in STORAGES) + f"; tsurf < 0 {cold}; bare {bare}")
            if case == "one_snowy":
                assert nsa(o["snow"] > 0)[1] >= 100 and bare[1] >= 100 and bare[2] >= 10        # (b)
                rows = born(o, had_snow=True)
                print(f"{case}: wavefront {w}: ice is born from snow in an ice-free wavefront in rows {rows}")
                assert rows
            elif case == "freezing_rain_one":
                assert nsa(ice)[1] >= 100
                rows = born(o, had_snow=False)
                print(f"{case}: wavefront {w}: water freezes in an ice-free wavefront in rows {rows}")
                assert rows
            elif case == "sleet_ladder":
                assert cold[1] >= 100 and nsa(o["water"] > 0)[1] >= 100 and nsa(o["snow"] > 0)[2] >= 100
            elif case == "rain_on_snow":
                # wet snow: snow over more water than the pores hold; its melting: a lane's snow gone within a step
                # and the water grown by more than the step's rain
                d = {k: np.diff(o[k], axis=1) for k in STORAGES}
                gone = (o["snow"][:, :-1] > 0) & (o["snow"][:, 1:] == 0)
                melted = gone & (d["water"] > f["prec"][64 * w:64 * w + 64, 1:] / sc.SPK)
                wet = (o["snow"] > 0) & (o["water"] > p.MaxPormms)
                print(f"{case}: wavefront {w}: snow over standing water in {int(wet.sum())} lane-rows, melted at once "
                      f"on {int(melted.any(axis=1).sum())} lanes, water at MaxWatmms in "
                      f"{int((o['water'] == p.MaxWatmms).sum())} lane-rows")
                assert wet.any() and melted.any() and (o["water"] == p.MaxWatmms).any()
                assert cold[1] >= 100 and nsa(o["snow"] > 0)[1] >= 100
            elif case == "melt_out":
                for k in ("snow", "water", "ice", "ice2"):
                    assert min(nsa(o[k] > 0)) >= 100, (case, k)
                assert min(cold) >= 20                                                         # (c)
            elif case in ("thaw_ramp", "minus_zero"):
                assert bare == (0, 0, L)  # every storage +0.0 in every row
                assert min(cold) >= (20 if case == "thaw_ramp" else 10) and cold[1] >= 100     # (c)
            elif case == "frost_ladder":
                others = np.logical_and.reduce([is_pos_zero(o[k]) for k in ("snow", "water", "ice", "ice2")])
                frost_only = (o["deposit"] > 0).all(axis=0) & others.all(axis=0)
                print(f"{case}: wavefront {w}: {int(frost_only.sum())} rows with deposit on every lane and every "
                      f"other storage +0.0")
                assert int(frost_only.sum()) >= 100 and bare[2] == 0 and nsa(o["snow"] > 0)[1] >= 100
                # deposit -> ice where the snow arrives: the lane's deposit is gone within a step, its ice there
                lane = np.nonzero(sc.LANE[64 * w:64 * w + 64] == sc.ONE)[0][0]
                turn = (o["deposit"][lane, :-1] > 0) & (o["deposit"][lane, 1:] == 0) & (o["ice"][lane, 1:] >
                                                                                         o["ice"][lane, :-1])
                # (the first flakes are under MinSnowmms: the snow row may still read 0 there) and snow is falling
                assert turn.any() and (f["prec"][64 * w + lane, 1:][turn] > 0).all()
                assert (f["precphase"][64 * w + lane, 1:][turn] == 3).all()
            elif case == "odd_prec":
                wet_lanes = nsa(f["prec"][64 * w:64 * w + 64] != 0.0)
                print(f"{case}: wavefront {w}: indices with (no / some / all) lanes' precipitation not +-0: {wet_lanes}")
                if w == 0:
                    assert wet_lanes[1] >= 100
                else:
                    assert wet_lanes == (L, 0, 0) and bare == (0, 0, L)
            elif case == "heavy_snow_one":
                assert nsa(o["snow"] > 0)[1] >= 100
                drops = int((np.diff(o["snow"], axis=1) < -40.0).sum())
                print(f"{case}: wavefront {w}: {drops} drops of snow by more than 40 mm in a step, "
                      f"{int((o['ice'] == p.MaxIcemms).sum())} lane-rows with ice at MaxIcemms")
                assert drops >= 1 and (o["ice"] == p.MaxIcemms).any() and o["snow"].max() > 0.99 * p.MaxSnowmms  # (d)
        # (a) the named lanes, and only they, carry the named storage
        one = set(sc.points_of(sc.ONE).tolist())
        if case == "one_snowy":
            assert carriers(ora["snow"]) == carriers(ora["ice"]) == carriers(ora["ice2"]) == one
            assert not carriers(ora["water"]) and not carriers(ora["deposit"])
        elif case == "freezing_rain_one":
            assert carriers(ora["ice"]) == carriers(ora["ice2"]) == one
            assert is_pos_zero(ora["water"]).all() and not carriers(ora["snow"]) and not carriers(ora["deposit"])
        elif case in ("sleet_ladder", "melt_out", "rain_on_snow"):
            assert carriers(ora["snow"]) == everyone
            if case == "sleet_ladder":
                assert 0 < len(carriers(ora["water"])) < N
        elif case == "frost_ladder":
            assert carriers(ora["deposit"]) == everyone and carriers(ora["snow"]) == carriers(ora["ice"]) == one
        elif case == "odd_prec":
            lanes = {sc.ODD["phase7"], sc.ODD["phase_auto"]}  # (points of the first wavefront)
            assert carriers(ora["snow"]) == carriers(ora["ice"]) == lanes
            rest = np.delete(np.arange(N), sorted(lanes))
            assert all(is_pos_zero(ora[k][rest]).all() for k in STORAGES)
            # (-0.0 at the knots' own indices; -0.0 + r * 0.0 / spk is +0.0 between them)
            assert np.signbit(f["prec"][sc.ODD["minus_zero"], ::sc.SPK]).all() and (f["prec"][sc.ODD["minus_zero"]] == 0).all()
            assert (f["prec"][sc.ODD["negative"]] == -0.05).all()
            assert (0 < f["prec"][sc.ODD["tiny"]]).all() and (f["prec"][sc.ODD["tiny"]] / sc.SPK < p.MinPrecmm).all()
        elif case == "heavy_snow_one":
            assert carriers(ora["snow"]) == carriers(ora["ice"]) == set(sc.points_of(sc.HEAVY_60, sc.HEAVY_99).tolist())
        elif case == "minus_zero":
            neg, pos = sc.points_of(sc.MZ_NEG), sc.points_of(sc.MZ_POS)
            assert np.signbit(f["tair"][neg][:, ::sc.SPK]).all() and (f["tair"][neg] == 0).all()
            assert is_pos_zero(f["tair"][pos]).all()
            assert np.signbit(f["tsurfobs"][neg, 0]).all() and is_pos_zero(f["tsurfobs"][pos, 0]).all()


def test_every_wavefront_of_the_mixed_batch_mixes_cases(batches):
    K, f, ora, failed, slot = batches[True]
    assert sorted(slot.tolist()) == list(range(N * len(sc.CASES)))
    per_wave = [len(set(sc.case_of_point(slot[b:b + 64]).tolist())) for b in range(0, len(slot), 64)]
    print(f"cases per wavefront of the mixed batch: {min(per_wave)} .. {max(per_wave)}")
    assert min(per_wave) >= 5
    # the rows went with the points
    refs = sc.references()
    for s in (0, 77, 640, len(slot) - 1):
        c, i = divmod(int(slot[s]), N)
        assert kh.same_bits(ora["tsurf"][s], refs[sc.CASES[c]][2]["tsurf"][i])
        assert kh.same_bits(K["prec"][s], refs[sc.CASES[c]][0]["prec"][i])


# ---- fp64: every flavour against the oracle ----------------------------------------------------------------------

def _differing(got, ora, what, points=None):
    """Prints, per output, how many points differ from the oracle in their bits; returns them."""
    bad_all = {}
    for k in OUT:
        assert got[k].shape == ora[k].shape and got[k].dtype == ora[k].dtype, (what, k)
        bad = np.nonzero((got[k].view(np.int64) != ora[k].view(np.int64)).any(axis=1))[0]
        nval = int((got[k].view(np.int64) != ora[k].view(np.int64)).sum())
        print(f"{what}: {k}: {nval} values in {len(bad)} of {got[k].shape[0]} points differ from the oracle in their bits")
        if len(bad):
            bad_all[k] = (bad if points is None else points[bad])[:8].tolist()
    return bad_all


def _run(fl, K, f, precision=64):
    return kh.run_flavour(fl, K, f, sc.settings(), abi.default_parameters(), sc.local(), start_hour=sc.START_HOUR,
                          precision=precision)


@pytest.mark.gpu
@pytest.mark.parametrize("fl", kh.FLAVOURS, ids=kh.flavour_id)
@pytest.mark.parametrize("case", sc.CASES)
def test_case_equals_the_oracle(refs, case, fl):
    K, f, ora, failed = refs[case]
    got, first_failed = _run(fl, K, f)
    bad = _differing(got, ora, f"{kh.flavour_id(fl)}: {case}")
    assert np.array_equal(first_failed, failed), (first_failed.nonzero(), failed.nonzero())
    assert not bad, (case, fl, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("fl", kh.FLAVOURS, ids=kh.flavour_id)
def test_mixed_batch_equals_the_oracle(batches, fl):
    K, f, ora, failed, slot = batches[True]
    got, first_failed = _run(fl, K, f)
    bad = _differing(got, ora, f"{kh.flavour_id(fl)}: mixed batch", points=slot)
    assert np.array_equal(first_failed, failed)
    assert not bad, (fl, {k: [(sc.CASES[q // N], q % N) for q in v] for k, v in bad.items()})


# ---- fp32: lane logic, limits, who carries snow and ice ------------------------------------------------------------

def f32_distribution(got, ora):
    """Per case and output: |fp32 - fp64| over the case's 128 x 721 values (crafted batch)."""
    lines = []
    for c, case in enumerate(sc.CASES):
        for k in OUT:
            d = np.abs(got[k][c * N:(c + 1) * N].astype(np.float64) - ora[k][c * N:(c + 1) * N])
            q = np.quantile(d, [0.5, 0.99, 0.999])
            lines.append(f"{case:18s} {k:8s} median {q[0]:.3e}  99 % {q[1]:.3e}  99.9 % {q[2]:.3e}  max {d.max():.3e}"
                         f"  over 0.05: {int((d > 0.05).sum())} of {d.size}")
    return lines


@pytest.mark.gpu
@pytest.mark.parametrize("fl", kh.FLAVOURS_F32, ids=kh.flavour_id)
def test_fp32_wave_logic_is_lane_logic(batches, fl):
    p = abi.default_parameters()
    Kc, fc, ora, failed, _ = batches[False]
    Km, fm, _, _, slot = batches[True]
    crafted, failed_c = _run(fl, Kc, fc, precision=32)
    mixed, failed_m = _run(fl, Km, fm, precision=32)
    assert not failed_c.any() and not failed_m.any()
    for k in OUT:
        a, b = np.ascontiguousarray(crafted[k][slot]), np.ascontiguousarray(mixed[k])
        it = {4: np.int32, 8: np.int64}[a.itemsize]
        ndiff = int((a.view(it) != b.view(it)).sum())
        print(f"fp32 {kh.flavour_id(fl)}: {k}: {ndiff} of {a.size} values differ between the crafted and the mixed order")
        assert not np.isnan(a).any() and ndiff == 0, k
    for k, hi in (("snow", p.MaxSnowmms), ("water", p.MaxWatmms), ("ice", p.MaxIcemms), ("deposit", p.MaxDepmms),
                  ("ice2", p.MaxIcemms)):
        lo_, hi_ = float(crafted[k].min()), float(crafted[k].max())
        print(f"fp32 {kh.flavour_id(fl)}: {k}: {lo_} .. {hi_} (limit {hi})")
        assert lo_ >= 0.0 and hi_ <= hi * (1 + 1e-6), (k, lo_, hi_)
    for case in ("one_snowy", "freezing_rain_one", "heavy_snow_one"):
        rows = slice(sc.CASES.index(case) * N, (sc.CASES.index(case) + 1) * N)
        icy = lambda o: carriers(o["snow"][rows]) | carriers(o["ice"][rows]) | carriers(o["ice2"][rows])
        print(f"fp32 {kh.flavour_id(fl)}: {case}: snow or ice on points {sorted(icy(crafted))}, "
              f"by the oracle {sorted(icy(ora))}")
        assert icy(crafted) == icy(ora), case
    for line in f32_distribution(crafted, ora):
        print(f"fp32 {kh.flavour_id(fl)}: |fp32 - fp64| {line}")


# ---- the driver's raw-series instances -----------------------------------------------------------------------------

DRIVER_CASES = ("one_snowy", "melt_out", "thaw_ramp", "heavy_snow_one")
RAW_NAMES = ("tair", "rhz", "vz", "prec", "sw", "lw")


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["plan_order", "natural"])
@pytest.mark.parametrize("case", DRIVER_CASES)
def test_driver_raw_series_equals_its_oracle(case, order, monkeypatch):
    import driver_helpers as dh
    import oracle_helpers as oh
    from roadsurf_amd import driver, lib
    monkeypatch.setenv("ROADSURF_HIP_CLUSTER", "1" if order == "plan_order" else "0")
    K = sc.knots_of(case)
    t0 = dh.START + sc.START_HOUR * 3600
    # (the last knot once more an hour behind the end: the reference's interpolation leaves an index ON the last raw
    # time missing)
    src = [driver.RawSource(t0 + 3600 * np.arange(sc.NK + 1, dtype=np.int64),
                            {k: np.ascontiguousarray(np.concatenate([K[k], K[k][:, -1:]], axis=1), np.float64)
                             for k in RAW_NAMES}, False)]
    s = sc.settings()
    s.outputStep = 1  # every second index is kept
    p = abi.default_parameters()
    o = dh.oracle_run("ref" if oh.have_ref() else "port", src, s, p, t0, t0)
    g = driver.run(src, s, p, t0, t0, device=0)
    assert lib.load().rs_driver_last_raw_launches() > 0  # the raw-series instance, not the windows
    assert g["step"] == o["step"] == 2 and g["tsurf"].shape == (N, (L + 1) // 2)
    assert np.array_equal(g["status"], o["status"]) and not o["status"].any()
    assert np.array_equal(g["missing_index"], o["missing_index"])
    bad = _differing({k: g[k] for k in OUT}, {k: o[k] for k in OUT}, f"driver, {order}: {case}")
    assert not bad, (case, bad)
    assert (o["tsurf"] > -100.0).all()
