"""GPU: the boundary-layer loop without the stability correction of its exit pass, and the air's vapour pressure made
where a wavefront needs it (rs_physics_body.inc, DRY TAIL: THE LAST PASS, EAIR ON DEMAND) against the reference oracle.

The partner is the CPU oracle (the reference's own Fortran where it is built, the C restatement otherwise), all six
outputs at every index and the first failed index, bit for bit.  128 points x 6 h (721 indices), hand-made hourly
knots, parameters (but for `rough`) and settings at their defaults, through variant 3 (the knot-reading two-wavefront kernel, launches
of 60 indices, natural order: the wavefronts stay as they are made here) and variant 1 (one point per lane).

  unstable_dry  every lane dry and warmer than the air by day: the skip fires at every step, no lane's final
                correction is evaluated and the air's vapour pressure is never formed
  ladder        night, wind under the calm limit, the surface 5 to 30 K above the air across the lanes: the final Stab
                lies on both sides of stabSafe (rs_consts_dev.h) inside one wavefront - the correction runs for the
                wavefront and the tail with it, while the reference still zeroes every le
  mixed_regime  night, wind at the calm limit, dry lanes within +-0.5 K of the air at 30 % humidity: stable and
                unstable exits in one wavefront, stage 1 of the dry tail without stage 2, lanes that leave the loop at
                different passes, one of them in the slow band of the stable side (Tsurf - Tair ~ -2.6 VZ^2)
  one_wet       `unstable_dry` with rain on one lane around the second hour: the wavefront's tail is alive and the
                final correction runs for all its lanes
  condense      air 3 K warmer than the surface at 95 % humidity: le < 0, nothing dead
  nan_rh        `unstable_dry` with one lane's relative humidity NaN at one knot: the compiled reference's
                Min((0.01*Rhz), 1.0) returns the 1.0 and the lane computes what its dry twin computes (the C
                restatement keeps the NaN instead: this case holds against the reference's own Fortran)
  rough         `ladder` on the parameter set of tests/param_helpers.py with the smallest logMom = log((ZRefW + ZMom)
                /ZMom) among its first forty draws (ROUGH_SEED: 2.14 against the default 3.26, stabSafe -0.88): the
                oracle stays finite, lanes sit on both sides of stabSafe, the hottest run out of passes (RS_BL_MAXIT)
                and logMom + PSIM comes down to 0.43 of logMom - no band of param_helpers reaches a non-positive raNum
The second wavefront of every case repeats the first with the lanes reversed.

test_the_cases_are_what_they_claim needs no GPU: a plain numpy restatement of the loop on the oracle's own surface
temperatures classifies every lane-step, and every case must contain the situation it is named for.

Then the points' independence of their wavefront: 1 024 points x 12 h of the bench workload, plan order against
natural order, each flavour against itself."""
import numpy as np
import pytest

import knot_helpers as kh
import oracle_helpers as oh
import param_helpers as ph
from roadsurf_amd import abi

SPK = 120
N, NK, L, CHUNK = 128, 7, 721, 60
OUT = oh.F64_OUT
CASES = ("unstable_dry", "ladder", "mixed_regime", "one_wet", "condense", "nan_rh", "rough")
WET_LANE, NAN_LANE = 17, 5
NIGHT_START, DAY_START = 22, 9  # 22:00 - 04:00 lies in the default night (NightOn 19, NightOff 4); 09:00 - 15:00 by day
ROUGH_SEED = 17


def _local():
    l = abi.default_local(); l.InitLenI = 1
    return l


def start_hour_of(case):
    return NIGHT_START if case in ("ladder", "mixed_regime", "rough") else DAY_START


def params_of(case):
    return ph.draw(ROUGH_SEED) if case == "rough" else abi.default_parameters()


def knots_of(case):
    """knots [N][NK] per field (+ phase, tsurf0 [N])"""
    lane = np.concatenate([np.arange(64), np.arange(64)[::-1]]).astype(np.float64)
    col = lambda v: np.repeat(np.asarray(v, np.float64)[:, None], NK, axis=1)
    K = {"tair": col(5.0 + 0.01 * lane), "tdew": col(np.full(N, -5.0)), "vz": col(3.0 + 0.02 * lane),
         "rhz": col(np.full(N, 30.0)), "prec": np.zeros((N, NK)), "sw": col(np.full(N, 400.0)),
         "lw": col(np.full(N, 300.0)), "phase": np.ones((N, NK), np.int32)}
    K["tsurf0"] = 10.0 + 0.02 * lane
    if case in ("ladder", "rough"):
        K["tair"] = col(np.full(N, -20.0))
        K["tdew"] = col(np.full(N, -30.0))
        K["vz"] = col(np.full(N, 0.3))  # under the night's calm limit (0.4 m/s by default): the limit is the wind
        K["tsurf0"] = -20.0 + 5.0 + 25.0 * lane / 63.0
        K["sw"] = np.zeros((N, NK))
        K["lw"] = col(np.full(N, 220.0))
    elif case == "mixed_regime":
        K["tair"] = col(np.full(N, 2.0))
        K["vz"] = col(np.full(N, 0.4))
        K["tsurf0"] = 2.0 + (lane - 31.5) / 63.0  # -0.5 .. +0.5 K about the air
        K["sw"] = np.zeros((N, NK))
        K["lw"] = col(260.0 + 1.2 * lane)  # lanes drift apart: cooling below, warming above the air
    elif case == "one_wet":
        K["prec"][WET_LANE, 1:3] = 0.5
        K["prec"][64 + WET_LANE, 1:3] = 0.5
    elif case == "condense":
        K["tair"] = col(-2.0 + 0.01 * lane)
        K["tsurf0"] = K["tair"][:, 0] - 3.0
        K["rhz"] = col(np.full(N, 95.0))
        K["sw"] = np.zeros((N, NK))
        K["lw"] = col(np.full(N, 250.0))
    elif case == "nan_rh":
        K["rhz"][NAN_LANE, 2] = np.nan
    else:
        assert case == "unstable_dry"
    return {k: np.ascontiguousarray(v) for k, v in K.items()}


def reference_of(case):
    """(knots, expanded forcing, oracle outputs [N][L], first failed index [N])"""
    K = knots_of(case)
    f = kh.expand(K, L, SPK, start_hour=start_hour_of(case))
    ora, failed = kh.reference(f, abi.default_settings(L), params_of(case), _local())
    return K, f, ora, failed


@pytest.fixture(scope="module")
def references():
    return {case: reference_of(case) for case in CASES}


def _compare(case, got, ora, what):
    for k in OUT:
        bad = [i for i in range(N)
               if not kh.same_bits(got[k][i], ora[k][i], nan_equal=(case == "nan_rh" and i == NAN_LANE))]
        print(f"{what}: {case}: {k}: {len(bad)} of {N} points differ from the oracle in their bits")
        assert not bad, (what, case, k, bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_knot_reading_two_wavefront_kernel_equals_the_oracle(references, case):
    K, f, ora, failed = references[case]
    res = kh.run_knots(K, abi.default_settings(L), params_of(case), _local(), chunks=CHUNK, order="natural",
                       start_hour=start_hour_of(case))
    assert res["moved"] == 0
    assert np.array_equal(res["first_failed"], failed), (res["first_failed"].nonzero(), failed.nonzero())
    _compare(case, res["out"], ora, "two wavefronts")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_one_point_per_lane_kernel_equals_the_oracle(references, case):
    from roadsurf_amd import device
    K, f, ora, failed = references[case]
    got, nfail = device.run_points(f, abi.default_settings(L), params_of(case), _local(), chunk=CHUNK,
                                   variant=1, device=0)
    assert nfail == int((failed > 0).sum())
    _compare(case, got, ora, "one point per lane")


OTHER_FLAVOURS = [fl for fl in kh.FLAVOURS if fl not in (("knots",), ("points", 1, True, True))]  # (the two above)


@pytest.mark.gpu
@pytest.mark.parametrize("fl", OTHER_FLAVOURS, ids=kh.flavour_id)
def test_every_other_flavour_equals_the_oracle(references, fl):
    """The same cases through the flavours of knot_helpers.FLAVOURS that the two tests above do not reach: the
    window-reading two-wavefront launch, and run_points with every variant, LEAN and FULL, whole and in launches."""
    for case in CASES:
        K, f, ora, failed = references[case]
        got, first_failed = kh.run_flavour(fl, K, f, abi.default_settings(L), params_of(case), _local(),
                                           start_hour=start_hour_of(case))
        assert np.array_equal(first_failed, failed), (case, first_failed.nonzero(), failed.nonzero())
        _compare(case, got, ora, kh.flavour_id(fl))


# ---- what the cases contain: the loop restated in numpy (no GPU) --------------------------------------------------

def stab_safe(p):
    """rs_consts_dev.h rs_stab_safe on the logarithms of the parameter set"""
    log_mom, log_heat = np.log((p.ZRefW + p.ZMom) / p.ZMom), np.log((p.ZRefW + p.ZHeat) / p.ZHeat)
    sq = 2.0 * np.exp(min(log_heat / 2.0, log_mom / 1.2) / 2.0) - 1.0
    return (1.0 - sq * sq) / 16.0


def classify(case, f, ora):
    """Per lane-step [N][L-1] of the step from index i to i+1 (the oracle's row i is the surface the step starts from):
    the loop's trip count, its final Stab, raNum from the final correction, and the dry-tail tests' inputs.  Plain
    double arithmetic: a classification with margins, not a bit-exact restatement."""
    p = params_of(case)
    vk = p.VK_Const
    log_mom, log_heat = np.log((p.ZRefW + p.ZMom) / p.ZMom), np.log((p.ZRefW + p.ZHeat) / p.ZHeat)
    log_ustar = np.log((p.ZRefW - p.ZeroDisp + p.ZMom) / p.ZMom)
    log_cond = np.log((p.ZRefW - p.ZeroDisp + p.ZHeat) / p.ZHeat)
    sl = slice(1, L)
    tsurf, tair, rhz = ora["tsurf"][:, :-1], f["tair"][:, sl], f["rhz"][:, sl]
    hour = np.asarray(f["hour"]).reshape(-1)[sl][None, :] if np.asarray(f["hour"]).ndim == 1 else np.asarray(f["hour"])[:, sl]
    night = (hour >= p.NightOn) | (hour <= p.NightOff)
    vz = np.maximum(f["vz"][:, sl], np.where(night, p.CalmLimNgt, p.CalmLimDay))
    tak = tair + 273.15
    avc = (1005.0 + (tak - 250.0) ** 2 / 3364.0) * (100000.0 / (287.05 * tak))
    den0, d_t = avc * tak, tsurf - tair
    psim, psih, bl = np.zeros_like(tair), np.zeros_like(tair), np.zeros_like(tair)
    stab, trips = np.zeros_like(tair), np.full(tair.shape, 41)
    live = np.ones(tair.shape, bool)
    with np.errstate(all="ignore"):
        for j in range(1, 41):
            ustar = vk * vz / (log_ustar + psim)
            bl_new = avc * vk * ustar / (log_cond + psih)
            st = np.minimum(-vk * p.ZRefT * p.Grav * bl_new * d_t / (den0 * ustar ** 3), 1.0)
            h = np.where(st > 0, 4.7 * st, -2.0 * np.log((1.0 + np.sqrt(1.0 - 16.0 * np.minimum(st, 0.0))) / 2.0))
            m = np.where(st > 0, h, 0.6 * h)
            done = live & (j >= 5) & (np.abs(bl_new - bl) < 0.001)
            stab, psim, psih, bl = (np.where(live, a, b) for a, b in ((st, stab), (m, psim), (h, psih), (bl_new, bl)))
            trips = np.where(done, j, trips)
            live &= ~done
        e = lambda t: 0.61078 * np.exp(np.where(t < 0, 21.875, 17.269) * t / (t + np.where(t < 0, 265.5, 237.3)))
        e_air = np.fmin(0.01 * rhz, 1.0) * e(tair)
        n_le = avc * (e(tsurf) - e_air)
    wat = ora["water"][:, :-1] + f["prec"][:, sl] / SPK  # (prec / 3600 x DTSecs; every case rains as rain, if at all)
    dry = wat <= 0.0
    return dict(trips=trips, stab=stab, ra_num=(log_mom + psim) * (log_heat + psih), dry=dry, n_le=n_le,
                warm=dry & (tsurf >= tair + 0.01), d_t=d_t, vz=vz, safe=stab_safe(p), log_mom=log_mom, psim=psim)


def _waves(a):
    return a[:64], a[64:]


def test_the_cases_are_what_they_claim(references):
    for case in CASES:
        K, f, ora, failed = references[case]
        assert not np.delete(failed, NAN_LANE if case == "nan_rh" else []).any(), case
        c = classify(case, f, ora)
        dead = c["warm"] | (c["dry"] & (c["n_le"] > 0))
        safe = c["safe"]
        assert -3.0 < abi_safe_default() < -2.6
        for w in range(2):
            g = {k: _waves(v)[w] for k, v in c.items() if isinstance(v, np.ndarray)}
            dd = _waves(dead)[w]
            skipped = dd.all(axis=0) & (g["stab"] > safe).all(axis=0)
            print(f"{case}: wavefront {w}: {int(skipped.sum())} of {L - 1} steps skip the final correction, "
                  f"all-warm in {int(g['warm'].all(axis=0).sum())}, dead in {int(dd.all(axis=0).sum())}; Stab "
                  f"{np.nanmin(g['stab']):.3f} .. {np.nanmax(g['stab']):.3f} (stabSafe {safe:.3f}); trips "
                  f"{g['trips'].min()} .. {g['trips'].max()}; least raNum {np.nanmin(g['ra_num']):.3f}")
            if case in ("unstable_dry", "nan_rh"):
                lanes = np.delete(np.arange(64), NAN_LANE) if (case == "nan_rh" and w == 0) else np.arange(64)
                assert g["warm"][lanes].all() and (g["stab"][lanes] < 0).all() and (g["stab"][lanes] > 0.8 * safe).all()
                assert skipped.all() or case == "nan_rh"
            elif case == "rough":
                # lanes on both sides of this set's stabSafe in one wavefront, and lanes that run out of passes
                fallback = g["warm"].all(axis=0) & (g["stab"] < safe).any(axis=0) & (g["stab"] > safe).any(axis=0)
                assert int(fallback.sum()) > 20 and not skipped[fallback].any()
                assert (g["ra_num"] > 0).all() and g["trips"].max() == 41  # (41: no exit within RS_BL_MAXIT passes)
            elif case == "ladder":
                # every lane dead by stage 2, and in one wavefront lanes at least 20 % beyond the threshold on each side
                below, above = (g["stab"] < 1.2 * safe).any(axis=0), (g["stab"] > 0.8 * safe).any(axis=0)
                both = g["warm"].all(axis=0) & below & above
                assert int(both.sum()) > 100, (case, int(both.sum()))
                assert (g["ra_num"][:, both] > 0).all()  # ... while the reference still zeroes every le
                assert not skipped[both].any()
            elif case == "mixed_regime":
                stable, unstable = (g["stab"] > 0), ~(g["stab"] > 0)
                mixed = stable.any(axis=0) & unstable.any(axis=0)
                stage1_only = dd.all(axis=0) & ~g["warm"].all(axis=0)
                spread = g["trips"].max(axis=0) > g["trips"].min(axis=0)
                assert int((mixed & stage1_only & spread & skipped).sum()) > 100
                # a lane in the slow band: many passes on the stable side, near Tsurf - Tair = -2.6 VZ^2
                slow = (g["trips"] >= 12) & stable
                assert slow.any()
                ratio = (g["d_t"] / g["vz"] ** 2)[slow]
                assert (ratio < -1.5).all() and (ratio > -4.0).all(), (ratio.min(), ratio.max())
            elif case == "one_wet":
                lane = WET_LANE  # (points WET_LANE and 64 + WET_LANE)
                wet = ~g["dry"][lane]
                assert 100 < int(wet.sum()) < 400 and np.delete(g["dry"], lane, axis=0).all()
                assert not skipped[wet].any() and skipped[~wet].all()
            elif case == "condense":
                assert (g["n_le"] < 0).all() and not dd.any() and not skipped.any()
        if case == "rough":  # how near a non-positive factor of raNum comes: (logMom + PSIM) / logMom at its least
            least = float(np.nanmin((c["log_mom"] + c["psim"]) / c["log_mom"]))
            print(f"rough: logMom {c['log_mom']:.3f}; least (logMom + PSIM)/logMom {least:.3f}")
            assert c["log_mom"] < 2.6 and least < 0.45


def abi_safe_default():
    return stab_safe(abi.default_parameters())


# ---- a point does not depend on who shares its wavefront ---------------------------------------------------------

NW, HOURS_W = 1024, 12


def _series(variant, resort):
    import torch
    from roadsurf_amd import device, workload
    Lw = HOURS_W * SPK + 1
    plan = device.Plan(NW, abi.default_settings(Lw), abi.default_parameters(), 0)
    plan.set_variant(variant)
    run = workload.SyntheticRun(plan, 2025, HOURS_W, CHUNK, point_offset=333_000, plan_order=True, resort=resort)
    out = {k: torch.full((Lw, NW), float("nan"), dtype=torch.float64, device=plan.device) for k in device.OUT_FIELDS}
    moved = []

    def on_launch(c, t0, ns):
        o = run.orders[c][:NW].long()
        moved.append(int((o != torch.arange(NW, device=plan.device)).sum()))
        for k in device.OUT_FIELDS:
            out[k][t0 - 1:t0 - 1 + ns, o] = run.out.tensors[k][:ns, :NW]

    run.run_pass(on_launch)
    plan.sync()
    assert plan.failed_count() == 0
    assert (max(moved) > 0) == resort
    res = {k: v.cpu().numpy() for k, v in out.items()}
    del run
    plan.close()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [3, 1], ids=["two_wavefronts", "one_point_per_lane"])
def test_a_point_does_not_depend_on_who_shares_its_wavefront(variant):
    natural, planned = _series(variant, False), _series(variant, True)
    assert len(natural) == 6
    for k in natural:
        assert not np.isnan(natural[k]).any() and not np.isnan(planned[k]).any(), k
        ndiff = int((natural[k].view(np.uint64) != planned[k].view(np.uint64)).sum())
        print(f"variant {variant}: {k}: {ndiff} of {natural[k].size} values differ between natural and plan order")
        assert ndiff == 0, k
    # the skip has something to skip on this workload: dry points with no water for most of the series
    assert (natural["water"] == 0.0).mean() > 0.5
