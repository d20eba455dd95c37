"""GPU: CalcLE's tail where the reference discards it (rs_physics_body.inc, DRY TAIL) against the reference oracle.

The shortcut is in the physics text that every fp64 flavour compiles, so one flavour against another proves nothing:
the partner is the CPU oracle (the reference's own Fortran where it is built, the C restatement otherwise), all six
outputs at every index, bit for bit.  128 points x 6 h (721 indices), parameters and settings at their defaults,
through variant 3 (the knot-reading two-wavefront kernel, launches of 60 indices, natural order: the wavefronts
stay as they are made here) and variant 1 (one point per lane).

The forcing is made by hand as hourly knots, so that the 64 points of a wavefront are what the skip can get wrong:
  dry        every lane dry and evaporating (sun, warm surface, dry air): both stages skip at every step
  condense   air 3 K warmer than the surface at 95 % humidity: le < 0, deposit grows, nothing to skip
  one_wet    `dry` with rain of 0.5 mm/h on one lane around the second hour: a mixed wavefront runs the full text,
             and skips again once the water is gone (the warm road evaporates each step's rain within the step: the
             water row stays 0 and the lane shows it in its temperature)
  margin     humidity 100 %, surface minus air within +-0.02 K of the second stage's 0.01 K margin at the start (lanes
             0.000625 K apart), the air then warming past the surface over six hours: every lane crosses the margin
             and then ESurf = EAir at a step of its own (by the oracle: 58 steps with lanes on both sides), dew follows
  zero       air and surface temperatures on both sides of 0 degrees within a wavefront: both Magnus branches
  nan_rh     `dry` with one lane's relative humidity NaN at one knot (two hours of NaN between its neighbours):
             CheckValues lets a NaN through, and the compiled reference's Min((0.01*Rhz), 1.0) returns the 1.0 - the
             lane computes what its dry twin computes, no point fails (the C restatement keeps the NaN instead: this
             case holds against the reference's own Fortran)
The second wavefront of every case repeats the first with the lanes reversed and the surface 0.25 K warmer.

Then the points' independence of their wavefront on a workload where the skip fires (the bench workload: 62 % of
its wave-steps are bare roads): 1 024 points x 12 h, plan order against natural order, each flavour against itself."""
import numpy as np
import pytest

import knot_helpers as kh
import oracle_helpers as oh
from roadsurf_amd import abi

pytestmark = pytest.mark.gpu
SPK = 120
N, NK, L, CHUNK = 128, 7, 721, 60
OUT = oh.F64_OUT
CASES = ("dry", "condense", "one_wet", "margin", "zero", "nan_rh")
WET_LANE, NAN_LANE = 17, 5


def _local():
    l = abi.default_local(); l.InitLenI = 1
    return l


def knots_of(case):
    """knots [N][NK] per field (+ phase, tsurf0 [N]); the clock starts at 09:00, daylight throughout"""
    lane = np.concatenate([np.arange(64), np.arange(64)[::-1]]).astype(np.float64)
    second = (np.arange(N) >= 64).astype(np.float64)
    col = lambda v: np.repeat(np.asarray(v, np.float64)[:, None], NK, axis=1)
    K = {"tair": col(5.0 + 0.01 * lane), "tdew": col(np.full(N, -5.0)), "vz": col(3.0 + 0.02 * lane),
         "rhz": col(np.full(N, 30.0)), "prec": np.zeros((N, NK)), "sw": col(np.full(N, 400.0)),
         "lw": col(np.full(N, 300.0)), "phase": np.ones((N, NK), np.int32)}
    K["tsurf0"] = 10.0 + 0.02 * lane + 0.25 * second
    if case == "condense":
        K["tair"] = col(-2.0 + 0.01 * lane)
        K["tsurf0"] = K["tair"][:, 0] - 3.0 + 0.25 * second
        K["rhz"] = col(np.full(N, 95.0))
        K["sw"] = np.zeros((N, NK))
        K["lw"] = col(np.full(N, 250.0))
    elif case == "one_wet":
        K["prec"][WET_LANE, 1:3] = 0.5
        K["prec"][64 + WET_LANE, 1:3] = 0.5
    elif case == "margin":
        m = float(np.float32(0.01))
        K["tsurf0"] = 2.0 + m + (lane - 32.0) * (4.0 * m / 64.0) + 0.25 * second
        K["tair"] = np.repeat((2.0 + np.linspace(0.0, 3.0, NK))[None, :], N, axis=0)
        K["rhz"] = col(np.full(N, 100.0))
        K["sw"] = col(np.full(N, 30.0))
        K["lw"] = col(np.full(N, 320.0))
    elif case == "zero":
        K["tair"] = col((lane - 32.0) / 64.0)  # -0.5 .. 0.484, lane 32 at 0.0
        K["tair"][31] = -0.0
        K["tsurf0"] = K["tair"][:, 0] + 0.3 + 0.25 * second
        K["rhz"] = col(np.full(N, 50.0))
        K["sw"] = col(np.full(N, 120.0))
    elif case == "nan_rh":
        K["rhz"][NAN_LANE, 2] = np.nan
    else:
        assert case == "dry"
    return {k: np.ascontiguousarray(v) for k, v in K.items()}


def reference_of(case):
    """(knots, expanded forcing, oracle outputs [N][L], first failed index [N])"""
    K = knots_of(case)
    f = kh.expand(K, L, SPK, start_hour=9)
    ora, failed = kh.reference(f, abi.default_settings(L), abi.default_parameters(), _local())
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


@pytest.mark.parametrize("case", CASES)
def test_knot_reading_two_wavefront_kernel_equals_the_oracle(references, case):
    K, f, ora, failed = references[case]
    res = kh.run_knots(K, abi.default_settings(L), abi.default_parameters(), _local(), chunks=CHUNK, order="natural",
                       start_hour=9)
    assert res["moved"] == 0
    assert np.array_equal(res["first_failed"], failed), (res["first_failed"].nonzero(), failed.nonzero())
    _compare(case, res["out"], ora, "two wavefronts")


@pytest.mark.parametrize("case", CASES)
def test_one_point_per_lane_kernel_equals_the_oracle(references, case):
    from roadsurf_amd import device
    K, f, ora, failed = references[case]
    got, nfail = device.run_points(f, abi.default_settings(L), abi.default_parameters(), _local(), chunk=CHUNK,
                                   variant=1, device=0)
    assert nfail == int((failed > 0).sum())
    _compare(case, got, ora, "one point per lane")


OTHER_FLAVOURS = [fl for fl in kh.FLAVOURS if fl not in (("knots",), ("points", 1, True, True))]  # (the two above)


@pytest.mark.parametrize("fl", OTHER_FLAVOURS, ids=kh.flavour_id)
def test_every_other_flavour_equals_the_oracle(references, fl):
    """The same cases through the flavours of knot_helpers.FLAVOURS that the two tests above do not reach: the
    window-reading two-wavefront launch, and run_points with every variant, LEAN and FULL, whole and in launches."""
    for case in CASES:
        K, f, ora, failed = references[case]
        got, first_failed = kh.run_flavour(fl, K, f, abi.default_settings(L), abi.default_parameters(), _local(),
                                           start_hour=9)
        assert np.array_equal(first_failed, failed), (case, first_failed.nonzero(), failed.nonzero())
        _compare(case, got, ora, kh.flavour_id(fl))


def test_the_cases_are_what_they_claim(references):
    """What the oracle's own outputs say about the cases: dry roads stay dry, the condensing one gathers deposit,
    the wet lane alone differs from its dry twin, the margin case has wavefronts on both sides of the margin."""
    for case in CASES:
        K, f, ora, failed = references[case]
        assert not np.delete(failed, NAN_LANE if case == "nan_rh" else []).any(), case
    assert (references["dry"][2]["water"] == 0.0).all() and (references["dry"][2]["deposit"] == 0.0).all()
    assert (references["condense"][2]["deposit"][:, -1] > 0.0).all()
    wet, dry = references["one_wet"][2]["tsurf"], references["dry"][2]["tsurf"]
    assert (wet[WET_LANE] != dry[WET_LANE]).any() and (np.delete(wet, [WET_LANE, 64 + WET_LANE], axis=0) ==
                                                       np.delete(dry, [WET_LANE, 64 + WET_LANE], axis=0)).all()
    f, ora = references["margin"][1], references["margin"][2]
    warm = (ora["tsurf"] - f["tair"])[:64] >= float(np.float32(0.01))
    assert int((warm.any(axis=0) & ~warm.all(axis=0)).sum()) > 20  # steps with lanes on both sides of the margin


# ---- a point does not depend on who shares its wavefront ---------------------------------------------------------

NW, HOURS_W = 1024, 12


def _series(variant, resort):
    import torch
    from roadsurf_amd import device, workload
    Lw = HOURS_W * SPK + 1
    plan = device.Plan(NW, abi.default_settings(Lw), abi.default_parameters(), 0)
    plan.set_variant(variant)
    run = workload.SyntheticRun(plan, 2024, HOURS_W, CHUNK, point_offset=777_000, plan_order=True, resort=resort)
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
