"""GPU: the device's driver data path (rs_driver_expand, rs_driver_run, rs_driver_run_kept) against the reference's
own C++ driver directly - oracle/_ref/libroadrunner_ref.so, see tests/test_driver_reference.py - on generated driver
inputs of 96 stations (a wavefront and a half).  Every comparison is bit for bit."""
import numpy as np
import pytest

import driver_ref_helpers as rh
from roadsurf_amd import driver, roadrunner

pytestmark = pytest.mark.gpu

R = rh.REJECTS
SPECS = {
    "plain": rh.Spec(seed=21, n=96, order=("fc", "obs"), rejects=R[0:7]),
    # every station of a file on one time axis: the shared-axis kernels
    "relaxation_coupling": rh.Spec(seed=22, n=96, order=("fc", "obs"), relaxation=True, coupling=True, shared=True,
                                   rejects=("no_hum", "prec_hole", "no_sw", "lw_m100", "vz_hole", "tair_m100")),
    # per-station axes, three files, the other zone, sky view and horizons, parameters
    "sky_view": rh.Spec(seed=23, n=96, zone="eet", order=("obs", "fc", "obs2"), relaxation=True, coupling=True,
                        sky="both", params=True, step=20, rejects=R[4:11]),
    "dt45": rh.Spec(seed=24, n=96, order=("fc", "obs"), coupling=True, dtsecs=45, rejects=R[0:6]),
    "dt90": rh.Spec(seed=25, n=96, zone="eet", order=("obs", "fc"), coupling=True, dtsecs=90, step=15,
                    rejects=R[6:12]),
}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """name -> the files, the reference's read_input and run, and roadrunner.prepare's view; made on first use."""
    rh.require_reference()
    made = {}

    def get(name):
        if name not in made:
            spec = SPECS[name]
            tmp = tmp_path_factory.mktemp(name)
            with rh.timezone(rh.ZONES[spec.zone][0]):
                case = rh.make_case(tmp, spec)
                ref = rh.reference_view(case)
                run = rh.reference_run(case) if spec.dtsecs == 30 else None
                pc = roadrunner.prepare(case["config"], case["cli_time"])
            made[name] = {"case": case, "ref": ref, "run": run, "pc": pc}
        return made[name]
    return get


def _compare_expand(g, ref):
    n = len(ref["ids"])
    for name in driver.MERGED_FIELDS:
        bad = [k for k in range(n) if not rh.same_bits(g["merged"][name][k], ref["merged"][name][k])]
        assert not bad, (name, bad[:8])
    want = [rh.scan_status(ref["merged"], k) for k in range(n)]
    assert [(int(a), int(b)) for a, b in zip(g["status"], g["missing_index"])] == want
    assert np.array_equal(g["status"] == 0, ref["success"])
    mine = rh.local_fields(g["local"])
    for name in rh.LOCAL_INTS:
        assert np.array_equal(mine[name], ref["local"][name]), name
    for name in rh.LOCAL_REALS:
        assert rh.same_bits(mine[name], ref["local"][name]), name


@pytest.mark.parametrize("name", ["relaxation_coupling", "sky_view", "plain"])
def test_expand_equals_the_reference_read_input(cases, name):
    c = cases(name)
    pc, ref = c["pc"], c["ref"]
    per_point = [np.ndim(s.times) == 2 for s in pc.sources]
    assert not any(per_point) if SPECS[name].shared else any(per_point)
    assert 0.6 * len(ref["ids"]) <= ref["success"].sum() < len(ref["ids"])
    g = driver.read_input(pc.sources, pc.settings, pc.start_time, pc.forecast_time, local=rh.copy_local(pc.local))
    _compare_expand(g, ref)


@pytest.mark.parametrize("name", ["plain", "relaxation_coupling", "sky_view"])
def test_run_config_equals_the_reference_driver(cases, name):
    """roadrunner.run_config = rs_driver_run over the files, against read_input + runsimulation of the reference at
    save_output's rows."""
    c = cases(name)
    ref, want = c["ref"], c["run"]
    with rh.timezone(c["case"]["tz"]):
        res = roadrunner.run_config(c["case"]["config"], c["case"]["cli_time"])
    step = int(ref["settings"]["outputStep"] * 60 / ref["settings"]["DTSecs"])
    assert res["step"] == step
    assert np.array_equal(res["status"] == 0, want["success"]) and want["success"].sum() >= 50
    for k in driver.OUT_FIELDS:
        assert rh.same_bits(res[k], want[k][:, ::step]), k
        assert np.all(res[k][~want["success"]] == -9999.0)
    # (the model itself gives up on a few accepted stations - a -99.9999 degree forecast, src/InputOutput.f90:55-67 -
    # and leaves -9999.0 from there on: those rows are compared above like any others)
    assert np.all(want["tsurf"][want["success"]][:, ::step] != -9999.0, axis=1).sum() >= 50


def test_kept_rows_and_deficit_equal_the_reference(cases):
    c = cases("relaxation_coupling")
    pc, ref, want = c["pc"], c["ref"], c["run"]
    res = driver.run(pc.sources, pc.settings, pc.params, pc.start_time, pc.forecast_time,
                     local=rh.copy_local(pc.local), cal=pc.cal, horizons=pc.horizons, kept=("tair", "tdew"),
                     deficit=True)
    step = res["step"]
    tair, tdew, tsurf = ref["merged"]["tair"][:, ::step], ref["merged"]["tdew"][:, ::step], want["tsurf"][:, ::step]
    assert rh.same_bits(res["kept"]["tair"], tair) and rh.same_bits(res["kept"]["tdew"], tdew)
    ok = (tsurf > -9000.0) & (tdew > -9000.0)  # both operands present (include/roadsurf.h, rs_driver_run_kept)
    deficit = np.where(ok, tsurf - tdew, -9999.0)
    assert ok[want["success"]].all(axis=1).sum() >= 50 and not ok[~want["success"]].any()
    assert rh.same_bits(res["deficit"], deficit)
    assert rh.same_bits(res["tsurf"], tsurf)


@pytest.mark.parametrize("name", ["dt45", "dt90"])
def test_time_steps_off_the_minute_grid_equal_the_reference_or_are_refused(cases, name):
    """DTSecs 45 and 90: minute stamps fall between simulation times and the reference's walk never moves on from the
    segment it is in.  The device equals the reference or refuses the call with a message; never a silent difference."""
    c = cases(name)
    pc, ref = c["pc"], c["ref"]
    assert ref["simlen"] == {"dt45": 481, "dt90": 241}[name]
    try:
        g = driver.read_input(pc.sources, pc.settings, pc.start_time, pc.forecast_time, local=rh.copy_local(pc.local))
    except RuntimeError as e:
        assert len(str(e)) > 20, e
        return
    _compare_expand(g, ref)
