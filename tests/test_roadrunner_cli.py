"""GPU: `python -m roadsurf_amd.roadrunner` on the reference's operational shape, in a fresh child process, from
files only: the reference's own example_config.json (tests/golden/roadrunner_example_config.json, verbatim), the
scenario of tests/test_hip_operational.py written as the two JSON sources of that config, and the fixture's
sky-view factors and local horizons written as its two text files.  The output file must carry the reference's
outputs (tests/golden/e2e_operational.npz) bit for bit, with the reference's layout: a null entry for every
rejected station before the last accepted one."""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import driver_helpers as dh
import golden_helpers as gh
from roadsurf_amd import driver
from roadsurf_amd import roadrunner as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CONFIG = os.path.join(ROOT, "tests", "golden", "roadrunner_example_config.json")
RUN_TIMEOUT_S = 300  # a child: torch import, 401 stations parsed, one rs_driver_run of 8 881 steps, the write
JSON_NAME = {v: k for k, v in driver.JSON_VARIABLES.items()}


def _write_source(path, src, ids, lat, lon, order):
    times = np.asarray(src.times)
    assert (times % 60 == 0).all()  # the scenario's stamps are on minute boundaries: "%Y-%m-%d %H:%M" holds them
    stamps = [time.strftime("%Y-%m-%d %H:%M", time.gmtime(int(t))) for t in times]
    stations = []
    for p in order:
        st = {"statId": int(ids[p]), "lat": float(lat[p]), "lon": float(lon[p]), "time": stamps}
        for k, a in src.fields.items():
            st[JSON_NAME[k]] = a[p].tolist()
        stations.append(st)
    with open(path, "w") as fh:
        json.dump(stations, fh)  # (floats as repr: they parse back to the same doubles)


def _write_case(d, z, case):
    src, s, p, t0, tf, local, hz = dh.operational_case(z, case)
    assert (t0, tf, s.SimLen) == (dh.START, dh.START + 48 * 3600, 8881)
    n = len(z["lat"])
    ids = 100118 + 2 * np.arange(n)
    lat, lon = z["lat"], z["lon"]
    sv = [local[q].sky_view for q in range(n)]
    # source 0 in station order; the observations in reverse order, so that they are found by statId
    _write_source(os.path.join(d, "example_forecast.json"), src[0], ids, lat, lon, range(n))
    _write_source(os.path.join(d, "example_observations.json"), src[1], ids, lat, lon, range(n - 1, -1, -1))
    with open(os.path.join(d, "example_skyview.txt"), "w") as fh:
        for q in range(n - 1, -1, -1):
            fh.write(f"{ids[q]} point{ids[q]} {lat[q]!r} {lon[q]!r} {sv[q]!r}\n")
    with open(os.path.join(d, "example_local_horizons.txt"), "w") as fh:
        for q in range(n):
            fh.write(f"{ids[q]} point{ids[q]} {lat[q]!r} {lon[q]!r} " + " ".join(map(repr, hz[q].tolist())) + "\n")
    shutil.copyfile(GOLDEN_CONFIG, os.path.join(d, "example_config.json"))
    return ids


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Both cases, each through the command in a fresh child process: case -> (output, station ids)."""
    z = gh.load("e2e_operational.npz")
    env = dict(os.environ)
    env["TZ"] = "UTC"  # mktime / localtime then agree with the fixture's UTC calendar
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env.pop("ROADSURF_HIP_CLUSTER", None)  # the library's own default, as a user runs it
    out = {}
    for case in ("files", "sky"):
        d = str(tmp_path_factory.mktemp(f"roadrunner_{case}"))
        ids = _write_case(d, z, case)
        cmd = [sys.executable, "-m", "roadsurf_amd.roadrunner", "-t", "20240112T0000", "example_config.json"]
        r = subprocess.run(cmd, cwd=d, env=env, capture_output=True, text=True, timeout=RUN_TIMEOUT_S)
        print(f"[{case}] exit {r.returncode}\n{r.stdout}{r.stderr}")
        assert r.returncode == 0, r.stderr
        path = os.path.join(d, "example_output.json")
        assert os.path.exists(path)
        with open(path) as fh:
            out[case] = (json.load(fh), ids)
    return z, out


@pytest.mark.parametrize("case", ["files", "sky"])
def test_roadrunner_command_gives_the_reference_outputs(runs, case):
    z, out = runs
    got, ids = out[case]
    status = z[f"{case}_status"]
    n = len(z["lat"])
    rejected = np.nonzero(status != 0)[0]
    assert len(rejected) == 13 and status[-1] == 0  # all rejections interior: null entries, none trailing
    assert isinstance(got, list) and len(got) == n == 401
    assert [q for q, e in enumerate(got) if e is None] == rejected.tolist()
    ok = np.nonzero(status == 0)[0]
    want_times = [time.strftime("%Y-%m-%dT%H:%M", time.gmtime(dh.START + 3600 * h)) for h in range(75)]
    assert want_times[0] == "2024-01-10T00:00"
    for q in ok:
        e = got[q]
        assert e["statId"] == ids[q] and e["lat"] == z["lat"][q] and e["lon"] == z["lon"][q], q
        assert e["time"] == want_times, q
    rows = z["rows"]
    for name, k in rr.OUTPUT_FIELDS:
        a = np.array([got[q][name] for q in ok], np.float64)
        assert a.shape == (len(ok), 75)
        ref = np.ascontiguousarray(z[f"{case}_{k}"][ok])
        same = np.ascontiguousarray(a[:, rows]).view(np.int64) == ref.view(np.int64)
        assert same.all(), (case, name, int((~same).sum()), float(np.abs(a[:, rows] - ref).max()))


def test_roadrunner_command_applies_the_sky_view_files(runs):
    """As in tests/test_hip_operational.py: the sky case moves more than a third of the accepted stations."""
    z, out = runs
    ok = np.nonzero(z["files_status"] == 0)[0]
    a = np.array([out["files"][0][q]["RoadTemperature"] for q in ok])
    b = np.array([out["sky"][0][q]["RoadTemperature"] for q in ok])
    moved = (np.abs(a - b).max(1) > 1e-3).sum()
    print(f"sky view moves {moved} of {len(ok)} accepted stations")
    assert moved > len(ok) // 3
