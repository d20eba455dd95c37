"""Write a run of `python -m roadsurf_amd.roadrunner` for N synthetic stations, to time the command at scale.
usage: python tools/make_roadrunner_case.py N HOURS DIR

DIR receives example_config.json, example_forecast.json, example_observations.json, example_skyview.txt and
example_local_horizons.txt in the reference's formats.  The weather is roadsurf_amd/driver_workload.py's (the
series tools/bench_driver_path.py times) in its "skycoupling" mode: an hourly forecast from an hour before the start
to an hour behind the end (with direct short-wave and net long-wave), 10-minute observations over the first six hours
(air temperature, humidity, wind, road temperature), a sky-view factor and 360 horizon angles per station.  The
configuration's analysis is those six hours and its forecast the remaining HOURS - 6, with relaxation and coupling
on; time.now is the end of the observations.  Values are written with two decimals (horizons with one), as
station files carry them.  Run the case from DIR (the reference's file names are relative):
    cd DIR && TZ=UTC python -m roadsurf_amd.roadrunner -v example_config.json
"""
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from roadsurf_amd import driver, driver_workload  # noqa: E402

MODE = "skycoupling"


def _stamp(t):
    return time.strftime("%Y-%m-%d %H:%M", time.gmtime(int(t)))


def write_source(path, src, ids, lat, lon):
    """The reference's JSON input schema (JsonSource.cpp:206-286): one object per station."""
    names = {v: k for k, v in driver.JSON_VARIABLES.items()}
    nt = len(src.times)
    times = json.dumps([_stamp(t) for t in src.times])
    row = "[" + ", ".join(["%.2f"] * nt) + "]"
    cols = [(names[k], a.tolist()) for k, a in src.fields.items()]
    with open(path, "w") as fh:
        fh.write("[")
        for p in range(len(ids)):
            fh.write(",\n" if p else "\n")
            parts = [f'"statId": {ids[p]}, "lat": {lat[p]:.5f}, "lon": {lon[p]:.5f}, "time": {times}']
            parts += [f'"{name}": ' + row % tuple(a[p]) for name, a in cols]
            fh.write("{" + ", ".join(parts) + "}")
        fh.write("\n]\n")


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    n, hours, out = int(argv[0]), int(argv[1]), argv[2]
    if n < 1 or hours <= driver_workload.OBS_HOURS:
        raise SystemExit(f"N >= 1 and HOURS > {driver_workload.OBS_HOURS} please")
    os.makedirs(out, exist_ok=True)
    w = driver_workload.DriverWorkload(n, hours)
    fc, ob = w.sources(MODE)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # numpy guesses the struct's dtype: it guesses right
        a = np.ctypeslib.as_array(w.local(MODE))
    ids = (100000 + np.arange(n)).tolist()
    lat, lon = a["lat"].tolist(), a["lon"].tolist()
    write_source(os.path.join(out, "example_forecast.json"), fc, ids, lat, lon)
    write_source(os.path.join(out, "example_observations.json"), ob, ids, lat, lon)
    with open(os.path.join(out, "example_skyview.txt"), "w") as fh:
        for p in range(n):
            fh.write(f"{ids[p]} point{ids[p]} {lat[p]:.7f} {lon[p]:.7f} {w.sky_view[p]:.3f}\n")
    hz = w.horizons().tolist()
    row = " ".join(["%.1f"] * 360)
    with open(os.path.join(out, "example_local_horizons.txt"), "w") as fh:
        for p in range(n):
            fh.write(f"{ids[p]} point{ids[p]} {lat[p]:.7f} {lon[p]:.7f} " + row % tuple(hz[p]) + "\n")
    now = driver_workload.START + driver_workload.OBS_HOURS * 3600
    cfg = {
        "time": {"now": time.strftime("%Y%m%dT%H%M", time.gmtime(now)), "analysis": driver_workload.OBS_HOURS,
                 "forecast": hours - driver_workload.OBS_HOURS},
        "model": {"use_coupling": 1, "use_relaxation": 1, "DTSecs": 30.0},
        "parameters": {"sky_view_file": "example_skyview.txt", "local_horizon_file": "example_local_horizons.txt"},
        "output": {"step": 60, "filename": "example_output.json"},
        "input": [
            {"name": "forecast", "path": "example_forecast.json", "type": "json", "source": "forecast"},
            {"name": "observations", "path": "example_observations.json", "type": "json", "source": "observations"},
        ],
    }
    with open(os.path.join(out, "example_config.json"), "w") as fh:
        json.dump(cfg, fh, indent=4)
    mb = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) / 1e6
    print(f"{out}: {n} stations x {hours} h (time.now {cfg['time']['now']}, UTC), {mb:.0f} MB")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
