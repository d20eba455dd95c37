"""CPU: the definition of the kept input rows and the dew-point deficit (roadsurf_amd/kept.py) against a literal
per-element loop, the ctypes binding of RsDriverKept against the C header, and driver.save_output's extra keys."""
import ctypes as C
import json
import math
import os
import struct
import subprocess
import time

import numpy as np
import pytest

from roadsurf_amd import driver, kept

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _deficit_one(a: float, b: float) -> float:
    """calc_difference's rule for one pair, in plain Python floats (IEEE doubles)"""
    if math.isnan(a) or math.isnan(b) or not a > -9000.0 or not b > -9000.0:
        return -9999.0
    return a - b


@pytest.mark.parametrize("step", [1, 2, 14, 120, 5000])
def test_kept_rows_against_a_loop(step):
    rs = np.random.RandomState(step)
    m = rs.uniform(-30, 30, (3, 5, 1441))
    got = kept.kept_rows(m, step)
    n_out = (1441 + step - 1) // step
    assert got.shape == (3, 5, n_out)
    for f in range(3):
        for p in range(5):
            for r in range(n_out):
                assert struct.pack("d", got[f, p, r]) == struct.pack("d", m[f, p, r * step])
    assert kept.kept_rows(m[0, 0], step).shape == (n_out,)
    with pytest.raises(ValueError):
        kept.kept_rows(m, 0)


def test_fields_are_the_drivers():
    assert kept.FIELDS == driver.MERGED_FIELDS and len(kept.FIELDS) == 10


def test_deficit_against_a_loop():
    rs = np.random.RandomState(5)
    a = rs.uniform(-40, 40, (7, 13))
    b = rs.uniform(-40, 40, (7, 13))
    special = (np.nan, -9999.0, -9999.9, -9000.0, -0.0, 0.0, np.inf, -np.inf, np.nextafter(-9000.0, 0.0))
    for k, v in enumerate(special):
        a[k % 7, k] = v
        b[(k + 3) % 7, 12 - k] = v
    a[6, 6] = b[6, 6] = np.inf
    got = kept.dew_point_deficit(a, b)
    assert got.dtype == np.float64 and got.shape == a.shape
    want = np.array([[_deficit_one(float(a[i, j]), float(b[i, j])) for j in range(13)] for i in range(7)])
    assert _same_bits(got, want)
    assert np.isnan(got[6, 6]) and (got == -9999.0).any() and (got > 0).any() and (got < 0).any()
    # float32 operands are widened exactly; the operands are not written
    a0, b0 = a.copy(), b.copy()
    kept.dew_point_deficit(a, b)
    assert _same_bits(a, a0) and _same_bits(b, b0)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    assert _same_bits(kept.dew_point_deficit(a32, b32), kept.dew_point_deficit(a32.astype(np.float64), b32.astype(np.float64)))


OPERANDS = [
    # tsurf, tdew, deficit
    (np.nan, -3.0, -9999.0),                # NaN in either operand
    (1.5, np.nan, -9999.0),
    (np.nan, np.nan, -9999.0),
    (-9999.0, -3.0, -9999.0),               # Tsurf = -9999.0: a row the simulation never saved, a rejected point
    (1.5, -9999.9, -9999.0),                # tdew = -9999.9: the missing input
    (-9000.0, -3.0, -9999.0),               # exactly -9000.0 is missing HERE (is_missing would keep it)
    (1.5, -9000.0, -9999.0),
    (np.nextafter(-9000.0, 0.0), 0.0, np.nextafter(-9000.0, 0.0)),   # ... and the next double above it is not
    (-0.0, 0.0, -0.0 - 0.0),                # -0.0 - 0.0 = -0.0
    (0.0, -0.0, 0.0),
    (-0.0, -0.0, 0.0),                      # -0.0 - -0.0 = +0.0
    (2.25, 2.25, 0.0),
    (np.inf, -3.0, np.inf),                 # +inf is above the threshold: an operand like any other
    (1.5, np.inf, -np.inf),
    (np.inf, np.inf, np.nan),
    (-np.inf, -3.0, -9999.0),               # -inf is not above it
    (1.5, -np.inf, -9999.0),
    (-1.25, 0.5, -1.75),
    (0.1, 0.3, 0.1 - 0.3),                  # one rounding, that of the subtraction
]


@pytest.mark.parametrize("tsurf,tdew,want", OPERANDS)
def test_deficit_operand_cases(tsurf, tdew, want):
    got = kept.dew_point_deficit(np.array([tsurf]), np.array([tdew]))
    if math.isnan(want):
        assert math.isnan(got[0])
    else:
        assert struct.pack("d", got[0]) == struct.pack("d", want), (tsurf, tdew, got[0])
    assert _same_bits(got, [_deficit_one(tsurf, tdew)])
    # scalars work too
    assert _same_bits(kept.dew_point_deficit(tsurf, tdew), np.float64(_deficit_one(tsurf, tdew)))


def test_struct_layout_against_the_header(tmp_path):
    """sizeof / offsetof of RsDriverKept as a C compiler sees include/roadsurf.h = the ctypes binding's"""
    src = tmp_path / "kept_layout.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n"
        f'#include "{ROOT}/include/roadsurf.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %zu %zu %zu\\n", sizeof(RsDriverKept), offsetof(RsDriverKept, merged), offsetof(RsDriverKept, deficit),\n'
        "         sizeof(((RsDriverKept *)0)->merged) / sizeof(((RsDriverKept *)0)->merged[0]), sizeof(((RsDriverKept *)0)->merged[0]));\n"
        "  return 0;\n}\n")
    exe = tmp_path / "kept_layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    size, off_merged, off_deficit, count, elem = (int(x) for x in out)
    K = driver.RsDriverKept
    assert C.sizeof(K) == size == 88
    assert K.merged.offset == off_merged == 0 and K.deficit.offset == off_deficit == 80
    assert count == len(driver.MERGED_FIELDS) == len(kept.FIELDS) == 10 and elem == C.sizeof(C.c_void_p)
    assert K.merged.size == count * elem and K.deficit.size == elem


def _result(n, n_out, seed=1):
    rs = np.random.RandomState(seed)
    res = {k: rs.uniform(-5, 5, (n, n_out)) for k in driver.OUT_FIELDS}
    res["status"] = np.zeros(n, np.int32)
    res["status"][1] = 3
    res["step"] = 40
    return res


def test_save_output_extra_keys(tmp_path):
    n, n_out = 4, 5
    res = _result(n, n_out)
    ids, lats, lons = [11, 12, 13, 14], [60.0, 61.5, 62.0, 63.25], [24.0, 25.0, 26.5, 27.0]
    t0 = 1704844800
    # what the file has always held, restated
    tstr = [time.strftime("%Y-%m-%dT%H:%M", time.gmtime(t0 + r * 40 * 30)) for r in range(n_out)]
    today = [{"statId": ids[p], "lat": lats[p], "lon": lons[p], "time": tstr,
              "RoadTemperature": res["tsurf"][p].tolist(), "Water": res["water"][p].tolist(),
              "Ice": res["ice"][p].tolist(), "Snow": res["snow"][p].tolist(), "Deposit": res["deposit"][p].tolist()}
             for p in range(n) if p != 1]
    plain = tmp_path / "plain.json"
    driver.save_output(str(plain), res, ids, lats, lons, t0, 30)
    assert plain.read_bytes() == json.dumps(today, indent=3).encode()
    none = tmp_path / "none.json"
    driver.save_output(str(none), res, ids, lats, lons, t0, 30, extra=None)
    assert none.read_bytes() == plain.read_bytes()
    rs = np.random.RandomState(2)
    tair, tdew = rs.uniform(-5, 5, (n, n_out)), rs.uniform(-8, 2, (n, n_out))
    tdew[2, 3] = -9999.9
    extra = {"tair": tair, "tdew": tdew, "deficit": kept.dew_point_deficit(res["tsurf"], tdew)}
    full = tmp_path / "full.json"
    driver.save_output(str(full), res, ids, lats, lons, t0, 30, extra=extra)
    got = json.loads(full.read_text())
    assert [g["statId"] for g in got] == [11, 13, 14]
    for g, p in zip(got, (0, 2, 3)):
        assert list(g)[-3:] == ["AirTemperature", "DewPoint", "DewPointDeficit"]
        assert g["AirTemperature"] == tair[p].tolist() and g["DewPoint"] == tdew[p].tolist()
        assert g["DewPointDeficit"] == extra["deficit"][p].tolist()
        for k in ("AirTemperature", "DewPoint", "DewPointDeficit"):
            del g[k]
    assert got == json.loads(plain.read_text())
    assert json.loads(full.read_text())[1]["DewPointDeficit"][3] == -9999.0
