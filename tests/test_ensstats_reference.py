"""CPU: the definition of the per-station ensemble statistics (roadsurf_amd/ensstats.py) and the host half of the
library behind them - the member table (rs_ens_member_table, csrc/rs_ens_table.hpp), which needs no device.

reduce_members is held against a plain double loop written here, against groups.reduce_groups where the two say the
same thing, and to the properties a consumer relies on; the C table builder against ensstats.member_table through
ctypes and, on its own, under AddressSanitizer + UBSan.  Every comparison is exact (-0.0 equals 0.0: which zero lands
at which rank of a sort is not part of the contract)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ensemble_helpers as eh
from roadsurf_amd import ensemble, ensstats, groups, lib, summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("tsurf", "snow", "water", "ice", "deposit", "ice2")
QUANT = (0.0, 0.1, 0.5, 0.9, 1.0)
IRREGULAR = ((np.arange(350) * 37 + 11) % 69).astype(np.int32)


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _series(n, nrows, seed):
    rs = np.random.RandomState(seed)
    d = {"tsurf": rs.normal(-1.0, 3.0, (n, nrows))}
    for k in OUT[1:]:
        d[k] = np.abs(rs.normal(0.0, 0.4, (n, nrows)))
    return d


def _loop_reference(d, group, spec):
    """The cells by a plain double loop over rows and stations: Python floats, one operation at a time."""
    n, nrows = d["tsurf"].shape
    ng = spec.ngroups
    out = np.full((nrows, ng, ensstats.RS_ENS_COLS + len(spec.quantiles)), -9999.0)
    for r in range(nrows):
        for g in range(ng):
            members = [p for p in range(n) if group[p] == g]            # ascending point index
            valid = [p for p in members if float(d["tsurf"][p, r]) != -9999.0]
            used = [p for p in valid if not math.isnan(float(d["tsurf"][p, r]))]
            k = len(used)
            out[r, g, 0], out[r, g, 1] = len(valid), k
            if k == 0:
                continue
            x = [float(d["tsurf"][p, r]) for p in used]
            s = x[0]
            for v in x[1:]:
                s = s + v
            mean = s / k
            q = (x[0] - mean) * (x[0] - mean)
            for v in x[1:]:
                dv = v - mean
                q = q + dv * dv
            out[r, g, 2], out[r, g, 3] = mean, math.sqrt(q / k)
            for c, name in enumerate(OUT[1:]):
                s = float(d[name][used[0], r])
                for p in used[1:]:
                    s = s + float(d[name][p, r])
                out[r, g, 4 + c] = s / k
            y = sorted(x)
            for j, qq in enumerate(spec.quantiles):
                h = qq * (k - 1)
                lo = int(math.floor(h))
                hi = min(lo + 1, k - 1)
                out[r, g, 9 + j] = y[lo] + (h - lo) * (y[hi] - y[lo])
    return out


def _toy():
    """4 stations with 0 / 1 / 3 / 5 members dealt over 11 points (two of them of no station), a -9999.0 member, a NaN
    Tsurf and a NaN storage."""
    group = np.array([3, 2, -1, 3, 1, 3, 2, 3, 7, 2, 3], np.int32)
    d = _series(len(group), 6, 5)
    d["tsurf"][3, 2:] = -9999.0          # station 3 loses a member from row 2 on
    d["tsurf"][6, 1] = np.nan            # a NaN Tsurf: valid, not used
    d["snow"][9, 3] = np.nan             # a NaN storage of a used member
    d["tsurf"][4, 5] = -9999.0           # station 1's only member: an empty cell at row 5
    return d, group, ensstats.EnsSpec(4, 5, QUANT)


def test_reduce_members_equals_a_plain_double_loop_on_a_toy_case():
    d, group, spec = _toy()
    assert ensstats.cols(spec) == 9 + len(QUANT)
    got = ensstats.reduce_members(*[d[k] for k in OUT], group, spec)
    want = _loop_reference(d, group, spec)
    assert got.shape == (6, 4, 14) and got.dtype == np.float64
    assert _eq(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]
    # what the toy is there for
    assert (got[:, 0, :2] == 0).all() and (got[:, 0, 2:] == -9999.0).all()           # a station without members
    assert (got[:2, 3, 0] == 5).all() and (got[2:, 3, 0] == 4).all()                 # the -9999.0 member
    assert got[1, 2, 0] == 3 and got[1, 2, 1] == 2 and not np.isnan(got[1, 2]).any()  # the NaN Tsurf is not used
    assert np.isnan(got[3, 2, 4]) and np.isnan(got[3, 2]).sum() == 1                  # the NaN snow: that mean alone
    assert (got[5, 1, :2] == 0).all() and (got[5, 1, 2:] == -9999.0).all()           # k = 0 through -9999.0
    assert got[0, 1, 3] == 0.0 and (got[0, 1, 9:] == d["tsurf"][4, 0]).all()          # one member: no spread
    # fp32 series are widened exactly
    d32 = {k: v.astype(np.float32) for k, v in d.items()}
    assert _eq(ensstats.reduce_members(*[d32[k] for k in OUT], group, spec),
               ensstats.reduce_members(*[d32[k].astype(np.float64) for k in OUT], group, spec))


def test_counts_and_extreme_quantiles_are_the_group_series():
    d, group, spec = _toy()
    big = _series(350, 9, 8)
    big["tsurf"][::17, 4:] = -9999.0
    big["tsurf"][5, 2] = np.nan
    for dd, gid, sp in ((d, group, spec), (big, IRREGULAR, ensstats.EnsSpec(70, 6, QUANT))):
        got = ensstats.reduce_members(*[dd[k] for k in OUT], gid, sp)
        grp = groups.reduce_groups(*[dd[k] for k in OUT], gid, groups.GroupSpec(summary.SummarySpec(), sp.ngroups))
        assert np.array_equal(got[:, :, ensstats.N_VALID], grp[:, :, groups.COUNT])
        some = got[:, :, ensstats.N_USED] > 0
        assert some.any() and (~some).any()
        assert np.array_equal(got[:, :, ensstats.QUANT + 0][some], grp[:, :, groups.TMIN][some])
        assert np.array_equal(got[:, :, ensstats.QUANT + 4][some], grp[:, :, groups.TMAX][some])
        assert (got[:, :, 2:][~some] == -9999.0).all()


def test_median_of_an_odd_number_is_the_middle_value():
    for k in (1, 3, 5, 21, 63):
        d = _series(k, 4, k)
        got = ensstats.reduce_members(*[d[n] for n in OUT], np.zeros(k, np.int32), ensstats.EnsSpec(1, 64, (0.5,)))
        assert np.array_equal(got[:, 0, 9], np.sort(d["tsurf"], axis=0)[k // 2])


def test_permuting_points_with_their_ids_keeps_counts_and_quantiles():
    d = _series(350, 5, 3)
    d["tsurf"][::13, 2:] = -9999.0
    spec = ensstats.EnsSpec(70, 6, QUANT)
    a = ensstats.reduce_members(*[d[k] for k in OUT], IRREGULAR, spec)
    perm = np.random.RandomState(9).permutation(350)
    b = ensstats.reduce_members(*[d[k][perm] for k in OUT], IRREGULAR[perm], spec)
    keep = [0, 1] + list(range(9, 14))
    assert np.array_equal(a[:, :, keep], b[:, :, keep])
    assert not np.array_equal(a[:, :, 2], b[:, :, 2])     # (the sums do depend on the order: that is why it is fixed)
    assert np.allclose(a[:, :, 2:9], b[:, :, 2:9], rtol=1e-12, atol=1e-12)


def _layouts():
    rs = np.random.RandomState(2)
    outside = IRREGULAR.copy()
    outside[rs.rand(350) < 0.1] = -1
    outside[rs.rand(350) < 0.1] = 70 + rs.randint(0, 3)
    return [("parents", ensemble.parents(70, 5), ensstats.EnsSpec(70, 5, (0.5,))),
            ("parents, 64 members", ensemble.parents(3, 64), ensstats.EnsSpec(3, 64)),
            ("irregular, station 69 without a member", IRREGULAR, ensstats.EnsSpec(70, 6, QUANT)),
            ("ids outside the range", outside, ensstats.EnsSpec(70, 6)),
            ("one point", np.zeros(1, np.int32), ensstats.EnsSpec(1, 1)),
            ("no member at all", np.full(9, -1, np.int32), ensstats.EnsSpec(4, 1))]


def _c_table(gid, spec):
    L = lib.load()
    sp = lib.ens_spec(spec)
    gid = np.ascontiguousarray(gid, np.int32)
    ints = L.rs_ens_table_ints(len(gid), C.byref(sp))
    assert ints == ensstats.table_ints(len(gid), spec) == spec.ngroups + 1 + len(gid)
    table = np.full(ints + 2, 987654, np.int32)     # a guard behind and before
    rc = L.rs_ens_member_table(len(gid), C.c_void_p(gid.ctypes.data), C.byref(sp), C.c_void_p(table[1:].ctypes.data))
    assert table[0] == 987654 and table[-1] == 987654
    return rc, table[1:-1]


def test_the_library_builds_the_table_of_the_definition():
    """rs_ens_member_table through ctypes (no device) against ensstats.member_table."""
    for name, gid, spec in _layouts():
        want = ensstats.member_table(gid, spec)
        assert want.dtype == np.int32 and want.shape == (spec.ngroups + 1 + len(gid),), name
        rc, got = _c_table(gid, spec)
        assert rc == 0, (name, lib.last_error())
        assert np.array_equal(got, want), name
    # the table itself, on the irregular layout
    t = ensstats.member_table(IRREGULAR, ensstats.EnsSpec(70, 6))
    start, members = t[:71], t[71:]
    assert start[0] == 0 and start[69] == start[70] == 350 and not (members == -1).any()
    for g in (0, 11, 68):
        mine = members[start[g]:start[g + 1]]
        assert np.array_equal(mine, np.nonzero(IRREGULAR == g)[0])
    # one member too many: both refuse and name the first such station
    first = int(np.nonzero(np.bincount(IRREGULAR) > 5)[0][0])
    with pytest.raises(ValueError, match=f"station {first} has 6 members"):
        ensstats.member_table(IRREGULAR, ensstats.EnsSpec(70, 5))
    rc, _ = _c_table(IRREGULAR, ensstats.EnsSpec(70, 5))
    assert rc == -1 and f"station {first} has 6 members, more than max_members = 5" in lib.last_error()


def test_cols_and_bad_specs_agree_with_the_library():
    L = lib.load()
    assert {"rs_hip_ens_cols", "rs_ens_table_ints", "rs_ens_member_table", "rs_hip_outputs_ens"} <= set(lib.EXPORTS)
    assert (lib.RS_ENS_MAX_MEMBERS, lib.RS_ENS_MAX_QUANT, lib.RS_ENS_COLS) == (64, 8, 9) == \
        (ensstats.RS_ENS_MAX_MEMBERS, ensstats.RS_ENS_MAX_QUANT, ensstats.RS_ENS_COLS)
    for spec in (ensstats.EnsSpec(1, 1), ensstats.EnsSpec(70, 5, (0.5,)), ensstats.EnsSpec(50000, 64, QUANT),
                 ensstats.EnsSpec(3, 20, tuple(np.linspace(0, 1, 8)))):
        assert lib.ens_cols(spec) == ensstats.cols(spec) == 9 + len(spec.quantiles)
        assert L.rs_ens_table_ints(1000, C.byref(lib.ens_spec(spec))) == ensstats.table_ints(1000, spec)
    bad = [ensstats.EnsSpec(0, 5), ensstats.EnsSpec(-2, 5), ensstats.EnsSpec(3, 0), ensstats.EnsSpec(3, 65),
           ensstats.EnsSpec(3, 5, tuple(np.linspace(0, 1, 9))), ensstats.EnsSpec(3, 5, (0.5, 0.5)),
           ensstats.EnsSpec(3, 5, (0.9, 0.1)), ensstats.EnsSpec(3, 5, (-0.1,)), ensstats.EnsSpec(3, 5, (1.0001,)),
           ensstats.EnsSpec(3, 5, (float("nan"),))]
    for spec in bad:
        with pytest.raises(ValueError):
            ensstats.cols(spec)
        sp = lib.ens_spec(spec)
        assert L.rs_hip_ens_cols(C.byref(sp)) < 0, spec
        assert L.rs_ens_table_ints(10, C.byref(sp)) < 0, spec
        with pytest.raises(RuntimeError, match="bad spec"):
            lib.ens_cols(spec)
        gid = np.zeros(4, np.int32)
        table = np.zeros(64, np.int32)
        assert L.rs_ens_member_table(4, C.c_void_p(gid.ctypes.data), C.byref(sp), C.c_void_p(table.ctypes.data)) == -1
        assert "bad spec" in lib.last_error() and not table.any()
    assert L.rs_ens_table_ints(-1, C.byref(lib.ens_spec(ensstats.EnsSpec(1, 1)))) < 0


def test_runner_refuses_stats_before_any_device_work():
    c = eh.lean_case()
    args = (c["S"], c["L"], c["B"], c["settings"], [c["local"]] * c["S"], None)
    ensemble.check(*args, c["parent"], stats=ensstats.EnsSpec(c["S"], c["M"], (0.5,)))
    with pytest.raises(ValueError, match="ngroups"):
        ensemble.check(*args, c["parent"], stats=ensstats.EnsSpec(c["S"] + 1, c["M"]))
    with pytest.raises(ValueError, match=f"station 0 has {c['M']} members, more than max_members = {c['M'] - 1}"):
        ensemble.check(*args, c["parent"], stats=ensstats.EnsSpec(c["S"], c["M"] - 1))
    crowded = c["parent"].copy()
    crowded[-1] = 4                          # station 4 gets a sixth member
    with pytest.raises(ValueError, match="station 4 has 6 members"):
        ensemble.check(*args, crowded, stats=ensstats.EnsSpec(c["S"], c["M"]))
    # ... and run_ensemble gets there before it asks for a device
    with pytest.raises(ValueError, match="station 4 has 6 members"):
        ensemble.run_ensemble(c["stations"], c["tails"], c["B"], c["settings"], c["params"], c["local"],
                              parent=crowded, stats=ensstats.EnsSpec(c["S"], c["M"]))
    with pytest.raises(ValueError, match="ngroups"):
        ensemble.run_ensemble(c["stations"], c["tails"], c["B"], c["settings"], c["params"], c["local"],
                              parent=c["parent"], stats=ensstats.EnsSpec(1, 64))


def test_table_builder_alone_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """roadsurf_amd/sanitize/ens_table_check.cpp - its own main over csrc/rs_ens_table.hpp, nothing else - compiled
    with the compiler that links the Makefile's asan build and run as a process of its own: the layouts above and
    the refusals, every table in a heap block of exactly its size."""
    rocm = os.environ.get("ROCM", "/opt/rocm")
    cxx = os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        pytest.fail(cxx + " is missing: the compiler of `make -C roadsurf_amd asan`")
    src = os.path.join(ROOT, "roadsurf_amd", "sanitize", "ens_table_check.cpp")
    exe = str(tmp_path / "ens_table_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    env = dict(os.environ)
    env.update({"ASAN_OPTIONS": "detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode == 0 and "ens table check ok" in out, out[-3000:]
