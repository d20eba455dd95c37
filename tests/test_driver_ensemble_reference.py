"""CPU: the host rules of the driver's ensemble form (driver.run_ensemble, rs_driver_run_ensemble).

* ``driver.branch_index`` / ``driver.member_rows`` against a brute-force walk over the time axes.
* The sharing argument - a member's merged series are its station's before the branch, and so are the decisions that
  act there - held to the driver oracle (oracle/driver_oracle.c) on ``driver.replicate_sources``.
* roadsurf_amd/sanitize/driver_ens_check.cpp, the C++ statement of the rules (csrc/rs_driver_ens.hpp) with a main of
  its own, compiled and run under ASan + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import driver_helpers as dh
from roadsurf_amd import abi, driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START, DT = dh.START, 30


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _settings(L, step_minutes=10, **kw):
    s = abi.default_settings(L)
    s.outputStep = step_minutes
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _brute(start, dt, L, step, t0):
    """(B, first_row, n_tail) by walking the simulation times and the kept rows; None where the call is refused."""
    if t0 <= start:
        return None
    k = next((i for i in range(L) if start + i * dt >= t0), None)
    if k is None or not 1 <= k <= L - 1:
        return None
    n_out = len(range(0, L, step))
    first_row = next((r for r in range(n_out + 1) if r * step >= k))
    return k, first_row, n_out - first_row


@pytest.mark.parametrize("L, step_minutes", [(1081, 10), (1081, 1), (1082, 10), (241, 60), (2, 1)])
def test_branch_index_and_member_rows_agree_with_a_walk_over_the_axes(L, step_minutes):
    s = _settings(L, step_minutes)
    step, n_out = driver.output_rows(s)
    offsets = {"on a simulation time": DT * (L // 2), "between two": DT * (L // 2) + 7, "B = 1": DT,
               "B = 1, between": 1, "B = L - 1": DT * (L - 1), "B = L - 1, between": DT * (L - 2) + 1,
               "not a multiple of step": DT * (step * 3 + 1), "at the start": 0, "before the start": -3600,
               "one second behind the end": DT * (L - 1) + 1, "far beyond the end": DT * L * 50}
    accepted = 0
    for name, off in offsets.items():
        want = _brute(START, DT, L, step, START + off)
        if want is None:
            with pytest.raises(ValueError):
                driver.branch_index(START, DT, L, START + off)
            with pytest.raises(ValueError):
                driver.member_rows(s, START, START + off)
            continue
        accepted += 1
        assert driver.branch_index(START, DT, L, START + off) == want[0], name
        assert driver.member_rows(s, START, START + off) == want, name
        assert 0 <= want[2] <= n_out and want[1] * step >= want[0] > (want[1] - 1) * step, name
    assert accepted >= 2
    assert _brute(START, DT, L, step, START + DT)[0] == 1 and _brute(START, DT, L, step, START + DT * (L - 1))[0] == L - 1
    for off in (0, -1, DT * (L - 1) + 1):
        assert _brute(START, DT, L, step, START + off) is None


def _member_source(n_members, first_hour, hours, seed=11):
    """An hourly forecast of the members' own, from `first_hour` to an hour behind the end."""
    rs = np.random.RandomState(seed)
    t = START + 3600 * np.arange(first_hour, hours + 2, dtype=np.int64)
    shape = (n_members, len(t))
    tair = rs.uniform(-8, 4, shape)
    return driver.RawSource(t, {"tair": tair, "tdew": tair - rs.uniform(0.2, 4, shape), "vz": rs.uniform(0.5, 9, shape),
                                "prec": rs.uniform(0, 1, shape) * (rs.rand(*shape) < 0.3), "sw": rs.uniform(0, 200, shape),
                                "lw": rs.uniform(200, 330, shape)})


def test_replicate_sources_gathers_rows_and_inserts_the_member_source():
    src, L, t0, tf = dh.scenario(7, hours=9, obs_hours=6)
    parent = np.repeat(np.arange(7), 3)
    mem = _member_source(21, 6, 9)
    assert driver.default_position(src) == 1          # behind the forecast, before the observations
    rep = driver.replicate_sources(src, mem, parent)
    assert [r.is_observation for r in rep] == [False, False, True] and rep[1] is mem
    for a, b in ((src[0], rep[0]), (src[1], rep[2])):
        assert np.array_equal(a.times, b.times)
        for k in a.fields:
            assert np.array_equal(_u64(a.fields[k][parent]), _u64(b.fields[k]))
    rag = dh.ragged(src[1])
    rep = driver.replicate_sources([src[0], rag], mem, parent, position=0)
    assert rep[0] is mem and np.array_equal(rep[2].times, rag.times[parent]) and np.array_equal(rep[2].lengths, rag.lengths[parent])
    with pytest.raises(ValueError):
        driver.replicate_sources(src, mem, parent, position=3)
    assert np.array_equal(driver.check_parent(parent, 7), parent)
    for bad, msg in ((parent[::-1], "member 3: parent 5 below"), (parent + 1, "member 18: parent 7 outside"),
                     (parent - 1, "member 0: parent -1 outside")):
        with pytest.raises(ValueError, match=msg):
            driver.check_parent(bad, 7)


@pytest.mark.parametrize("coupling", [False, True])
def test_members_share_their_stations_series_and_decisions_before_the_branch(coupling):
    """The argument the ensemble call rests on, on the driver oracle: with a member source that starts at hour 6, every
    merged series of a member is its station's at the indices before k_b, InitLenI and the coupling decisions are the
    station's, and relaxation targets of a member's own occur only where InitLenI >= B - where they act behind the
    branch alone."""
    n, hours = 7, 9
    src, L, t0, tf = dh.scenario(n, hours=hours, obs_hours=6)
    parent = np.repeat(np.arange(n, dtype=np.int32), 3)
    mem = _member_source(len(parent), 6, hours)
    s = _settings(L, use_relaxation=1, use_coupling=1 if coupling else 0)
    B, first_row, n_tail = driver.member_rows(s, t0, int(mem.times[0]))
    assert B == 720 and (first_row, n_tail) == (36, 55 - 36)
    st = dh.oracle_read_input(src, s, t0, tf)
    me = dh.oracle_read_input(driver.replicate_sources(src, mem, parent), s, t0, tf)
    for k in driver.MERGED_FIELDS:
        a, b = st["merged"][k][parent], me["merged"][k]
        assert np.array_equal(_u64(a[:, :B]), _u64(b[:, :B])), k
    assert any(not np.array_equal(_u64(st["merged"][k][parent][:, B:]), _u64(me["merged"][k][:, B:])) for k in ("tair", "vz"))
    own_targets = shared_targets = 0
    for q, p in enumerate(parent):
        a, l = me["local"][q], st["local"][int(p)]
        if st["status"][p] != 0:   # rejected by a hole before the branch: the member has it too
            assert 1 <= st["status"][p] <= 6 and st["missing_index"][p] < B
            assert me["status"][q] == st["status"][p] and me["missing_index"][q] == st["missing_index"][p]
            continue
        assert me["status"][q] == 0
        assert a.InitLenI == l.InitLenI
        if coupling:
            assert a.couplingIndexI == l.couplingIndexI
            assert np.array_equal(_u64([a.couplingTsurf]), _u64([l.couplingTsurf]))
            assert l.couplingIndexI + 1 <= B      # (the rule of the call holds on this scenario)
        same = all(np.array_equal(_u64([getattr(a, f)]), _u64([getattr(l, f)])) for f in ("tair_relax", "VZ_relax", "RH_relax"))
        if not same:
            assert l.InitLenI >= B, (q, l.InitLenI)
            own_targets += 1
        elif l.InitLenI < B:
            shared_targets += 1
    assert own_targets > 0 and shared_targets > 0   # both kinds of station occur


def test_host_rules_alone_are_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """roadsurf_amd/sanitize/driver_ens_check.cpp - its own main over csrc/rs_driver_ens.hpp, nothing else - compiled
    with the compiler that links the Makefile's asan build and run as a process of its own."""
    rocm = os.environ.get("ROCM", "/opt/rocm")
    cxx = os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        pytest.fail(cxx + " is missing: the compiler of `make -C roadsurf_amd asan`")
    src = os.path.join(ROOT, "roadsurf_amd", "sanitize", "driver_ens_check.cpp")
    exe = str(tmp_path / "driver_ens_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    env = dict(os.environ)
    env.update({"ASAN_OPTIONS": "detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode == 0 and "driver ens check ok" in out, out[-3000:]
