"""CPU: the definition of the per-point aggregates over output periods (roadsurf_amd/periods.py, reduce_series) on
hand-written rows with known answers, its feed contract (rows in time order, cut anywhere, give the one-call result bit
for bit), its agreement with the per-point summaries over the same rows, and the row-to-period rule that the library
and its kernel share (roadsurf_amd/csrc/rs_period_rule.hpp) as a stand-alone program under ASan + UBSan.  The device
reducer is held to this definition by tests/test_hip_periods.py.  Every comparison is exact."""
import os
import random
import subprocess

import numpy as np
import pytest

from roadsurf_amd import periods, summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
NAN = np.nan
M = -9999.0
OUT = ("tsurf", "snow", "water", "ice", "deposit", "ice2")


def _series(t, snow=None, water=None, ice=None, deposit=None, ice2=None):
    t = np.asarray(t, np.float64)
    z = np.zeros_like(t)
    return [t] + [z if s is None else np.asarray(s, np.float64) for s in (snow, water, ice, deposit, ice2)]


def _cell(n, tmin, tmax, tsum, nbelow, last, last_index, smax=(0.0,) * 5, scount=(0,) * 5):
    return [n, tmin, tmax, tsum, nbelow, last, last_index, *smax, *scount]


EMPTY = _cell(0, INF, -INF, 0.0, 0, M, 0, (-INF,) * 5)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _random_series(n, nrows, seed):
    """Few values, exact in fp32 too - ties and threshold hits everywhere -, -9999.0 tails, an invalid point, NaN."""
    rs = np.random.RandomState(seed)
    tv = np.array([-2.0, -0.5, 0.0, 0.0, 0.5, 1.5])
    sv = np.array([0.0, 0.125, 0.125, 0.75])
    d = [tv[rs.randint(0, len(tv), (n, nrows))]] + [sv[rs.randint(0, len(sv), (n, nrows))] for _ in range(5)]
    for p in range(0, n, 5):
        d[0][p, rs.randint(0, nrows):] = M
    if n >= 3:
        d[0][n // 2] = M
    d[0][n - 1, nrows // 2] = NAN
    d[1][n - 1, 0] = NAN
    return d


def test_known_answers():
    """Periods of three indices from index 4 on: [4, 6], [7, 9] and [10, 12], of which the rows reach 11 - a partial
    last period -, with two rows before the first period and two behind the last."""
    spec = periods.PeriodSpec(4, 3, 3, tsurf_below=0.0, storage_above=(0.5, 0.0, 0.1, 0.0, 0.0))
    index = np.array([2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14])
    t = [[9.0, 9.0, 1.0, -2.0, -2.0, 3.0, 3.0, 0.0, -1.0, 0.5, 9.0, 9.0],   # ties; 0.0 equals the threshold
         [5.0, 5.0, 2.0, -1.0, M, M, M, M, M, M, M, M],                      # a failed point: the -9999.0 tail
         [M] * 12,                                                           # invalid throughout
         [0.0, 0.0, NAN, -3.0, 4.0, 1.0, NAN, NAN, 2.0, 2.0, 0.0, 0.0],      # NaN: valid rows that win nothing
         [0.0, 0.0, 1e16, 1.0, 1.0, 1.0, 1.0, 1e16, 0.1, 0.2, 0.0, 0.0]]     # the sum is ordered
    snow = [[9.0, 9.0, 0.5, 0.6, 0.5, 0.7, 0.0, 0.0, 0.5, 0.5, 9.0, 9.0],    # equal to its threshold: not above
            [0.0, 0.0, 0.9, 0.2, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0],    # storages of invalid rows do not count
            [9.0] * 12,
            [0.0, 0.0, NAN, 1.0, 0.2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
            [0.0] * 12]
    ice = [[1.0, 1.0, 0.0, 0.1, 0.2, 0.1, 0.1, 0.1, 0.3, 0.0, 1.0, 1.0]] + [[0.0] * 12] * 4
    got = periods.reduce_series(*_series(t, snow=snow, ice=ice), index, spec)
    assert got.shape == (5, 3, periods.RS_PER_COLS) and got.dtype == np.float64
    want = np.array([
        [_cell(3, -2.0, 1.0, -3.0, 2, -2.0, 6, (0.6, 0.0, 0.2, 0.0, 0.0), (1, 0, 1, 0, 0)),
         _cell(3, 0.0, 3.0, 6.0, 0, 0.0, 9, (0.7, 0.0, 0.1, 0.0, 0.0), (1, 0, 0, 0, 0)),
         _cell(2, -1.0, 0.5, -0.5, 1, 0.5, 11, (0.5, 0.0, 0.3, 0.0, 0.0), (0, 0, 1, 0, 0))],
        [_cell(2, -1.0, 2.0, 1.0, 1, -1.0, 5, (0.9, 0.0, 0.0, 0.0, 0.0), (1, 0, 0, 0, 0)), EMPTY, EMPTY],
        [EMPTY, EMPTY, EMPTY],
        [_cell(3, -3.0, 4.0, NAN, 1, 4.0, 6, (1.0, 0.0, 0.0, 0.0, 0.0), (1, 0, 0, 0, 0)),
         _cell(3, 1.0, 1.0, NAN, 0, NAN, 9),
         _cell(2, 2.0, 2.0, 4.0, 0, 2.0, 11)],
        [_cell(3, 1.0, 1e16, 1e16, 0, 1.0, 6),            # (1e16 + 1) + 1: each 1 is rounded away
         _cell(3, 1.0, 1e16, 1e16 + 2.0, 0, 1e16, 9),     # (1 + 1) + 1e16
         _cell(2, 0.1, 0.2, 0.1 + 0.2, 0, 0.2, 11)],
    ], np.float64)
    assert _same(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert _same(periods.empty(2, spec), np.array([[EMPTY] * 3] * 2))
    m = periods.mean(got)
    assert m.shape == (5, 3) and m[0, 0] == -1.0 and m[0, 1] == 2.0 and m[4, 2] == (0.1 + 0.2) / 2
    assert np.isnan(m[2]).all() and np.isnan(m[1, 1]) and np.isnan(m[3, 0]) and m[3, 2] == 2.0
    # the rule, on its own
    assert periods.period_of(index, spec).tolist() == [-1, -1, 0, 0, 0, 1, 1, 1, 2, 2, -1, -1]


def test_float32_series_widen_exactly():
    spec = periods.PeriodSpec(1, 3, 1, tsurf_below=np.float32(0.1), storage_above=(np.float32(0.3),) + (0.0,) * 4)
    t = np.array([[0.1, 0.2, -9999.0]], np.float32)
    snow = np.array([[0.3, 0.7, 0.9]], np.float32)
    got = periods.reduce_series(t, snow, *[np.zeros((1, 3), np.float32)] * 4, np.array([1, 2, 3]), spec)[0, 0]
    assert got[periods.COUNT] == 2 and got[periods.N_BELOW] == 0 and got[periods.STORAGE_COUNT] == 1
    assert got[periods.TMIN] == float(np.float32(0.1)) != 0.1
    assert got[periods.TSUM] == float(np.float32(0.1)) + float(np.float32(0.2)) != float(np.float32(0.1) + np.float32(0.2))
    assert got[periods.LAST] == float(np.float32(0.2)) and got[periods.LAST_INDEX] == 2
    assert got[periods.STORAGE_MAX] == float(np.float32(0.7))


@pytest.mark.parametrize("index_step", [1, 3])
def test_rows_in_time_order_cut_anywhere_give_the_one_call_result(index_step):
    n, nrows = 40, 37
    rs = np.random.RandomState(11)
    d = _random_series(n, nrows, 5)
    d[0] = d[0] + np.where(d[0] == M, 0.0, rs.standard_normal((n, nrows)) * 1e-3 + 1e3 * rs.randint(0, 2, (n, nrows)))
    index = 3 + index_step * np.arange(nrows)
    spec = periods.PeriodSpec(7, 5 * index_step, 6, 0.0, (0.125, 0.0, 0.125, 0.75, 0.125))   # five rows a period
    one = periods.reduce_series(*d, index, spec)
    assert (one[:, :, periods.COUNT] > 1).any() and (periods.period_of(index, spec) < 0).any()
    for trial in range(6):
        cuts = sorted(set(rs.randint(1, nrows, rs.randint(1, 9)).tolist()))
        acc = None
        for lo, hi in zip([0] + cuts, cuts + [nrows]):
            acc = periods.reduce_series(*[s[:, lo:hi] for s in d], index[lo:hi], spec, acc=acc)
        assert _same(acc, one), (trial, cuts)
    # a row at a time, the accumulator handed on - and not changed by the call it is handed to
    acc = periods.empty(n, spec)
    for r in range(nrows):
        before = acc.copy()
        nxt = periods.reduce_series(*[s[:, r:r + 1] for s in d], index[r:r + 1], spec, acc=acc)
        assert _same(acc, before)
        acc = nxt
    assert _same(acc, one)
    # the other columns do not depend on the order of feeding; the sum does
    back = None
    for r in range(nrows - 1, -1, -1):
        back = periods.reduce_series(*[s[:, r:r + 1] for s in d], index[r:r + 1], spec, acc=back)
    cols = [c for c in range(periods.RS_PER_COLS) if c != periods.TSUM]
    assert _same(back[:, :, cols], one[:, :, cols])
    assert not _same(back[:, :, periods.TSUM], one[:, :, periods.TSUM])


def test_periods_of_one_index_reproduce_the_rows():
    n, nrows = 12, 19
    d = _random_series(n, nrows, 3)
    index = 5 + np.arange(nrows)
    spec = periods.PeriodSpec(5, 1, nrows, 0.0, (0.125,) * 5)
    got = periods.reduce_series(*d, index, spec)
    t = d[0]
    ok = t != M
    assert np.array_equal(got[:, :, periods.COUNT], ok.astype(float))
    fin = ok & ~np.isnan(t)
    assert _same(got[:, :, periods.TMIN], np.where(fin, t, INF)) and _same(got[:, :, periods.TMAX], np.where(fin, t, -INF))
    assert _same(got[:, :, periods.TSUM], np.where(ok, t, 0.0))
    assert _same(got[:, :, periods.LAST], np.where(ok, t, M))
    assert _same(got[:, :, periods.LAST_INDEX], np.where(ok, index[None, :], 0).astype(float))
    assert _same(got[:, :, periods.N_BELOW], (ok & (t < 0.0)).astype(float))
    for k in range(5):
        s = d[1 + k]
        assert _same(got[:, :, periods.STORAGE_MAX + k], np.where(ok & ~np.isnan(s), s, -INF))
        assert _same(got[:, :, periods.STORAGE_COUNT + k], (ok & (s > 0.125)).astype(float))


def test_periods_that_cover_the_rows_agree_with_the_summaries():
    n, nrows = 30, 48
    d = _random_series(n, nrows, 9)
    index = 1 + np.arange(nrows)
    th = (0.0, (0.125, 0.0, 0.125, 0.75, 0.125))
    for length in (5, 7, 48):   # 5 and 7 do not divide 48: the last period is partial
        spec = periods.PeriodSpec(1, length, -(-nrows // length), *th)
        per = periods.reduce_series(*d, index, spec)
        tot = summary.reduce_series(*d, index, summary.SummarySpec(*th))
        assert np.array_equal(per[:, :, periods.COUNT].sum(axis=1), tot[:, summary.COUNT])
        assert np.array_equal(per[:, :, periods.TMIN].min(axis=1), tot[:, summary.TMIN])
        assert np.array_equal(per[:, :, periods.TMAX].max(axis=1), tot[:, summary.TMAX])
        assert np.array_equal(per[:, :, periods.N_BELOW].sum(axis=1), tot[:, summary.N_BELOW])
        for k in range(5):
            assert np.array_equal(per[:, :, periods.STORAGE_MAX + k].max(axis=1), tot[:, summary.STORAGE_MAX + k])
            assert np.array_equal(per[:, :, periods.STORAGE_COUNT + k].sum(axis=1), tot[:, summary.STORAGE_COUNT + k])
    assert (tot[:, summary.COUNT] == 0).any() and (tot[:, summary.COUNT] == nrows).any()


def test_the_sample_column_is_the_decimated_series():
    """first_index = 2 and length = step: period w ends at the driver's kept row w + 1, the index 1 + (w + 1) * step."""
    n, step, kept = 9, 6, 8
    nrows = 1 + (kept - 1) * step
    d = _random_series(n, nrows, 21)
    d[0][n // 2] = np.arange(nrows)          # (instead of the invalid point: a series that names its own index)
    d[0][n - 1, 2 * step] = NAN              # a kept row that is a NaN
    spec = periods.PeriodSpec(2, step, kept - 1)
    got = periods.reduce_series(*d, 1 + np.arange(nrows), spec)
    kept_t, kept_i = d[0][:, step::step], 1 + step * np.arange(1, kept)
    valid = kept_t != M
    assert valid.sum() > valid.size // 2 and (~valid).any() and np.isnan(kept_t).any()
    assert _same(got[:, :, periods.LAST][valid], kept_t[valid])
    assert np.array_equal(got[:, :, periods.LAST_INDEX][valid], np.broadcast_to(kept_i, valid.shape)[valid])
    # where the kept row was never saved, the sample is the last row that was - column 6 says which - or none
    stale = got[:, :, periods.LAST_INDEX][~valid]
    assert (stale < np.broadcast_to(kept_i, valid.shape)[~valid]).all() and (stale == 0).any() and (stale > 0).any()
    assert got[n // 2, :, periods.TMIN].tolist() == [1 + w * step for w in range(kept - 1)]
    assert got[n // 2, :, periods.TMAX].tolist() == [(w + 1) * step for w in range(kept - 1)]


def test_check_spec_refusals():
    periods.check_spec(periods.PeriodSpec(1, 1, 1))
    periods.check_spec(periods.PeriodSpec(2**31 - 1, 2**31 - 1, 1))
    periods.check_spec(periods.PeriodSpec(1, 65536, 32767))
    for bad, what in ((periods.PeriodSpec(0, 1, 1), "first_index"), (periods.PeriodSpec(1, 0, 1), "length"),
                      (periods.PeriodSpec(1, 1, 0), "nperiods"), (periods.PeriodSpec(1, 65536, 32768), "2\\*\\*31"),
                      (periods.PeriodSpec(1, 2**31 - 1, 2), "2\\*\\*31"),
                      (periods.PeriodSpec(1, 1, 1, tsurf_below=NAN), "finite"),
                      (periods.PeriodSpec(1, 1, 1, storage_above=(0.0, 0.0, INF, 0.0, 0.0)), "finite"),
                      (periods.PeriodSpec(1, 1, 1, storage_above=(0.0,) * 4), "five")):
        with pytest.raises(ValueError, match=what):
            periods.check_spec(bad)
        with pytest.raises(ValueError, match=what):
            periods.reduce_series(*_series([[1.0]]), np.array([1]), bad)
        with pytest.raises(ValueError, match=what):
            periods.empty(1, bad)


def _rule_cases():
    """Lines `first length nperiods index0 index_step nrows r want` with the period computed in Python integers."""
    big = 2**31 - 1
    rnd = random.Random(17)
    specs = [(1, 1, 1), (4, 5, 3), (2, 120, 48), (big, 1, big), (big, big, 1), (1, big, 1), (1, 1, big),
             (big - 5, 46341, 46340), (1000, 65535, 32768), (7, 32768, 65535)]
    calls = [(1, 1, 1), (2, 1, 23), (2, 3, 23), (big, big, big), (big, 1, big), (1, big, big), (-2**31, big, 5),
             (big - 3, big - 1, 1000), (-5, 7, 100), (0, 1, 10)]
    for _ in range(40):
        specs.append((rnd.randint(1, big), rnd.randint(1, 100000), rnd.randint(1, 20000)))
        calls.append((rnd.randint(-100, big), rnd.choice([1, 2, 120, rnd.randint(1, big)]), rnd.randint(1, big)))
    lines = []
    for first, length, nper in specs:
        assert length * nper <= big
        for index0, step, nrows in calls:
            # rows at both ends of the call, at both ends of the periods and of one period in the middle, and between
            rows = {0, 1, nrows - 1, nrows // 2, rnd.randrange(nrows)}
            for i in (first - 1, first, first + length - 1, first + length, first + length * nper - 1,
                      first + length * nper, first + length * (nper // 2), first + length * (nper // 2) - 1):
                r = (i - index0) // step
                rows |= {r, r + 1}
            for r in sorted(rows):
                if 0 <= r < nrows:
                    off = index0 + r * step - first
                    want = off // length if 0 <= off < length * nper else -1
                    lines.append(f"{first} {length} {nper} {index0} {step} {nrows} {r} {want}")
    return lines


def test_the_python_rule_is_the_rule_of_the_cases():
    """periods.period_of (numpy int64) against the same Python-integer values the C++ program is held to."""
    for line in _rule_cases()[::7]:
        first, length, nper, index0, step, nrows, r, want = (int(x) for x in line.split())
        assert int(periods.period_of(index0 + r * step, periods.PeriodSpec(first, length, nper))) == want, line


def test_row_to_period_rule_alone_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """roadsurf_amd/sanitize/period_rule_check.cpp - its own main over csrc/rs_period_rule.hpp, nothing else - compiled
    with the compiler that links the Makefile's asan build and run as a process of its own on cases whose periods
    were computed here: index0 and index_step near INT32_MAX, length * nperiods at its limit."""
    rocm = os.environ.get("ROCM", "/opt/rocm")
    cxx = os.path.join(rocm, "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        pytest.fail(cxx + " is missing: the compiler of `make -C roadsurf_amd asan`")
    src = os.path.join(ROOT, "roadsurf_amd", "sanitize", "period_rule_check.cpp")
    exe = str(tmp_path / "period_rule_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = _rule_cases()
    assert len(lines) > 5000 and any(l.endswith(" -1") for l in lines) and any(not l.endswith(" -1") for l in lines)
    big = str(2**31 - 1)
    assert any(l.split()[3] == big and l.split()[4] == big and not l.endswith(" -1") for l in lines)
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    env = dict(os.environ)
    env.update({"ASAN_OPTIONS": "detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode == 0 and f"period rule check ok ({len(lines)} cases)" in out, out[-3000:]
