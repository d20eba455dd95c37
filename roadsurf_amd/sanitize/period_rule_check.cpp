/*
 * period_rule_check.cpp — the row-to-period rule of the aggregates over output periods (csrc/rs_period_rule.hpp) on
 * its own: a program with its own main and nothing of the library or the device in it, to be compiled with
 * -fsanitize=address,undefined (tests/test_periods_reference.py does), so that an int32 or int64 overflow anywhere in
 * the mapping is the sanitizer's to report.  Usage: period_rule_check CASES, a text file of lines
 *     first_index length nperiods index0 index_step nrows r want
 * where `want` is the period of row r as the caller computed it (the test: in Python, whose integers do not
 * overflow).  Every line is checked three ways: period_of_row(r) == want; rows_of_period(want) holds r (and, where
 * want is -1, no period of periods_of_call holds it at either end); periods_of_call holds want.  Then the spec check's
 * refusals, and a brute-force sweep of small calls: the rows of every period are exactly the rows that map to it.
 * Exit status 0 and "period rule check ok": everything was as expected.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../csrc/rs_period_rule.hpp"

static int failures = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      ++failures;                    \
      std::printf("FAILED: " __VA_ARGS__); \
      std::printf("\n");             \
    }                                \
  } while (0)

static RsPeriodSpec spec_of(int32_t first, int32_t length, int32_t nperiods) {
  RsPeriodSpec sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.first_index = first;
  sp.length = length;
  sp.nperiods = nperiods;
  return sp;
}

static void check_case(long long first, long long length, long long nper, long long index0, long long step,
                       long long nrows, long long r, long long want) {
  const RsPeriodSpec sp = spec_of((int32_t)first, (int32_t)length, (int32_t)nper);
  EXPECT(rs_per::check(&sp) == 0, "spec %lld %lld %lld refused: %s", first, length, nper,
         rs_per::check_message(rs_per::check(&sp)));
  const int32_t i0 = (int32_t)index0, st = (int32_t)step, nr = (int32_t)nrows;
  const int64_t got = rs_per::period_of_row(sp, i0, st, r);
  EXPECT(got == want, "spec %lld %lld %lld, index0 %lld step %lld row %lld: period %lld, expected %lld", first, length,
         nper, index0, step, r, (long long)got, want);
  const rs_per::Span span = rs_per::periods_of_call(sp, i0, st, nr);
  EXPECT(span.lo >= 0 && span.hi < nper, "span [%lld, %lld] outside the %lld periods", (long long)span.lo,
         (long long)span.hi, nper);
  if (want >= 0) {
    EXPECT(span.lo <= want && want <= span.hi, "period %lld outside the call's span [%lld, %lld]", want,
           (long long)span.lo, (long long)span.hi);
    const rs_per::Rows rows = rs_per::rows_of_period(sp, i0, st, nr, want);
    EXPECT(0 <= rows.lo && rows.lo <= r && r < rows.hi && rows.hi <= nrows, "row %lld outside rows [%lld, %lld) of its period %lld",
           r, (long long)rows.lo, (long long)rows.hi, want);
  } else if (span.lo <= span.hi) {
    const rs_per::Rows a = rs_per::rows_of_period(sp, i0, st, nr, span.lo), b = rs_per::rows_of_period(sp, i0, st, nr, span.hi);
    EXPECT(!(a.lo <= r && r < a.hi) && !(b.lo <= r && r < b.hi), "row %lld of no period lies in a period's rows", r);
  }
}

/* every period's rows are exactly the rows that map to it, and they lie inside [0, nrows) */
static void sweep(const RsPeriodSpec &sp, int32_t index0, int32_t step, int32_t nrows) {
  const rs_per::Span span = rs_per::periods_of_call(sp, index0, step, nrows);
  int64_t covered = 0;
  for (int64_t w = span.lo; w <= span.hi; ++w) {
    const rs_per::Rows rows = rs_per::rows_of_period(sp, index0, step, nrows, w);
    EXPECT(0 <= rows.lo && rows.lo <= rows.hi && rows.hi <= nrows, "rows [%lld, %lld) of period %lld outside [0, %d)",
           (long long)rows.lo, (long long)rows.hi, (long long)w, nrows);
    for (int64_t r = rows.lo; r < rows.hi; ++r)
      EXPECT(rs_per::period_of_row(sp, index0, step, r) == w, "row %lld is in the rows of period %lld but maps to %lld",
             (long long)r, (long long)w, (long long)rs_per::period_of_row(sp, index0, step, r));
    covered += rows.hi - rows.lo;
  }
  int64_t mapped = 0;
  for (int64_t r = 0; r < nrows; ++r) {
    const int64_t w = rs_per::period_of_row(sp, index0, step, r);
    EXPECT(w >= -1 && w < sp.nperiods, "row %lld maps to %lld", (long long)r, (long long)w);
    if (w >= 0) {
      ++mapped;
      EXPECT(span.lo <= w && w <= span.hi, "row %lld maps to %lld outside the span", (long long)r, (long long)w);
    }
  }
  EXPECT(mapped == covered, "%lld rows map to a period, the periods' rows are %lld", (long long)mapped, (long long)covered);
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::printf("usage: period_rule_check CASES\n");
    return 2;
  }
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) {
    std::printf("cannot read %s\n", argv[1]);
    return 2;
  }
  long long v[8], lines = 0;
  while (std::fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7]) == 8) {
    check_case(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
    ++lines;
  }
  std::fclose(f);
  EXPECT(lines > 0, "no cases in %s", argv[1]);

  /* the spec's limits */
  {
    RsPeriodSpec sp = spec_of(1, 1, 1);
    EXPECT(rs_per::check(&sp) == 0, "the smallest spec refused");
    EXPECT(rs_per::check(nullptr) == 1, "a null spec accepted");
    sp = spec_of(0, 1, 1);
    EXPECT(rs_per::check(&sp) == 2, "first_index 0 accepted");
    sp = spec_of(1, 0, 1);
    EXPECT(rs_per::check(&sp) == 3, "length 0 accepted");
    sp = spec_of(1, 1, 0);
    EXPECT(rs_per::check(&sp) == 4, "nperiods 0 accepted");
    sp = spec_of(INT32_MAX, INT32_MAX, 1);
    EXPECT(rs_per::check(&sp) == 0, "length * nperiods = 2^31 - 1 refused");
    sp = spec_of(INT32_MAX, 1, INT32_MAX);
    EXPECT(rs_per::check(&sp) == 0, "length * nperiods = 2^31 - 1 refused");
    sp = spec_of(1, 65536, 32768);
    EXPECT(rs_per::check(&sp) == 5, "length * nperiods = 2^31 accepted");
    sp = spec_of(1, INT32_MAX, INT32_MAX);
    EXPECT(rs_per::check(&sp) == 5, "length * nperiods = (2^31 - 1)^2 accepted");
    sp = spec_of(1, 1, 1);
    sp.reserved = 1;
    EXPECT(rs_per::check(&sp) == 6, "reserved 1 accepted");
    sp = spec_of(1, 1, 1);
    sp.th.tsurf_below = NAN;
    EXPECT(rs_per::check(&sp) == 7, "a NaN threshold accepted");
    sp = spec_of(1, 1, 1);
    sp.th.storage_above[4] = INFINITY;
    EXPECT(rs_per::check(&sp) == 7, "an infinite threshold accepted");
    for (int c = 0; c <= 7; ++c) EXPECT(std::strlen(rs_per::check_message(c)) > 0, "no message for code %d", c);
  }
  /* the cell of no rows */
  for (int c = 0; c < RS_PER_COLS; ++c) {
    const double e = rs_per::empty(c);
    const double want = c == 1 ? INFINITY : (c == 2 || (c >= 7 && c <= 11)) ? -INFINITY : c == 5 ? -9999.0 : 0.0;
    EXPECT(e == want, "empty(%d) = %g", c, e);
  }
  /* small calls, rows before, inside and behind the periods; steps above and below the length; the far corners */
  const int32_t firsts[] = {1, 4, 1000, INT32_MAX - 40, INT32_MAX};
  const int32_t lengths[] = {1, 5, 7, 120};
  const int32_t npers[] = {1, 3, 9};
  const int32_t steps[] = {1, 3, 8, 1000, INT32_MAX};
  for (int32_t first : firsts)
    for (int32_t length : lengths)
      for (int32_t nper : npers) {
        const RsPeriodSpec sp = spec_of(first, length, nper);
        for (int32_t step : steps)
          for (int32_t nrows : {1, 2, 23, 50})
            for (int64_t back : {-60, -3, 0, 2, 11, 40}) {
              const int64_t i0 = (int64_t)first + back;
              if (i0 < INT32_MIN || i0 > INT32_MAX) continue;
              sweep(sp, (int32_t)i0, step, nrows);
            }
      }
  {
    const RsPeriodSpec sp = spec_of(INT32_MAX, 1, INT32_MAX);
    sweep(spec_of(INT32_MAX, 1000, 1000), INT32_MAX, INT32_MAX, 50);
    sweep(spec_of(INT32_MAX, 1000, 1000), INT32_MIN, INT32_MAX, 50);
    sweep(sp, INT32_MAX - 10, 1, 50);
  }
  if (failures) {
    std::printf("period rule check: %d failures\n", failures);
    return 1;
  }
  std::printf("period rule check ok (%lld cases)\n", lines);
  return 0;
}
