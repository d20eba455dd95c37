/*
 * rs_period_rule.hpp — which output period a row belongs to, and what a period's cell is before any row
 * (include/roadsurf.h, rs_hip_outputs_periods; the definition is roadsurf_amd/periods.py).  Stated here once, plain
 * C++ without HIP, for the host entry (rs_api.hip), the kernels (rs_cluster.hip) and a stand-alone program
 * (sanitize/period_rule_check.cpp, which tests/test_periods_reference.py builds under ASan + UBSan).  Every index is
 * int64 from the first operation on: index0 and index_step may be INT32_MAX, length * nperiods 2^31 - 1, and no sum
 * or product here leaves 2^63.
 */
#ifndef RS_PERIOD_RULE_HPP
#define RS_PERIOD_RULE_HPP

#include <cstdint>

#include "../../include/roadsurf.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RS_PER_FN __host__ __device__ inline
#else
#define RS_PER_FN inline
#endif

namespace rs_per {

/* 0, or which member is out of its limits: 1 a null spec, 2 first_index < 1, 3 length < 1, 4 nperiods < 1,
 * 5 length * nperiods > 2^31 - 1, 6 reserved != 0, 7 a threshold that is not finite */
RS_PER_FN int check(const RsPeriodSpec *sp) {
  if (!sp) return 1;
  if (sp->first_index < 1) return 2;
  if (sp->length < 1) return 3;
  if (sp->nperiods < 1) return 4;
  if ((int64_t)sp->length * (int64_t)sp->nperiods > (int64_t)INT32_MAX) return 5;
  if (sp->reserved != 0) return 6;
  const double big = __builtin_huge_val();
  if (!(sp->th.tsurf_below > -big && sp->th.tsurf_below < big)) return 7; /* (a NaN fails both) */
  for (int k = 0; k < 5; ++k)
    if (!(sp->th.storage_above[k] > -big && sp->th.storage_above[k] < big)) return 7;
  return 0;
}

inline const char *check_message(int code) {
  switch (code) {
    case 0: return "ok";
    case 1: return "spec is NULL";
    case 2: return "spec: first_index < 1";
    case 3: return "spec: length < 1";
    case 4: return "spec: nperiods < 1";
    case 5: return "spec: length * nperiods above 2^31 - 1";
    case 6: return "spec: reserved is not 0";
    default: return "spec: a threshold is not finite";
  }
}

/* the absolute 1-based time index of row r of a call */
RS_PER_FN int64_t index_of_row(int32_t index0, int32_t index_step, int64_t r) {
  return (int64_t)index0 + r * (int64_t)index_step;
}

/* the period of time index i: first_index + w*length <= i < first_index + (w+1)*length, or -1 outside
 * [first_index, first_index + length*nperiods) */
RS_PER_FN int64_t period_of_index(const RsPeriodSpec &sp, int64_t i) {
  const int64_t off = i - (int64_t)sp.first_index;
  if (off < 0 || off >= (int64_t)sp.length * (int64_t)sp.nperiods) return -1;
  return off / (int64_t)sp.length;
}

/* the period of row r of a call, or -1 */
RS_PER_FN int64_t period_of_row(const RsPeriodSpec &sp, int32_t index0, int32_t index_step, int64_t r) {
  return period_of_index(sp, index_of_row(index0, index_step, r));
}

/* the same mapping from the period's side: the rows r in [0, nrows) of a call with period_of_row(r) == w are
 * [lo, hi) - consecutive, since the index grows with r (index_step >= 1); lo == hi: none */
struct Rows {
  int64_t lo, hi;
};
RS_PER_FN int64_t rows_below(int64_t i, int32_t index0, int32_t index_step, int64_t nrows) {
  /* how many rows of the call have an index below i */
  const int64_t d = i - (int64_t)index0;
  if (d <= 0) return 0;
  const int64_t q = (d + (int64_t)index_step - 1) / (int64_t)index_step;
  return q < nrows ? q : nrows;
}
RS_PER_FN Rows rows_of_period(const RsPeriodSpec &sp, int32_t index0, int32_t index_step, int32_t nrows, int64_t w) {
  const int64_t i_lo = (int64_t)sp.first_index + w * (int64_t)sp.length;
  Rows r;
  r.lo = rows_below(i_lo, index0, index_step, nrows);
  r.hi = rows_below(i_lo + (int64_t)sp.length, index0, index_step, nrows);
  return r;
}

/* the periods a call of nrows >= 1 rows can touch: [lo, hi], or lo > hi: none.  (With index_step > length some of
 * them have no row: rows_of_period says so.) */
struct Span {
  int64_t lo, hi;
};
RS_PER_FN Span periods_of_call(const RsPeriodSpec &sp, int32_t index0, int32_t index_step, int32_t nrows) {
  const int64_t total = (int64_t)sp.length * (int64_t)sp.nperiods;
  int64_t a = index_of_row(index0, index_step, 0) - (int64_t)sp.first_index;
  int64_t b = index_of_row(index0, index_step, (int64_t)nrows - 1) - (int64_t)sp.first_index;
  Span s;
  s.lo = 0;
  s.hi = -1;
  if (nrows < 1 || b < 0 || a >= total) return s;
  if (a < 0) a = 0;
  if (b > total - 1) b = total - 1;
  s.lo = a / (int64_t)sp.length;
  s.hi = b / (int64_t)sp.length;
  return s;
}

/* the cell of no rows: counts 0, min +inf, maxima -inf, sum 0, the sample -9999.0 at index 0 */
RS_PER_FN double empty(int c) {
  return c == 1 ? __builtin_huge_val() : (c == 2 || (c >= 7 && c < 12)) ? -__builtin_huge_val() : c == 5 ? -9999.0 : 0.0;
}

}  // namespace rs_per

#endif
