/*
 * rs_ens_table.hpp — the member table of the ensemble statistics (include/roadsurf.h, rs_ens_member_table): host
 * code only, no HIP, so that a stand-alone program can compile it (tests/test_ensstats_reference.py builds one under
 * ASan + UBSan).  roadsurf_amd/ensstats.py (member_table) is the same thing in numpy.
 */
#ifndef RS_ENS_TABLE_HPP
#define RS_ENS_TABLE_HPP

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/roadsurf.h"

namespace rs_ens {

/* RS_ENS_COLS + nquant, or -1: a bad spec */
inline int32_t cols(const RsEnsSpec *sp) {
  if (!sp || sp->ngroups < 1 || sp->max_members < 1 || sp->max_members > RS_ENS_MAX_MEMBERS || sp->nquant < 0 ||
      sp->nquant > RS_ENS_MAX_QUANT)
    return -1;
  for (int32_t j = 0; j < sp->nquant; ++j) {
    const double q = sp->quant[j];
    if (!(q >= 0.0 && q <= 1.0) || (j > 0 && !(q > sp->quant[j - 1]))) return -1; /* (a NaN fails the first) */
  }
  return RS_ENS_COLS + sp->nquant;
}

/* ints of the table: ngroups + 1 starts, npoints entries; -1: a bad spec or npoints < 0 */
inline int64_t table_ints(int32_t npoints, const RsEnsSpec *sp) {
  if (cols(sp) < 0 || npoints < 0) return -1;
  return (int64_t)sp->ngroups + 1 + (int64_t)npoints;
}

/* The table of group[npoints] into table[table_ints]: a counting sort by station, stable, so that a station's members
 * come in ascending point index.  0, or -1 with a message in err[errlen]. */
inline int member_table(int32_t npoints, const int32_t *group, const RsEnsSpec *sp, int32_t *table, char *err,
                        size_t errlen) {
  if (table_ints(npoints, sp) < 0) {
    snprintf(err, errlen, "rs_ens_member_table: bad spec (ngroups >= 1, 1 <= max_members <= RS_ENS_MAX_MEMBERS, at most "
                          "RS_ENS_MAX_QUANT quantiles in [0, 1], strictly increasing) or npoints < 0");
    return -1;
  }
  if (!table || (npoints > 0 && !group)) {
    snprintf(err, errlen, "rs_ens_member_table: null argument (a group row and a table are required)");
    return -1;
  }
  const int32_t ng = sp->ngroups;
  int32_t *start = table, *entry = table + (size_t)ng + 1;
  for (int32_t g = 0; g <= ng; ++g) start[g] = 0;
  for (int32_t p = 0; p < npoints; ++p) {
    const int32_t g = group[p];
    if (g >= 0 && g < ng) ++start[g + 1]; /* the members of g, for now */
  }
  for (int32_t g = 0; g < ng; ++g) {
    if (start[g + 1] > sp->max_members) {
      snprintf(err, errlen, "rs_ens_member_table: station %d has %d members, more than max_members = %d", (int)g,
               (int)start[g + 1], (int)sp->max_members);
      return -1;
    }
  }
  for (int32_t g = 0; g < ng; ++g) start[g + 1] += start[g];
  std::vector<int32_t> next(start, start + ng);
  for (int32_t p = 0; p < npoints; ++p) {
    const int32_t g = group[p];
    if (g >= 0 && g < ng) entry[next[g]++] = p;
  }
  for (int32_t e = start[ng]; e < npoints; ++e) entry[e] = -1;
  return 0;
}

}  // namespace rs_ens

#endif
