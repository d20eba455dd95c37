/*
 * rs_group_rule.hpp — what a column of a group cell is (include/roadsurf.h, rs_hip_outputs_groups; the definition is
 * roadsurf_amd/groups.py): a count, a minimum or a maximum.  Stated here once, constexpr, for the device (the reducers
 * of rs_cluster.hip) and the host (rs_driver_run's empty cells and the merge of a fan-out's blocks).
 */
#ifndef RS_GROUP_RULE_HPP
#define RS_GROUP_RULE_HPP

#include "../../include/roadsurf.h"

namespace rs_grp {

enum Kind { COUNT, MIN, MAX };

/* column 1: the minimum; column 2 and 9..RS_GRP_COLS-1: maxima; every other column, the histogram included: a count */
constexpr Kind kind(int c) { return c == 1 ? MIN : (c == 2 || (c >= 9 && c < RS_GRP_COLS)) ? MAX : COUNT; }

/* the empty value of column c: counts 0, min +inf, maxima -inf */
constexpr double empty(int c) {
  return kind(c) == MIN ? __builtin_huge_val() : kind(c) == MAX ? -__builtin_huge_val() : 0.0;
}

/* a and b of column c merged: counts add, extremes are the extremes of the two */
constexpr double merge(int c, double a, double b) {
  return kind(c) == MIN ? (b < a ? b : a) : kind(c) == MAX ? (b > a ? b : a) : a + b;
}

}  // namespace rs_grp

#endif
