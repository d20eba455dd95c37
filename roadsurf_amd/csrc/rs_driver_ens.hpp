/*
 * rs_driver_ens.hpp — the host rules of the driver's ensemble form (include/roadsurf.h, rs_driver_run_ensemble): where
 * the members branch off their stations, what a parent row must be, and how the stations are cut into tiles whose
 * members fit.  Plain C++ without HIP, so that a stand-alone program can compile it (sanitize/driver_ens_check.cpp,
 * which tests/test_driver_ensemble_reference.py builds under ASan + UBSan).  roadsurf_amd/driver.py (branch_index,
 * member_rows, check_parent) states the same rules in Python.
 */
#ifndef RS_DRIVER_ENS_HPP
#define RS_DRIVER_ENS_HPP

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace rs_dens {

/* JsonSource::interpolate writes nothing to a simulation time before a source's first raw time
 * (JsonSource.cpp:61-84), so with k_b the smallest 0-based simulation index whose time start_time + k*dt is at or
 * behind first_time, the indices k < k_b do not see the source: B = k_b is the last shared 1-based time index, and
 * kept row r - 0-based index r*step (roadrunner.cpp:303) - is a member's own from first_row = ceil(k_b / step) on.
 * 0, or -1 with the reason in err: first_time <= start_time, or B outside [1, simlen - 1]. */
inline int branch(int64_t start_time, int32_t dt, int32_t simlen, int32_t step, int64_t first_time, int32_t *B,
                  int32_t *first_row, char *err, size_t errlen) {
  if (dt < 1 || simlen < 1 || step < 1) {
    snprintf(err, errlen, "rs_driver_run_ensemble: DTSecs >= 1, SimLen >= 1 and an output step >= 1 are required");
    return -1;
  }
  if (first_time <= start_time) {
    snprintf(err, errlen, "rs_driver_run_ensemble: the member source starts at %lld, at or before start_time = %lld: "
                          "times[0] > start_time is required (index 1 is the stations')",
             (long long)first_time, (long long)start_time);
    return -1;
  }
  /* (unsigned: the difference of two int64 that are in order is below 2^64) */
  const uint64_t diff = (uint64_t)first_time - (uint64_t)start_time;
  const uint64_t k = diff / (uint64_t)dt + (diff % (uint64_t)dt ? 1 : 0);
  if (k > (uint64_t)(simlen - 1)) {
    snprintf(err, errlen, "rs_driver_run_ensemble: the member source starts behind the last simulation index but one: "
                          "B = %llu outside [1, SimLen - 1 = %d] (both the stations and the members need an index)",
             (unsigned long long)k, (int)(simlen - 1));
    return -1;
  }
  *B = (int32_t)k;
  *first_row = (int32_t)((k + (uint64_t)step - 1) / (uint64_t)step);
  return 0;
}

/* parent[n_members]: non-decreasing, every entry in [0, n_stations) - the members of a station side by side, a
 * station may have none.  On success starts[n_stations + 1]: station s has the members starts[s] .. starts[s + 1] - 1.
 * 0, or -1 with the first offending member named in err. */
inline int check_parent(int32_t n_members, const int32_t *parent, int32_t n_stations, std::vector<int32_t> &starts,
                        char *err, size_t errlen) {
  if (n_members < 1 || n_stations < 1 || !parent) {
    snprintf(err, errlen, "rs_driver_run_ensemble: n_members >= 1, n_stations >= 1 and a parent row are required");
    return -1;
  }
  starts.assign((size_t)n_stations + 1, 0);
  for (int32_t q = 0; q < n_members; ++q) {
    const int32_t s = parent[q];
    if (s < 0 || s >= n_stations) {
      snprintf(err, errlen, "rs_driver_run_ensemble: member %d: parent %d outside [0, n_stations = %d)", (int)q, (int)s,
               (int)n_stations);
      return -1;
    }
    if (q > 0 && s < parent[q - 1]) {
      snprintf(err, errlen, "rs_driver_run_ensemble: member %d: parent %d below member %d's parent %d: parent must be "
                            "non-decreasing (the members of a station side by side)",
               (int)q, (int)s, (int)(q - 1), (int)parent[q - 1]);
      return -1;
    }
    ++starts[(size_t)s + 1];
  }
  for (int32_t s = 0; s < n_stations; ++s) starts[(size_t)s + 1] += starts[s];
  return 0;
}

/* the first station with more than max_points members, or -1 */
inline int32_t first_crowded(const std::vector<int32_t> &starts, int64_t max_points) {
  for (size_t s = 0; s + 1 < starts.size(); ++s)
    if ((int64_t)starts[s + 1] - starts[s] > max_points) return (int32_t)s;
  return -1;
}

/* The tile that begins at station s0: the longest run of whole stations [s0, s0 + ms) with ms <= max_stations whose
 * members, starts[s0] .. starts[s0 + ms] - 1, number at most max_members.  Returns ms; 0: station s0 alone has more
 * members than that (first_crowded tells beforehand), or s0 is the end. */
inline int32_t tile_stations(const std::vector<int32_t> &starts, int32_t s0, int64_t max_stations, int64_t max_members) {
  const int32_t S = (int32_t)starts.size() - 1;
  int32_t ms = 0;
  while (s0 + ms < S && ms + 1 <= max_stations && (int64_t)starts[(size_t)s0 + ms + 1] - starts[s0] <= max_members) ++ms;
  return ms;
}

}  // namespace rs_dens

#endif
