/*
 * driver_ens_check.cpp — the host rules of the driver's ensemble form (csrc/rs_driver_ens.hpp) on their own: a program
 * with its own main and nothing of the library or the device in it, to be compiled with -fsanitize=address,undefined
 * (tests/test_driver_ensemble_reference.py does).  The branch index is held to a brute-force walk over the simulation
 * times, the parent check and the tile partition to their contracts; every parent row and every table sits in a heap
 * block of exactly its size, so a read or write past either end is the sanitizer's to report.  Exit status 0 and
 * "driver ens check ok": every result and refusal was as expected.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/rs_driver_ens.hpp"

static int failures = 0;
#define EXPECT(cond, ...)                  \
  do {                                     \
    if (!(cond)) {                         \
      ++failures;                          \
      std::printf("FAILED: " __VA_ARGS__); \
      std::printf("\n");                   \
    }                                      \
  } while (0)

/* the definition: the first simulation time at or behind the source's first raw time, found by walking the axis */
static void check_branch(int64_t start, int32_t dt, int32_t L, int32_t step, int64_t first_time) {
  int64_t k = -1;
  for (int64_t i = 0; i < L; ++i)
    if (start + i * dt >= first_time) {
      k = i;
      break;
    }
  const bool ok = first_time > start && k >= 1 && k <= L - 1;
  int32_t B = -7, row = -7;
  char err[400] = "";
  const int rc = rs_dens::branch(start, dt, L, step, first_time, &B, &row, err, sizeof(err));
  EXPECT((rc == 0) == ok, "branch(%lld, dt %d, L %d, first %lld): status %d, expected %s (%s)", (long long)start, dt, L,
         (long long)first_time, rc, ok ? "ok" : "a refusal", err);
  if (rc != 0) {
    EXPECT(B == -7 && row == -7 && err[0], "a refusal wrote its outputs or left no message");
    return;
  }
  int32_t first_row = 0; /* the first kept row r whose index r*step is a member's own */
  while ((int64_t)first_row * step < k) ++first_row;
  EXPECT(B == k && row == first_row, "branch(%lld, dt %d, L %d, step %d, first %lld) = (%d, %d), the walk gives (%lld, %d)",
         (long long)start, dt, L, step, (long long)first_time, B, row, (long long)k, first_row);
}

static void check_parents(const char *name, const std::vector<int32_t> &parent, int32_t S, const char *refusal) {
  std::vector<int32_t> starts;
  char err[400] = "";
  const int rc = rs_dens::check_parent((int32_t)parent.size(), parent.data(), S, starts, err, sizeof(err));
  if (refusal) {
    EXPECT(rc == -1 && std::strstr(err, refusal), "%s: status %d, message \"%s\" (expected \"%s\")", name, rc, err, refusal);
    return;
  }
  EXPECT(rc == 0, "%s: refused: %s", name, err);
  if (rc != 0) return;
  EXPECT((int32_t)starts.size() == S + 1 && starts[0] == 0 && starts[S] == (int32_t)parent.size(), "%s: starts", name);
  for (int32_t s = 0; s < S; ++s)
    for (int32_t q = starts[s]; q < starts[s + 1]; ++q) EXPECT(parent[q] == s, "%s: member %d is not station %d's", name, q, s);
  /* every partition covers the stations once, in order, and no tile passes either limit */
  for (int64_t maxs : {1, 3, 64, 1000})
    for (int64_t maxm : {1, 5, 7, 64, 100000}) {
      const int32_t crowded = rs_dens::first_crowded(starts, maxm);
      int32_t want = -1;
      for (int32_t s = 0; s < S && want < 0; ++s)
        if (starts[s + 1] - starts[s] > maxm) want = s;
      EXPECT(crowded == want, "%s: first_crowded(%lld) = %d, expected %d", name, (long long)maxm, crowded, want);
      if (crowded >= 0) {
        EXPECT(rs_dens::tile_stations(starts, crowded, maxs, maxm) == 0, "%s: a crowded station got a tile", name);
        continue;
      }
      int32_t s0 = 0, tiles = 0;
      while (s0 < S) {
        const int32_t ms = rs_dens::tile_stations(starts, s0, maxs, maxm);
        EXPECT(ms >= 1 && ms <= maxs && s0 + ms <= S && starts[s0 + ms] - starts[s0] <= maxm,
               "%s: tile at station %d: %d stations under (%lld, %lld)", name, s0, ms, (long long)maxs, (long long)maxm);
        if (ms < 1) break;
        /* greedy: the next station would not have fitted */
        if (s0 + ms < S)
          EXPECT(ms == maxs || starts[s0 + ms + 1] - starts[s0] > maxm, "%s: tile at station %d stops early", name, s0);
        s0 += ms;
        ++tiles;
      }
      EXPECT(s0 == S && tiles >= 1, "%s: the tiles end at station %d of %d", name, s0, S);
      EXPECT(rs_dens::tile_stations(starts, S, maxs, maxm) == 0, "%s: a tile behind the last station", name);
    }
}

int main() {
  const int64_t start = 1704844800;
  for (int32_t dt : {30, 7})
    for (int32_t L : {2, 5, 1081})
      for (int32_t step : {1, 20, 120}) {
        /* on a simulation time, between two, one step behind the start (B = 1), at the last index (B = L - 1), at and
         * before the start, at and beyond the end */
        for (int64_t off : {(int64_t)0, (int64_t)-1, (int64_t)-3600, (int64_t)1, (int64_t)dt, (int64_t)dt + 1,
                            (int64_t)dt * 2 - 1, (int64_t)dt * (L / 2), (int64_t)dt * (L / 2) + dt / 2,
                            (int64_t)dt * (L - 2) + 1, (int64_t)dt * (L - 1), (int64_t)dt * (L - 1) + 1, (int64_t)dt * L,
                            (int64_t)dt * L * 1000})
          check_branch(start, dt, L, step, start + off);
      }
  /* axes at the ends of int64: no sum or difference leaves the type */
  check_branch(INT64_MIN + 5, 30, 100, 20, INT64_MIN + 5 + 90);
  {
    int32_t B = 0, row = 0;
    char err[400] = "";
    EXPECT(rs_dens::branch(INT64_MIN, 30, 100, 20, INT64_MAX, &B, &row, err, sizeof(err)) == -1 && std::strstr(err, "outside"),
           "the widest axis: %s", err);
    EXPECT(rs_dens::branch(INT64_MAX - 10, 1, 100, 20, INT64_MAX, &B, &row, err, sizeof(err)) == 0 && B == 10 && row == 1,
           "the axis at INT64_MAX: (%d, %d) %s", B, row, err);
    EXPECT(rs_dens::branch(0, 0, 100, 20, 5, &B, &row, err, sizeof(err)) == -1, "dt = 0 accepted");
    EXPECT(rs_dens::branch(0, 30, 100, 0, 5, &B, &row, err, sizeof(err)) == -1, "step = 0 accepted");
  }

  /* parent rows: ragged with an empty station, S x M, one member, empty stations at both ends */
  std::vector<int32_t> ragged;
  for (int s = 0; s < 37; ++s)
    for (int m = 0; m < (s * 7 + 3) % 6; ++m) ragged.push_back(s);
  check_parents("ragged", ragged, 37, nullptr);
  check_parents("ragged, stations behind", ragged, 50, nullptr);
  std::vector<int32_t> sm;
  for (int s = 0; s < 13; ++s)
    for (int m = 0; m < 5; ++m) sm.push_back(s);
  check_parents("13 x 5", sm, 13, nullptr);
  check_parents("one member", std::vector<int32_t>(1, 0), 1, nullptr);
  check_parents("one member of the last station", std::vector<int32_t>(1, 8), 9, nullptr);
  check_parents("257 x 1", [] { std::vector<int32_t> v; for (int s = 0; s < 257; ++s) v.push_back(s); return v; }(), 257, nullptr);
  /* refusals name the first offending member */
  std::vector<int32_t> bad = sm;
  bad[17] = 13;
  check_parents("parent = S", bad, 13, "member 17: parent 13 outside");
  bad = sm;
  bad[4] = -1;
  check_parents("parent < 0", bad, 13, "member 4: parent -1 outside");
  bad = sm;
  bad[30] = 2;
  check_parents("decreasing", bad, 13, "member 30: parent 2 below member 29's parent 5");
  check_parents("no member", std::vector<int32_t>(), 13, "n_members >= 1");
  {
    std::vector<int32_t> starts;
    char err[400] = "";
    EXPECT(rs_dens::check_parent(5, nullptr, 13, starts, err, sizeof(err)) == -1, "null parent accepted");
    EXPECT(rs_dens::check_parent(5, sm.data(), 0, starts, err, sizeof(err)) == -1, "no station accepted");
  }
  if (failures) {
    std::printf("driver ens check: %d failures\n", failures);
    return 1;
  }
  std::printf("driver ens check ok\n");
  return 0;
}
