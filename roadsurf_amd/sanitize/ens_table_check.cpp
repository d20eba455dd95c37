/*
 * ens_table_check.cpp — the member-table builder of the ensemble statistics (csrc/rs_ens_table.hpp) on its own: a
 * program with its own main and nothing of the library or the device in it, to be compiled with
 * -fsanitize=address,undefined (tests/test_ensstats_reference.py does).  Every table sits in a heap block of exactly
 * rs_ens_table_ints ints, so a write past either end is the sanitizer's to report; the contents are checked here
 * against the table's own contract.  Exit status 0 and "ens table check ok": every layout and refusal was as expected.
 */
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/rs_ens_table.hpp"

static int failures = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      ++failures;                    \
      std::printf("FAILED: " __VA_ARGS__); \
      std::printf("\n");             \
    }                                \
  } while (0)

static RsEnsSpec spec_of(int32_t ngroups, int32_t max_members) {
  RsEnsSpec sp;
  std::memset(&sp, 0, sizeof(sp));
  sp.ngroups = ngroups;
  sp.max_members = max_members;
  sp.nquant = 3;
  sp.quant[0] = 0.1;
  sp.quant[1] = 0.5;
  sp.quant[2] = 0.9;
  return sp;
}

/* the contract, stated without the builder's method: starts ascending from 0, station g's entries exactly its points
 * in ascending order, the tail -1 */
static void check_layout(const char *name, const std::vector<int32_t> &group, int32_t ngroups, int32_t max_members) {
  const RsEnsSpec sp = spec_of(ngroups, max_members);
  const int32_t n = (int32_t)group.size();
  const int64_t ints = rs_ens::table_ints(n, &sp);
  EXPECT(ints == (int64_t)ngroups + 1 + n, "%s: table_ints = %lld", name, (long long)ints);
  if (ints < 0) return;
  std::vector<int32_t> exact((size_t)ints); /* (its own heap block: ASan guards both ends) */
  char err[256] = "";
  const int rc = rs_ens::member_table(n, group.data(), &sp, exact.data(), err, sizeof(err));
  EXPECT(rc == 0, "%s: refused: %s", name, err);
  if (rc != 0) return;
  const int32_t *start = exact.data(), *entry = exact.data() + ngroups + 1;
  EXPECT(start[0] == 0, "%s: start[0] = %d", name, start[0]);
  int32_t members = 0;
  for (int32_t p = 0; p < n; ++p) members += group[p] >= 0 && group[p] < ngroups;
  EXPECT(start[ngroups] == members, "%s: start[ngroups] = %d, members = %d", name, start[ngroups], members);
  for (int32_t g = 0; g < ngroups; ++g) {
    EXPECT(start[g + 1] >= start[g] && start[g + 1] - start[g] <= max_members, "%s: station %d: %d .. %d", name, g,
           start[g], start[g + 1]);
    int32_t e = start[g];
    for (int32_t p = 0; p < n; ++p) {
      if (group[p] != g) continue;
      EXPECT(e < start[g + 1] && entry[e] == p, "%s: station %d: entry %d is not point %d", name, g, e, p);
      ++e;
    }
    EXPECT(e == start[g + 1], "%s: station %d has %d entries, its points are %d", name, g, start[g + 1] - start[g],
           e - start[g]);
  }
  for (int32_t e = members; e < n; ++e) EXPECT(entry[e] == -1, "%s: tail entry %d = %d", name, e, entry[e]);
}

static void check_refusal(const char *name, const std::vector<int32_t> &group, const RsEnsSpec &sp, const char *what) {
  const int32_t n = (int32_t)group.size();
  std::vector<int32_t> table((size_t)(sp.ngroups > 0 ? sp.ngroups : 0) + 1 + group.size(), 12345);
  char err[256] = "";
  const int rc = rs_ens::member_table(n, group.data(), &sp, table.data(), err, sizeof(err));
  EXPECT(rc == -1 && std::strstr(err, what), "%s: status %d, message \"%s\" (expected \"%s\")", name, rc, err, what);
}

int main() {
  /* parents(S, M): members of a station side by side */
  for (int S : {1, 13, 70})
    for (int M : {1, 5, 64}) {
      std::vector<int32_t> g;
      for (int s = 0; s < S; ++s)
        for (int m = 0; m < M; ++m) g.push_back(s);
      check_layout("parents", g, S, M);
    }
  /* members of a station far apart, station 69 without a member */
  std::vector<int32_t> irregular(350);
  for (int i = 0; i < 350; ++i) irregular[i] = (i * 37 + 11) % 69;
  check_layout("irregular", irregular, 70, 6);
  /* ids that belong to no station */
  std::vector<int32_t> outside = irregular;
  for (int i = 0; i < 350; i += 7) outside[i] = -1;
  for (int i = 3; i < 350; i += 11) outside[i] = 70 + i % 3;
  outside[349] = INT32_MAX;
  outside[348] = INT32_MIN;
  check_layout("ids outside", outside, 70, 6);
  /* no point at all, and no member at all */
  check_layout("no points", std::vector<int32_t>(), 4, 1);
  check_layout("no members", std::vector<int32_t>(9, -1), 4, 1);
  /* one member too many: the first such station is named */
  std::vector<int32_t> over = irregular; /* stations 0 .. 68 have 5 or 6 members */
  {
    RsEnsSpec sp = spec_of(70, 5);
    int first = -1, cnt[70] = {0};
    for (int v : over) ++cnt[v];
    for (int g = 0; g < 70 && first < 0; ++g)
      if (cnt[g] > 5) first = g;
    char want[64];
    std::snprintf(want, sizeof(want), "station %d has 6 members", first);
    EXPECT(first >= 0, "over: no station with six members");
    check_refusal("one too many", over, sp, want);
  }
  /* bad specs */
  {
    RsEnsSpec sp = spec_of(0, 5);
    check_refusal("ngroups 0", irregular, sp, "bad spec");
    sp = spec_of(70, 0);
    check_refusal("max_members 0", irregular, sp, "bad spec");
    sp = spec_of(70, RS_ENS_MAX_MEMBERS + 1);
    check_refusal("max_members 65", irregular, sp, "bad spec");
    sp = spec_of(70, 6);
    sp.nquant = RS_ENS_MAX_QUANT + 1;
    check_refusal("nine quantiles", irregular, sp, "bad spec");
    sp = spec_of(70, 6);
    sp.quant[1] = 0.1;
    check_refusal("equal quantiles", irregular, sp, "bad spec");
    sp = spec_of(70, 6);
    sp.quant[2] = 1.5;
    check_refusal("quantile above 1", irregular, sp, "bad spec");
    EXPECT(rs_ens::cols(nullptr) < 0 && rs_ens::table_ints(-1, &sp) < 0, "null spec or npoints < 0 accepted");
    sp = spec_of(70, 6);
    EXPECT(rs_ens::cols(&sp) == RS_ENS_COLS + 3, "cols = %d", rs_ens::cols(&sp));
    char err[64];
    EXPECT(rs_ens::member_table(350, irregular.data(), &sp, nullptr, err, sizeof(err)) == -1, "null table accepted");
    EXPECT(rs_ens::member_table(350, nullptr, &sp, over.data(), err, sizeof(err)) == -1, "null group accepted");
  }
  if (failures) {
    std::printf("ens table check: %d failures\n", failures);
    return 1;
  }
  std::printf("ens table check ok\n");
  return 0;
}
