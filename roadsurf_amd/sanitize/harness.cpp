// Drives the product's host code from many threads, as the reference driver's worker pool does (/root/reference/
// examples/example1/src/WorkQueue.h:16-129, roadrunner.cpp:454-497), in the sanitizer builds (`make tsan`, `make
// asan`): the library is compiled host-only against sanitize/hip_stub.cpp - a device that never computes - so
// results mean nothing and every race / invalid access of the host side is reported.
//   phase 1  T threads x N points through `runsimulation`, two groups of settings (SimLen differs), the coalescer
//            limited to ROADSURF_HIP_COALESCE_MAX callers per batch (set by the test: 5 < threads)
//   phase 2  threads that come and go (thread-local caches adopted by later threads, rs_host.hip CallerCache)
//   phase 3  four concurrent runsimulation_batch calls of different sizes (arena / plan bookkeeping)
//   phase 4  rs_driver_run_episodes, the older entry that fills every member of an RsDriverRequest (rs_driver_run and
//            its kin are wrappers of the same run with fewer members set), with and without the summaries from
//            three threads (shards, segment table, per-block worker threads, the blocks' merge into the one array of
//            group series, the blocks' rows of the kept inputs, the deficit and the threshold episodes)
//   phase 5  the device API's answers to its arguments, single-threaded and independent of the two arguments below:
//            one accepted call per path and one rejected call per rejection of the step entry points and the row
//            consumers, one line each between two marker lines (tests/golden/api_argument_record.txt)
// usage: harness [threads=64] [points=640]      exit code 0 and "sanitize harness ok" when every call returned
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "roadsurf.h"

namespace {

struct PointData {
  std::vector<double> tair, tdew, vz, rhz, prec, sw, lw, sw_dir, lw_net, obs, depth, hz;
  std::vector<int32_t> phase, year, month, day, hour, minute, second;
  std::vector<double> out[6];
  explicit PointData(int L)
      : tair(L, -3.0), tdew(L, -5.0), vz(L, 2.0), rhz(L, 85.0), prec(L, 0.0), sw(L, 50.0), lw(L, 270.0), sw_dir(L, 30.0),
        lw_net(L, -40.0), obs(L, -9999.9), depth(L, -9999.9), hz(360, 0.0), phase(L, -9999), year(L, 2024), month(L, 1),
        day(L, 10), hour(L), minute(L), second(L) {
    for (auto &o : out) o.assign(L, -9999.0);
    for (int t = 0; t < L; ++t) {
      const int sec = t * 30;
      hour[t] = (sec / 3600) % 24;
      minute[t] = (sec / 60) % 60;
      second[t] = sec % 60;
    }
    obs[0] = -3.5;
  }
  void pointers(InputPointers &ip, OutputPointers &op, int L) {
    std::memset(&ip, 0, sizeof(ip));
    ip.inputLen = L;
    ip.c_tair = tair.data(); ip.c_tdew = tdew.data(); ip.c_VZ = vz.data(); ip.c_Rhz = rhz.data();
    ip.c_prec = prec.data(); ip.c_SW = sw.data(); ip.c_LW = lw.data(); ip.c_SW_dir = sw_dir.data();
    ip.c_LW_net = lw_net.data(); ip.c_TSurfObs = obs.data(); ip.c_PrecPhase = phase.data();
    ip.c_local_horizons = hz.data(); ip.c_Depth = depth.data();
    ip.c_year = year.data(); ip.c_month = month.data(); ip.c_day = day.data();
    ip.c_hour = hour.data(); ip.c_minute = minute.data(); ip.c_second = second.data();
    op.outputLen = L;
    op.c_TsurfOut = out[0].data(); op.c_SnowOut = out[1].data(); op.c_WaterOut = out[2].data();
    op.c_IceOut = out[3].data(); op.c_DepositOut = out[4].data(); op.c_Ice2Out = out[5].data();
  }
};

struct Group {
  int L;
  InputSettings s;
  InputParameters p;
  LocalParameters l;
  explicit Group(int L_) : L(L_) {
    rs_default_settings(&s, L);
    rs_default_parameters(&p, s.DTSecs);
    rs_default_local(&l);
    l.InitLenI = 1;
  }
};

std::atomic<int> g_errors{0};

void one_point_calls(const Group &g, std::atomic<int> &next, int N) {
  PointData d(g.L);
  for (;;) {
    const int pt = next.fetch_add(1);
    if (pt >= N) break;
    d.tair[1] = -3.0 + 0.001 * pt;
    InputPointers ip;
    OutputPointers op;
    d.pointers(ip, op, g.L);
    LocalParameters l = g.l;
    runsimulation(&op, &ip, &g.s, &g.p, &l);
    if (d.out[0][g.L - 1] < -9000.0) { /* runsimulation's own failure mark */
      fprintf(stderr, "runsimulation failed for point %d: %s\n", pt, rs_last_error());
      g_errors++;
    }
  }
}

void batch_call(const Group &g, int n) {
  std::vector<PointData> pts;
  pts.reserve(n);
  for (int k = 0; k < n; ++k) pts.emplace_back(g.L);
  std::vector<InputPointers> ip(n);
  std::vector<OutputPointers> op(n);
  std::vector<LocalParameters> l(n, g.l);
  for (int k = 0; k < n; ++k) pts[k].pointers(ip[k], op[k], g.L);
  int32_t st = 99;
  std::vector<int32_t> ff(n, -1);
  runsimulation_batch_ex(n, op.data(), ip.data(), &g.s, &g.p, l.data(), &st, ff.data());
  if (st != 0) {
    fprintf(stderr, "runsimulation_batch_ex(%d) -> %d: %s\n", n, st, rs_last_error());
    g_errors++;
  }
}

/* rs_driver_run: an hourly forecast on a shared axis + 10-minute observations on per-point axes (the shape of
 * examples/example1's two JSON files), `n` points, relaxation (and coupling) on: the host side cuts shards over
 * ROADSURF_HIP_DEVICES, builds the segment table of the raw times and runs one worker thread per block.
 * `gridded`: the forecast goes in as fields with two-node stencils (rs_driver_run_grid): the calling thread checks
 * the stencils and uploads the fields once per device, the blocks' tiles upload their slices of the stencils */
void driver_call(int n, int hours, bool coupling, bool gridded = false) {
  const int L = hours * 120 + 1, nf = hours + 1, no = 6 * 3 + 1; /* observations over the first three hours */
  const int64_t t0 = 1704844800; /* 2024-01-10 00:00 UTC */
  std::vector<int64_t> tf(nf), to((size_t)n * no);
  std::vector<int32_t> olen(n);
  for (int k = 0; k < nf; ++k) tf[k] = t0 + 3600 * k;
  auto series = [&](size_t w, double base) {
    std::vector<double> v((size_t)n * w);
    for (size_t q = 0; q < v.size(); ++q) v[q] = base + 0.01 * (double)(q % 37);
    return v;
  };
  std::vector<double> f_tair = series(nf, -4.0), f_rh = series(nf, 80.0), f_vz = series(nf, 2.0), f_prec = series(nf, 0.0),
                      f_sw = series(nf, 40.0), f_lw = series(nf, 260.0), f_swd = series(nf, 20.0), f_lwn = series(nf, -40.0);
  std::vector<double> o_tair = series(no, -3.5), o_rh = series(no, 82.0), o_vz = series(no, 1.5), o_ts = series(no, -2.0);
  for (int p = 0; p < n; ++p) {
    olen[p] = no - (p % 3); /* ragged: some stations stop reporting early */
    for (int k = 0; k < no; ++k) to[(size_t)p * no + k] = t0 + 600 * k;
  }
  RsRawSource src[2];
  std::memset(src, 0, sizeof(src));
  src[0].n_times = nf; src[0].times = tf.data();
  src[0].tair = f_tair.data(); src[0].rhz = f_rh.data(); src[0].vz = f_vz.data(); src[0].prec = f_prec.data();
  src[0].sw = f_sw.data(); src[0].lw = f_lw.data(); src[0].sw_dir = f_swd.data(); src[0].lw_net = f_lwn.data();
  src[1].n_times = no; src[1].is_observation = 1; src[1].times = to.data(); src[1].times_per_point = 1;
  src[1].lengths = olen.data();
  src[1].tair = o_tair.data(); src[1].rhz = o_rh.data(); src[1].vz = o_vz.data(); src[1].tsurfobs = o_ts.data();
  RsGridSource grid;
  std::memset(&grid, 0, sizeof(grid));
  std::vector<int32_t> node((size_t)n * 2);
  std::vector<double> weight((size_t)n * 2);
  const RsGridSource *grids[2] = {gridded ? &grid : nullptr, nullptr};
  if (gridded) { /* the same arrays read as [nf][n_nodes = n] */
    grid.n_nodes = n; grid.stencil = 2; grid.node = node.data(); grid.weight = weight.data();
    grid.tair = src[0].tair; grid.rhz = src[0].rhz; grid.vz = src[0].vz; grid.prec = src[0].prec;
    grid.sw = src[0].sw; grid.lw = src[0].lw; grid.sw_dir = src[0].sw_dir; grid.lw_net = src[0].lw_net;
    src[0].tair = src[0].rhz = src[0].vz = src[0].prec = src[0].sw = src[0].lw = src[0].sw_dir = src[0].lw_net = nullptr;
    for (int p = 0; p < n; ++p) {
      node[(size_t)p * 2] = p; node[(size_t)p * 2 + 1] = (p % 5) ? (p + 1) % n : -1; /* (-1 under a zero weight) */
      weight[(size_t)p * 2] = (p % 5) ? 0.75 : 1.0; weight[(size_t)p * 2 + 1] = (p % 5) ? 0.25 : 0.0;
    }
  }
  std::vector<int32_t> yy(L, 2024), mo(L, 1), dd(L, 10), hh(L), mi(L), ss(L);
  for (int t = 0; t < L; ++t) { hh[t] = (t / 120) % 24; mi[t] = (t / 2) % 60; ss[t] = (t % 2) * 30; }
  RsDriverInput in;
  std::memset(&in, 0, sizeof(in));
  in.n_points = n; in.n_sources = 2; in.sources = src; in.start_time = t0; in.forecast_time = t0 + 3 * 3600;
  in.year = yy.data(); in.month = mo.data(); in.day = dd.data(); in.hour = hh.data(); in.minute = mi.data(); in.second = ss.data();
  InputSettings s;
  InputParameters p;
  rs_default_settings(&s, L);
  rs_default_parameters(&p, s.DTSecs);
  s.use_relaxation = 1;
  s.use_coupling = coupling ? 1 : 0;
  std::vector<LocalParameters> local(n);
  for (auto &l : local) rs_default_local(&l);
  const int step = (int)((double)(s.outputStep * 60) / s.DTSecs), n_out = (L + step - 1) / step;
  std::vector<double> o[6];
  for (auto &v : o) v.assign((size_t)n * n_out, -9999.0);
  std::vector<int32_t> status(n, -1), missing(n, -2);
  RsDriverOutput out;
  out.n_out = n_out;
  out.tsurf = o[0].data(); out.snow = o[1].data(); out.water = o[2].data(); out.ice = o[3].data(); out.deposit = o[4].data();
  out.ice2 = o[5].data(); out.status = status.data(); out.missing_index = missing.data();
  /* the coupled call also asks for the per-point summaries of the second half of its rows: every block's worker fills
   * its points' rows of the one host array */
  std::vector<double> sums((size_t)n * RS_SUM_COLS, -1.0);
  RsDriverSummary q;
  std::memset(&q, 0, sizeof(q));
  q.first_row = n_out / 2;
  q.last_row = n_out - 1;
  q.summary = sums.data();
  /* ... and both calls for the group series of the same rows, three groups with bins: every block's worker merges its
   * cells into the one host array */
  RsDriverGroups g;
  std::memset(&g, 0, sizeof(g));
  g.spec.ngroups = 3;
  g.spec.nedges = 2;
  g.spec.edges[0] = -1.0;
  g.spec.edges[1] = 1.0;
  std::vector<int32_t> gid(n);
  for (int k = 0; k < n; ++k) gid[k] = k % 4 - 1; /* -1: no group */
  const int32_t gcols = rs_hip_group_cols(&g.spec);
  if (gcols != RS_GRP_COLS + 3) {
    fprintf(stderr, "rs_hip_group_cols -> %d\n", gcols);
    g_errors++;
    return;
  }
  std::vector<double> cells((size_t)(n_out - n_out / 2) * 3 * gcols, -1.0);
  g.group = gid.data();
  g.first_row = n_out / 2;
  g.last_row = n_out - 1;
  g.series = cells.data();
  /* ... and the coupled call for three of the inputs at the kept rows and the dew-point deficit: every block's worker
   * fills its points' rows of the host arrays */
  std::vector<double> k_tair((size_t)n * n_out, -1.0), k_tdew(k_tair), k_obs(k_tair), k_def(k_tair);
  RsDriverKept kept;
  std::memset(&kept, 0, sizeof(kept));
  kept.merged[0] = k_tair.data();
  kept.merged[1] = k_tdew.data();
  kept.merged[9] = k_obs.data();
  kept.deficit = k_def.data();
  if (rs_driver_kept_fields() != 10) {
    fprintf(stderr, "rs_driver_kept_fields -> %d\n", rs_driver_kept_fields());
    g_errors++;
    return;
  }
  /* ... and the coupled and the gridded call for the threshold episodes of the same rows, "Tsurf < 0 and deficit < 0":
   * the coupled call's tiles make the deficit once for both, the gridded call's for the episodes alone; every block's
   * worker fills its points' rows of the one host array */
  RsDriverEpisodes epi;
  std::memset(&epi, 0, sizeof(epi));
  epi.spec.use = 1 | (1 << 6);
  epi.spec.peak = 6;
  epi.spec.min_rows = 1;
  epi.spec.max_episodes = 3;
  for (int k = 0; k < RS_EPI_VARS; ++k) { epi.spec.above[k] = -HUGE_VAL; epi.spec.below[k] = k == 0 || k == 6 ? 0.0 : HUGE_VAL; }
  const int32_t ecols = rs_hip_episode_cols(&epi.spec);
  if (ecols != RS_EPI_HEAD + 3 * RS_EPI_REC) {
    fprintf(stderr, "rs_hip_episode_cols -> %d\n", ecols);
    g_errors++;
    return;
  }
  std::vector<double> erows((size_t)n * ecols, -1.0);
  epi.first_row = n_out / 2;
  epi.last_row = n_out - 1;
  epi.episodes = erows.data();
  const int rc = rs_driver_run_episodes(&in, gridded ? grids : nullptr, &s, &p, local.data(), &out, coupling ? &q : nullptr,
                                        &g, coupling ? &kept : nullptr, coupling || gridded ? &epi : nullptr, -1);
  if (rc != 0) {
    fprintf(stderr, "rs_driver_run(%d points) -> %d: %s\n", n, rc, rs_last_error());
    g_errors++;
  }
  if (rc == 0 && (coupling || gridded)) { /* every block wrote its points' rows: nothing of the fill is left */
    size_t left = 0;
    for (double v : erows) left += v == -1.0 ? 1 : 0;
    if (left) {
      fprintf(stderr, "rs_driver_run_episodes(%d points): %zu of %zu episode columns never written\n", n, left, erows.size());
      g_errors++;
    }
  }
}

/* ---- phase 5: the device API's answers to its arguments -------------------------------------------------------------
 * On the stub a "device" pointer is a host buffer: one zeroed block of doubles and one of int32 stand for every stream,
 * row and accumulator (nothing computes, so nothing is written to them). */
extern "C" long rs_stub_kernel_launches(void);

/* one record line: entry point | case | status | kernel launches of the call | rs_last_error() after it.  A call that
 * fails on purpose comes first, so that a call that leaves the thread's message alone reads "(untouched)" */
template <class F>
void api_call(const char *fn, const char *name, F &&call) {
  rs_hip_sync(nullptr);
  const std::string before = rs_last_error();
  const long l0 = rs_stub_kernel_launches();
  const int st = call();
  const long launches = rs_stub_kernel_launches() - l0;
  const std::string after = rs_last_error();
  printf("%s | %s | status %d | launches %ld | %s\n", fn, name, st, launches, after == before ? "(untouched)" : after.c_str());
}

struct ApiArgs {
  static constexpr int NP = 130, PAD = 256, L = 240; /* npoints < np_pad; SimLen */
  std::vector<double> z = std::vector<double>((size_t)L * PAD, 0.0);
  std::vector<int32_t> zi = std::vector<int32_t>((size_t)L * PAD, 0);
  int fake_stream = 0;
  void *stream() { return &fake_stream; }
  RsPlan *plan(bool coupling, int bits) {
    InputSettings s;
    InputParameters p;
    rs_default_settings(&s, L);
    rs_default_parameters(&p, s.DTSecs);
    s.use_relaxation = 1; /* (acts only where a call passes tair_relax) */
    s.use_coupling = coupling ? 1 : 0;
    RsConstants c;
    int32_t status = -1;
    rs_build_constants(&s, &p, &c, &status);
    RsPlan *pl = status == 0 ? rs_hip_plan_create(0, NP, &c, nullptr) : nullptr;
    if (pl && bits == 32 && rs_hip_set_precision(pl, 32) != 0) pl = nullptr;
    if (!pl) {
      fprintf(stderr, "phase 5: no plan: %s\n", rs_last_error());
      g_errors++;
    }
    return pl;
  }
  RsForcing forcing(bool full = false, bool sky = false) {
    RsForcing f;
    std::memset(&f, 0, sizeof(f));
    f.tair = f.vz = f.rhz = f.prec = f.sw = f.lw = z.data();
    f.precphase = f.hour = zi.data();
    f.t_stride = PAD;
    if (full) f.tdew = z.data();
    if (sky) f.sw_dir = f.lw_net = f.sun = z.data();
    return f;
  }
  RsOutputs outputs() {
    RsOutputs o;
    std::memset(&o, 0, sizeof(o));
    o.tsurf = o.snow = o.water = o.ice = o.deposit = o.ice2 = z.data();
    o.t_stride = PAD;
    o.decimate = 1;
    return o;
  }
  RsPointParams params(bool sky = false, bool coupling = false) {
    RsPointParams pp;
    std::memset(&pp, 0, sizeof(pp));
    pp.tbottom = z.data();
    if (sky) pp.sky_view = pp.sin_lat = pp.cos_lat = pp.lon_rad = z.data();
    if (coupling) {
      pp.coupling_index = zi.data();
      pp.coupling_tsurf = z.data();
    }
    return pp;
  }
};

void api_step_cases(ApiArgs &A, RsPlan *pa, RsPlan *pb, RsPlan *pc, RsPlan *pd) {
  const char *fn = "rs_hip_step";
  auto step = [&](const char *name, RsPlan *pl, RsForcing f, RsOutputs o, RsPointParams pp, int t0 = 1, int ns = ApiArgs::L) {
    api_call(fn, name, [&] { return rs_hip_step(pl, &f, &o, &pp, t0, ns); });
  };
  auto accepted = [&](const char *suffix) {
    const std::string s = suffix;
    step(("LEAN" + s).c_str(), pa, A.forcing(), A.outputs(), A.params());
    step(("FULL" + s).c_str(), pa, A.forcing(true), A.outputs(), A.params());
    step(("sky view" + s).c_str(), pa, A.forcing(true, true), A.outputs(), A.params(true));
    step(("coupled whole series" + s).c_str(), pb, A.forcing(true), A.outputs(), A.params(false, true));
  };
  accepted("");
  step("fp32 LEAN", pc, A.forcing(), A.outputs(), A.params());
  step("fp32 coupled whole series", pd, A.forcing(true), A.outputs(), A.params(false, true));
  step("a window inside the series, decimated", pa, A.forcing(), [&] { RsOutputs o = A.outputs(); o.decimate = 4; o.row0 = 3; return o; }(),
       A.params(), 11, 50);
  /* one thing wrong each */
  step("null plan", nullptr, A.forcing(), A.outputs(), A.params());
  { RsForcing f = A.forcing(); f.hour = nullptr; step("forcing without hour", pa, f, A.outputs(), A.params()); }
  { RsForcing f = A.forcing(); f.t_stride = ApiArgs::NP - 1; step("forcing t_stride below npoints", pa, f, A.outputs(), A.params()); }
  { RsPointParams pp = A.params(); pp.tbottom = nullptr; step("no tbottom", pa, A.forcing(), A.outputs(), pp); }
  { RsOutputs o = A.outputs(); o.ice2 = nullptr; step("output without ice2", pa, A.forcing(), o, A.params()); }
  { RsOutputs o = A.outputs(); o.t_stride = ApiArgs::NP - 1; step("output t_stride below npoints", pa, A.forcing(), o, A.params()); }
  { RsOutputs o = A.outputs(); o.decimate = 0; step("decimate 0", pa, A.forcing(), o, A.params()); }
  step("t0 = 0", pa, A.forcing(), A.outputs(), A.params(), 0, 10);
  { RsOutputs o = A.outputs(); o.row0 = 1; step("row0 beyond the first row", pa, A.forcing(), o, A.params()); }
  { RsPointParams pp = A.params(); pp.tair_relax = A.z.data(); step("tair_relax alone", pa, A.forcing(), A.outputs(), pp); }
  { RsForcing f = A.forcing(true, true); f.sun = nullptr; step("sky view without sun", pa, f, A.outputs(), A.params(true)); }
  { RsForcing f = A.forcing(true, true); f.hour_pstride = 1; step("sky view with per-point hours", pa, f, A.outputs(), A.params(true)); }
  { RsPointParams pp = A.params(false, true); pp.coupling_tsurf = nullptr; step("coupling without coupling_tsurf", pb, A.forcing(true), A.outputs(), pp); }
  step("coupling over part of the series", pb, A.forcing(true), A.outputs(), A.params(false, true), 1, 10);
  step("coupled plan without coupling_index", pb, A.forcing(true), A.outputs(), A.params());
  if (RsPlan *pe = A.plan(false, 64)) { /* diagnostics switched on while fp64, then the plan made an fp32 one */
    if (rs_hip_set_diagnostics(pe, 1) != 0 || rs_hip_set_precision(pe, 32) != 0) g_errors++;
    step("fp32 with diagnostics", pe, A.forcing(), A.outputs(), A.params());
    rs_hip_plan_destroy(pe);
  }
  if (rs_hip_set_writeback(pc, A.z.data(), A.z.data(), A.z.data(), ApiArgs::PAD) != 0) g_errors++;
  step("fp32 sky view with write-back", pc, A.forcing(true, true), A.outputs(), A.params(true));
  if (rs_hip_set_writeback(pc, nullptr, nullptr, nullptr, 0) != 0) g_errors++;
  /* timed: the accepted calls once more and a rejected one, which must leave the event pairs alone */
  if (rs_hip_timing_reset(pa) != 0 || rs_hip_timing_reset(pb) != 0) g_errors++;
  accepted(", timed");
  { RsOutputs o = A.outputs(); o.decimate = 0; step("decimate 0, timed", pa, A.forcing(), o, A.params()); }
}

void api_knots_cases(ApiArgs &A, RsPlan *pa, RsPlan *pb, RsPlan *pc) {
  const char *fn = "rs_hip_step_knots";
  RsSynthSpec spec;
  std::memset(&spec, 0, sizeof(spec));
  spec.steps_per_knot = 120;
  auto step = [&](const char *name, RsPlan *pl, RsSynthSpec sp, const double *knots, int nknots, RsOutputs o, RsPointParams pp,
                  int t0 = 1, int ns = ApiArgs::L) {
    api_call(fn, name, [&] { return rs_hip_step_knots(pl, &sp, knots, 0, nknots, &o, &pp, t0, ns); });
  };
  const double *k = A.z.data();
  auto full = [&] { RsPointParams pp = A.params(); pp.initlen = A.zi.data(); return pp; };
  step("LEAN, timed", pa, spec, k, 3, A.outputs(), A.params());
  step("FULL, timed", pa, spec, k, 3, A.outputs(), full());
  step("fp32 LEAN", pc, spec, k, 3, A.outputs(), A.params());
  step("no knots", pa, spec, nullptr, 3, A.outputs(), A.params());
  { RsPointParams pp = A.params(); pp.tbottom = nullptr; step("no tbottom", pa, spec, k, 3, A.outputs(), pp); }
  { RsOutputs o = A.outputs(); o.tsurf = nullptr; step("output without tsurf", pa, spec, k, 3, o, A.params()); }
  { RsOutputs o = A.outputs(); o.t_stride = ApiArgs::NP - 1; step("output t_stride below npoints", pa, spec, k, 3, o, A.params()); }
  { RsOutputs o = A.outputs(); o.decimate = 0; step("decimate 0", pa, spec, k, 3, o, A.params()); }
  step("window beyond SimLen", pa, spec, k, 3, A.outputs(), A.params(), 2, ApiArgs::L);
  { RsSynthSpec sp = spec; sp.steps_per_knot = 0; step("steps_per_knot 0", pa, sp, k, 3, A.outputs(), A.params()); }
  step("too few knots", pa, spec, k, 2, A.outputs(), A.params());
  { RsOutputs o = A.outputs(); o.row0 = 1; step("row0 beyond the first row", pa, spec, k, 3, o, A.params()); }
  step("sky view", pa, spec, k, 3, A.outputs(), A.params(true));
  step("coupling", pb, spec, k, 3, A.outputs(), A.params(false, true));
  { RsPointParams pp = full(); pp.tair_relax = pp.vz_relax = A.z.data(); step("relaxation without rh_relax", pa, spec, k, 3, A.outputs(), pp); }
}

/* rs_hip_step_cpl and rs_hip_cpl_replay share their checks: the same cases through both */
void api_cpl_cases(ApiArgs &A, RsPlan *pa, RsPlan *pb, RsPlan *pd, bool replay) {
  const char *fn = replay ? "rs_hip_cpl_replay" : "rs_hip_step_cpl";
  auto step = [&](const char *name, RsPlan *pl, RsForcing f, RsOutputs o, RsPointParams pp, int t0 = 1, int ns = 100) {
    api_call(fn, name, [&] {
      int32_t rounds = -1;
      return replay ? rs_hip_cpl_replay(pl, &f, &o, &pp, t0, ns, &rounds) : rs_hip_step_cpl(pl, &f, &o, &pp, t0, ns);
    });
  };
  if (replay) {
    unsetenv("ROADSURF_HIP_CPL_REPLAY");
    step("ROADSURF_HIP_CPL_REPLAY unset", pb, A.forcing(true), A.outputs(), A.params(false, true));
    setenv("ROADSURF_HIP_CPL_REPLAY", "general", 1);
    step("ROADSURF_HIP_CPL_REPLAY=general", pb, A.forcing(true), A.outputs(), A.params(false, true));
    setenv("ROADSURF_HIP_CPL_REPLAY", "lockstep", 1);
    step("ROADSURF_HIP_CPL_REPLAY=lockstep", pb, A.forcing(true), A.outputs(), A.params(false, true));
    unsetenv("ROADSURF_HIP_CPL_REPLAY");
    step("a block that ends at SimLen", pb, A.forcing(true), A.outputs(), A.params(false, true), 141, 100);
  } else {
    step("a chunk", pb, A.forcing(true), A.outputs(), A.params(false, true));
    step("the last chunk", pb, A.forcing(true), A.outputs(), A.params(false, true), 141, 100);
  }
  step("sky view", pb, A.forcing(true, true), A.outputs(), A.params(true, true));
  step("null plan", nullptr, A.forcing(true), A.outputs(), A.params(false, true));
  { RsForcing f = A.forcing(true); f.tair = nullptr; step("forcing without tair", pb, f, A.outputs(), A.params(false, true)); }
  { RsForcing f = A.forcing(true); f.t_stride = ApiArgs::NP - 1; step("forcing t_stride below npoints", pb, f, A.outputs(), A.params(false, true)); }
  { RsPointParams pp = A.params(false, true); pp.coupling_tsurf = nullptr; step("no coupling_tsurf", pb, A.forcing(true), A.outputs(), pp); }
  step("plan without coupling", pa, A.forcing(true), A.outputs(), A.params(false, true));
  step("fp32 plan", pd, A.forcing(true), A.outputs(), A.params(false, true));
  { RsForcing f = A.forcing(true, true); f.lw_net = nullptr; step("sky view without lw_net", pb, f, A.outputs(), A.params(true, true)); }
  { RsForcing f = A.forcing(true, true); f.hour_pstride = 1; step("sky view with per-point hours", pb, f, A.outputs(), A.params(true, true)); }
  if (rs_hip_set_writeback(pb, A.z.data(), A.z.data(), A.z.data(), ApiArgs::PAD) != 0) g_errors++;
  step("sky view with write-back", pb, A.forcing(true, true), A.outputs(), A.params(true, true));
  if (rs_hip_set_writeback(pb, nullptr, nullptr, nullptr, 0) != 0) g_errors++;
  { RsPointParams pp = A.params(false, true); pp.tair_relax = pp.vz_relax = pp.rh_relax = A.z.data(); step("relaxation without initlen", pb, A.forcing(true), A.outputs(), pp); }
  { RsOutputs o = A.outputs(); o.water = nullptr; step("output without water", pb, A.forcing(true), o, A.params(false, true)); }
  { RsOutputs o = A.outputs(); o.t_stride = ApiArgs::NP - 1; step("output t_stride below npoints", pb, A.forcing(true), o, A.params(false, true)); }
  { RsOutputs o = A.outputs(); o.decimate = 0; step("decimate 0", pb, A.forcing(true), o, A.params(false, true)); }
  step("nsteps = 0", pb, A.forcing(true), A.outputs(), A.params(false, true), 1, 0);
}

void api_consumer_cases(ApiArgs &A, RsPlan *pa, RsPlan *pc) {
  double *z = A.z.data();
  const int32_t *order = A.zi.data();
  const int NP = ApiArgs::NP;
  auto short_rows = [&] { RsOutputs o = A.outputs(); o.t_stride = NP - 1; return o; };
  auto no_snow = [&] { RsOutputs o = A.outputs(); o.snow = nullptr; return o; };
  {
    const char *fn = "rs_hip_outputs_by_point";
    double *dst[6] = {z, z, z, z, z, z};
    auto call = [&](const char *name, RsPlan *pl, RsOutputs o, int nrows, const int32_t *ord, double *const *d, void *st) {
      api_call(fn, name, [&] { return rs_hip_outputs_by_point(pl, &o, nrows, ord, d, 8, 2, st); });
    };
    call("the plan's order (made here)", pa, A.outputs(), 4, nullptr, dst, nullptr);
    call("the plan's order", pa, A.outputs(), 4, nullptr, dst, nullptr);
    call("a kept order row on a stream of the caller's", pa, A.outputs(), 4, order, dst, A.stream());
    call("nrows = 0", pa, A.outputs(), 0, order, dst, nullptr);
    call("rows beyond dst_rows", pa, A.outputs(), 7, order, dst, nullptr);
    call("fp32 plan", pc, A.outputs(), 4, order, dst, nullptr);
    call("source without snow", pa, no_snow(), 4, order, dst, nullptr);
    { double *d2[6] = {z, z, z, nullptr, z, z}; call("destination without ice", pa, A.outputs(), 4, order, d2, nullptr); }
    call("t_stride below npoints", pa, short_rows(), 4, order, dst, nullptr);
    call("a stream of the caller's without an order row", pa, A.outputs(), 4, nullptr, dst, A.stream());
  }
  {
    api_call("rs_hip_summary_reset", "the plan's stream", [&] { return rs_hip_summary_reset(pa, z, nullptr); });
    api_call("rs_hip_summary_reset", "a stream of the caller's", [&] { return rs_hip_summary_reset(pa, z, A.stream()); });
    api_call("rs_hip_summary_reset", "no accumulator", [&] { return rs_hip_summary_reset(pa, nullptr, nullptr); });
    const char *fn = "rs_hip_outputs_summary";
    RsSummarySpec spec;
    std::memset(&spec, 0, sizeof(spec));
    auto call = [&](const char *name, RsPlan *pl, RsOutputs o, int index0, const int32_t *ord, void *st) {
      api_call(fn, name, [&] { return rs_hip_outputs_summary(pl, &o, 4, index0, 1, ord, &spec, z, st); });
    };
    call("the plan's order", pa, A.outputs(), 1, nullptr, nullptr);
    call("a kept order row on a stream of the caller's", pa, A.outputs(), 1, order, A.stream());
    call("fp32 plan", pc, A.outputs(), 1, order, nullptr);
    call("index0 = 0", pa, A.outputs(), 0, order, nullptr);
    call("source without snow", pa, no_snow(), 1, order, nullptr);
    call("t_stride below npoints", pa, short_rows(), 1, order, nullptr);
    call("a stream of the caller's without an order row", pa, A.outputs(), 1, nullptr, A.stream());
  }
  {
    RsGroupSpec spec, bad;
    std::memset(&spec, 0, sizeof(spec));
    spec.ngroups = 3;
    spec.nedges = 2;
    spec.edges[0] = -1.0;
    spec.edges[1] = 1.0;
    bad = spec;
    bad.edges[1] = -2.0;
    api_call("rs_hip_group_reset", "the plan's stream", [&] { return rs_hip_group_reset(pa, z, 8, &spec, nullptr); });
    api_call("rs_hip_group_reset", "a stream of the caller's", [&] { return rs_hip_group_reset(pa, z, 8, &spec, A.stream()); });
    api_call("rs_hip_group_reset", "acc_rows = 0", [&] { return rs_hip_group_reset(pa, z, 0, &spec, nullptr); });
    api_call("rs_hip_group_reset", "edges not increasing", [&] { return rs_hip_group_reset(pa, z, 8, &bad, nullptr); });
    const char *fn = "rs_hip_outputs_groups";
    auto call = [&](const char *name, RsPlan *pl, RsOutputs o, const int32_t *group, const RsGroupSpec &sp, int64_t acc_row0,
                    const int32_t *ord, void *st) {
      api_call(fn, name, [&] { return rs_hip_outputs_groups(pl, &o, 4, group, ord, &sp, z, 8, acc_row0, st); });
    };
    call("the plan's order", pa, A.outputs(), order, spec, 2, nullptr, nullptr);
    call("a kept order row on a stream of the caller's", pa, A.outputs(), order, spec, 2, order, A.stream());
    call("fp32 plan", pc, A.outputs(), order, spec, 2, order, nullptr);
    call("no group row", pa, A.outputs(), nullptr, spec, 2, order, nullptr);
    call("edges not increasing", pa, A.outputs(), order, bad, 2, order, nullptr);
    call("rows beyond acc_rows", pa, A.outputs(), order, spec, 5, order, nullptr);
    call("source without snow", pa, no_snow(), order, spec, 2, order, nullptr);
    call("t_stride below npoints", pa, short_rows(), order, spec, 2, order, nullptr);
    call("a stream of the caller's without an order row", pa, A.outputs(), order, spec, 2, nullptr, A.stream());
  }
  {
    RsEpisodeSpec spec, bad, with_deficit;
    std::memset(&spec, 0, sizeof(spec));
    spec.use = 1;
    spec.min_rows = 1;
    spec.max_episodes = 3;
    for (int k = 0; k < RS_EPI_VARS; ++k) { spec.above[k] = -HUGE_VAL; spec.below[k] = k == 0 ? 0.0 : HUGE_VAL; }
    bad = spec;
    bad.max_episodes = 0;
    with_deficit = spec;
    with_deficit.use = 1 | (1 << 6);
    for (int fin = 0; fin < 2; ++fin) {
      const char *fn = fin ? "rs_hip_episodes_finish" : "rs_hip_episodes_reset";
      auto call = [&](const char *name, const RsEpisodeSpec *sp, double *acc, void *st) {
        api_call(fn, name, [&] { return fin ? rs_hip_episodes_finish(pa, sp, acc, st) : rs_hip_episodes_reset(pa, sp, acc, st); });
      };
      call("the plan's stream", &spec, z, nullptr);
      call("a stream of the caller's", &spec, z, A.stream());
      call("no accumulator", &spec, nullptr, nullptr);
      call("max_episodes = 0", &bad, z, nullptr);
    }
    const char *fn = "rs_hip_outputs_episodes";
    auto call = [&](const char *name, RsPlan *pl, RsOutputs o, const void *deficit, int index_step, const RsEpisodeSpec &sp,
                    const int32_t *ord, void *st) {
      api_call(fn, name, [&] { return rs_hip_outputs_episodes(pl, &o, deficit, 4, 1, index_step, ord, &sp, z, st); });
    };
    call("the plan's order", pa, A.outputs(), nullptr, 1, spec, nullptr, nullptr);
    call("a kept order row on a stream of the caller's, with the deficit", pa, A.outputs(), z, 1, with_deficit, order, A.stream());
    call("fp32 plan", pc, A.outputs(), nullptr, 1, spec, order, nullptr);
    call("index_step = 0", pa, A.outputs(), nullptr, 0, spec, order, nullptr);
    call("max_episodes = 0", pa, A.outputs(), nullptr, 1, bad, order, nullptr);
    call("a spec that tests the deficit, without one", pa, A.outputs(), nullptr, 1, with_deficit, order, nullptr);
    call("source without snow", pa, no_snow(), nullptr, 1, spec, order, nullptr);
    call("t_stride below npoints", pa, short_rows(), nullptr, 1, spec, order, nullptr);
    call("a stream of the caller's without an order row", pa, A.outputs(), nullptr, 1, spec, nullptr, A.stream());
  }
  {
    const char *fn = "rs_hip_gather_nodes";
    auto call = [&](const char *name, const double *src, int stencil, int64_t src_stride, int64_t dst_stride, const int32_t *ord,
                    void *st) {
      api_call(fn, name, [&] {
        return rs_hip_gather_nodes(pa, src, 4, 100, src_stride, order, z, stencil, ord, -100.0, -9999.9, z, dst_stride, st);
      });
    };
    call("the plan's order", z, 2, 100, ApiArgs::PAD, nullptr, nullptr);
    call("a kept order row on a stream of the caller's", z, 2, 100, ApiArgs::PAD, order, A.stream());
    call("no source", nullptr, 2, 100, ApiArgs::PAD, order, nullptr);
    call("stencil = 0", z, 0, 100, ApiArgs::PAD, order, nullptr);
    call("src_stride below n_nodes", z, 2, 99, ApiArgs::PAD, order, nullptr);
    call("dst_stride below npoints", z, 2, 100, NP - 1, order, nullptr);
    call("a stream of the caller's without an order row", z, 2, 100, ApiArgs::PAD, nullptr, A.stream());
  }
}

void api_argument_phase() {
  ApiArgs A;
  RsPlan *pa = A.plan(false, 64), *pb = A.plan(true, 64), *pc = A.plan(false, 32), *pd = A.plan(true, 32);
  if (!pa || !pb || !pc || !pd) return;
  if (rs_hip_plan_npoints(pa) != ApiArgs::NP || rs_hip_plan_state_bytes(pa) % ((size_t)ApiArgs::PAD * sizeof(double)) != 0) {
    fprintf(stderr, "phase 5: the plan's padding is not %d\n", ApiArgs::PAD);
    g_errors++;
  }
  printf("phase 5: the device API's answers to its arguments: begin\n");
  api_consumer_cases(A, pa, pc); /* first: the first of them makes the plan's order row */
  api_step_cases(A, pa, pb, pc, pd); /* leaves the timing of pa and pb on */
  api_knots_cases(A, pa, pb, pc);
  api_cpl_cases(A, pa, pb, pd, false);
  api_cpl_cases(A, pa, pb, pd, true);
  RsPlan *timed[2] = {pa, pb};
  for (int k = 0; k < 2; ++k) {
    int32_t n = -1;
    const double ms = rs_hip_timing_step_ms(timed[k], &n);
    printf("rs_hip_timing_step_ms | %s | nlaunches %d | %s\n", k ? "the coupled plan" : "the default plan", n, ms >= 0.0 ? "ok" : "failed");
  }
  printf("phase 5: the device API's answers to its arguments: end\n");
  rs_hip_plan_destroy(pa);
  rs_hip_plan_destroy(pb);
  rs_hip_plan_destroy(pc);
  rs_hip_plan_destroy(pd);
}

}  // namespace

int main(int argc, char **argv) {
  const int T = argc > 1 ? std::max(2, atoi(argv[1])) : 64;
  const int N = argc > 2 ? std::max(T, atoi(argv[2])) : 640;
  const Group ga(241), gb(361); /* two hours / three hours: the coalescer keeps the groups apart */
  {
    std::atomic<int> na{0}, nb{0};
    std::vector<std::thread> th;
    for (int k = 0; k < T; ++k) th.emplace_back([&, k] { one_point_calls((k & 1) ? gb : ga, (k & 1) ? nb : na, N / 2); });
    for (auto &x : th) x.join();
  }
  int64_t batches = 0, points = 0;
  rs_coalesce_stats(&batches, &points);
  printf("phase 1: %d threads, %d points: %lld coalesced batches, %lld points in them\n", T, N, (long long)batches, (long long)points);
  for (int round = 0; round < 3; ++round) { /* threads that end: their caches are adopted by the next ones */
    std::atomic<int> na{0};
    std::vector<std::thread> th;
    for (int k = 0; k < 8; ++k) th.emplace_back([&] { one_point_calls(ga, na, 24); });
    for (auto &x : th) x.join();
  }
  printf("phase 2: short-lived caller threads done\n");
  {
    std::vector<std::thread> th;
    const int sizes[4] = {1, 7, 300, 1025};
    for (int k = 0; k < 4; ++k) th.emplace_back([&, k] { batch_call((k & 1) ? gb : ga, sizes[k]); });
    for (auto &x : th) x.join();
  }
  printf("phase 3: concurrent runsimulation_batch_ex calls done\n");
  {
    std::vector<std::thread> th;
    th.emplace_back([] { driver_call(9000, 6, false); });
    th.emplace_back([] { driver_call(700, 5, true); });
    th.emplace_back([] { driver_call(5000, 4, false, true); });
    for (auto &x : th) x.join();
  }
  printf("phase 4: concurrent rs_driver_run calls done\n");
  api_argument_phase();
  if (g_errors.load() != 0) {
    printf("sanitize harness: %d calls failed\n", g_errors.load());
    return 1;
  }
  printf("sanitize harness ok\n");
  return 0;
}
