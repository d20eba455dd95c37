/* rs_kernels.h — kernel argument blocks and host launchers (internal). */
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>
#include "../../include/roadsurf.h"
#include "rs_synth.h"
#include "rs_raw.hpp"
#include "rs_step_select.hpp"

namespace rs {

/* where the sky-view kernels leave the reference's in-place edits of the input arrays
 * (rs_hip_set_writeback): rows like the forcing window's, all NULL = not wanted */
struct Writeback {
  double *sw, *sw_dir, *lw;
  int64_t t_stride;
};

/* Every field defaults to null / zero: an entry point sets what its launch uses (rs_api.hip).  The kernels read the
 * block as their kernel argument: its layout is pinned below. */
struct StepArgs {
  const void *consts = nullptr; /* the plan's constants in HBM: RsConstants (fp64 kernels) or RsConstantsF
                                   (fp32 kernels); read through the scalar cache (address space 4) */
  RsForcing f{};
  RsOutputs o{};
  RsPointParams pp{};
  double *state = nullptr;
  int64_t npoints = 0, np_pad = 0;
  int32_t t0 = 0, nsteps = 0;
  Writeback wb{};
  /* coupling rounds (step_kernel_coupled): thread g works on point cpl_list[g] (NULL: point g);
   * cpl_stop: a point parks right after the Coupling_control of its window end */
  const int32_t *cpl_list = nullptr;
  int32_t cpl_nlist = 0, cpl_stop = 0;
  /* lock-step replay kernels: a listed point may run up to this many replays of its window in ONE
   * launch, until its Coupling_control stops asking (0 or 1: one replay, the round structure of
   * rs_hip_cpl_replay); cpl_prio: raise the wavefronts' issue priority (a sparse late round beside
   * another plan's full launches runs at the speed of its own dependency chain) */
  int32_t cpl_inner = 0, cpl_prio = 0;
  /* coupling kernels: the outputs of slot s go to column out_index[s] of the output window
   * (NULL: column s).  With the plan order as index the (decimated) outputs land in point order
   * whatever order the slots are in (rs_hip_set_output_by_point). */
  const int32_t *out_index = nullptr;
  /* two-wavefront flavour: wavefront w steps the slots [wave_start[w], wave_start[w] + wave_cnt[w]) and the
   * launch has wave_n workgroups (rs_cluster_wave_table: no wavefront mixes two classes of the sort key);
   * NULL: wavefront w steps the slots 64 w ... */
  const int32_t *wave_start = nullptr, *wave_cnt = nullptr;
  int32_t wave_n = 0;
  /* knot-reading kernels: bit 1 (& 2) set - the knots carry a dew point, run CheckValues' dew-point test */
  int32_t knots_tdew = 0;
  /* two-wavefront flavour: the surface wave runs at raised issue priority (rs_api.hip: set while all live
   * plans of the device together leave its SIMDs underfilled) */
  int32_t surface_prio = 0;
  /* two-wavefront flavour on the synthetic workload (rs_hip_step_knots): no forcing window - the ground
   * wave makes the forcing of the next index from the hourly knots itself, with expand_kernel's arithmetic
   * (knots [knot - knot_k0][RS_KNOT_FIELDS][np_pad] in point order, column knot_gather[slot]; NULL knots:
   * the window `f`) */
  const double *knots = nullptr;
  const int32_t *knot_gather = nullptr;
  int32_t knot_k0 = 0, knot_n = 0, spk = 0, start_hour = 0;
  double r_spk = 0.0;
  /* two-wavefront flavour behind rs_driver_run (rs_step_raw): no forcing window either - the ground wave
   * makes the forcing of the next index from the RAW series (JsonSource::interpolate + the GetWeather
   * overlay, rs_raw.hpp); raw.nsrc = 0: not this launch */
  RawForcing raw{};
  /* the plan's diagnostics block (rs_hip_set_diagnostics; rs_state.h RsDiagRow), or NULL */
  double *diag = nullptr;
};
static_assert(std::is_trivially_copyable<StepArgs>::value, "StepArgs is a kernel argument");
static_assert(sizeof(StepArgs) == 912 && offsetof(StepArgs, f) == 8 && offsetof(StepArgs, o) == 136 &&
                  offsetof(StepArgs, pp) == 208 && offsetof(StepArgs, state) == 328 && offsetof(StepArgs, t0) == 352 &&
                  offsetof(StepArgs, wb) == 360 && offsetof(StepArgs, cpl_list) == 392 &&
                  offsetof(StepArgs, out_index) == 416 && offsetof(StepArgs, wave_n) == 440 &&
                  offsetof(StepArgs, knots_tdew) == 444 && offsetof(StepArgs, surface_prio) == 448 &&
                  offsetof(StepArgs, knots) == 456 && offsetof(StepArgs, r_spk) == 488 &&
                  offsetof(StepArgs, raw) == 496 && offsetof(StepArgs, diag) == 904,
              "the kernels' view of StepArgs");

struct InitArgs {
  const void *consts;
  RsForcing f;
  RsPointParams pp;
  double *state;
  int64_t npoints, np_pad;
};

struct ForecastArgs {
  const void *consts; /* RsConstants (the predictor runs in fp64 for either flavour) */
  const void *state;
  int32_t f32;        /* the state block holds floats */
  int64_t npoints, np_pad;
  RsPreview pv;
  uint32_t *keys, *slots;
  int32_t compact; /* 1: the key is stored right-aligned in its own bits (counting sort), 0: left-aligned
                      in RS_SORT_KEY_BITS (library sort) */
  int32_t low_bits; /* compact keys: bits of the ground digit below the others (rs_forecast_key_low_bits) */
  int32_t extra_log; /* field 0 of the mode: 0 = the previews' extra passes summed, saturating at 7; 1 = the
                        LONGEST loop expected in the window (previews, the last index stepped, a passage through
                        the loop's slow band) in classes 5, 6, 7, 8, 9-12, 13-20, 21-30, 31+ */
  /* filled by rs_launch_forecast_keys from pv.mode, so that no thread divides by ten: the mode's decimal digits
   * (its shorthands 0..3 spelled out), four bits each, the most significant in the highest nibble used; how many;
   * whether one of them is the ground digit 9 */
  uint64_t mode_digits;
  int32_t mode_ndigits, mode_ground;
};

struct KnotArgs {
  RsSynthSpec spec;
  double *knots;
  int64_t npoints, np_pad;
  int32_t k0, nknots;
};

struct ExpandArgs {
  RsForcing f;
  const double *knots;
  int64_t npoints, np_pad;
  int32_t k0, t0, spk, start_hour;
  int32_t kfirst, nsteps;
  double r_spk; /* RN(1 / spk): the interpolation's division has a uniform denominator (rs_div_u) */
  const int32_t *gather; /* NULL, or: the knots of window column p are knot column gather[p] */
};

}  // namespace rs

hipError_t rs_read_div_mismatch(unsigned long long *out /*[3]*/, hipStream_t stream);
hipError_t rs_read_div_samples(double *out /*[64][4]*/, hipStream_t stream);
hipError_t rs_read_bl_stats(unsigned long long *out /*[57]*/, hipStream_t stream);
hipError_t rs_launch_math_test(int fn, int64_t n, const double *x, double *y, hipStream_t stream);
/* raw-series Tdew<->RH completion (needs the math tables: create a plan first) */
hipError_t rs_launch_humidity_fill(const double *tair, double *tdew, double *rhz, int64_t n,
                                   hipStream_t stream);
/* exp/log tables of the device (same for every plan) */
hipError_t rs_upload_math_tables(hipStream_t stream);
/* the step kernel rs::select_step chose (rs_step_select.hpp), with its grid, workgroup and dynamic LDS: the fp64
 * instances here, the fp32 ones in rs_kernels_f32.hip; hipErrorInvalidValue for an instance of the other precision */
hipError_t rs_launch_step(const rs::StepArgs &a, const rs::StepLaunch &l, hipStream_t stream);
struct RsPlan;
/* the replay rounds of a coupled plan whose lock-step chunks run through rs_step_raw: as rs_hip_cpl_replay, the
 * forcing of the block [t0, t0 + nsteps) from the raw series (no sky view; the block must end before SimLen) */
int rs_cpl_replay_raw(RsPlan *pl, const rs::RawForcing *raw, const RsOutputs *o, const RsPointParams *pp,
                      int32_t t0, int32_t nsteps, bool out_by_point, int32_t *rounds);
/* Elements per stream of a window that the kernels with 32-bit byte offsets can address (2^29 doubles = 4 GiB).
 * The launchers that need it refuse larger windows; rs_driver_run cuts its point tiles so that a tile's output
 * window stays below it.  ROADSURF_HIP_A32_LIMIT (elements) can only LOWER it: the tests reach the limit with
 * windows of megabytes instead of gigabytes. */
uint64_t rs_a32_limit(void);
bool rs_step_raw_ok(const RsPlan *pl); /* a plan whose settings rs_step_raw can run */
/* the step of rs_driver_run's blocks (rs_api.hip): NLayers = 15, fp64, no output depth; pp in SLOT order, raw
 * series in point order behind raw.col.  A coupled plan (use_coupling, pp->coupling_index): a LOCK-STEP chunk as
 * rs_hip_step_cpl runs it - points park behind their coupling window until rs_hip_cpl_replay has run. */
int rs_step_raw(RsPlan *pl, const rs::RawForcing *raw, const double *sun, const RsOutputs *o,
                const RsPointParams *pp, int32_t t0, int32_t nsteps, bool out_by_point);
/* out[2] (device): min couplingStartI / max couplingEndI over the points that ask for a replay */
hipError_t rs_launch_cpl_window_bounds(const rs::StepArgs &a, int32_t *out, hipStream_t stream);
/* list of the points whose coupling asks for another replay (start_coupling_again): list[0..*count) */
size_t rs_cpl_select_scratch_bytes(int64_t npoints);
hipError_t rs_cpl_select_again(const double *state, int64_t np_pad, int64_t npoints, int32_t *flags,
                               int32_t *list, int32_t *count_dev, void *tmp, size_t tmp_bytes,
                               hipStream_t stream);
hipError_t rs_launch_init(const rs::InitArgs &a, hipStream_t stream);
hipError_t rs_launch_knots(const rs::KnotArgs &a, int32_t nknots, hipStream_t stream);
hipError_t rs_launch_expand(const rs::ExpandArgs &a, int32_t nintervals, hipStream_t stream);
/* out[0] = shader-clock ticks, out[1] = 100 MHz ticks over the same ~spin_us microseconds (spin_us is
 * clamped to RS_CLOCK_PROBE_MAX_US; out[1] = 0 if the 100 MHz counter did not advance) */
#define RS_CLOCK_PROBE_MAX_US 10000u
hipError_t rs_launch_clock_probe(uint64_t *out, uint32_t spin_us, hipStream_t stream);
hipError_t rs_launch_count_failed(const double *st, int64_t np_pad, int64_t npoints,
                                  unsigned long long *out, hipStream_t stream);

hipError_t rs_launch_forecast_keys(const rs::ForecastArgs &a, hipStream_t stream);

/* plan order (rs_cluster.hip) */
#define RS_SORT_KEY_BITS 24
hipError_t rs_cluster_identity(int32_t *order, int64_t np_pad, hipStream_t stream);
hipError_t rs_cluster_outputs_by_point(const double *const src[6], double *const dst[6], const int32_t *order,
                                       int64_t npoints, int64_t src_stride, int32_t nrows, int64_t dst_rows,
                                       int64_t dst_row0, hipStream_t stream);
/* per-point summaries of output rows (rs_hip_outputs_summary): acc[RS_SUM_COLS][np_pad] in point order;
 * src: six T[nrows][src_stride] windows, T = float with f32; order NULL = column s is point s */
hipError_t rs_cluster_summary_reset(double *acc, int64_t np_pad, hipStream_t stream);
hipError_t rs_cluster_outputs_summary(const void *const src[6], bool f32, const int32_t *order, int64_t npoints,
                                      int64_t src_stride, int32_t nrows, int32_t index0, int32_t index_step,
                                      const RsSummarySpec &spec, double *acc, int64_t np_pad, hipStream_t stream);
/* per-point aggregates over output periods (rs_hip_outputs_periods): acc[nperiods][RS_PER_COLS][np_pad] in point
 * order; src and order as above; the spec was checked by the caller (rs_period_rule.hpp, rs_per::check) */
hipError_t rs_cluster_periods_reset(double *acc, int64_t np_pad, const RsPeriodSpec &spec, hipStream_t stream);
hipError_t rs_cluster_outputs_periods(const void *const src[6], bool f32, const int32_t *order, int64_t npoints,
                                      int64_t src_stride, int32_t nrows, int32_t index0, int32_t index_step,
                                      const RsPeriodSpec &spec, double *acc, int64_t np_pad, hipStream_t stream);
/* per-group series of output rows (rs_hip_outputs_groups): acc_row0[nrows][ngroups][cols] is the caller's accumulator
 * from its row acc_row0 on; group[npoints] in point order; src and order as above.  rs_cluster_group_cols checks the
 * spec (<0: bad), rs_cluster_group_path chooses the kernel (1: cells in LDS, 2: global cells directly) */
int32_t rs_cluster_group_cols(const RsGroupSpec *spec);
int32_t rs_cluster_group_path(const RsGroupSpec *spec);
hipError_t rs_cluster_group_reset(double *acc, int64_t acc_rows, const RsGroupSpec &spec, hipStream_t stream);
hipError_t rs_cluster_outputs_groups(const void *const src[6], bool f32, const int32_t *order, const int32_t *group,
                                     int64_t npoints, int64_t src_stride, int32_t nrows, const RsGroupSpec &spec,
                                     double *acc_row0, hipStream_t stream);
/* per-station ensemble statistics of output rows (rs_hip_outputs_ens): acc_row0[nrows][ngroups][cols] is WRITTEN;
 * table[ngroups + 1 + npoints] as rs_ens_member_table makes it (rs_ens_table.hpp), inv[npoints] the inverse of the
 * order row the window was stepped in (rs_cluster_inverse), src as above.  rs_cluster_ens_waves: the wavefronts per
 * workgroup the host chooses from max_members alone (<0: bad spec), rs_cluster_ens_lds_bytes: the workgroup's LDS */
int32_t rs_cluster_ens_waves(const RsEnsSpec *spec);
size_t rs_cluster_ens_lds_bytes(const RsEnsSpec *spec);
hipError_t rs_cluster_outputs_ens(const void *const src[6], bool f32, const int32_t *table, const int32_t *inv,
                                  int64_t npoints, int64_t src_stride, int32_t nrows, const RsEnsSpec &spec,
                                  double *acc_row0, hipStream_t stream);
/* per-point threshold episodes of output rows (rs_hip_outputs_episodes): acc[cols][np_pad] in point order; src and
 * order as above, deficit: a seventh window of the same layout and type, or NULL.  rs_cluster_episode_cols checks the
 * spec (<0: bad) */
int32_t rs_cluster_episode_cols(const RsEpisodeSpec *spec);
hipError_t rs_cluster_episodes_reset(double *acc, int64_t np_pad, const RsEpisodeSpec &spec, hipStream_t stream);
hipError_t rs_cluster_outputs_episodes(const void *const src[6], const void *deficit, bool f32, const int32_t *order,
                                       int64_t npoints, int64_t src_stride, int32_t nrows, int32_t index0,
                                       int32_t index_step, const RsEpisodeSpec &spec, double *acc, int64_t np_pad,
                                       hipStream_t stream);
hipError_t rs_cluster_episodes_finish(double *acc, int64_t npoints, int64_t np_pad, const RsEpisodeSpec &spec,
                                      hipStream_t stream);
/* per-station probabilities of conditions over the members (rs_hip_outputs_prob): acc_row0[nrows][ngroups][cols] is
 * WRITTEN; src, deficit and order as for the episodes, table and inv as for the ensemble statistics; ever[np_pad] the
 * carry in point order; words[nrows][wstride >= npoints]: one word per row and slot, filled by the first kernel and read
 * by the second.  rs_cluster_prob_cols checks the spec (<0: bad), rs_cluster_prob_needs_deficit: 1 iff bit 6 is used */
int32_t rs_cluster_prob_cols(const RsProbSpec *spec);
int32_t rs_cluster_prob_needs_deficit(const RsProbSpec *spec);
hipError_t rs_cluster_outputs_prob(const void *const src[6], const void *deficit, bool f32, const int32_t *order,
                                   const int32_t *table, const int32_t *inv, int64_t npoints, int64_t src_stride,
                                   int32_t nrows, const RsProbSpec &spec, int32_t *ever, uint32_t *words,
                                   int64_t wstride, double *acc_row0, hipStream_t stream);
/* gridded fields gathered to points (rs_grid.hip, rs_hip_gather_nodes): dst[r][slot] for r < nrows, slot < npoints;
 * node / weight [point][stencil]; order NULL = column s is point s */
hipError_t rs_grid_gather(const double *src, int32_t nrows, int64_t n_nodes, int64_t src_stride, const int32_t *node,
                          const double *weight, int32_t stencil, const int32_t *order, double present_above,
                          double missing, double *dst, int64_t dst_stride, int64_t npoints, hipStream_t stream);
size_t rs_cluster_scratch_bytes(int64_t npoints);
hipError_t rs_cluster_sort(const double *state, bool f32, int64_t np_pad, int64_t npoints,
                           uint32_t *scratch, void *tmp, size_t tmp_bytes, hipStream_t stream);
/* same with keys/slots already in scratch[0..np_pad) / scratch[2*np_pad..) */
hipError_t rs_cluster_sort_keys(int64_t np_pad, int64_t npoints, uint32_t *scratch, void *tmp,
                                size_t tmp_bytes, hipStream_t stream);
/* the plan's own stable counting sort for keys of at most 12 bits (rs_cluster.hip) */
size_t rs_cluster_count_scratch_bytes(int64_t npoints, int nbits);
hipError_t rs_cluster_wave_table(int class_bits, uint32_t *class_total, int32_t *wstart, int32_t *wcnt,
                                 int32_t maxw, hipStream_t stream);
hipError_t rs_cluster_count_sort(int64_t np_pad, int64_t npoints, int nbits, uint32_t *scratch, void *tmp,
                                 size_t tmp_bytes, hipStream_t stream, uint32_t *class_total = nullptr,
                                 int class_bits = 0, int low_bits = 0);
/* significant bits of the forecast key for a field list (RsPreview::mode), without the ground digit ... */
int rs_forecast_key_bits(int32_t mode);
/* ... and the bits of the ground digit below them (field 9: 7, else 0) */
int rs_forecast_key_low_bits(int32_t mode);
hipError_t rs_cluster_apply(const double *state_src, double *state_dst, bool f32,
                            const int32_t *order_src, int32_t *order_dst, const uint32_t *perm,
                            int64_t np_pad, int64_t npoints, int nlayers, int cpl_rows,
                            hipStream_t stream);
/* the carried state of src's points into dst's slots (rs_hip_state_fanout): dst slot s takes the rows of src's point
 * parent[order_dst[s]], which sits in slot inv_src[...] (rs_cluster_inverse of src's order row; NULL: its own number);
 * order_dst NULL: slot s holds point s; nlayers, cpl_rows as for rs_cluster_apply */
hipError_t rs_cluster_inverse(const int32_t *order, int64_t npoints, int32_t *inv, hipStream_t stream);
hipError_t rs_cluster_fanout(const double *state_src, double *state_dst, bool f32, const int32_t *order_dst,
                             const int32_t *parent, const int32_t *inv_src, int64_t np_pad_src, int64_t npoints_src,
                             int64_t np_pad_dst, int64_t npoints_dst, int nlayers, int cpl_rows, hipStream_t stream);

/* fp32 flavour (rs_kernels_f32.hip) */
/* single-precision mirror of the constants: fills *dst (device, rs32_constants_bytes() bytes) */
size_t rs32_constants_bytes(void);
hipError_t rs32_upload_constants(void *dst, const RsConstants *c, hipStream_t stream);
hipError_t rs32_launch_step(const rs::StepArgs &a, const rs::StepLaunch &l, hipStream_t stream);
hipError_t rs32_launch_init(const rs::InitArgs &a, hipStream_t stream);
hipError_t rs32_launch_expand(const rs::ExpandArgs &a, int32_t nintervals, hipStream_t stream);
