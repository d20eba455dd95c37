/* rs_step_select.hpp — which step-kernel instance a launch takes, with its grid, workgroup size and dynamic LDS:
 * the one statement of those rules.  Plain host C++, no HIP: the entry points of rs_api.hip
 * describe a launch as a StepShape, select_step() answers, and one switch per precision (rs_launch_step in
 * rs_kernels.hip, rs32_launch_step in rs_kernels_f32.hip) launches the answer.  tests/test_step_selection.py builds
 * this header with the host compiler and pins the table.  Nothing here reads the environment: the callers read
 * ROADSURF_HIP_VARIANT, ..._A32_LIMIT, ..._CPL_REPLAY and pass the results in. */
#pragma once
#include <cstdint>

#define RS_BLOCK 256

enum { RS_VARIANT_AUTO = 0, RS_VARIANT_REG = 1, RS_VARIANT_LDS = 2, RS_VARIANT_DUO = 3, RS_VARIANT_HYBRID = 4 };
/* AUTO takes the two-wavefronts-per-64-points flavour for launches of at most this many points:
 * 1 024 wavefronts, a quarter of the chip's slots (measured, tools/r3_duo.sh: two plans of 62 500
 * points 1.13e10 against 1.06e10 point-timesteps/s with one point per lane; four such plans in
 * flight at once are better off with one point per lane - a caller that runs that many sets the
 * flavour itself, as bench.py does) */
#ifndef RS_DUO_MAX_POINTS
#define RS_DUO_MAX_POINTS 65536
#endif

/* Every step-kernel instance: X(enum value, the kernel as its demangled name reads).  Template arguments as the
 * kernels declare them - step_kernel_duo<NL, SCORE, SRC (0 window, 1 knots, 2 raw series), FULL, SKY, CPL, REPLAY>,
 * step_kernel_reg<NL, FULL, SCORE, A32>, step_kernel_hybrid<SCORE, A32>, step_kernel_lds<FULL, DIAG>,
 * step_kernel_f32duo<SRC (0 window, 1 knots), SCORE, FULL, SKY>.  The order is the order in which the launchers
 * instantiated them until the table existed: the device compiler lays the code object out - and allocates the
 * kernels' LDS and constants - in that order, and each kernel's code follows (tools/compare_device_code.py). */
#define RS_STEP_KERNELS_F64(X)                                                          \
  X(DUO_SKY_SCORE, rs::step_kernel_duo<15, true, 0, true, true, false, false>)          \
  X(DUO_SKY, rs::step_kernel_duo<15, false, 0, true, true, false, false>)               \
  X(SKY_LDS_DIAG, rs::step_kernel_sky<true>)                                            \
  X(SKY_HYBRID, rs::step_kernel_sky_h<4>)                                               \
  X(SKY_LDS, rs::step_kernel_sky<false>)                                                \
  X(DUO_KNOTS_FULL_SCORE, rs::step_kernel_duo<15, true, 1, true, false, false, false>)  \
  X(DUO_KNOTS_FULL, rs::step_kernel_duo<15, false, 1, true, false, false, false>)       \
  X(DUO_KNOTS_LEAN_SCORE, rs::step_kernel_duo<15, true, 1, false, false, false, false>) \
  X(DUO_KNOTS_LEAN, rs::step_kernel_duo<15, false, 1, false, false, false, false>)      \
  X(DUO_RAW_CPL_SKY, rs::step_kernel_duo<15, true, 2, true, true, true, false>)         \
  X(DUO_RAW_CPL, rs::step_kernel_duo<15, true, 2, true, false, true, false>)            \
  X(DUO_RAW_SKY_SCORE, rs::step_kernel_duo<15, true, 2, true, true, false, false>)      \
  X(DUO_RAW_SKY, rs::step_kernel_duo<15, false, 2, true, true, false, false>)           \
  X(DUO_RAW_SCORE, rs::step_kernel_duo<15, true, 2, true, false, false, false>)         \
  X(DUO_RAW, rs::step_kernel_duo<15, false, 2, true, false, false, false>)              \
  X(DUO_RAW_REPLAY, rs::step_kernel_duo<15, true, 2, true, false, true, true>)          \
  X(CPL_HYBRID_SKY, rs::step_kernel_cpl_h<3, true>)                                     \
  X(CPL_HYBRID, rs::step_kernel_cpl_h<3, false>)                                        \
  X(CPL_LDS_SKY, rs::step_kernel_cpl<true>)                                             \
  X(CPL_LDS, rs::step_kernel_cpl<false>)                                                \
  X(CPL_REPLAY_HYBRID_SKY, rs::step_kernel_cpl_replay_h<3, true>)                       \
  X(CPL_REPLAY_HYBRID, rs::step_kernel_cpl_replay_h<3, false>)                          \
  X(CPL_REPLAY_LDS_SKY, rs::step_kernel_cpl_replay<true>)                               \
  X(CPL_REPLAY_LDS, rs::step_kernel_cpl_replay<false>)                                  \
  X(COUPLED_DIAG, rs::step_kernel_coupled<true>)                                        \
  X(COUPLED, rs::step_kernel_coupled<false>)                                            \
  X(DUO_FULL_SCORE, rs::step_kernel_duo<15, true, 0, true, false, false, false>)        \
  X(DUO_FULL, rs::step_kernel_duo<15, false, 0, true, false, false, false>)             \
  X(DUO_LEAN_SCORE, rs::step_kernel_duo<15, true, 0, false, false, false, false>)       \
  X(DUO_LEAN, rs::step_kernel_duo<15, false, 0, false, false, false, false>)            \
  X(HYBRID_A64, rs::step_kernel_hybrid<false, false>)                                   \
  X(HYBRID_A32, rs::step_kernel_hybrid<false, true>)                                    \
  X(HYBRID_SCORE_A64, rs::step_kernel_hybrid<true, false>)                              \
  X(HYBRID_SCORE_A32, rs::step_kernel_hybrid<true, true>)                               \
  X(REG_LEAN_SCORE_A64, rs::step_kernel_reg<15, false, true, false>)                    \
  X(REG_LEAN_SCORE_A32, rs::step_kernel_reg<15, false, true, true>)                     \
  X(REG_LEAN_A64, rs::step_kernel_reg<15, false, false, false>)                         \
  X(REG_LEAN_A32, rs::step_kernel_reg<15, false, false, true>)                          \
  X(REG_FULL_SCORE_A64, rs::step_kernel_reg<15, true, true, false>)                     \
  X(REG_FULL_SCORE_A32, rs::step_kernel_reg<15, true, true, true>)                      \
  X(REG_FULL_A64, rs::step_kernel_reg<15, true, false, false>)                          \
  X(REG_FULL_A32, rs::step_kernel_reg<15, true, false, true>)                           \
  X(LDS_DIAG, rs::step_kernel_lds<true, true>)                                          \
  X(LDS_FULL, rs::step_kernel_lds<true, false>)                                         \
  X(LDS_LEAN, rs::step_kernel_lds<false, false>)

#define RS_STEP_KERNELS_F32(X)                                                 \
  X(F32_DUO_SKY_SCORE, rs32::step_kernel_f32duo<0, true, true, true>)          \
  X(F32_DUO_SKY, rs32::step_kernel_f32duo<0, false, true, true>)               \
  X(F32_DUO_FULL_SCORE, rs32::step_kernel_f32duo<0, true, true, false>)        \
  X(F32_DUO_FULL, rs32::step_kernel_f32duo<0, false, true, false>)             \
  X(F32_DUO_LEAN_SCORE, rs32::step_kernel_f32duo<0, true, false, false>)       \
  X(F32_DUO_LEAN, rs32::step_kernel_f32duo<0, false, false, false>)            \
  X(F32_LDS, rs32::step_kernel_f32_lds)                                        \
  X(F32_DUO_KNOTS_FULL_SCORE, rs32::step_kernel_f32duo<1, true, true, false>)  \
  X(F32_DUO_KNOTS_FULL, rs32::step_kernel_f32duo<1, false, true, false>)       \
  X(F32_DUO_KNOTS_LEAN_SCORE, rs32::step_kernel_f32duo<1, true, false, false>) \
  X(F32_DUO_KNOTS_LEAN, rs32::step_kernel_f32duo<1, false, false, false>)      \
  X(F32_COUPLED, rs32::step_kernel_f32_coupled)

namespace rs {

#define RS_STEP_ENUM(id, ...) id,
enum class StepKernel : int32_t {
  NONE, /* no instance for this shape: the caller reports hipErrorInvalidValue */
  RS_STEP_KERNELS_F64(RS_STEP_ENUM) RS_STEP_KERNELS_F32(RS_STEP_ENUM)
};
#undef RS_STEP_ENUM

enum class StepSource : int32_t {
  WINDOW, /* a forcing window (RsForcing) */
  KNOTS,  /* the hourly knots, interpolated by the ground wave (rs_hip_step_knots) */
  RAW     /* the raw series of rs_driver_run (rs_step_raw, rs_cpl_replay_raw) */
};

enum class StepCoupling : int32_t {
  NONE,    /* no coupling in this launch */
  GENERAL, /* rs_hip_step's whole-series rounds - park, general replay rounds, finish - and rs_hip_cpl_replay's
              general rounds: the kernel with a time index per lane */
  CHUNK,   /* a lock-step chunk (rs_hip_step_cpl; rs_step_raw of a coupled plan) */
  REPLAY   /* a lock-step replay round over the list (rs_hip_cpl_replay; rs_cpl_replay_raw) */
};

struct StepShape {
  bool f32 = false;
  int32_t nlayers = 15;
  StepSource src = StepSource::WINDOW;
  bool full = false;  /* the FULL feature set (rs_hip_step / rs_hip_step_knots: what makes the LEAN kernel inexact) */
  bool sky = false;   /* per-point sky view */
  bool depth = false; /* an output depth: a depth stream or tsurfOutputDepth >= 0 */
  StepCoupling cpl = StepCoupling::NONE;
  bool a32 = false;   /* every stream of the windows within 32-bit offsets (rs_api.hip window_a32) */
  bool diag = false;  /* the plan's diagnostics block */
  bool score = true;  /* leave the history score (rs_hip_set_history_score) */
  int32_t variant = RS_VARIANT_AUTO;
  int64_t npoints = 0;
  int32_t wave_n = 0; /* > 0: a valid wave table of that many workgroups (StepArgs::wave_start) */
  bool cpl_list = false; /* the launch steps the listed points (StepArgs::cpl_list) ... */
  int32_t cpl_nlist = 0; /* ... this many of them */
};

struct StepLaunch {
  StepKernel kernel = StepKernel::NONE;
  uint32_t grid = 0; /* workgroups; 0: nothing to launch (an empty list) */
  uint32_t block = RS_BLOCK;
  uint32_t lds = 0; /* dynamic LDS bytes */
};

inline uint32_t blocks_of(int64_t n, int64_t per) { return (uint32_t)((n + per - 1) / per); }

inline StepLaunch select_fp32(const StepShape &s) {
  const bool nl15 = s.nlayers == 15;
  const uint32_t g = blocks_of(s.npoints, RS_BLOCK), g2 = blocks_of(s.npoints, 128); /* two points per lane */
  auto duo = [&](StepKernel k) { return StepLaunch{k, g2, 128, 0}; };
  if (s.src == StepSource::RAW || s.cpl == StepCoupling::CHUNK || s.cpl == StepCoupling::REPLAY) return {};
  if (s.src == StepSource::KNOTS) {
    if (!nl15) return {};
    return duo(s.full ? (s.score ? StepKernel::F32_DUO_KNOTS_FULL_SCORE : StepKernel::F32_DUO_KNOTS_FULL)
                      : (s.score ? StepKernel::F32_DUO_KNOTS_LEAN_SCORE : StepKernel::F32_DUO_KNOTS_LEAN));
  }
  /* the general kernel: a coupled plan's whole series (every point replays its coupling window inside the one
   * launch), an output depth, or the FULL feature set / sky view at a layer count the two-points-per-lane kernels are
   * not built for (they would have no instance) */
  if (s.cpl == StepCoupling::GENERAL || s.depth || ((s.full || s.sky) && !nl15))
    return {StepKernel::F32_COUPLED, g, RS_BLOCK, (uint32_t)(s.nlayers * RS_BLOCK * sizeof(float))};
  if (s.sky) return duo(s.score ? StepKernel::F32_DUO_SKY_SCORE : StepKernel::F32_DUO_SKY);
  /* two points per lane, two wavefronts per 128 points (round 6); RS_VARIANT_REG / _LDS: round 2-5's one point per
   * lane with the profile in LDS, for A/B (and what other layer counts take) */
  if (nl15 && (s.full || (s.variant != RS_VARIANT_REG && s.variant != RS_VARIANT_LDS)))
    return duo(s.full ? (s.score ? StepKernel::F32_DUO_FULL_SCORE : StepKernel::F32_DUO_FULL)
                      : (s.score ? StepKernel::F32_DUO_LEAN_SCORE : StepKernel::F32_DUO_LEAN));
  return {StepKernel::F32_LDS, g, RS_BLOCK, (uint32_t)(s.nlayers * RS_BLOCK * sizeof(float))};
}

inline StepLaunch select_fp64(const StepShape &s) {
  const bool nl15 = s.nlayers == 15;
  const uint32_t lds = (uint32_t)(s.nlayers * RS_BLOCK * sizeof(double)); /* the LDS profile: NLayers x RS_BLOCK */
  const uint32_t g = blocks_of(s.npoints, RS_BLOCK);
  /* two wavefronts per 64 points: one workgroup per row of the wave table, else per 64 points */
  const uint32_t gd = s.wave_n > 0 ? (uint32_t)s.wave_n : blocks_of(s.npoints, 64);
  auto duo = [&](StepKernel k, uint32_t block = 128) { return StepLaunch{k, gd, block, 0}; };
  auto pick = [](bool c, StepKernel yes, StepKernel no) { return c ? yes : no; };
  const bool no_list = !s.cpl_list || s.cpl_nlist < 1; /* a replay round with nothing to replay: no launch */

  if (s.src == StepSource::KNOTS) {
    if (!nl15 || s.sky || s.cpl != StepCoupling::NONE) return {};
    return duo(s.full ? pick(s.score, StepKernel::DUO_KNOTS_FULL_SCORE, StepKernel::DUO_KNOTS_FULL)
                      : pick(s.score, StepKernel::DUO_KNOTS_LEAN_SCORE, StepKernel::DUO_KNOTS_LEAN));
  }
  if (s.src == StepSource::RAW) { /* the FULL feature set as the driver has it; NLayers = 15, no output depth */
    if (!nl15 || s.depth) return {};
    /* a coupled plan's lock-step chunk keeps the history score; its replay rounds (one replay per round, no sky
     * view) run two wavefronts per 64 listed points */
    if (s.cpl == StepCoupling::REPLAY) {
      if (s.sky) return {};
      return {StepKernel::DUO_RAW_REPLAY, no_list ? 0 : blocks_of(s.cpl_nlist, 64), 128, 0};
    }
    if (s.cpl == StepCoupling::CHUNK) return s.sky ? duo(StepKernel::DUO_RAW_CPL_SKY, 192) : duo(StepKernel::DUO_RAW_CPL);
    if (s.cpl != StepCoupling::NONE) return {};
    return s.sky ? duo(pick(s.score, StepKernel::DUO_RAW_SKY_SCORE, StepKernel::DUO_RAW_SKY), 192)
                 : duo(pick(s.score, StepKernel::DUO_RAW_SCORE, StepKernel::DUO_RAW));
  }

  switch (s.cpl) {
    case StepCoupling::GENERAL: { /* the listed points, else every point; (diagnostics: the instance that carries
                                   * bl_diagnose - here and below) */
      const int64_t n = s.cpl_list ? (int64_t)s.cpl_nlist : s.npoints;
      return {pick(s.diag, StepKernel::COUPLED_DIAG, StepKernel::COUPLED), n < 1 ? 0 : blocks_of(n, RS_BLOCK),
              RS_BLOCK, lds};
    }
    /* Lock-step chunks and replay rounds (no diagnostics instance).  NLayers = 15: the hybrid profile at three waves
     * per SIMD (measured, tools/r3_cpl.sh, rs_driver_run with coupling, 1 M points: 7.75e9; LDS profile at 3 waves
     * 7.0e9, hybrid at 4 waves - spills - 6.6e9; a profile wholly in registers was twice as slow); other layer
     * counts: the LDS profile. */
    case StepCoupling::CHUNK:
      if (nl15) return {pick(s.sky, StepKernel::CPL_HYBRID_SKY, StepKernel::CPL_HYBRID), g, RS_BLOCK, 0};
      return {pick(s.sky, StepKernel::CPL_LDS_SKY, StepKernel::CPL_LDS), g, RS_BLOCK, lds};
    case StepCoupling::REPLAY: {
      const uint32_t gl = no_list ? 0 : blocks_of(s.cpl_nlist, RS_BLOCK);
      if (nl15) return {pick(s.sky, StepKernel::CPL_REPLAY_HYBRID_SKY, StepKernel::CPL_REPLAY_HYBRID), gl, RS_BLOCK, 0};
      return {pick(s.sky, StepKernel::CPL_REPLAY_LDS_SKY, StepKernel::CPL_REPLAY_LDS), gl, RS_BLOCK, lds};
    }
    case StepCoupling::NONE: break;
  }

  if (s.sky) {
    /* Two wavefronts per 64 points where the launch has no output depth and 32-bit window offsets - no spills (128
     * registers) where the one-point-per-lane sky kernels spill 62-106 - for launches of at most RS_DUO_MAX_POINTS
     * points, like the other two-wavefront instances: rs_driver_run with sky view, 65 536 points 3.5e9 -> 4.8e9,
     * 200 000 points (four blocks) 7.6e9 -> 8.6e9; at 1 M points (blocks of 250 000) 1.06e10 -> 1.03e10 - four of
     * its wavefronts leave a SIMD no register for the other blocks' window expansion, which then queues. */
    if (nl15 && s.npoints <= RS_DUO_MAX_POINTS && !s.depth && s.a32 && !s.diag)
      return duo(pick(s.score, StepKernel::DUO_SKY_SCORE, StepKernel::DUO_SKY));
    /* NLayers = 15: the hybrid profile at four waves per SIMD (measured, rs_driver_run with sky view, 262 144 points
     * in four blocks: LDS profile at three waves 6.9e9, hybrid at three 7.1e9, at four 7.4e9); other layer counts:
     * the LDS profile. */
    if (s.diag) return {StepKernel::SKY_LDS_DIAG, g, RS_BLOCK, lds};
    if (nl15) return {StepKernel::SKY_HYBRID, g, RS_BLOCK, 0};
    return {StepKernel::SKY_LDS, g, RS_BLOCK, lds};
  }

  /* Measured (tools/r3_full2.sh, 1 M points): FULL feature set - layers 8-15 in LDS at 4 waves/SIMD 1.36e10, all in
   * registers at 3 waves/SIMD (167 VGPRs) 1.34e10, at 4 waves (14 doubles spilled) 1.23e10, all in LDS 1.28e10.
   * LEAN: registers, 4 waves.  (tools/bench_driver_path.py relax, 1 M points, one plan: the FULL feature set in the
   * register flavour at 3 waves/SIMD 0.745 s, at 2 waves 0.80 s, at 4 waves - 130 spilled VGPRs - 0.87 s; with the
   * profile in LDS 0.86 s (3 waves) / 0.88 s (4 waves).)  The waves-per-SIMD bound was a digit of the variant until
   * round 6; the measured choices are the kernels' launch bounds now. */
  const int as_auto = !nl15 ? RS_VARIANT_LDS : s.full ? RS_VARIANT_HYBRID : RS_VARIANT_REG;
  int v = s.diag ? RS_VARIANT_LDS : s.variant == RS_VARIANT_AUTO ? as_auto : s.variant;
  /* small shards: two wavefronts per 64 points (step_kernel_duo).  Measured on MI355X (tools/r3_eval.sh): faster
   * than one point per lane below RS_DUO_MAX_POINTS points per launch.  Not for a FULL launch with an output depth. */
  const bool duo_ok = (!s.full || !s.depth) && nl15 && s.a32;
  if (v == RS_VARIANT_DUO && !duo_ok) v = as_auto; /* not this launch: as AUTO */
  else if (v == RS_VARIANT_DUO || (s.variant == RS_VARIANT_AUTO && !s.diag && duo_ok && s.npoints <= RS_DUO_MAX_POINTS))
    return duo(s.full ? pick(s.score, StepKernel::DUO_FULL_SCORE, StepKernel::DUO_FULL)
                      : pick(s.score, StepKernel::DUO_LEAN_SCORE, StepKernel::DUO_LEAN));
  if (v == RS_VARIANT_HYBRID && (!nl15 || !s.full)) v = nl15 ? RS_VARIANT_REG : RS_VARIANT_LDS; /* not this launch: as AUTO */
  if (v == RS_VARIANT_HYBRID)
    return {s.score ? pick(s.a32, StepKernel::HYBRID_SCORE_A32, StepKernel::HYBRID_SCORE_A64)
                    : pick(s.a32, StepKernel::HYBRID_A32, StepKernel::HYBRID_A64), g, RS_BLOCK, 0};
  if (v == RS_VARIANT_REG) {
    if (!nl15) return {}; /* the register profile is built for NLayers = 15 only */
    static const StepKernel reg[2][2][2] = { /* [full][score][a32] */
        {{StepKernel::REG_LEAN_A64, StepKernel::REG_LEAN_A32}, {StepKernel::REG_LEAN_SCORE_A64, StepKernel::REG_LEAN_SCORE_A32}},
        {{StepKernel::REG_FULL_A64, StepKernel::REG_FULL_A32}, {StepKernel::REG_FULL_SCORE_A64, StepKernel::REG_FULL_SCORE_A32}}};
    return {reg[s.full][s.score][s.a32], g, RS_BLOCK, 0};
  }
  /* (diagnostics: the FULL instance whatever the launch's feature set - it reads a missing optional stream as "no
   * value" and is exact for a LEAN launch too) */
  return {s.diag ? StepKernel::LDS_DIAG : pick(s.full, StepKernel::LDS_FULL, StepKernel::LDS_LEAN), g, RS_BLOCK, lds};
}

/* the instance, grid, workgroup size and dynamic LDS of a step launch */
inline StepLaunch select_step(const StepShape &s) { return s.f32 ? select_fp32(s) : select_fp64(s); }

}  // namespace rs
