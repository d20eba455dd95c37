/* rs_general_body.inc - what the kernels say about the state block, coupling (src/Coupling.f90), the rules of
 * runsimulation's loop between two steps (sky view, coupling window, relaxation, observation forcing: "the rules
 * between the steps" below, called by every loop shape), the general time loop with a time index per lane and the
 * initial state, written once and compiled per arithmetic type like rs_physics_body.inc.  Unlike that file it is included INSIDE the flavour's namespace (rs in rs_kernels.hip, rs32 in
 * rs_kernels_f32.hip), behind the flavour's own helpers, because it stands on them:
 *   kBlock, ConstsAS, consts_of, KernArgs, MathTab                     types of the flavour
 *   gather_forcing(ka, p, i, t0), gather_sky(ka, p, i, t0, sw_dir, lw_net), store_point(ka, row, p, s, valid)
 *                                       the flavour's view of the forcing and output streams
 *   sky_view_radiation(...)             on the flavour's reals (rs_skyview.hpp is fp64)
 *   bl_diagnose(...)                    fp64 only (RS_GEN_FP64_FEATURES)
 * and on the flavour macros RS_REAL, R4(x), RS_DIVC, RS_SECANT_DIV, RS_PROFILE_PIN, RS_CPL_SLOTS(c),
 * RS_CPL_DECAY_TABLE, RS_RELAX_TABLE, RS_GEN_PREFETCH, RS_GEN_FP64_FEATURES, RS_INIT_KERNEL, RS_INIT_ANCHOR, RS_INIT_ZERO_TAIL
 * (rs_physics.hpp; the head of rs_kernels_f32.hip), each of which says there which flavour has what. */

/* Output row of time index i: false when the decimation skips it.  UNI: the index is the same in
 * every lane (lock-step kernels) and the row is formed once per step, ahead of the divergent
 * branches, so that it stays in scalar registers (a row computed at each store site is merged by
 * the compiler into a per-lane value). */
template <bool UNI>
__device__ __forceinline__ bool output_row(KernArgs ka, int32_t i, int64_t &row) {
  int32_t r = i - 1;
  const int32_t dec = ka->o.decimate;
  if (dec > 1) {
    if (r % dec != 0) return false;
    r /= dec;
  }
  if (UNI) r = __builtin_amdgcn_readfirstlane(r);
  row = ((int64_t)r - ka->o.row0) * ka->o.t_stride;
  return true;
}

template <int NL>
struct RegProfile {
  RS_REAL v[NL];
  static constexpr bool kUnrolled = true; /* the layer count is a compile-time constant */
  __device__ __forceinline__ constexpr int nlayers() const { return NL; }
  __device__ __forceinline__ RS_REAL get(int j) const { return v[j - 1]; }
  __device__ __forceinline__ void set(int j, RS_REAL x) { v[j - 1] = x; }
  /* "the new profile exists here": without it the compiler sinks the update of the layers nothing in
   * the rest of the step reads (3..N) behind the storages into the loop latch, where the layer
   * constants no longer fit the scalar registers (124 v_readlane/v_writelane per step) */
  __device__ __forceinline__ void pin() {
#if RS_PROFILE_PIN
#pragma unroll
    for (int j = 0; j < NL; ++j) asm volatile("" : "+v"(v[j]));
#endif
  }
};

struct LdsProfile {
  RS_REAL *col; /* &lds[threadIdx.x]; layer stride = kBlock values */
  int n;
  static constexpr bool kUnrolled = false;
  __device__ __forceinline__ int nlayers() const { return n; }
  __device__ __forceinline__ RS_REAL get(int j) const { return col[(j - 1) * kBlock]; }
  __device__ __forceinline__ void set(int j, RS_REAL x) { col[(j - 1) * kBlock] = x; }
  __device__ __forceinline__ void pin() {}
};

/* FULL: with the relaxation anchors (untouched by the LEAN variant).  TNW = false: TmpNw(1:2) are taken from the
 * profile, not from their slots (the fp32 one-point-per-lane kernels).
 * (`#pragma unroll` here and in store_state is for the profiles with a compile-time layer count; over LdsProfile's
 * runtime count the compiler answers "loop not unrolled" (-Wpass-failed) once per instance, in either flavour.  The
 * pragma stays unconditional: the fp64 kernels' machine code is held to what this very text gives.) */
template <bool FULL, class Prof, bool TNW = true>
__device__ __forceinline__ void load_state(const RS_REAL *__restrict__ st, int64_t np, int64_t p,
                                           Prof &T, Scalars &s) {
  const int N = T.nlayers();
#pragma unroll
  for (int j = 1; j <= N; ++j) T.set(j, st[(int64_t)(RS_ST_TMP0 + j - 1) * np + p]);
  s.tnw1 = TNW ? st[(int64_t)RS_ST_TNW1 * np + p] : T.get(1);
  s.tnw2 = TNW ? st[(int64_t)RS_ST_TNW2 * np + p] : T.get(2);
  s.tsurf = st[(int64_t)RS_ST_TSURF * np + p];
  s.wat = st[(int64_t)RS_ST_WAT * np + p];
  s.snow = st[(int64_t)RS_ST_SNOW * np + p];
  s.ice = st[(int64_t)RS_ST_ICE * np + p];
  s.ice2 = st[(int64_t)RS_ST_ICE2 * np + p];
  s.dep = st[(int64_t)RS_ST_DEP * np + p];
  s.q2melt = st[(int64_t)RS_ST_Q2MELT * np + p];
  s.t4melt = st[(int64_t)RS_ST_T4MELT * np + p];
  s.albedo = st[(int64_t)RS_ST_ALBEDO * np + p];
  s.verycold = st[(int64_t)RS_ST_VERYCOLD * np + p] != R4(0.0);
  s.failed = st[(int64_t)RS_ST_FAILED * np + p] != R4(0.0);
  if (FULL) {
    s.tair_end = st[(int64_t)RS_ST_TAIR_END * np + p];
    s.vz_end = st[(int64_t)RS_ST_VZ_END * np + p];
    s.rh_end = st[(int64_t)RS_ST_RH_END * np + p];
  } else {
    s.tair_end = s.vz_end = s.rh_end = 0.0;
  }
}

/* ANCHORS: the relaxation anchors are part of the Scalars (the general kernel); the lock-step loop writes them to
 * the state block at the index that sets them and carries differences.  TNW = false: the TmpNw(1:2) slots are left
 * alone (step_kernel_f32_lds) */
template <bool FULL, class Prof, bool ANCHORS = false, bool TNW = true>
__device__ __forceinline__ void store_state(RS_REAL *__restrict__ st, int64_t np, int64_t p,
                                            const Prof &T, const Scalars &s) {
  const int N = T.nlayers();
#pragma unroll
  for (int j = 1; j <= N; ++j) st[(int64_t)(RS_ST_TMP0 + j - 1) * np + p] = T.get(j);
  if (TNW) {
    st[(int64_t)RS_ST_TNW1 * np + p] = s.tnw1;
    st[(int64_t)RS_ST_TNW2 * np + p] = s.tnw2;
  }
  st[(int64_t)RS_ST_TSURF * np + p] = s.tsurf;
  st[(int64_t)RS_ST_WAT * np + p] = s.wat;
  st[(int64_t)RS_ST_SNOW * np + p] = s.snow;
  st[(int64_t)RS_ST_ICE * np + p] = s.ice;
  st[(int64_t)RS_ST_ICE2 * np + p] = s.ice2;
  st[(int64_t)RS_ST_DEP * np + p] = s.dep;
  st[(int64_t)RS_ST_Q2MELT * np + p] = s.q2melt;
  st[(int64_t)RS_ST_T4MELT * np + p] = s.t4melt;
  st[(int64_t)RS_ST_ALBEDO * np + p] = s.albedo;
  st[(int64_t)RS_ST_VERYCOLD * np + p] = s.verycold ? R4(1.0) : R4(0.0);
  /* RS_ST_FAILED is written where the failure is detected (the index it happened at) */
  if (FULL && ANCHORS) {
    st[(int64_t)RS_ST_TAIR_END * np + p] = s.tair_end;
    st[(int64_t)RS_ST_VZ_END * np + p] = s.vz_end;
    st[(int64_t)RS_ST_RH_END * np + p] = s.rh_end;
  }
}

/* ---- coupling: src/Coupling.f90 -------------------------------------------------
 * Per-point state machine that re-runs the point's coupling window with a scaled
 * short- or long-wave input until the simulated surface temperature at the end of
 * the window matches the last observation (secant / halving / doubling, <= 25
 * replays).  On the device every lane carries its OWN time index: a replay sets it
 * back to the window start (src/Coupling.f90:61-78), so forcing reads and output
 * writes are per-lane gathers/scatters into the (whole-series) windows, and a wave
 * runs until its slowest lane is through.  The saved state of
 * saveDataForCoupling (:172-210) is parked in the HBM state block. */
struct Coupling {
  RS_REAL tabove, tbelow, radcoeff, rcabove, rcbelow, rcprev, swcof, lwcof, swcorr, lwcorr,
      tend1, lastobs;
  int32_t iter, cs, ce; /* Coupling_iterations, couplingStartI, couplingEndI */
  int32_t msg;          /* bits 3-4 of RS_ST_CPL_FLAGS: what Coupling_control has printed for the point (rs_state.h) */
  bool again, failed, on;
};

/* Coupling_control, src/Coupling.f90:292-481 (called with Coupling_failed == .false.).
 * TsurfAve and LastTsurfObs make a round trip through Kelvin (+273.16, -273.16); the
 * rounding that leaves behind is part of the reference's result. */
__device__ __forceinline__ void coupling_control(Coupling &q, RS_REAL &tsurf) {
  q.again = false;
  tsurf = tsurf + R4(273.16);
  q.lastobs = q.lastobs + R4(273.16);
  if (q.iter == 0) q.tend1 = tsurf;
  if (q.iter == 25) {
    if (rs_fabs(q.tend1 - q.lastobs) < rs_fabs(tsurf - q.lastobs)) q.again = true;
    q.swcof = R4(1.0); q.lwcof = R4(1.0); q.swcorr = R4(0.0); q.lwcorr = R4(0.0);
    q.radcoeff = R4(1.0);
    q.failed = true;
  } else if (q.lastobs < -100) {
    q.swcof = R4(1.0); q.lwcof = R4(1.0); q.swcorr = R4(0.0); q.lwcorr = R4(0.0);
    q.radcoeff = R4(1.0);
    q.failed = true;
    q.again = true;
  } else if (tsurf < R4(170.0) || tsurf > R4(400.0)) {
    q.swcof = R4(1.0); q.lwcof = R4(1.0); q.swcorr = R4(0.0); q.lwcorr = R4(0.0);
    q.failed = true;
    q.again = true;
    q.radcoeff = R4(1.0);
  } else if (tsurf - q.lastobs > R4(0.1)) {
    if (q.tabove < -100) {
      q.tabove = tsurf;
      q.rcabove = q.radcoeff;
    } else if (q.tabove - q.lastobs > tsurf - q.lastobs) {
      q.tabove = tsurf;
      q.rcabove = q.radcoeff;
    }
    q.again = true;
    if (q.tabove > -100 && q.tbelow > -100) {
      const RS_REAL da = q.tabove - q.lastobs, db = q.lastobs - q.tbelow;
      q.radcoeff = q.rcabove - RS_SECANT_DIV(da, da + db) * (q.rcabove - q.rcbelow);
    } else {
      q.radcoeff = R4(0.5) * q.radcoeff;
    }
    if (rs_fabs(q.radcoeff - q.rcprev) < R4(0.00005)) {
      q.tabove = -9999;
      q.tbelow = -9999;
    }
    if (q.radcoeff < R4(0.01)) { /* "coupling coefficient too small, coupling failed" (:400-401) */
      q.msg |= RS_CPL_MSG_SMALL;
      q.radcoeff = R4(1.0);
      q.failed = true;
      q.swcof = R4(1.0); q.lwcof = R4(1.0); q.swcorr = R4(0.0); q.lwcorr = R4(0.0);
    }
    q.rcprev = q.radcoeff;
  } else if (q.lastobs - tsurf > R4(0.1)) {
    if (q.tbelow < -100) {
      q.tbelow = tsurf;
      q.rcbelow = q.radcoeff;
    } else if (q.tbelow - q.lastobs < tsurf - q.lastobs) {
      q.tbelow = tsurf;
      q.rcbelow = q.radcoeff;
    }
    q.again = true;
    if (q.tabove > -100 && q.tbelow > -100) {
      const RS_REAL da = q.tabove - q.lastobs, db = q.lastobs - q.tbelow;
      q.radcoeff = q.rcabove - RS_SECANT_DIV(da, da + db) * (q.rcabove - q.rcbelow);
    } else {
      q.radcoeff = R4(2.0) * q.radcoeff;
    }
    if (rs_fabs(q.radcoeff - q.rcprev) < R4(0.00005)) {
      q.tabove = -9999;
      q.tbelow = -9999;
    }
    q.rcprev = q.radcoeff;
  } else {
    if (q.radcoeff > R4(3.0)) { /* "coupling coefficient too big, coupling failed" (:451-452) */
      q.msg |= RS_CPL_MSG_BIG;
      q.failed = true;
      q.radcoeff = R4(1.0);
      q.swcof = R4(1.0); q.lwcof = R4(1.0); q.swcorr = R4(0.0); q.lwcorr = R4(0.0);
    }
    q.swcorr = q.swcof - R4(1.0);
    q.lwcorr = q.lwcof - R4(1.0);
    q.failed = false;
    q.iter = -1;
    q.tabove = R4(-9999.0); q.tbelow = R4(-9999.0);
    q.radcoeff = R4(1.0);
    q.rcabove = R4(-9999.0); q.rcbelow = R4(-9999.0);
    q.rcprev = R4(1.0);
  }
  tsurf = tsurf - R4(273.16);
  q.lastobs = q.lastobs - R4(273.16);
}

__device__ __forceinline__ void load_coupling(const RS_REAL *st, int64_t np, int64_t p, Coupling &q) {
  q.iter = (int32_t)st[(int64_t)RS_ST_CPL_ITER * np + p];
  const int32_t fl = (int32_t)st[(int64_t)RS_ST_CPL_FLAGS * np + p];
  q.again = fl & 1; q.failed = (fl >> 1) & 1; q.msg = fl & (RS_CPL_MSG_SMALL | RS_CPL_MSG_BIG);
  q.tabove = st[(int64_t)RS_ST_CPL_TABOVE * np + p]; q.tbelow = st[(int64_t)RS_ST_CPL_TBELOW * np + p];
  q.radcoeff = st[(int64_t)RS_ST_CPL_RADCOEFF * np + p];
  q.rcabove = st[(int64_t)RS_ST_CPL_RCABOVE * np + p]; q.rcbelow = st[(int64_t)RS_ST_CPL_RCBELOW * np + p];
  q.rcprev = st[(int64_t)RS_ST_CPL_RCPREV * np + p];
  q.swcof = st[(int64_t)RS_ST_CPL_SWCOF * np + p]; q.lwcof = st[(int64_t)RS_ST_CPL_LWCOF * np + p];
  q.swcorr = st[(int64_t)RS_ST_CPL_SWCORR * np + p]; q.lwcorr = st[(int64_t)RS_ST_CPL_LWCORR * np + p];
  q.tend1 = st[(int64_t)RS_ST_CPL_TEND1 * np + p];
  q.lastobs = st[(int64_t)RS_ST_CPL_LASTOBS * np + p];
}

__device__ __forceinline__ void store_coupling(RS_REAL *st, int64_t np, int64_t p, const Coupling &q) {
  st[(int64_t)RS_ST_CPL_ITER * np + p] = (RS_REAL)q.iter;
  const int32_t keep = ((int32_t)st[(int64_t)RS_ST_CPL_FLAGS * np + p]) & 4;
  st[(int64_t)RS_ST_CPL_FLAGS * np + p] = (RS_REAL)(keep | (q.again ? 1 : 0) | (q.failed ? 2 : 0) | q.msg);
  st[(int64_t)RS_ST_CPL_TABOVE * np + p] = q.tabove; st[(int64_t)RS_ST_CPL_TBELOW * np + p] = q.tbelow;
  st[(int64_t)RS_ST_CPL_RADCOEFF * np + p] = q.radcoeff;
  st[(int64_t)RS_ST_CPL_RCABOVE * np + p] = q.rcabove; st[(int64_t)RS_ST_CPL_RCBELOW * np + p] = q.rcbelow;
  st[(int64_t)RS_ST_CPL_RCPREV * np + p] = q.rcprev;
  st[(int64_t)RS_ST_CPL_SWCOF * np + p] = q.swcof; st[(int64_t)RS_ST_CPL_LWCOF * np + p] = q.lwcof;
  st[(int64_t)RS_ST_CPL_SWCORR * np + p] = q.swcorr; st[(int64_t)RS_ST_CPL_LWCORR * np + p] = q.lwcorr;
  st[(int64_t)RS_ST_CPL_TEND1 * np + p] = q.tend1;
  st[(int64_t)RS_ST_CPL_LASTOBS * np + p] = q.lastobs;
}

/* the stale TmpNw of a replay's first step, parked in the state block (one column per point) */
struct GlobalProfile {
  const RS_REAL *col;
  int64_t stride;
  __device__ __forceinline__ RS_REAL get(int j) const { return col[(int64_t)(j - 1) * stride]; }
};

/* exp(-(DT*i - DT*couplingEndI)/couplingEffectReduction), src/Coupling.f90:80-88: from the plan's
 * table where the argument is a function of i - couplingEndI alone (rs_consts_dev.h), else here */
__device__ __forceinline__ RS_REAL cpl_decay(const ConstsAS &c, const MathTab &mt, int32_t i, int32_t ce) {
#if RS_CPL_DECAY_TABLE
  const uint32_t d = (uint32_t)(i - ce);
  if (c.cpl_tab && d <= (uint32_t)c.SimLen) return ((const double *)c.cpl_tab)[d];
#endif
  return rs_exp(mt, rs_div(-((c.DTSecs * i) - (c.DTSecs * ce)), c.cplReduction));
}

/* ---- the rules between the steps: what runsimulation's loop decides per point and per index, each stated once --------
 * The loop shapes call these: the lock-step loop (time_loop), the surface and sky wavefronts of the two- and
 * three-wavefront one (duo_surface, duo_sky) and the general loop below.  A point is addressed as (row0, lane) - base[row0 + lane] with the
 * row base on the scalar unit - or as (p, 0) where the loop has no uniform base.
 * Sites that keep their own spelling, because the shared one costs machine code that does not come back
 * (tools/compare_device_code.py against the text before):
 *   - duo_ground, the ground wavefront: its relaxation, observation forcing and window start (relax_targets,
 *     relax_valid, relax_factor, relax_apply, obs_forced, cpl_window): through them step_kernel_duo<15, ., SRC_RAW, FULL> grew by 26 instructions and the driver path's
 *     relaxation leg measured 0.1 % under the slowest of ten runs of the text before (median of ten, alternating);
 *   - relax_valid and obs_forced in time_loop: as functions of values they are simplified before they are inlined
 *     and every FULL one-point-per-lane kernel came out in another instruction order;
 *   - x2d_ground (rs_kernels_f32.hip), the fp32 two-points-per-lane ground wave: sky_point, horizon_row,
 *     sky_limits_bad, relax_valid and obs_forced fit a component of its f2 forms, but with them the FULL instances
 *     spill two to twelve registers more and the LEAN knot-reading ones allocate differently; it reads as before;
 *   - the horizon row of the general loop (time_loop_coupled): formed inside the loop from the point's own index -
 *     with SkyPoint::hcol carried across the loop step_kernel_coupled spilled four registers more;
 *   - cpl_window_bounds_kernel: see cpl_window. */

/* Sky view.  The point's set-up, examples/example1/src/Simulation.f90:154-156: fp64 arithmetic in both flavours (the
 * sun's position decides which degree of the horizon is read: rs_skyview.hpp; sky_view_radiation on floats converts in
 * and out), the limits are REAL(4) literals.  sin / cos of the longitude once per launch: the addition theorem's point
 * half.  hcol: the point's column of the local-horizon table (RsPointParams::horizon_index).  The caller has checked
 * that the plan carries sky view (ka->pp.sky_view). */
struct SkyPoint {
  double skyv = R4(1.0), sinlat = 0, coslat = 0, lonrad = 0, coslon = 1.0, sinlon = 0;
  uint32_t hcol = 0;
  bool on = false;
};
__device__ __forceinline__ SkyPoint sky_point(KernArgs ka, int64_t row0, uint32_t lane = 0u) {
  SkyPoint k;
  k.skyv = (ka->pp.sky_view + row0)[lane];
  k.on = (k.skyv < R4(1.0) && k.skyv > R4(-0.01));
  if (k.on) {
    k.sinlat = (ka->pp.sin_lat + row0)[lane];
    k.coslat = (ka->pp.cos_lat + row0)[lane];
    k.lonrad = (ka->pp.lon_rad + row0)[lane];
    k.coslon = ::cos(k.lonrad);
    k.sinlon = ::sin(k.lonrad);
  }
  k.hcol = ka->pp.horizon_index ? (uint32_t)(ka->pp.horizon_index + row0)[lane] : (uint32_t)row0 + lane;
  return k;
}
/* the horizon row of column hcol and the stride between its degrees: [point][360] or [360][np_pad] */
__device__ __forceinline__ const double *horizon_row(KernArgs ka, int64_t hcol, int64_t &stride) {
  const double *row = ka->pp.horizons ? ka->pp.horizons + (ka->pp.horizons_by_point ? hcol * 360 : hcol) : nullptr;
  stride = ka->pp.horizons_by_point ? (int64_t)1 : ka->np_pad;
  return row;
}
/* CheckValues with sky view, src/InputOutput.f90:68-74: the limits of SW_dir and LW_net; :75-77: SW_dir <= SW */
__device__ __forceinline__ bool sky_limits_bad(RS_REAL sw_dir, RS_REAL lw_net) {
  return sw_dir < R4(-0.1) || sw_dir > R4(4000.0) || lw_net < R4(-1000.0) || lw_net > R4(1000.0);
}
__device__ __forceinline__ RS_REAL sky_clamp_direct(RS_REAL sw_dir, RS_REAL sw) { return sw_dir > sw ? sw : sw_dir; }
/* The caller's arrays as the reference leaves them, where the launch asks for that (StepArgs::wb): SW_dir clamped by
 * CheckValues, SW / SW_dir / LW edited by ModRadiationBySurroundings (src/ModRadiation.f90:57-71); a replay overwrites
 * them.  k: the window row; put(base, v): the loop's own store of its point's element of the row at base. */
template <class Put>
__device__ __forceinline__ void sky_write_back(KernArgs ka, int32_t k, int64_t row0, bool sky_on, double sw_dir,
                                               double sw, double lw, Put put) {
  if (ka->wb.sw_dir) {
    const int64_t wrow = (int64_t)k * ka->wb.t_stride + row0;
    put(ka->wb.sw_dir + wrow, sw_dir);
    if (sky_on) {
      put(ka->wb.sw + wrow, sw);
      put(ka->wb.lw + wrow, lw);
    }
  }
}

/* Coupling.  The window's times: setInputParam + initCouplingTimes, src/InputOutput.f90:30-36, src/Coupling.f90:486-534.
 * (Filled through a reference: returned by value, step_kernel_cpl_replay<false> spilled five scalar registers fewer -
 * a difference all the same, tools/compare_device_code.py.  Kept spelled out: cpl_window_bounds_kernel, the replay
 * call's coverage check, which knows the plan is coupled - through this function its register count changed, 8 -> 6.) */
struct CplWindow {
  int32_t cs = -99, ce = -99; /* couplingStartI, couplingEndI */
  bool on = false;
};
__device__ __forceinline__ void cpl_window(KernArgs ka, const ConstsAS &c, int64_t row0, uint32_t lane, CplWindow &w) {
  const int32_t cidx = ka->pp.coupling_index ? (ka->pp.coupling_index + row0)[lane] : 0;
  w.on = c.use_coupling && ka->pp.coupling_index && !((ka->pp.coupling_tsurf + row0)[lane] < -100 || cidx < 1);
  if (w.on) {
    w.ce = cidx;
    w.cs = ((RS_REAL)cidx <= c.cplLenR) ? 1 : cidx - c.cplLenI;
  }
}
/* saveDataForCoupling, src/Coupling.f90:172-210: the surface scalars, VeryCold in bit 2 of the flag word.  The layers
 * (RS_ST_CPL_SAVE_TMP0 ...) are the caller's: each wavefront saves and restores the ones it owns. */
__device__ __forceinline__ void cpl_save_surface(RS_REAL *st, int64_t np, int64_t p, const Scalars &s) {
  st[(int64_t)RS_ST_CPL_SAVE_TSURF * np + p] = s.tsurf;
  st[(int64_t)RS_ST_CPL_SAVE_WAT * np + p] = s.wat;
  st[(int64_t)RS_ST_CPL_SAVE_ICE2 * np + p] = s.ice2;
  st[(int64_t)RS_ST_CPL_SAVE_DEP * np + p] = s.dep;
  st[(int64_t)RS_ST_CPL_SAVE_SNOW * np + p] = s.snow;
  st[(int64_t)RS_ST_CPL_SAVE_ALBEDO * np + p] = s.albedo;
  const int32_t fl = ((int32_t)st[(int64_t)RS_ST_CPL_FLAGS * np + p]) & (3 | RS_CPL_MSG_SMALL | RS_CPL_MSG_BIG);
  st[(int64_t)RS_ST_CPL_FLAGS * np + p] = (RS_REAL)(fl | (s.verycold ? 4 : 0));
}
/* uploadDataForCoupling, src/Coupling.f90:213-255: SrfIcemms, Q2Melt, T4Melt and TmpNw are NOT restored (TmpNw keeps
 * the end-of-window profile for the first step).  CLEAR_AGAIN: start_coupling_again = .false. goes to the flag word
 * here (the lock-step loops; the general loop carries the flag in its Coupling and stores it at its end). */
template <bool CLEAR_AGAIN>
__device__ __forceinline__ void cpl_restore_surface(RS_REAL *st, int64_t np, int64_t p, Scalars &s) {
  s.tsurf = st[(int64_t)RS_ST_CPL_SAVE_TSURF * np + p];
  s.wat = st[(int64_t)RS_ST_CPL_SAVE_WAT * np + p];
  s.ice2 = st[(int64_t)RS_ST_CPL_SAVE_ICE2 * np + p];
  s.dep = st[(int64_t)RS_ST_CPL_SAVE_DEP * np + p];
  s.snow = st[(int64_t)RS_ST_CPL_SAVE_SNOW * np + p];
  s.albedo = st[(int64_t)RS_ST_CPL_SAVE_ALBEDO * np + p];
  const int32_t fl = (int32_t)st[(int64_t)RS_ST_CPL_FLAGS * np + p];
  s.verycold = (fl & 4) != 0;
  if (CLEAR_AGAIN) st[(int64_t)RS_ST_CPL_FLAGS * np + p] = (RS_REAL)(fl & ~1);
}
/* SWRadCof / LWRadCof of a replay, src/Coupling.f90:68-76: short-wave scaling by day, long-wave by night - and always
 * with sky view */
__device__ __forceinline__ void cpl_rewind_coefs(RS_REAL radcoeff, RS_REAL sw, RS_REAL lw, bool sky_on, RS_REAL &swcof,
                                                 RS_REAL &lwcof) {
  if (sw > lw && !sky_on) {
    swcof = radcoeff;
    lwcof = R4(1.0);
  } else {
    swcof = R4(1.0);
    lwcof = radcoeff;
  }
}
/* behind the window the corrections decay, :80-88 */
__device__ __forceinline__ void cpl_decayed_coefs(const ConstsAS &c, const MathTab &mt, int32_t i, int32_t ce,
                                                  RS_REAL swcorr, RS_REAL lwcorr, RS_REAL &swcof, RS_REAL &lwcof) {
  const RS_REAL e = cpl_decay(c, mt, i, ce);
  swcof = R4(1.0) + swcorr * e;
  lwcof = R4(1.0) + lwcorr * e;
}
/* lastValues (src/InputOutput.f90:169-198) runs no CouplingOperations1: coupling%inCouplingPhase and SW/LWRadCof keep
 * the values of index SimLen - 1 - decayed behind the window; where the window reaches the end of the series, as the
 * last pass left them in the state block.  (The general loop carries the coefficients and needs the phase only.) */
__device__ __forceinline__ void cpl_last_values(const ConstsAS &c, const MathTab &mt, const CplWindow &w, RS_REAL swcorr,
                                                RS_REAL lwcorr, const RS_REAL *st, int64_t np, int64_t p,
                                                CouplingInputs &cp) {
  const int32_t j = c.SimLen - 1;
  cp.in_phase = (j >= w.cs && j <= w.ce);
  if (j > w.ce) {
    cpl_decayed_coefs(c, mt, j, w.ce, swcorr, lwcorr, cp.sw_cof, cp.lw_cof);
  } else if (j >= w.cs) {
    cp.sw_cof = st[(int64_t)RS_ST_CPL_SWCOF * np + p];
    cp.lw_cof = st[(int64_t)RS_ST_CPL_LWCOF * np + p];
  }
}
/* snowIceCheck, src/Coupling.f90:259-289 (in the coupling phase) */
__device__ __forceinline__ void snow_ice_check(const ConstsAS &c, RS_REAL lastobs, Scalars &s) {
  if (lastobs > c.TLimMeltSnow && s.snow > R4(0.00)) { s.wat = s.wat + s.snow; s.snow = R4(0.00); }
  if (lastobs > c.TLimMeltIce && s.ice > R4(0.00)) { s.wat = s.wat + s.ice; s.ice = R4(0.00); }
  if (lastobs > c.TLimMeltIce && s.ice2 > R4(0.00)) s.ice2 = R4(0.00);
  if (lastobs > c.TLimMeltDep && s.dep > R4(0.00)) { s.wat = s.wat + s.dep; s.dep = R4(0.00); }
}
/* CheckEndCoupling + CouplingOperations2 at the window end, src/Coupling.f90:98-141, for a point whose coupling has not
 * failed.  A point that failed CheckValues at this very index still runs Coupling_control (CheckEndCoupling does not
 * look at simulation_failed), but its loop exits before any rewind: it asks for no replay - the rows behind its window
 * stay -9999.0 - and is not listed. */
__device__ __forceinline__ void cpl_decide(Coupling &q, Scalars &s) {
  if (q.iter == 0) q.tend1 = s.tsurf;
  coupling_control(q, s.tsurf);
  q.iter = q.iter + 1;
  if (s.failed) q.again = false;
}
/* ... where CouplingVariables live in the state block (the lock-step loops: Coupling_failed is .false. before the first
 * decision).  The corrections and the observation - which went to Kelvin and back in Coupling_control - return to the
 * caller's registers; parked: the point replays its window in the rounds (RS_ST_CPL_RESUME = i + 1). */
__device__ __forceinline__ void cpl_window_end(RS_REAL *st, int64_t np, int64_t p, const CplWindow &w, Scalars &s,
                                               RS_REAL &swcorr, RS_REAL &lwcorr, RS_REAL &lastobs, bool &parked) {
  Coupling q;
  load_coupling(st, np, p, q);
  q.cs = w.cs; q.ce = w.ce; q.on = true;
  if (!q.failed) {
    cpl_decide(q, s);
    store_coupling(st, np, p, q);
    swcorr = q.swcorr;
    lwcorr = q.lwcorr;
    lastobs = q.lastobs;
    parked = q.again;
  }
}

/* Relaxation, src/Relaxation.f90:10-47.  The targets pass through REAL(4) (setInputParam, src/InputOutput.f90:19-26);
 * RelaxationOperations (:34-43) only ever uses target - anchor, the anchors being the forcing of index InitLenI. */
__device__ __forceinline__ void relax_targets(KernArgs ka, int64_t row0, uint32_t lane, RS_REAL &tairR, RS_REAL &vzR,
                                              RS_REAL &rhR) {
  tairR = (RS_REAL)(float)(ka->pp.tair_relax + row0)[lane];
  vzR = (RS_REAL)(float)(ka->pp.vz_relax + row0)[lane];
  rhR = (RS_REAL)(float)(ka->pp.rh_relax + row0)[lane];
}
__device__ __forceinline__ bool relax_valid(RS_REAL tairR, RS_REAL vzR, RS_REAL rhR) {
  return !(tairR < R4(-100.0) || tairR > R4(100.0) || vzR < R4(0.0) || vzR > R4(100.0) || rhR < R4(0.0) || rhR > 110);
}
/* exp(-(DT*i - DT*InitLenI)/14400), i > InitLenI: for an integral time step the argument is a function of i - InitLenI
 * alone and the plan holds the table (rs_consts_dev.h, host libm = the bits rs_exp returns); otherwise evaluated here.
 * TABLE = false: the general loop, which has never read the table, in either flavour. */
template <bool TABLE = (RS_RELAX_TABLE != 0)>
__device__ __forceinline__ RS_REAL relax_factor(const ConstsAS &c, const MathTab &mt, int32_t i, int32_t initlen) {
  RS_REAL e;
#if RS_RELAX_TABLE
  const uint32_t d = (uint32_t)(i - initlen);
  if (TABLE && c.relax_tab && d <= (uint32_t)c.SimLen) {
    e = ((const double *)c.relax_tab)[d];
  } else
#endif
  {
    const RS_REAL den = (RS_REAL)(4.f * 3600.f);
    e = rs_exp(mt, rs_div(-((c.DTSecs * i) - (c.DTSecs * initlen)), den));
  }
  return e;
}
/* d*: target - anchor */
__device__ __forceinline__ void relax_apply(RS_REAL e, RS_REAL dt, RS_REAL dv, RS_REAL dr, RS_REAL &tair, RS_REAL &vz,
                                            RS_REAL &rhz) {
  tair = tair - dt * e;
  vz = vz - dv * e;
  rhz = rhz - dr * e;
  if (rhz > R4(100.)) rhz = R4(100.0);
}

/* SetCurrentValues' observation forcing, src/InputOutput.f90:116-148: the observation goes on Tmp(1:2) during the
 * initialization phase (force_tsurf: always), but never from the start of the point's coupling window on (:120-121) */
__device__ __forceinline__ bool obs_forced(const ConstsAS &c, int32_t i, int32_t initlen, RS_REAL obs, bool cpl_on,
                                           int32_t cs) {
  return (i <= initlen || c.force_tsurf) && obs > R4(-100.0) && (!cpl_on || i < cs);
}

/* runsimulation's loop with coupling (examples/example1/src/Simulation.f90:57-115):
 * CheckValues -> CouplingOperations1 (may rewind i) -> SetCurrentValues -> relaxation ->
 * roadModelOneStep -> SaveOutput -> CheckEndCoupling. */
template <class Prof, bool DIAG = false>
__device__ __forceinline__ void time_loop_coupled(const MathTab &mt, Prof &T, Scalars &s,
                                                  Coupling &q, RS_REAL *st, int64_t np, int64_t p) {
  KernArgs ka = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const ConstsAS &c = consts_of(ka);
  const int N = T.nlayers();
  const int32_t t0 = ka->t0, tend = ka->t0 + ka->nsteps;
  const RS_REAL tbot = (RS_REAL)ka->pp.tbottom[p];
  const int32_t initlen = ka->pp.initlen ? ka->pp.initlen[p] : 0;
  bool relax = false;
  RS_REAL tairR = 0, vzR = 0, rhR = 0;
  if (c.use_relaxation && ka->pp.tair_relax) {
    relax_targets(ka, p, 0u, tairR, vzR, rhR);
    relax = relax_valid(tairR, vzR, rhR);
  }
  CplWindow w;
  cpl_window(ka, c, p, 0u, w);
  q.on = w.on; q.cs = w.cs; q.ce = w.ce;
  SkyPoint sky;
  if (ka->pp.sky_view) sky = sky_point(ka, p);
  const bool sky_on = sky.on;

  auto fail_at = [&](int32_t idx) {
    s.failed = true;
    st[(int64_t)RS_ST_FAILED * np + p] = (RS_REAL)idx;
  };
  /* rounds (rs_hip_step): the point resumes where it stopped; a parked point (resume = window
   * end + 1, start_coupling_again set) rewinds to its window start in the first iteration */
  const int32_t resume = RS_CPL_SLOTS(c) ? (int32_t)st[(int64_t)RS_ST_CPL_RESUME * np + p] : t0;
  int32_t i = resume > t0 ? resume : t0;
  int32_t written_hi = i - 1; /* highest index the point has saved an output for */
  bool stale_all = false; /* first step after a restore: TmpNw is the pre-restore profile */
  /* RS_GEN_PREFETCH: the forcing of index i+1 is fetched in the middle of step i (a replay that rewinds fetches
   * its row again): with two waves per SIMD a load issued at its point of use would stall every step */
  Forcing nxt;
  int32_t nxt_i = -1;
  if (RS_GEN_PREFETCH && i < tend && !s.failed) {
    nxt = gather_forcing(ka, p, i, t0);
    nxt_i = i;
  }
  while (i < tend) {
    if (s.failed) {
      /* the reference's loop has exited: outputs it never saved stay -9999.0 - but a point
       * that fails in the middle of a coupling replay keeps, beyond the failure, what the
       * EARLIER passes saved there (src/InputOutput.f90:151-165 only ever overwrites) */
      int64_t orow;
      if (i > written_hi && output_row<false>(ka, i, orow)) store_point(ka, orow, p, s, false);
      ++i;
      continue;
    }
    Forcing f = (RS_GEN_PREFETCH && nxt_i == i) ? nxt : gather_forcing(ka, p, i, t0);
    if (i == 1 && f.vz < R4(0.4)) f.vz = R4(0.4);
    CouplingInputs cp;
    RS_REAL sw_dir = 0.0, lw_net = 0.0;
    if (ka->f.sw_dir) gather_sky(ka, p, i, t0, sw_dir, lw_net);
    if (i < c.SimLen) {
      if (check_values(c, f, s.tsurf, ka->f.tdew != nullptr)) fail_at(i);
      if (sky_on && sky_limits_bad(sw_dir, lw_net)) fail_at(i);
      sw_dir = sky_clamp_direct(sw_dir, f.sw);
      if (q.on) {
        /* CouplingOperations1, src/Coupling.f90:10-96 */
        bool in_phase = (i >= q.cs && i <= q.ce);
        if (i == q.cs && q.iter == 0) {
          cpl_save_surface(st, np, p, s);
          for (int j = 1; j <= N; ++j) st[(int64_t)(RS_ST_CPL_SAVE_TMP0 + j - 1) * np + p] = T.get(j);
          q.swcof = R4(1.0); q.lwcof = R4(1.0); q.swcorr = R4(0.0); q.lwcorr = R4(0.0);
        }
        if (q.again) { /* back to the window start */
          i = q.cs;
          cpl_restore_surface<false>(st, np, p, s);
          for (int j = 1; j <= N; ++j) {
            st[(int64_t)(RS_ST_CPL_STALE_TMP0 + j - 1) * np + p] = T.get(j);
            T.set(j, st[(int64_t)(RS_ST_CPL_SAVE_TMP0 + j - 1) * np + p]);
          }
          stale_all = true;
          q.again = false;
          f = gather_forcing(ka, p, i, t0);
          if (i == 1 && f.vz < R4(0.4)) f.vz = R4(0.4);
          if (ka->f.sw_dir) {
            /* the restored window holds the arrays as CheckValues left them in the first
             * pass: SW_dir already clamped to SW (src/Coupling.f90:204-208,249-253) */
            gather_sky(ka, p, i, t0, sw_dir, lw_net);
            sw_dir = sky_clamp_direct(sw_dir, f.sw);
          }
          cpl_rewind_coefs(q.radcoeff, f.sw, f.lw, sky_on, q.swcof, q.lwcof);
        }
        if (i > q.ce) cpl_decayed_coefs(c, mt, i, q.ce, q.swcorr, q.lwcorr, q.swcof, q.lwcof);
        if (in_phase) snow_ice_check(c, q.lastobs, s);
        cp.in_phase = in_phase;
      }
      if (obs_forced(c, i, initlen, f.tsurfobs, q.on, q.cs)) {
        T.set(1, f.tsurfobs);
        T.set(2, f.tsurfobs);
        const RS_REAL depth = (c.tsurfOutputDepth >= R4(0.0)) ? c.tsurfOutputDepth : f.depth;
        s.tsurf = surface_temperature(c, T, tbot, depth);
      }
    } else {
      /* lastValues, src/InputOutput.f90:169-198 */
      s.tsurf = surface_temperature(c, T, tbot, f.depth);
      cp.in_phase = false; /* coupling%inCouplingPhase keeps its last value: index SimLen-1 */
      if (q.on) cp.in_phase = (c.SimLen - 1 >= q.cs && c.SimLen - 1 <= q.ce);
    }
    RS_REAL tair = f.tair, vz = f.vz, rhz = f.rhz;
    const RS_REAL prec_ts = RS_DIVC(f.prec, R4(3600.0), r_3600) * c.DTSecs;
    if (i < c.SimLen && relax) {
      if (i == initlen) { s.tair_end = tair; s.vz_end = vz; s.rh_end = rhz; } /* the anchors: part of this loop's Scalars */
      if (i > initlen)
        relax_apply(relax_factor<false>(c, mt, i, initlen), tairR - s.tair_end, vzR - s.vz_end, rhR - s.rh_end, tair, vz,
                    rhz);
    }
    cp.sw_cof = q.swcof; cp.lw_cof = q.lwcof; cp.last_tsurf_obs = q.lastobs;
    RS_REAL sw_in = f.sw, lw_in = f.lw;
    if (sky_on) {
      /* the reference runs this between PrecipitationToStorage and BalanceModelOneStep
       * (Simulation.f90:151-162); the two do not share data, so the order is free.  (The flavour's own
       * sky_view_radiation and, below, output_row + store_point spelled out here: with the conversions to double
       * or SaveOutput as one function in this text, step_kernel_coupled's machine code changed -
       * tools/compare_device_code.py) */
      if (!sky_view_radiation(ka->f.sun + (int64_t)(i - t0) * RS_SUN_COLS, sky.sinlat, sky.coslat, sky.lonrad, sky.coslon,
                              sky.sinlon, sky.skyv, ka->pp.albedo_surroundings,
                              ka->pp.horizons
                                  ? ka->pp.horizons + (ka->pp.horizon_index ? (int64_t)ka->pp.horizon_index[p] : p) *
                                                          (ka->pp.horizons_by_point ? 360 : 1)
                                  : nullptr,
                              ka->pp.horizons_by_point ? (int64_t)1 : np, sw_in, sw_dir, lw_in, lw_net))
        fail_at(i); /* the reference would `stop` the process here */
    }
#if RS_GEN_FP64_FEATURES
    sky_write_back(ka, i - t0, p, sky_on, sw_dir, sw_in, lw_in, [](double *base, double v) { *base = v; });
    if (DIAG) bl_diagnose(&c, mt.expT, mt.logT, mt.K, s.tsurf, tair, vz, rhz, f.hour, i, ka->diag, np, p);
#endif
    const Fluxes fx = model_step_fluxes(c, mt, s, tair, vz, rhz, prec_ts, sw_in, lw_in, f.phase,
                                        f.hour, cp);
    if (RS_GEN_PREFETCH && i + 1 < tend) { /* next index's forcing, half a step ahead of its use */
      nxt = gather_forcing(ka, p, i + 1, t0);
      nxt_i = i + 1;
    }
    if (stale_all) {
      /* observation forcing cannot follow a restore (i >= couplingStartI), so TmpNw(1:2)
       * are the stale values too */
      const GlobalProfile Tstale{st + (int64_t)RS_ST_CPL_STALE_TMP0 * np + p, np};
      model_step_ground(c, s, T, tbot, tair, fx, f.depth, cp, &Tstale);
      stale_all = false;
    } else {
      model_step_ground(c, s, T, tbot, tair, fx, f.depth, cp);
    }
    int64_t orow;
    if (output_row<false>(ka, i, orow)) store_point(ka, orow, p, s, true);
    if (i > written_hi) written_hi = i;
    if (i < c.SimLen && q.on && i == q.ce && !q.failed) {
      cpl_decide(q, s);
#if RS_GEN_FP64_FEATURES
      if (ka->cpl_stop) { /* park: the next round decides between a replay and going on */
        ++i;
        break;
      }
#endif
    }
    ++i;
  }
  if (RS_CPL_SLOTS(c)) st[(int64_t)RS_ST_CPL_RESUME * np + p] = (RS_REAL)i;
}

/* Device part of Initialization (src/Initialization.f90:65-147): initial
 * profile (initTemp :238-287), surface state (initSurf :290-308), T4Melt
 * (condInit :518), albedo (InitParam :339).  The first CalcBLCondAndLE call
 * (:138-139) and the first CalcHCapHCond (:109) only produce values that are
 * overwritten before they are read, so they are not executed.  The kernel's name is the flavour's (RS_INIT_KERNEL). */
__global__ void __launch_bounds__(kBlock) RS_INIT_KERNEL(const rs::InitArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.npoints) return;
  const ConstsAS &c = consts_of(&a);
  const int N = c.NLayers;
  const RS_REAL tair = ((const RS_REAL *)a.f.tair)[p];
  const RS_REAL tobs = a.f.tsurfobs ? ((const RS_REAL *)a.f.tsurfobs)[p] : R4(-9999.9);
  const RS_REAL depth = a.f.depth ? ((const RS_REAL *)a.f.depth)[p] : R4(-9999.9);
  const RS_REAL tbot = (RS_REAL)a.pp.tbottom[p];
  const RS_REAL t4 = (tobs > -100) ? tobs : tair;
  const int64_t np = a.np_pad;
  RS_REAL *st = (RS_REAL *)a.state;
  for (int i = 1; i <= 4; ++i) st[(int64_t)(RS_ST_TMP0 + i - 1) * np + p] = t4;
  for (int i = 5; i <= N; ++i)
    st[(int64_t)(RS_ST_TMP0 + i - 1) * np + p] =
        t4 + (tbot - t4) / (c.ZDpth[N + 1] - c.ZDpth[4]) * (c.ZDpth[i] - c.ZDpth[4]);
  if (RS_INIT_ZERO_TAIL)
    for (int i = N + 1; i <= RS_MAX_LAYERS; ++i) st[(int64_t)(RS_ST_TMP0 + i - 1) * np + p] = 0.0;
  RS_REAL tsurf;
  if (depth >= 0) {
    /* getTempAtDepth on the fresh profile, src/Initialization.f90:129-136 */
    if (rs_fabs(depth - R4(0.0)) < R4(0.00001)) {
      tsurf = t4;
    } else if (depth > c.ZDpth[N + 1]) {
      tsurf = tbot;
    } else {
      tsurf = 0.0;
      for (int k = 1; k <= N; ++k) {
        if (depth > c.ZDpth[k] && depth <= c.ZDpth[k + 1]) {
          const RS_REAL tk = st[(int64_t)(RS_ST_TMP0 + k - 1) * np + p];
          const RS_REAL tk1 = (k == N) ? tbot : st[(int64_t)(RS_ST_TMP0 + k) * np + p];
          tsurf = tk + (depth - c.ZDpth[k]) * (tk1 - tk) / (c.ZDpth[k + 1] - c.ZDpth[k]);
          break;
        }
      }
    }
  } else {
    tsurf = (t4 + t4) / R4(2.0);
  }
  st[(int64_t)RS_ST_TNW1 * np + p] = t4;
  st[(int64_t)RS_ST_TNW2 * np + p] = t4;
  st[(int64_t)RS_ST_TSURF * np + p] = tsurf;
  st[(int64_t)RS_ST_WAT * np + p] = R4(0.0);
  st[(int64_t)RS_ST_SNOW * np + p] = R4(0.0);
  st[(int64_t)RS_ST_ICE * np + p] = R4(0.0);
  st[(int64_t)RS_ST_ICE2 * np + p] = R4(0.0);
  st[(int64_t)RS_ST_DEP * np + p] = R4(0.0);
  st[(int64_t)RS_ST_Q2MELT * np + p] = R4(0.0);
  st[(int64_t)RS_ST_T4MELT * np + p] = c.T4Melt0;
  st[(int64_t)RS_ST_ALBEDO * np + p] = c.Albedo0;
  st[(int64_t)RS_ST_VERYCOLD * np + p] = 0.0;
  st[(int64_t)RS_ST_FAILED * np + p] = 0.0;
  st[(int64_t)RS_ST_TAIR_END * np + p] = RS_INIT_ANCHOR; /* src/Initialization.f90:377-379 */
  st[(int64_t)RS_ST_VZ_END * np + p] = RS_INIT_ANCHOR;
  st[(int64_t)RS_ST_RH_END * np + p] = RS_INIT_ANCHOR;
  st[(int64_t)RS_ST_BLSCORE * np + p] = 0.0;
  if (RS_CPL_SLOTS(c)) {
    /* initCoupling, src/Coupling.f90:144-169 */
    st[(int64_t)RS_ST_CPL_ITER * np + p] = 0.0;
    st[(int64_t)RS_ST_CPL_FLAGS * np + p] = 0.0;
    st[(int64_t)RS_ST_CPL_TABOVE * np + p] = R4(-9999.0);
    st[(int64_t)RS_ST_CPL_TBELOW * np + p] = R4(-9999.0);
    st[(int64_t)RS_ST_CPL_RADCOEFF * np + p] = R4(1.0);
    st[(int64_t)RS_ST_CPL_RCABOVE * np + p] = R4(-9999.0);
    st[(int64_t)RS_ST_CPL_RCBELOW * np + p] = R4(-9999.0);
    st[(int64_t)RS_ST_CPL_RCPREV * np + p] = R4(1.0);
    st[(int64_t)RS_ST_CPL_SWCOF * np + p] = R4(1.0);
    st[(int64_t)RS_ST_CPL_LWCOF * np + p] = R4(1.0);
    st[(int64_t)RS_ST_CPL_SWCORR * np + p] = R4(0.0);
    st[(int64_t)RS_ST_CPL_LWCORR * np + p] = R4(0.0);
    st[(int64_t)RS_ST_CPL_TEND1 * np + p] = 0.0;
    st[(int64_t)RS_ST_CPL_LASTOBS * np + p] = a.pp.coupling_tsurf ? (RS_REAL)a.pp.coupling_tsurf[p] : R4(-9999.0);
    st[(int64_t)RS_ST_CPL_RESUME * np + p] = 1.0;
  }
}
