/* rs_general_body.inc - what the kernels say about the state block, coupling (src/Coupling.f90), the general
 * time loop with a time index per lane and the initial state, written once and compiled per arithmetic type like
 * rs_physics_body.inc.  Unlike that file it is included INSIDE the flavour's namespace (rs in rs_kernels.hip, rs32 in
 * rs_kernels_f32.hip), behind the flavour's own helpers, because it stands on them:
 *   kBlock, ConstsAS, consts_of, KernArgs, MathTab                     types of the flavour
 *   gather_forcing(ka, p, i, t0), gather_sky(ka, p, i, t0, sw_dir, lw_net), store_point(ka, row, p, s, valid)
 *                                       the flavour's view of the forcing and output streams
 *   sky_view_radiation(...)             on the flavour's reals (rs_skyview.hpp is fp64)
 *   bl_diagnose(...)                    fp64 only (RS_GEN_FP64_FEATURES)
 * and on the flavour macros RS_REAL, R4(x), RS_DIVC, RS_SECANT_DIV, RS_PROFILE_PIN, RS_CPL_SLOTS(c),
 * RS_CPL_DECAY_TABLE, RS_GEN_PREFETCH, RS_GEN_FP64_FEATURES, RS_INIT_KERNEL, RS_INIT_ANCHOR, RS_INIT_ZERO_TAIL
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
    tairR = (RS_REAL)(float)ka->pp.tair_relax[p];
    vzR = (RS_REAL)(float)ka->pp.vz_relax[p];
    rhR = (RS_REAL)(float)ka->pp.rh_relax[p];
    relax = !(tairR < R4(-100.0) || tairR > R4(100.0) || vzR < R4(0.0) || vzR > R4(100.0) ||
              rhR < R4(0.0) || rhR > 110);
  }
  /* setInputParam + initCouplingTimes, src/InputOutput.f90:30-36, src/Coupling.f90:486-534 */
  const int32_t cidx = ka->pp.coupling_index ? ka->pp.coupling_index[p] : 0;
  q.on = c.use_coupling && ka->pp.coupling_index &&
         !(ka->pp.coupling_tsurf[p] < -100 || cidx < 1);
  q.cs = -99; q.ce = -99;
  if (q.on) {
    q.ce = cidx;
    q.cs = ((RS_REAL)cidx <= c.cplLenR) ? 1 : cidx - c.cplLenI;
  }
  /* sky view, examples/example1/src/Simulation.f90:154-156: fp64 arithmetic in both flavours (the sun's position
   * decides which degree of the horizon is read: rs_skyview.hpp; sky_view_radiation on floats converts in and out),
   * the limits are REAL(4) literals */
  double skyv = R4(1.0), sinlat = 0, coslat = 0, lonrad = 0, coslon = 1.0, sinlon = 0;
  bool sky_on = false;
  if (ka->pp.sky_view) {
    skyv = ka->pp.sky_view[p];
    sky_on = (skyv < R4(1.0) && skyv > R4(-0.01));
    if (sky_on) {
      sinlat = ka->pp.sin_lat[p];
      coslat = ka->pp.cos_lat[p];
      lonrad = ka->pp.lon_rad[p];
      coslon = ::cos(lonrad);
      sinlon = ::sin(lonrad);
    }
  }

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
      if (sky_on && (sw_dir < R4(-0.1) || sw_dir > R4(4000.0) || lw_net < R4(-1000.0) ||
                     lw_net > R4(1000.0)))
        fail_at(i); /* src/InputOutput.f90:68-74 */
      if (sw_dir > f.sw) sw_dir = f.sw; /* :75-77 */
      if (q.on) {
        /* CouplingOperations1, src/Coupling.f90:10-96 */
        bool in_phase = (i >= q.cs && i <= q.ce);
        if (i == q.cs && q.iter == 0) {
          /* saveDataForCoupling :172-210 */
          st[(int64_t)RS_ST_CPL_SAVE_TSURF * np + p] = s.tsurf;
          st[(int64_t)RS_ST_CPL_SAVE_WAT * np + p] = s.wat;
          st[(int64_t)RS_ST_CPL_SAVE_ICE2 * np + p] = s.ice2;
          st[(int64_t)RS_ST_CPL_SAVE_DEP * np + p] = s.dep;
          st[(int64_t)RS_ST_CPL_SAVE_SNOW * np + p] = s.snow;
          st[(int64_t)RS_ST_CPL_SAVE_ALBEDO * np + p] = s.albedo;
          const int32_t fl = ((int32_t)st[(int64_t)RS_ST_CPL_FLAGS * np + p]) & (3 | RS_CPL_MSG_SMALL | RS_CPL_MSG_BIG);
          st[(int64_t)RS_ST_CPL_FLAGS * np + p] = (RS_REAL)(fl | (s.verycold ? 4 : 0));
          for (int j = 1; j <= N; ++j) st[(int64_t)(RS_ST_CPL_SAVE_TMP0 + j - 1) * np + p] = T.get(j);
          q.swcof = R4(1.0); q.lwcof = R4(1.0); q.swcorr = R4(0.0); q.lwcorr = R4(0.0);
        }
        if (q.again) {
          /* uploadDataForCoupling :213-255: back to the window start; SrfIcemms, Q2Melt,
           * T4Melt and TmpNw are NOT restored */
          i = q.cs;
          s.tsurf = st[(int64_t)RS_ST_CPL_SAVE_TSURF * np + p];
          s.wat = st[(int64_t)RS_ST_CPL_SAVE_WAT * np + p];
          s.ice2 = st[(int64_t)RS_ST_CPL_SAVE_ICE2 * np + p];
          s.dep = st[(int64_t)RS_ST_CPL_SAVE_DEP * np + p];
          s.snow = st[(int64_t)RS_ST_CPL_SAVE_SNOW * np + p];
          s.albedo = st[(int64_t)RS_ST_CPL_SAVE_ALBEDO * np + p];
          s.verycold = (((int32_t)st[(int64_t)RS_ST_CPL_FLAGS * np + p]) & 4) != 0;
          for (int j = 1; j <= N; ++j) {
            /* TmpNw keeps the end-of-window profile */
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
            if (sw_dir > f.sw) sw_dir = f.sw;
          }
          /* short-wave scaling only without sky view (:68-76) */
          if (f.sw > f.lw && !sky_on) {
            q.swcof = q.radcoeff;
            q.lwcof = R4(1.0);
          } else {
            q.swcof = R4(1.0);
            q.lwcof = q.radcoeff;
          }
        }
        if (i > q.ce) {
          const RS_REAL e = cpl_decay(c, mt, i, q.ce);
          q.swcof = R4(1.0) + q.swcorr * e;
          q.lwcof = R4(1.0) + q.lwcorr * e;
        }
        if (in_phase) {
          /* snowIceCheck :259-289 */
          if (q.lastobs > c.TLimMeltSnow && s.snow > R4(0.00)) { s.wat = s.wat + s.snow; s.snow = R4(0.00); }
          if (q.lastobs > c.TLimMeltIce && s.ice > R4(0.00)) { s.wat = s.wat + s.ice; s.ice = R4(0.00); }
          if (q.lastobs > c.TLimMeltIce && s.ice2 > R4(0.00)) s.ice2 = R4(0.00);
          if (q.lastobs > c.TLimMeltDep && s.dep > R4(0.00)) { s.wat = s.wat + s.dep; s.dep = R4(0.00); }
        }
        cp.in_phase = in_phase;
      }
      /* SetCurrentValues obs forcing, src/InputOutput.f90:116-148 */
      if ((i <= initlen || c.force_tsurf) && f.tsurfobs > R4(-100.0) && (!q.on || i < q.cs)) {
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
    if (i < c.SimLen && relax) { /* RelaxationOperations, src/Relaxation.f90:10-47 */
      if (i == initlen) { s.tair_end = tair; s.vz_end = vz; s.rh_end = rhz; }
      if (i > initlen) {
        const RS_REAL den = (RS_REAL)(4.f * 3600.f);
        const RS_REAL e = rs_exp(mt, rs_div(-((c.DTSecs * i) - (c.DTSecs * initlen)), den));
        tair = tair - (tairR - s.tair_end) * e;
        vz = vz - (vzR - s.vz_end) * e;
        rhz = rhz - (rhR - s.rh_end) * e;
        if (rhz > R4(100.)) rhz = R4(100.0);
      }
    }
    cp.sw_cof = q.swcof; cp.lw_cof = q.lwcof; cp.last_tsurf_obs = q.lastobs;
    RS_REAL sw_in = f.sw, lw_in = f.lw;
    if (sky_on) {
      /* the reference runs this between PrecipitationToStorage and BalanceModelOneStep
       * (Simulation.f90:151-162); the two do not share data, so the order is free.  (The flavour's own
       * sky_view_radiation and, below, output_row + store_point spelled out here: with the conversions to double
       * or SaveOutput as one function in this text, step_kernel_coupled's machine code changed -
       * tools/compare_device_code.py) */
      if (!sky_view_radiation(ka->f.sun + (int64_t)(i - t0) * RS_SUN_COLS, sinlat, coslat, lonrad, coslon, sinlon, skyv,
                              ka->pp.albedo_surroundings,
                              ka->pp.horizons
                                  ? ka->pp.horizons + (ka->pp.horizon_index ? (int64_t)ka->pp.horizon_index[p] : p) *
                                                          (ka->pp.horizons_by_point ? 360 : 1)
                                  : nullptr,
                              ka->pp.horizons_by_point ? (int64_t)1 : np, sw_in, sw_dir, lw_in, lw_net))
        fail_at(i); /* the reference would `stop` the process here */
    }
#if RS_GEN_FP64_FEATURES
    if (ka->wb.sw_dir) { /* in-place input edits of the reference; a replay overwrites them */
      const int64_t woff = (int64_t)(i - t0) * ka->wb.t_stride + p;
      ka->wb.sw_dir[woff] = sw_dir;
      if (sky_on) {
        ka->wb.sw[woff] = sw_in;
        ka->wb.lw[woff] = lw_in;
      }
    }
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
    /* CheckEndCoupling + CouplingOperations2, src/Coupling.f90:98-141 */
    if (i < c.SimLen && q.on && i == q.ce && !q.failed) {
      if (q.iter == 0) q.tend1 = s.tsurf;
      coupling_control(q, s.tsurf);
      q.iter = q.iter + 1;
      if (s.failed) q.again = false; /* failed at this index: the loop exits, no rewind, not listed */
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
