/*
 * rs_kernels.hip — HIP kernels (gfx950) of the RoadSurf hot path.
 *
 * Mapping: ONE POINT PER LANE, persistent over a window of time steps.  A
 * 256-thread workgroup owns 256 consecutive points; lane l of a wavefront reads
 * forcing[t][p0 + l], so each field-step is one coalesced 512-B wave access,
 * and writes the six outputs the same way.  The carried state (SURVEY.md
 * Appendix B, ~30 doubles) is loaded from the SoA state block once per launch,
 * lives in VGPRs for the whole window and is stored back once.
 *
 * Two flavours of the same physics (rs_physics.hpp):
 *   step_kernel_reg<NL>  NLayers known at compile time: the ground temperature
 *                        profile is a fully unrolled register array.
 *   step_kernel_lds      any NLayers <= RS_MAX_LAYERS: the profile is staged in
 *                        LDS as [layer][lane] columns (conflict-free: lane l
 *                        touches 8-byte word l of a 2-KiB row).
 * Each comes in a LEAN variant (no observation forcing beyond index 1, no output
 * depth, no relaxation, no Tdew check: the BASELINE workload) and a FULL variant.
 * These, step_kernel_hybrid and the lock-step sky-view and coupling kernels
 * (step_kernel_sky*, step_kernel_cpl*) share one body, step_lanes.
 *
 * No MFMA: there is no contraction anywhere in this path.  The time loop is
 * sequential per point (explicit Euler in time), points are independent.
 */
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "rs_physics.hpp"
#include "rs_state.h"
#include "rs_synth.h"
#include "rs_kernels.h"

#ifndef RS_CPL_WAVES
#define RS_CPL_WAVES 2 /* waves per SIMD the general (per-lane time index) kernel is compiled for */
#endif
#ifndef RS_REGIME_WINDOW
#define RS_REGIME_WINDOW 30 /* indices at the end of a launch that define a point's regime
                               (rs_hip_recluster; 8 ... 90 measured equal) */
#endif

namespace rs {

constexpr int kBlock = RS_BLOCK;

/* Model constants: one RsConstants block per plan in HBM, reached through a pointer in the
 * kernel arguments and read as constant memory (address space 4): every access is a scalar
 * load through the scalar cache.  (A per-plan block, not a __constant__ table: the reference
 * driver calls runsimulation from as many threads as it likes,
 * examples/example1/src/roadrunner.cpp:490-497, so the number of live plans is unbounded.)
 * The time loop re-derives the pointer through an empty asm every iteration so that the
 * compiler cannot hoist ~220 uniform doubles (= 440 SGPRs, against 102 available) out of the
 * loop and then spill them into VGPR lanes; loaded at the point of use they cost one s_load
 * each and no live range. */
typedef RsConstantsDev __attribute__((address_space(4))) ConstsAS;
template <class Args>
__device__ __forceinline__ const ConstsAS &consts_of(Args a) {
  return *(const ConstsAS *)a->consts;
}

/* The upper NREG layers in registers, the rest in LDS columns: what lets the FULL feature set (more
 * live values than the LEAN one) keep four waves per SIMD without scratch spills.  Layer indices are
 * compile-time constants after unrolling, so the split costs no selects. */
template <int NL, int NREG>
struct HybridProfile {
  double v[NREG];
  double *col; /* &lds[threadIdx.x]; layer NREG + 1 + r is col[r * kBlock] */
  static constexpr bool kUnrolled = true; /* the layer count is a compile-time constant */
  __device__ __forceinline__ constexpr int nlayers() const { return NL; }
  __device__ __forceinline__ double get(int j) const { return j <= NREG ? v[j - 1] : col[(j - NREG - 1) * kBlock]; }
  __device__ __forceinline__ void set(int j, double x) {
    if (j <= NREG) v[j - 1] = x;
    else col[(j - NREG - 1) * kBlock] = x;
  }
  __device__ __forceinline__ void pin() {
#pragma unroll
    for (int j = 0; j < NREG; ++j) asm volatile("" : "+v"(v[j]));
  }
};

/* The kernel arguments are read through the kernarg segment pointer (constant
 * address space: scalar loads) and that pointer is laundered once per time
 * step.  Effect: the 17 stream pointers + strides are s_load-ed at their point
 * of use instead of living in ~45 SGPRs for the whole time loop (SGPR spills go
 * to VGPR lanes and every use of a spilled value costs a v_readlane). */
typedef const StepArgs __attribute__((address_space(4))) *KernArgs;

__device__ __forceinline__ KernArgs kernargs() {
  return (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
}

/* Addressing: `base` pointers below are wave-uniform (row pointer + first point
 * of the workgroup), `lane` is the 32-bit index of the point inside the
 * workgroup, so every access is global_load/store saddr + 32-bit voffset with no
 * 64-bit per-lane arithmetic. */
/* base[lane] as saddr + 32-bit voffset.  Instruction selection works a basic block at a time and
 * takes that form only when it sees the 32-bit lane offset being widened in the block of the
 * access; a `lane * 8` from the kernel's entry block arrives as a 64-bit register pair and costs a
 * 64-bit vector add per access.  LaneOff therefore forms the byte offset behind an asm barrier in
 * the block that uses it (one v_lshlrev per group of accesses). */
struct LaneOff {
  uint32_t b8;
  __device__ __forceinline__ explicit LaneOff(uint32_t lane) {
    asm volatile("v_lshlrev_b32 %0, 3, %1" : "=v"(b8) : "v"(lane));
  }
  template <class T>
  __device__ __forceinline__ T ld(const T *base) const {
    static_assert(sizeof(T) == 8 || sizeof(T) == 4, "");
    return *(const T *)((const char *)base + (sizeof(T) == 8 ? b8 : b8 >> 1));
  }
  template <class T>
  __device__ __forceinline__ void st(T *base, T v) const {
    static_assert(sizeof(T) == 8 || sizeof(T) == 4, "");
    *(T *)((char *)base + (sizeof(T) == 8 ? b8 : b8 >> 1)) = v;
  }
};

/* A32 windows (the launcher's choice: every stream of the window spans < 4 GiB): the whole offset
 * of (row, point) fits the 32-bit vector offset, so the stream pointers are used as they come out
 * of the kernel arguments - no 64-bit scalar add per stream and step (2 x 13 streams), one scalar
 * multiply-add for the row and one vector add.  `slot` = row * t_stride + first point of the
 * workgroup (uniform, < 2^29). */
struct WinOff {
  uint32_t b8;
  __device__ __forceinline__ WinOff(uint32_t lane, uint32_t slot) {
    const uint32_t sb = slot << 3;
    asm volatile("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(b8) : "v"(lane), "s"(sb));
  }
  template <class T>
  __device__ __forceinline__ T ld(const T *base) const {
    static_assert(sizeof(T) == 8 || sizeof(T) == 4, "");
    return *(const T *)((const char *)base + (sizeof(T) == 8 ? b8 : b8 >> 1));
  }
  template <class T>
  __device__ __forceinline__ void st(T *base, T v) const {
    static_assert(sizeof(T) == 8 || sizeof(T) == 4, "");
    *(T *)((char *)base + (sizeof(T) == 8 ? b8 : b8 >> 1)) = v;
  }
};

template <bool FULL, bool A32 = false>
__device__ __forceinline__ Forcing load_forcing(KernArgs ka, int64_t row0, uint32_t lane,
                                                int32_t k) {
  Forcing o;
  if (A32) {
    const WinOff L(lane, (uint32_t)k * (uint32_t)ka->f.t_stride + (uint32_t)row0);
    o.tair = L.ld(ka->f.tair);
    o.vz = L.ld(ka->f.vz);
    o.rhz = L.ld(ka->f.rhz);
    o.prec = L.ld(ka->f.prec);
    o.sw = L.ld(ka->f.sw);
    o.lw = L.ld(ka->f.lw);
    o.phase = L.ld(ka->f.precphase);
    if (ka->f.hour_pstride) o.hour = L.ld(ka->f.hour);
    else o.hour = ka->f.hour[k];
    if (FULL) {
      o.tdew = ka->f.tdew ? L.ld(ka->f.tdew) : 0.0;
      o.tsurfobs = ka->f.tsurfobs ? L.ld(ka->f.tsurfobs) : R4(-9999.9);
      o.depth = ka->f.depth ? L.ld(ka->f.depth) : R4(-9999.9);
    } else {
      o.tdew = 0.0;
      o.tsurfobs = R4(-9999.9);
      o.depth = R4(-9999.9);
    }
    return o;
  }
  const int64_t row = (int64_t)k * ka->f.t_stride + row0;
  const LaneOff L(lane);
  o.tair = L.ld(ka->f.tair + row);
  o.vz = L.ld(ka->f.vz + row);
  o.rhz = L.ld(ka->f.rhz + row);
  o.prec = L.ld(ka->f.prec + row);
  o.sw = L.ld(ka->f.sw + row);
  o.lw = L.ld(ka->f.lw + row);
  o.phase = L.ld(ka->f.precphase + row);
  if (ka->f.hour_pstride) o.hour = L.ld(ka->f.hour + row);
  else o.hour = ka->f.hour[k];
  if (FULL) {
    o.tdew = ka->f.tdew ? L.ld(ka->f.tdew + row) : 0.0;
    o.tsurfobs = ka->f.tsurfobs ? L.ld(ka->f.tsurfobs + row) : R4(-9999.9);
    o.depth = ka->f.depth ? L.ld(ka->f.depth + row) : R4(-9999.9);
  } else {
    o.tdew = 0.0;
    o.tsurfobs = R4(-9999.9);
    o.depth = R4(-9999.9);
  }
  return o;
}

template <bool SCATTER = false, bool A32 = false>
__device__ __forceinline__ void store_outputs(KernArgs ka, int64_t row, int64_t row0, uint32_t lane,
                                              const Scalars &s, bool valid) {
  const double miss = R4(-9999.0); /* src/Initialization.f90:404-411 */
  if (A32 && !SCATTER) {
    const WinOff L(lane, (uint32_t)row + (uint32_t)row0);
    L.st(ka->o.tsurf, valid ? s.tsurf : miss);
    L.st(ka->o.snow, valid ? s.snow : miss);
    L.st(ka->o.water, valid ? s.wat : miss);
    L.st(ka->o.ice, valid ? s.ice : miss);
    L.st(ka->o.deposit, valid ? s.dep : miss);
    L.st(ka->o.ice2, valid ? s.ice2 : miss);
    return;
  }
  if (SCATTER && ka->out_index) { /* column = out_index[slot]: point order whatever the plan order */
    row += (int64_t)ka->out_index[row0 + lane];
    ka->o.tsurf[row] = valid ? s.tsurf : miss;
    ka->o.snow[row] = valid ? s.snow : miss;
    ka->o.water[row] = valid ? s.wat : miss;
    ka->o.ice[row] = valid ? s.ice : miss;
    ka->o.deposit[row] = valid ? s.dep : miss;
    ka->o.ice2[row] = valid ? s.ice2 : miss;
    return;
  }
  row += row0;
  const LaneOff L(lane);
  L.st(ka->o.tsurf + row, valid ? s.tsurf : miss);
  L.st(ka->o.snow + row, valid ? s.snow : miss);
  L.st(ka->o.water + row, valid ? s.wat : miss);
  L.st(ka->o.ice + row, valid ? s.ice : miss);
  L.st(ka->o.deposit + row, valid ? s.dep : miss);
  L.st(ka->o.ice2 + row, valid ? s.ice2 : miss);
}

/* Per-lane gather of the forcing of absolute index i (window row i - t0). */
__device__ __forceinline__ Forcing gather_forcing(KernArgs ka, int64_t p, int32_t i, int32_t t0) {
  Forcing o;
  const int64_t off = (int64_t)(i - t0) * ka->f.t_stride + p;
  o.tair = ka->f.tair[off]; o.vz = ka->f.vz[off]; o.rhz = ka->f.rhz[off];
  o.prec = ka->f.prec[off]; o.sw = ka->f.sw[off]; o.lw = ka->f.lw[off];
  o.phase = ka->f.precphase[off];
  o.hour = ka->f.hour_pstride ? ka->f.hour[off] : ka->f.hour[i - t0];
  o.tdew = ka->f.tdew ? ka->f.tdew[off] : 0.0;
  o.tsurfobs = ka->f.tsurfobs ? ka->f.tsurfobs[off] : R4(-9999.9);
  o.depth = ka->f.depth ? ka->f.depth[off] : R4(-9999.9);
  return o;
}

/* ... and of the two streams sky view adds */
__device__ __forceinline__ void gather_sky(KernArgs ka, int64_t p, int32_t i, int32_t t0, double &sw_dir, double &lw_net) {
  const int64_t off = (int64_t)(i - t0) * ka->f.t_stride + p;
  sw_dir = ka->f.sw_dir[off];
  lw_net = ka->f.lw_net[off];
}

/* SaveOutput for a lane with its own time index: the point's column of the index's row */
__device__ __forceinline__ void store_point(KernArgs ka, int64_t row, int64_t p, const Scalars &s, bool valid) {
  store_outputs<true>(ka, row, p, 0u, s, valid);
}

/* Diagnostics (rs_hip_set_diagnostics; ROADSURF_HIP_DIAGNOSTICS=1 on the host paths): what CalcBLCondAndLE prints
 * besides computing - "ERROR : UStar negative" inside the loop and "Max number of BLCond iterations" behind it
 * (src/BoundaryLayer.f90:69-74,98-101).  The loop of the step about to be taken is run once more, out of line, with
 * IEEE division and square root (the bits the bare sequences return, rs_math.hpp), and the first occurrence and the
 * count of either message go to the plan's diagnostics block (rs_state.h RsDiagRow; one lane owns a point: plain
 * read-modify-write).  Only the DIAG instances of the one-point-per-lane kernels with the profile in LDS call it
 * (step_kernel_lds<., true>, step_kernel_sky<true>, step_kernel_coupled<true>) - the launchers send a plan with
 * diagnostics there - so no other kernel carries the call. */
__device__ __attribute__((noinline)) void bl_diagnose(const ConstsAS *cp, const uint64_t *expT, const double *logT,
                                                      const double *K, double tsurf, double tair, double vz,
                                                      double rhz, int32_t hour, int32_t i, double *dg, int64_t np,
                                                      int64_t p) {
  const ConstsAS &c = *cp;
  MathTab mt;
  mt.expT = expT;
  mt.logT = logT;
  mt.K = K;
  mt.S = (rs::MathCoef)rs::c_gl_scoef;
  asm volatile("" : "+s"(mt.S));
  /* SetDayDependendVariables' calm limit (fluxes_pre) */
  const double calmN = c.CalmLimNgt, calmD = c.CalmLimDay;
  const bool night = ((double)hour >= c.NightOn) || ((double)hour <= c.NightOff);
  const double calm = night ? calmN : calmD;
  if (vz < calm) vz = calm;
  BlInv v;
  BlVar x;
  BlAux a;
  bl_setup<true>(c, tsurf, tair, vz, v, x, a);
  const double stab_num = bl_stab_num(c);
  double old = 0.0;
  int j = 1;
  for (; j <= RS_BL_MAXIT; ++j) {
    old = x.BLCond;
    if (rs_dvb<true>(v.vkvz, c.logUstar + x.PSIM) < 0.0) { /* :69-73, with BLCond as the pass before left it */
      const double n = dg[(int64_t)RS_DG_USTAR_N * np + p];
      if (n == 0.0) {
        dg[(int64_t)RS_DG_USTAR_I * np + p] = (double)i;
        dg[(int64_t)RS_DG_USTAR_TAIR * np + p] = tair;
        dg[(int64_t)RS_DG_USTAR_VZ * np + p] = vz;
        dg[(int64_t)RS_DG_USTAR_RHZ * np + p] = rhz;
        dg[(int64_t)RS_DG_USTAR_BL * np + p] = old;
        dg[(int64_t)RS_DG_USTAR_TSURF * np + p] = tsurf;
      }
      dg[(int64_t)RS_DG_USTAR_N * np + p] = n + 1.0;
    }
    if (bl_iteration<true>(c, mt, v, x, j, stab_num)) break;
  }
  if ((fabs(x.BLCond - old) > 10 * R4(0.001)) && (j >= 5)) { /* :98-101; j = MaxIter + 1 behind a DO loop that ran out */
    const double n = dg[(int64_t)RS_DG_MAXIT_N * np + p];
    if (n == 0.0) {
      dg[(int64_t)RS_DG_MAXIT_I * np + p] = (double)i;
      dg[(int64_t)RS_DG_MAXIT_J * np + p] = (double)j;
      dg[(int64_t)RS_DG_MAXIT_OLD * np + p] = old;
      dg[(int64_t)RS_DG_MAXIT_BL * np + p] = x.BLCond;
    }
    dg[(int64_t)RS_DG_MAXIT_N * np + p] = n + 1.0;
  }
}

/* the profiles, state-block access, coupling, the general time loop and init_kernel: one text for both flavours */
#include "rs_general_body.inc"

/* The time loop of runsimulation (examples/example1/src/Simulation.f90:57-115)
 * for one point over absolute indices [t0, t0+nsteps). */
/* SKY: sky view / local horizons (src/ModRadiation.f90, examples/example1/src/Simulation.f90:
 * 151-162) in the lock-step loop; with coupling the general kernel below does it. */
/* CPL: coupling in lock step (src/Coupling.f90), for everything except the replays themselves:
 * the state is saved at the window start (:172-210), the window's first pass runs in the coupling
 * phase, Coupling_control decides at the window end (:98-141,292-481) - a point that has to replay
 * PARKS there (start_coupling_again set, RS_ST_CPL_RESUME = window end + 1) and takes no further
 * step in lock step until the replay rounds (step_kernel_coupled over the compacted list of parked
 * points, rs_hip_cpl_replay) have cleared it - and behind the window the radiation corrections
 * decay (:80-88).  A lane steps index i only if i == its RS_ST_CPL_RESUME, so launches may
 * overlap in time: points that are ahead wait for the others. */
/* REPLAY (with CPL): one replay ROUND in lock step, for the points of the compacted list that asked
 * for another replay (start_coupling_again): the launch covers [first window start, last window
 * end + 1]; a lane waits for its window start, rewinds there - CheckValues of the index behind its
 * window end, as the reference's loop does before CouplingOperations1 takes it back
 * (examples/example1/src/Simulation.f90:62-71), then uploadDataForCoupling (src/Coupling.f90:
 * 213-255) and the radiation coefficient (:61-78) -, runs its window in the coupling phase and lets
 * Coupling_control decide again at the end.  `point` is the lane's slot: the list breaks the tie
 * between thread and point, so accesses are base[point] with the row base on the scalar unit. */
template <bool FULL, class Prof, bool SKY = false, bool SCORE = true, bool CPL = false,
          bool REPLAY = false, bool A32 = false, bool DIAG = false>
__device__ __forceinline__ void time_loop(const MathTab &mt, Prof &T, Scalars &s, int32_t &score,
                                          uint32_t point = 0u) {
  static_assert(!A32 || (!SKY && !CPL), "32-bit window offsets: the plain lock-step kernels only");
  static_assert(FULL || !SKY, "sky view belongs to the FULL feature set");
  static_assert(FULL || !CPL, "coupling belongs to the FULL feature set");
  static_assert(CPL || !REPLAY, "replays belong to coupling");
  KernArgs ka = kernargs();
  const uint32_t lane = REPLAY ? point : threadIdx.x;
  const int64_t row0 = REPLAY ? 0 : (int64_t)blockIdx.x * kBlock; /* first point of this workgroup */
  const int32_t nsteps = ka->nsteps, t0 = ka->t0;
  const double tbot = (ka->pp.tbottom + row0)[lane];
  SkyPoint sky;
  if (SKY) sky = sky_point(ka, row0, lane);
  const bool sky_on = sky.on;
  int32_t initlen = 0;
  bool relax = false;
  /* relaxation: the three differences target - anchor are what the loop carries (the targets are read again at
   * the one index that sets the anchors, the anchors go to the state block there and then) */
  double relax_dt = 0, relax_dv = 0, relax_dr = 0;
  if (FULL) {
    initlen = ka->pp.initlen ? (ka->pp.initlen + row0)[lane] : 0;
    if (consts_of(ka).use_relaxation && ka->pp.tair_relax) {
      double tairR, vzR, rhR;
      relax_targets(ka, row0, lane, tairR, vzR, rhR);
      relax = !(tairR < R4(-100.0) || tairR > R4(100.0) || vzR < R4(0.0) || vzR > R4(100.0) ||
                rhR < R4(0.0) || rhR > 110); /* (relax_valid, spelled out: see rs_general_body.inc) */
      relax_dt = tairR - s.tair_end;
      relax_dv = vzR - s.vz_end;
      relax_dr = rhR - s.rh_end;
    }
  }

  /* settings%simulation_failed (src/InputOutput.f90:66): sticky; the state block keeps the index
   * it was raised at (rs_hip_first_failed_index) */
  auto fail_at = [&](int32_t idx) {
    s.failed = true;
    ka->state[(int64_t)RS_ST_FAILED * ka->np_pad + row0 + lane] = (double)idx;
  };
  /* coupling, lock-step part: what a lane needs every step stays in registers, the rest of
   * CouplingVariables lives in the state block and is touched at the two events only */
  CplWindow cw;
  if (CPL) cpl_window(ka, consts_of(ka), row0, lane, cw);
  const bool cpl_on = cw.on;
  const int32_t cpl_cs = cw.cs, cpl_ce = cw.ce;
  bool parked = false;
  int32_t next_i = t0;
  double cpl_lastobs = 0.0, cpl_swcorr = 0.0, cpl_lwcorr = 0.0;
  if (CPL) {
    double *st = ka->state;
    const int64_t np = ka->np_pad, p = row0 + lane;
    cpl_lastobs = st[(int64_t)RS_ST_CPL_LASTOBS * np + p];
    cpl_swcorr = st[(int64_t)RS_ST_CPL_SWCORR * np + p];
    cpl_lwcorr = st[(int64_t)RS_ST_CPL_LWCORR * np + p];
    parked = (((int32_t)st[(int64_t)RS_ST_CPL_FLAGS * np + p]) & 1) != 0;
    next_i = (int32_t)st[(int64_t)RS_ST_CPL_RESUME * np + p];
    if (REPLAY) { /* a listed point: parked behind its window, wanting it again */
      parked = false;
      next_i = cpl_cs;
    }
  }
  /* REPLAY: SWRadCof / LWRadCof of the window being replayed, and "TmpNw is the stale profile" */
  double r_swcof = R4(1.0), r_lwcof = R4(1.0);
  bool stale_now = false;
  /* A failed point's rows read -9999.0 from behind the index that failed it (the reference's loop has
   * exited: src/Initialization.f90:404-411).  Without coupling they are written HERE - the rest of the
   * window when the failure is detected, the whole window for a point that arrives failed - and not by
   * a second store site in the time loop: the compiler merges two store sites of a loop into one and
   * pays for it with ~25 register moves on every step of every lane. */
  auto blank_rows = [&](int32_t i_from) {
    for (int32_t ii = i_from; ii < t0 + nsteps; ++ii) {
      int64_t r;
      if (output_row<false>(ka, ii, r)) store_outputs<false, false>(ka, r, row0, lane, s, false);
    }
  };
  if (!CPL && s.failed) blank_rows(t0);
  Forcing nxt = load_forcing<FULL, A32>(ka, row0, lane, 0);
  for (int32_t kv = 0; kv < nsteps; ++kv) {
    asm volatile("" : "+s"(ka));
    const ConstsAS &c = consts_of(ka);
    /* the loop counter is wave-uniform, but lanes that `continue` (failed, parked) make the
     * compiler keep it in a vector register, and with it every row offset: 64-bit vector
     * multiplies and two 64-bit vector adds per load and store.  Read back as a scalar, the row
     * arithmetic runs on the scalar unit and the accesses are saddr + 32-bit lane offset */
    const int32_t k = __builtin_amdgcn_readfirstlane(kv);
    const int32_t i = t0 + k;
    const Forcing f = nxt;
    int64_t orow = 0;
    const bool owrite = output_row<true>(ka, i, orow);

    if (CPL && (parked || i != next_i)) { /* parked behind its window, or ahead of this launch */
      if (k + 1 < nsteps) nxt = load_forcing<FULL, A32>(ka, row0, lane, k + 1);
      continue;
    }
    if (CPL) next_i = i + 1;
    if (s.failed) { /* loop has exited in the reference: outputs stay -9999.0 */
      /* (no forcing is fetched for a failed point: it never steps again, and a second fetch site would
       * be merged with the one in the middle of the step at the price of moves at the loop's end) */
      /* a point that fails in the middle of a replay keeps, up to its window end, what the earlier
       * passes saved there (src/InputOutput.f90:151-165 only ever overwrites) */
      if (CPL && owrite && (!REPLAY || i > cpl_ce)) store_outputs<CPL, A32>(ka, orow, row0, lane, s, false);
      continue;
    }
    double tair = f.tair, vz = f.vz, rhz = f.rhz;
    /* TmpNw(1:2) as CalcHCapHCond will see them (src/BalanceModel.f90:215): the values the last step
     * left - Tmp = TmpNw at its end (:60-62) - whatever observation forcing does to Tmp(1:2) below
     * (src/InputOutput.f90:122-124 does not touch TmpNw) */
    s.tnw1 = T.get(1);
    s.tnw2 = T.get(2);
    /* src/Initialization.f90:121-123: VZ(1) is raised to 0.4 in the input array */
    if (i == 1 && vz < R4(0.4)) vz = R4(0.4);
    const double prec_ts = RS_DIVC(f.prec, 3600.0, r_3600) * c.DTSecs; /* src/InputOutput.f90:111,186 */

    double sw_dir = 0.0, lw_net = 0.0;
    if (SKY) {
      const int64_t row = (int64_t)k * ka->f.t_stride + row0;
      const LaneOff L(lane);
      sw_dir = L.ld(ka->f.sw_dir + row);
      lw_net = L.ld(ka->f.lw_net + row);
    }
    CouplingInputs cp;
    if (i < c.SimLen) {
      if (REPLAY && i == cpl_cs) {
        /* the rewind: the reference's loop is at the index behind the window end when
         * CouplingOperations1 takes it back, and that is the index CheckValues has just seen -
         * with the surface temperature of the end of the window */
        const Forcing g = gather_forcing(ka, row0 + lane, cpl_ce + 1, t0);
        if (check_values(c, g, s.tsurf, FULL && ka->f.tdew != nullptr)) fail_at(cpl_ce + 1);
      } else {
        Forcing chk = f;
        chk.vz = vz;
        if (check_values(c, chk, s.tsurf, FULL && ka->f.tdew != nullptr)) fail_at(i);
      }
      if (SKY) {
        if (REPLAY && i == cpl_cs) {
          /* the rewind: CheckValues has just seen the index behind the window end (above) */
          if (sky_on) {
            const int64_t off = (int64_t)(cpl_ce + 1 - t0) * ka->f.t_stride + row0 + lane;
            if (sky_limits_bad(ka->f.sw_dir[off], ka->f.lw_net[off])) fail_at(cpl_ce + 1);
          }
        } else if (sky_on && sky_limits_bad(sw_dir, lw_net))
          fail_at(i);
        sw_dir = sky_clamp_direct(sw_dir, f.sw);
      }
      if (CPL && cpl_on) {
        /* CouplingOperations1, src/Coupling.f90:10-96, first pass of the window */
        cp.in_phase = (i >= cpl_cs && i <= cpl_ce);
        /* inCouplingPhase is set from the loop index BEFORE a rewind takes it back (:22-27 against
         * :61-66): the step at the window start of a replay runs outside the coupling phase */
        if (REPLAY && i == cpl_cs) cp.in_phase = false;
        if (REPLAY && i == cpl_cs) {
          double *st = ka->state;
          const int64_t np = ka->np_pad, p = row0 + lane;
          cpl_restore_surface<true>(st, np, p, s);
          const int N = T.nlayers();
          for (int j = 1; j <= N; ++j) {
            st[(int64_t)(RS_ST_CPL_STALE_TMP0 + j - 1) * np + p] = T.get(j);
            T.set(j, st[(int64_t)(RS_ST_CPL_SAVE_TMP0 + j - 1) * np + p]);
          }
          stale_now = true;
          cpl_rewind_coefs(st[(int64_t)RS_ST_CPL_RADCOEFF * np + p], f.sw, f.lw, SKY && sky_on, r_swcof, r_lwcof);
          st[(int64_t)RS_ST_CPL_SWCOF * np + p] = r_swcof; /* Coupling_control reads them at the end */
          st[(int64_t)RS_ST_CPL_LWCOF * np + p] = r_lwcof;
        }
        if (!REPLAY && i == cpl_cs) { /* Coupling_iterations == 0 here */
          double *st = ka->state;
          const int64_t np = ka->np_pad, p = row0 + lane;
          cpl_save_surface(st, np, p, s);
          const int N = T.nlayers();
          for (int j = 1; j <= N; ++j) st[(int64_t)(RS_ST_CPL_SAVE_TMP0 + j - 1) * np + p] = T.get(j);
          /* SW/LWRadCof = 1, SW/LW_correction = 0: what the registers hold before the window end */
        }
        if (i > cpl_ce) cpl_decayed_coefs(c, mt, i, cpl_ce, cpl_swcorr, cpl_lwcorr, cp.sw_cof, cp.lw_cof);
        if (REPLAY && i >= cpl_cs && i <= cpl_ce) {
          cp.sw_cof = r_swcof;
          cp.lw_cof = r_lwcof;
        }
        if (cp.in_phase) snow_ice_check(c, cpl_lastobs, s);
      }
      if (FULL) {
        /* (obs_forced, spelled out: see rs_general_body.inc) */
        if ((i <= initlen || c.force_tsurf) && f.tsurfobs > R4(-100.0) &&
            (!CPL || !cpl_on || i < cpl_cs)) {
          T.set(1, f.tsurfobs);
          T.set(2, f.tsurfobs);
          const double depth = (c.tsurfOutputDepth >= R4(0.0)) ? c.tsurfOutputDepth : f.depth;
          s.tsurf = surface_temperature(c, T, tbot, depth);
        }
        if (relax) {
          if (i == initlen) { /* the anchors: once per point */
            double tairR, vzR, rhR;
            relax_targets(ka, row0, lane, tairR, vzR, rhR);
            relax_dt = tairR - tair;
            relax_dv = vzR - vz;
            relax_dr = rhR - rhz;
            double *st = ka->state;
            const int64_t np = ka->np_pad, p = row0 + lane;
            st[(int64_t)RS_ST_TAIR_END * np + p] = tair;
            st[(int64_t)RS_ST_VZ_END * np + p] = vz;
            st[(int64_t)RS_ST_RH_END * np + p] = rhz;
          }
          if (i > initlen) relax_apply(relax_factor(c, mt, i, initlen), relax_dt, relax_dv, relax_dr, tair, vz, rhz);
        }
      }
    } else {
      /* lastValues, src/InputOutput.f90:169-198: no checks, no obs forcing, no
       * relaxation; the pre-step surface temperature uses depth(SimLen) only */
      if (FULL) s.tsurf = surface_temperature(c, T, tbot, f.depth);
      if (CPL && cpl_on) cpl_last_values(c, mt, cw, cpl_swcorr, cpl_lwcorr, ka->state, ka->np_pad, row0 + lane, cp);
    }
    if (CPL) cp.last_tsurf_obs = cpl_lastobs;
    double sw_in = f.sw, lw_in = f.lw;
    if (SKY && sky_on) {
      /* the reference runs this between PrecipitationToStorage and BalanceModelOneStep
       * (Simulation.f90:151-162); the two do not share data, so the order is free */
      int64_t hstride;
      const double *hrow = horizon_row(ka, sky.hcol, hstride);
      if (!sky_view_radiation(ka->f.sun + (int64_t)k * RS_SUN_COLS, sky.sinlat, sky.coslat, sky.lonrad, sky.coslon,
                              sky.sinlon, sky.skyv, ka->pp.albedo_surroundings, hrow, hstride, sw_in, sw_dir, lw_in, lw_net))
        fail_at(i); /* the reference would `stop` the process here */
    }
    if (SKY) sky_write_back(ka, k, row0, sky_on, sw_dir, sw_in, lw_in, [&](double *base, double v) { base[lane] = v; });
    if (DIAG) /* (instances of their own, step_kernel_lds<., true> and step_kernel_sky<true>: see bl_diagnose) */
      bl_diagnose(&c, mt.expT, mt.logT, mt.K, s.tsurf, tair, vz, rhz, f.hour, i, ka->diag, ka->np_pad, row0 + lane);
    const Fluxes fx =
        model_step_fluxes<SCORE>(c, mt, s, tair, vz, rhz, prec_ts, sw_in, lw_in, f.phase, f.hour, cp);
    /* scheduling hint (bl_score_key): extra passes of this launch; bit 30 of the counter = the
     * point was in the unstable regime at some index of the launch's last RS_REGIME_WINDOW */
    if (SCORE) {
      score += (fx.trips & 63) - 5;
      if ((fx.trips & 64) && k >= nsteps - RS_REGIME_WINDOW) score |= 1 << 30;
    }
    /* next index's forcing: issued here, half a step before its first use, so the
     * HBM latency hides under the ground/storage half without holding 14 VGPRs
     * across the boundary-layer iteration */
    if (k + 1 < nsteps) nxt = load_forcing<FULL, A32>(ka, row0, lane, k + 1);
    if (REPLAY) {
      /* first step after the restore: CalcHCapHCond sees the pre-restore TmpNw in every layer
       * (observation forcing cannot follow a restore, so layers 1-2 are stale too) */
      const GlobalProfile Tstale{ka->state + (int64_t)RS_ST_CPL_STALE_TMP0 * ka->np_pad + row0 + lane,
                                 ka->np_pad};
      model_step_ground<Prof, GlobalProfile>(c, s, T, tbot, tair, fx, f.depth, cp,
                                             stale_now ? &Tstale : nullptr);
      stale_now = false;
    } else {
      model_step_ground<Prof, Prof, FULL>(c, s, T, tbot, tair, fx, f.depth, cp);
    }
    if (owrite) store_outputs<CPL, A32>(ka, orow, row0, lane, s, true);
    if (!CPL && s.failed) blank_rows(i + 1); /* failed at this index: its own row is saved, the rest is not */
    if (CPL && cpl_on && i < c.SimLen && i == cpl_ce)
      cpl_window_end(ka->state, ka->np_pad, row0 + lane, cw, s, cpl_swcorr, cpl_lwcorr, cpl_lastobs, parked);
  }
  if (CPL) ka->state[(int64_t)RS_ST_CPL_RESUME * ka->np_pad + row0 + lane] = (double)next_i;
}

/* RS_ST_BLSCORE from the loop's counter: bits 0-18 extra passes (saturating), bit 19 cover,
 * bit 20 regime (the counter itself carries the regime flag in bit 30).
 * Sorted (descending: expensive first, rs_cluster.hip) the unstable-regime points come first,
 * by the passes they needed, then the stable-regime points, whose waves never enter the log/sqrt
 * branch (tools/bl_persistence.py). */
__device__ __forceinline__ double bl_score_key(int32_t score, const Scalars &s) {
  const int32_t extra = score & 0x3fffffff;
  const int32_t lo = extra > 0x7ffff ? 0x7ffff : extra;
  /* bit 20: something lies on the road (the storage and melting branches are skipped by a
   * wavefront whose lanes are all bare) */
  const int32_t covered = (s.wat > 0.0 || s.snow > 0.0 || s.ice > 0.0 || s.ice2 > 0.0 || s.dep > 0.0) ? 1 : 0;
  return (double)(lo | (covered << 19) | (((score >> 30) & 1) << 20));
}

/* The profile of this lane in a one-point-per-lane kernel; `lds`: the kernel's LDS columns of the profile,
 * [layer][lane] (none for RegProfile). */
template <int NL>
__device__ __forceinline__ void lane_profile(RegProfile<NL> &, double *, const StepArgs &) {}
template <int NL, int NREG>
__device__ __forceinline__ void lane_profile(HybridProfile<NL, NREG> &T, double *lds, const StepArgs &) {
  T.col = lds + threadIdx.x;
}
__device__ __forceinline__ void lane_profile(LdsProfile &T, double *lds, const StepArgs &a) {
  T.col = lds + threadIdx.x;
  T.n = consts_of(&a).NLayers;
}

/* One point per lane, lock step: the body of step_kernel_reg, _hybrid, _lds, _sky, _sky_h, _cpl, _cpl_h and
 * _cpl_replay_h (step_kernel_cpl_replay keeps a copy of its own: see there).  The workgroup fills the math tables;
 * a lane without a point leaves (no barriers below: each lane owns its column of the profile); the lane's state is
 * loaded, run through time_loop and stored back, and with SCORE its history score goes beside it.  The entry points
 * differ only in the profile (Prof, set up by lane_profile), time_loop's flags and their launch bounds.  They
 * declare the LDS themselves and pass it down (a __shared__ in a __device__ function goes through the module-LDS
 * lowering and can move): math_lds, and prof_lds for the columns of HybridProfile / LdsProfile.
 * REPLAY: the lane's point is its entry of the compacted list cpl_list, run at raised priority with cpl_prio, and
 * replays its window up to cpl_inner times in this launch, as long as its Coupling_control asks for another
 * (start_coupling_again, bit 0 of the flags it has just stored): the secant iteration of src/Coupling.f90:363-449
 * is per point - only the launches were sequential.  The state goes through the state block between two replays
 * exactly as it does between two rounds. */
template <class Prof, bool FULL, bool SKY = false, bool SCORE = true, bool CPL = false, bool REPLAY = false,
          bool A32 = false, bool DIAG = false>
__device__ __forceinline__ void step_lanes(const StepArgs &a, double *math_lds, double *prof_lds) {
  const MathTab mt = fill_math_tables(math_lds);
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= (REPLAY ? (int64_t)a.cpl_nlist : a.npoints)) return;
  const int64_t p = REPLAY ? (int64_t)a.cpl_list[g] : g;
  if (REPLAY && a.cpl_prio) __builtin_amdgcn_s_setprio(2);
  Prof T;
  lane_profile(T, prof_lds, a);
  Scalars s;
  int32_t score = 0;
#ifdef RS_WAVE_TIMING /* tools/wave_times.py: when each wavefront of step_kernel_reg<15, false> starts and ends (100 MHz ticks) */
  constexpr bool WT = !FULL && std::is_same<Prof, RegProfile<15>>::value;
  const uint64_t wt0 = WT ? __builtin_amdgcn_s_memrealtime() : 0;
#endif
  for (int32_t rnd = 0;; ++rnd) {
    load_state<FULL>(a.state, a.np_pad, p, T, s);
    time_loop<FULL, Prof, SKY, SCORE, CPL, REPLAY, A32, DIAG>(mt, T, s, score, REPLAY ? (uint32_t)p : 0u);
    store_state<FULL>(a.state, a.np_pad, p, T, s);
    if (!REPLAY || rnd + 1 >= a.cpl_inner) break;
    if ((((int32_t)a.state[(int64_t)RS_ST_CPL_FLAGS * a.np_pad + p]) & 1) == 0) break;
  }
  if (SCORE) a.state[(int64_t)RS_ST_BLSCORE * a.np_pad + p] = bl_score_key(score, s);
#ifdef RS_WAVE_TIMING
  if (WT) {
    a.state[(int64_t)RS_ST_VZ_END * a.np_pad + p] = (double)(wt0 & 0xffffffffffffull);
    a.state[(int64_t)RS_ST_RH_END * a.np_pad + p] = (double)(__builtin_amdgcn_s_memrealtime() & 0xffffffffffffull);
  }
#endif
}

/* (waves per SIMD: LEAN four, FULL three - measured, rs_step_select.hpp; the choice was a digit of the variant until
 * round 6) */
template <int NL, bool FULL, bool SCORE = true, bool A32 = false>
__global__ void __launch_bounds__(kBlock, FULL ? 3 : 4) step_kernel_reg(const StepArgs a) {
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  step_lanes<RegProfile<NL>, FULL, false, SCORE, false, false, A32>(a, math_lds, nullptr);
}

/* FULL feature set, NLayers = 15, four waves per SIMD: layers 1..RS_HYBRID_REG in registers, the
 * rest in LDS (HybridProfile). */
#ifndef RS_HYBRID_REG
#define RS_HYBRID_REG 7
#endif
template <bool SCORE, bool A32>
__global__ void __launch_bounds__(kBlock, 4) step_kernel_hybrid(const StepArgs a) {
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  __shared__ double prof_lds[(15 - RS_HYBRID_REG) * kBlock];
  step_lanes<HybridProfile<15, RS_HYBRID_REG>, true, false, SCORE, false, false, A32>(a, math_lds, prof_lds);
}

/* DIAG (here, step_kernel_sky and step_kernel_coupled): the instance a plan with diagnostics runs (bl_diagnose): a
 * call in the middle of the step costs the kernel around it 11 % even when it is not taken (measured, FULL: 1.70e10
 * -> 1.52e10, tools/experiments/r6_diag_hook_cost.sh), so the regular instances do not contain it */
template <bool FULL, bool DIAG = false>
__global__ void __launch_bounds__(kBlock, 4) step_kernel_lds(const StepArgs a) {
  extern __shared__ double lds[]; /* [NLayers][kBlock] */
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  step_lanes<LdsProfile, FULL, false, true, false, false, false, DIAG>(a, math_lds, lds);
}

/* ---- two wavefronts per 64 points: the flavour for small shards --------------------------------
 * A launch of one point per lane needs ~260 000 points to put four wavefronts on every SIMD; the
 * per-GPU shard of BASELINE config 4 (1 M points over 8 GPUs) has 125 000: under two waves per
 * SIMD, each of which must issue its ~2 300 instructions per time step one after the other, with
 * nothing to hide its waits behind.  Here a workgroup is TWO wavefronts that share 64 points:
 *   wave 0, "surface": everything of a time step that forms the serial chain - forcing, checks,
 *           precipitation, boundary layer, radiation, layers 1-2, melting, storages, outputs;
 *   wave 1, "ground":  layers 3..N of the explicit profile update (src/BalanceModel.f90:112-128),
 *           which only read the OLD temperatures of their neighbours.
 * They meet once per time step: the surface wave publishes its new Tmp(2), the ground wave its
 * new Tmp(3) (two LDS words per point, double-buffered, one s_barrier).  The serial chain of a
 * step shrinks from ~1 460 to ~1 020 vector instructions and the shard occupies twice as many
 * wave slots.  Same arithmetic in the same order per point: same bits (layer_step is the one
 * function both flavours call).  LEAN feature set, NLayers = 15, 32-bit window offsets. */
/* what a step needs of its forcing alone (ForcingPrep), [value][lane]: eight values, nine with the FULL feature set
 * (one more each where the air's vapour pressure is mailed: -DRS_NO_EAIR_SURFACE, rs_physics.hpp) */
#ifdef RS_EAIR_SURFACE
enum { PR_TAIR = 0, PR_VZ, PR_RHZ, PR_RAIN, PR_SNOW, PR_AVC, PR_SW, PR_LW, PR_OBS, PR_LEAN = PR_OBS, PR_FULL = PR_OBS + 1 };
#else
enum { PR_TAIR = 0, PR_VZ, PR_RHZ, PR_RAIN, PR_SNOW, PR_AVC, PR_EAIR, PR_SW, PR_LW, PR_OBS, PR_LEAN = PR_OBS, PR_FULL = PR_OBS + 1 };
#endif
template <int NPREP>
struct DuoMailT {
  double v[2][2][64]; /* [buffer][0: Tmp(2) from the surface wave, 1: Tmp(3) from the ground wave][lane] */
  /* [buffer = index parity][lane], written by the surface wave during the index BEFORE: the point's loop has
   * exited (the ground wave then leaves Tmp(3..N) alone, as the one-point-per-lane flavours do).  Double-buffered
   * like everything else in the mailbox: as one word per lane, set in the failing index itself, it held only as
   * long as the ground wave read it before the surface wave got that far - a ground wave that waits for a global
   * load first (the LEAN instances' bottom temperature behind a window's forcing loads) skipped the failing index's
   * own step (tests/test_hip_parity.py: the state of failed points). */
  uint32_t failed[2][64];
  /* round 4: what a step needs of its forcing alone (ForcingPrep, rs_physics_body.inc), worked out by
   * the ground wave one index ahead: [buffer = index parity][value][lane].  The traffic friction is the same for
   * every point of an index (one bit per buffer), VK x VZ and the products with the air's volumetric heat capacity
   * are multiplications for the surface wave.  Round 6: the air's density and specific heat travel as their product
   * (all the surface wave ever forms of them; a product is the same bits in either order) and the psychrometric
   * constant is three operations on the air temperature the surface wave has anyway: nine values instead of eleven
   * (+ 1.2 % at 1 M points).  The air's vapour pressure left too (RS_EAIR_SURFACE, rs_physics.hpp): a Magnus
   * quotient and an exp that the surface wave runs on the mailed tair and rhz, and only in a wavefront whose dry
   * tail does not skip them - eight values, 15 424 B per workgroup of the LEAN instances (see RS_DUO_LEAN_WAVES). */
  double prep[2][NPREP][64];
  /* bit 0: CheckValues' verdict on the forcing; bit 1: the index falls in the night of
   * SetDayDependendVariables (src/BalanceModel.f90:354-387) - per LANE: with RsForcing::hour_pstride = 1
   * (runsimulation_batch: every point brings its own calendar) the hour is the point's, not the index's */
  uint32_t prep_bad[2][64];
};

template <bool FULL, bool SKYG = false, class Mail>
__device__ __forceinline__ void duo_put_prep(Mail &mail, int buf, uint32_t lane, const ForcingPrep &q) {
  double (*w)[64] = mail.prep[buf];
  w[PR_TAIR][lane] = q.tair; w[PR_VZ][lane] = q.vz; w[PR_RHZ][lane] = q.rhz; w[PR_RAIN][lane] = q.rain;
  w[PR_SNOW][lane] = q.snow;
  w[PR_AVC][lane] = q.AirHCap * q.AirDens; /* AirVCap, forcing_prep_tail's expression */
#ifndef RS_EAIR_SURFACE
  w[PR_EAIR][lane] = q.EAir;
#endif
  if (!SKYG) { /* (SKYG: the radiation is the sky wave's to hand over, duo_sky) */
    w[PR_SW][lane] = q.sw;
    w[PR_LW][lane] = q.lw;
  }
  if (FULL) w[PR_OBS][lane] = q.tsurfobs;
  mail.prep_bad[buf][lane] = (q.bad ? 1u : 0u) | (q.night ? 2u : 0u) | (q.bad_rw ? 8u : 0u);
}
/* LATE (the LEAN instances): the humidity, the short- and long-wave radiation and the wind speed of the guard's
 * fallback are read from the mailbox where model_step_fluxes_prepped first uses them - behind the boundary-layer
 * loop, or in a wavefront whose dry tail is alive - instead of being held in registers across the loop.  Buffer
 * k & 1 stays as the ground wave left it until the barrier that ends index k: the ground wave writes the other one. */
struct DuoLatePrep : ForcingPrep {
  const double (*w)[64];
  uint32_t lane;
  __device__ __forceinline__ double rhz_late() const { return w[PR_RHZ][lane]; }
  __device__ __forceinline__ double vz_late() const { return w[PR_VZ][lane]; }
  __device__ __forceinline__ double sw_late() const { return w[PR_SW][lane]; }
  __device__ __forceinline__ double lw_late() const { return w[PR_LW][lane]; }
};
template <bool FULL, bool SKYG = false, bool LATE = false, class C, class Mail>
__device__ __forceinline__ auto duo_get_prep(const C &c, const Mail &mail, int buf, uint32_t lane,
                                             const uint32_t *skyfl = nullptr) {
  const double (*w)[64] = mail.prep[buf];
  typename std::conditional<LATE, DuoLatePrep, ForcingPrep>::type q;
  if constexpr (LATE) {
    q.w = w;
    q.lane = lane;
  }
  q.tair = w[PR_TAIR][lane]; q.vz = w[PR_VZ][lane]; q.rain = w[PR_RAIN][lane];
  if (!LATE) q.rhz = w[PR_RHZ][lane];
  q.snow = w[PR_SNOW][lane];
  const double AirVCap = w[PR_AVC][lane];
  q.AirVCap = AirVCap;
#ifndef RS_EAIR_SURFACE
  q.EAir = w[PR_EAIR][lane];
#endif
  if (!LATE) {
    q.sw = w[PR_SW][lane];
    q.lw = w[PR_LW][lane];
  }
  if (FULL) q.tsurfobs = w[PR_OBS][lane];
  uint32_t flags = mail.prep_bad[buf][lane];
  if (SKYG) flags |= skyfl[buf * 64 + lane]; /* the sky wave's share of CheckValues (bit 0) and its `stop` (bit 2) */
  { /* both constants first (scalar loads), then the lane picks a VALUE: see fluxes_pre */
    const double fricN = c.TrfFricNgt, fricD = c.TrFfricDay;
    q.night = (flags & 2u) != 0u;
    q.trffric = q.night ? fricN : fricD;
  }
  /* forcing_prep_tail's expressions on forcing_prep_tail's values */
#ifndef RS_BL_LAST /* (with it: model_step_fluxes_prepped forms the psychrometric constant where a wavefront needs it) */
  q.PsychC = R4(0.1) * (R4(0.00063) * (q.tair + R4(273.15)) + R4(0.47496));
#endif
  q.den0 = AirVCap * (q.tair + R4(273.15));
  q.vkvz = c.VK_Const * q.vz;
  q.avk = AirVCap * c.VK_Const;
  q.bad = (flags & 1u) != 0u;
  q.stop = SKYG && (flags & 4u) != 0u; /* only an instance with a sky wave raises it */
  q.bad_rw = (flags & 8u) != 0u;       /* (only a replay instance's ground wave raises it) */
  return q;
}

/* LDS writes done, then the workgroup barrier.  Not __syncthreads(): that also waits for the global
 * memory counter, i.e. for the six output stores of the step and the prefetched forcing loads. */
__device__ __forceinline__ void duo_meet() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

/* SKY (with FULL): sky view and local horizons (src/ModRadiation.f90, examples/example1/src/Simulation.f90:
 * 151-162) as the lock-step loop has them - the surface wave reads SW_dir and LW_net of the index itself (two
 * coalesced loads), runs CheckValues' sky-view tests and ModRadiationBySurroundings on the short- and long-wave
 * radiation the ground wave handed over, and writes the reference's in-place edits back where asked to. */
/* SKYG: a third wavefront does the sky view (duo_sky, the raw-series flavour): this wave gets the radiation as
 * the sky view leaves it and the sky wave's flags beside the ground wave's. */
/* OUTIDX: the launch may ask for its output rows in POINT order (StepArgs::out_index, the plan's order row:
 * the decimated rows of rs_driver_run go straight to their point's column, no copy kernel behind the launch). */
/* CPL: coupling in lock step, as time_loop<CPL> has it (src/Coupling.f90; everything but the replays): the state
 * saved at the window start (this wave its scalars and layers 1-2, the ground wave layers 3..N), the coupling
 * phase, Coupling_control at the window end - a point that has to replay PARKS -, the decaying corrections
 * behind the window.  A lane steps index i only if it is the index it is due for (RS_ST_CPL_RESUME); parked or
 * ahead, it is frozen for that index in both wavefronts (DuoMail::failed is rewritten before every meeting). */
/* REPLAY (with CPL): one replay ROUND of the coupling windows in lock step, as time_loop<REPLAY> has it, for the
 * points of the compacted list that asked for another replay (StepArgs::cpl_list): the launch covers [first
 * window start, last window end + 1]; a lane waits for its window start, rewinds there - CheckValues of the
 * index behind its window end, as the reference's loop does before CouplingOperations1 takes it back
 * (examples/example1/src/Simulation.f90:62-71: the forcing's verdict comes from the ground wave, ForcingPrep::
 * bad_rw), then uploadDataForCoupling (src/Coupling.f90:213-255) and the radiation coefficient (:61-78) -, runs
 * its window in the coupling phase and lets Coupling_control decide again at the end.  The list breaks the tie
 * between lane and point: `lane` below is the POINT (row0 = 0), `ml` the lane of the mailbox. */
template <int NL, bool SCORE, bool FULL = false, bool SKY = false, bool SKYG = false, bool OUTIDX = false,
          bool CPL = false, bool REPLAY = false>
__device__ __forceinline__ void duo_surface(const MathTab &mt, DuoMailT<FULL ? PR_FULL : PR_LEAN> &mail, const StepArgs &a,
                                            const uint32_t *skyfl = nullptr) {
  static_assert(FULL || !SKY, "sky view belongs to the FULL feature set");
  static_assert(!(SKY && SKYG), "the sky view is this wave's or the ground wave's");
  static_assert(FULL || !CPL, "coupling belongs to the FULL feature set");
  static_assert(CPL || !REPLAY, "replays belong to coupling");
  constexpr bool LATE = !FULL; /* duo_get_prep: the LEAN instances read part of the mailbox where it is used */
  KernArgs ka = kernargs();
  const uint32_t ml = threadIdx.x & 63u;
  /* the workgroup's slots: 64 from 64 * blockIdx.x, or what the wave table says (rs_cluster_wave_table);
   * REPLAY: entries 64 * blockIdx.x ... of the list */
  const int64_t listed = REPLAY ? (int64_t)blockIdx.x * 64 + ml : 0;
  const int64_t row0 = REPLAY ? 0 : a.wave_start ? (int64_t)a.wave_start[blockIdx.x] : (int64_t)blockIdx.x * 64;
  const uint32_t lane = REPLAY ? (listed < a.cpl_nlist ? (uint32_t)a.cpl_list[listed] : 0u) : ml;
  const int64_t p = row0 + lane;
  const bool live = REPLAY ? listed < a.cpl_nlist
                           : a.wave_start ? (int32_t)lane < a.wave_cnt[blockIdx.x] : p < a.npoints; /* a dead lane still walks to every barrier */
  RegProfile<2> T;
  Scalars s;
  {
    RegProfile<NL> all;
    if (live) {
      load_state<false>(a.state, a.np_pad, p, all, s);
    } else {
      for (int j = 1; j <= NL; ++j) all.set(j, 0.0);
      s = Scalars();
      s.failed = true;
    }
    T.set(1, all.get(1));
    T.set(2, all.get(2));
  }
  SkyPoint sky;
  if (SKY && live) sky = sky_point(ka, p);
  const bool sky_on = sky.on;
  const int32_t nsteps = ka->nsteps, t0 = ka->t0;
  /* coupling, lock-step part: what a lane needs every step in registers, the rest of CouplingVariables in the
   * state block, touched at the two events only */
  CplWindow cw;
  if (CPL && live) cpl_window(ka, consts_of(ka), p, 0u, cw);
  const bool cpl_on = cw.on;
  const int32_t cpl_cs = cw.cs, cpl_ce = cw.ce;
  bool parked = false;
  int32_t next_i = t0;
  double cpl_lastobs = 0.0, cpl_swcorr = 0.0, cpl_lwcorr = 0.0;
  if (CPL && live) {
    const double *st = a.state;
    const int64_t np = a.np_pad;
    cpl_lastobs = st[(int64_t)RS_ST_CPL_LASTOBS * np + p];
    cpl_swcorr = st[(int64_t)RS_ST_CPL_SWCORR * np + p];
    cpl_lwcorr = st[(int64_t)RS_ST_CPL_LWCORR * np + p];
    parked = (((int32_t)st[(int64_t)RS_ST_CPL_FLAGS * np + p]) & 1) != 0;
    next_i = (int32_t)st[(int64_t)RS_ST_CPL_RESUME * np + p];
    if (REPLAY) { /* a listed point: parked behind its window, wanting it again */
      parked = false;
      next_i = cpl_cs;
    }
  }
  /* REPLAY: SWRadCof / LWRadCof of the window being replayed */
  double r_swcof = R4(1.0), r_lwcof = R4(1.0);
  mail.v[0][0][ml] = T.get(2);
  /* arrives failed (or a dead lane): frozen from the first index; CPL: or not due for it */
  mail.failed[0][ml] = (s.failed || (CPL && (parked || t0 != next_i))) ? 1u : 0u;
  duo_meet();
  /* the index still steps (the ground wave is in it already); the next does not */
  auto fail_at = [&](int32_t idx) {
    s.failed = true;
    ka->state[(int64_t)RS_ST_FAILED * ka->np_pad + row0 + lane] = (double)idx;
  }; /* (the ground wave hears of it through the flag of the NEXT index, written before the meeting) */
  auto blank_rows = [&](int32_t i_from) {
    for (int32_t ii = i_from; ii < t0 + nsteps; ++ii) {
      int64_t r;
      if (output_row<false>(ka, ii, r)) {
        if (OUTIDX && ka->out_index) store_outputs<true, false>(ka, r, row0, lane, s, false);
        else store_outputs<false, false>(ka, r, row0, lane, s, false);
      }
    }
  };
  /* (CPL: from the index the point is due for - rows before it were written when it was stepped there, by a
   * replay launch that ran ahead of this chunk) */
  if (live && s.failed && !REPLAY) blank_rows(CPL && next_i > t0 ? next_i : t0);
  int32_t score = 0; /* scheduling hint of rs_hip_recluster, as in time_loop */
  /* The output row, launch-uniform and carried from index to index: what output_row<true> returns for every index
   * of the launch - the row offset of the next index that is written, which grows by the row stride per written
   * row, and how many indices lie before it (0 at every index without decimation).  One division per launch, for
   * an index t0 anywhere between two kept rows.  (The loop launders `ka` at every index: left to output_row it
   * loads decimate, row0 and the stride and multiplies them out at each.)  OUTIDX: the driver path's instances,
   * whose rows may go to the points' columns, keep asking output_row - the carried row cost the sky-view one a
   * vector register. */
  const int32_t odec = ka->o.decimate > 1 ? ka->o.decimate : 1;
  const int64_t ostride = ka->o.t_stride;
  int32_t owait = 0;
  int64_t orow_next = 0;
  if (!OUTIDX) {
    const int32_t r = t0 - 1, m = r % odec;
    owait = __builtin_amdgcn_readfirstlane(m == 0 ? 0 : odec - m);
    const int32_t row = __builtin_amdgcn_readfirstlane(r / odec + (m == 0 ? 0 : 1));
    orow_next = ((int64_t)row - ka->o.row0) * ostride;
  }
  /* (the forcing windows are the ground wave's to read: this wave gets what a step needs of them
   * through the mailbox, worked out one index ahead - ForcingPrep) */
  for (int32_t kv = 0; kv < nsteps; ++kv) {
    asm volatile("" : "+s"(ka));
    const ConstsAS &c = consts_of(ka);
    const int32_t k = __builtin_amdgcn_readfirstlane(kv);
    const int32_t i = t0 + k;
    int64_t orow = orow_next;
    bool owrite = owait == 0;
    if (OUTIDX) owrite = output_row<true>(ka, i, orow);
    /* Tmp(3) as the last step left it (LATE: read where layer 2 needs it, behind the boundary-layer loop - the
     * ground wave writes the other buffer during this index) */
    double t3 = LATE ? 0.0 : mail.v[k & 1][1][ml];
    bool go = true; /* CPL: the lane is due for this index (a failed lane keeps counting: its rows are blanked) */
    if (CPL) {
      go = !(parked || i != next_i);
      if (go) next_i = i + 1;
    }
    if (go && !s.failed) {
      const auto q = duo_get_prep<FULL, SKYG, LATE>(c, mail, k & 1, ml, skyfl);
      if (i < c.SimLen) { /* CheckValues: the forcing's verdict | the surface temperature's */
        /* REPLAY, at the rewind: the index CheckValues has just seen is the one behind the window end - with
         * the surface temperature of the end of the window */
        const bool rewind = REPLAY && i == cpl_cs;
        if ((rewind ? q.bad_rw : q.bad) | check_values_tsurf(c, s.tsurf)) fail_at(rewind ? cpl_ce + 1 : i);
      }
      if (SKYG && q.stop) fail_at(i); /* the sky wave's sky_view_radiation: at any index */
      s.tnw1 = T.get(1);
      s.tnw2 = T.get(2);
      CouplingInputs cp;
      if (CPL && cpl_on) { /* CouplingOperations1, src/Coupling.f90:10-96, first pass of the window */
        if (i < c.SimLen) {
          cp.in_phase = (i >= cpl_cs && i <= cpl_ce);
          if (REPLAY && i == cpl_cs) {
            /* inCouplingPhase is set from the loop index BEFORE a rewind takes it back (:22-27 against :61-66):
             * the step at the window start of a replay runs outside the coupling phase.  TmpNw is not restored:
             * s.tnw1/2 above hold the end-of-window values CalcHCapHCond sees in this step (the ground wave does
             * the same for 3..N) */
            cp.in_phase = false;
            double *st = ka->state;
            const int64_t np = ka->np_pad, pp_ = row0 + lane;
            cpl_restore_surface<true>(st, np, pp_, s);
            T.set(1, st[(int64_t)(RS_ST_CPL_SAVE_TMP0 + 0) * np + pp_]);
            T.set(2, st[(int64_t)(RS_ST_CPL_SAVE_TMP0 + 1) * np + pp_]);
            t3 = st[(int64_t)(RS_ST_CPL_SAVE_TMP0 + 2) * np + pp_]; /* layer 2's lower boundary: the restored Tmp(3) */
            /* (no sky view in this instance) */
            cpl_rewind_coefs(st[(int64_t)RS_ST_CPL_RADCOEFF * np + pp_], q.sw, q.lw, false, r_swcof, r_lwcof);
            st[(int64_t)RS_ST_CPL_SWCOF * np + pp_] = r_swcof; /* Coupling_control reads them at the end */
            st[(int64_t)RS_ST_CPL_LWCOF * np + pp_] = r_lwcof;
          }
          if (!REPLAY && i == cpl_cs) { /* this wave's share (the ground wave saves layers 3..N) */
            double *st = ka->state;
            const int64_t np = ka->np_pad, pp_ = row0 + lane;
            cpl_save_surface(st, np, pp_, s);
            st[(int64_t)(RS_ST_CPL_SAVE_TMP0 + 0) * np + pp_] = T.get(1);
            st[(int64_t)(RS_ST_CPL_SAVE_TMP0 + 1) * np + pp_] = T.get(2);
          }
          if (i > cpl_ce) cpl_decayed_coefs(c, mt, i, cpl_ce, cpl_swcorr, cpl_lwcorr, cp.sw_cof, cp.lw_cof);
          if (REPLAY && i >= cpl_cs && i <= cpl_ce) {
            cp.sw_cof = r_swcof;
            cp.lw_cof = r_lwcof;
          }
          if (cp.in_phase) snow_ice_check(c, cpl_lastobs, s);
        } else {
          cpl_last_values(c, mt, cw, cpl_swcorr, cpl_lwcorr, ka->state, ka->np_pad, row0 + lane, cp);
        }
      }
      if (CPL) cp.last_tsurf_obs = cpl_lastobs;
      if (FULL) {
        /* SetCurrentValues' observation forcing (src/InputOutput.f90:116-148; the ground wave decided
         * whether it applies at this index and uses the same value for Tmp(2)), and lastValues' surface
         * temperature (:169-198) - no depth stream and no tsurfOutputDepth in this flavour: the mean of
         * the two top layers (surface_temperature) */
        if (i < c.SimLen) {
          if (q.tsurfobs > R4(-100.0)) {
            T.set(1, q.tsurfobs);
            T.set(2, q.tsurfobs);
            s.tsurf = (T.get(1) + T.get(2)) / R4(2.0);
          }
        } else {
          s.tsurf = (T.get(1) + T.get(2)) / R4(2.0);
        }
      }
      const double tair = q.tair;
      auto qs = q;
      if (SKY) {
        const int64_t row = (int64_t)k * ka->f.t_stride + row0;
        const LaneOff L(lane);
        double sw_dir = L.ld(ka->f.sw_dir + row), lw_net = L.ld(ka->f.lw_net + row);
        if (i < c.SimLen) {
          if (sky_on && sky_limits_bad(sw_dir, lw_net)) fail_at(i);
          sw_dir = sky_clamp_direct(sw_dir, q.sw);
        }
        if (sky_on) {
          int64_t hstride;
          const double *hrow = horizon_row(ka, sky.hcol, hstride);
          if (!sky_view_radiation(ka->f.sun + (int64_t)k * RS_SUN_COLS, sky.sinlat, sky.coslat, sky.lonrad, sky.coslon,
                                  sky.sinlon, sky.skyv, ka->pp.albedo_surroundings, hrow, hstride, qs.sw, sw_dir, qs.lw,
                                  lw_net))
            fail_at(i); /* the reference would `stop` the process here */
        }
        sky_write_back(ka, k, row0, sky_on, sw_dir, qs.sw, qs.lw, [&](double *base, double v) { L.st(base, v); });
      }
      const Fluxes fx = model_step_fluxes_prepped<SCORE ? 1 : 2>(c, mt, s, qs, cp);
      if (SCORE) {
        score += (fx.trips & 63) - 5;
        if ((fx.trips & 64) && k >= nsteps - RS_REGIME_WINDOW) score |= 1 << 30;
      } else if (k == nsteps - 1) {
        score = fx.trips; /* the launch's last index: what forecast_key_kernel takes as one more preview */
      }
      /* layers 1-2 with Tmp(3) where a two-layer column has its lower boundary */
      if (LATE) t3 = mail.v[k & 1][1][ml];
      model_step_ground<RegProfile<2>, RegProfile<2>, false>(c, s, T, t3, tair, fx, R4(-9999.9), cp);
      if (owrite) {
        if (OUTIDX && ka->out_index) store_outputs<true, false>(ka, orow, row0, lane, s, true);
        else store_outputs<false, true>(ka, orow, row0, lane, s, true);
      }
      /* (REPLAY: a point that fails in the middle of a replay keeps, up to its window end, what the earlier
       * passes saved there: src/InputOutput.f90:151-165 only ever overwrites) */
      if (s.failed) blank_rows(REPLAY && cpl_ce + 1 > i + 1 ? cpl_ce + 1 : i + 1);
      if (CPL && cpl_on && i < c.SimLen && i == cpl_ce)
        cpl_window_end(ka->state, ka->np_pad, row0 + lane, cw, s, cpl_swcorr, cpl_lwcorr, cpl_lastobs, parked);
    }
    /* frozen at the NEXT index?  failed; CPL: or parked, or not due for it */
    mail.failed[(k & 1) ^ 1][ml] = (s.failed || (CPL && (parked || (i + 1) != next_i))) ? 1u : 0u;
    mail.v[(k & 1) ^ 1][0][ml] = T.get(2);
    if (!OUTIDX) {
      if (owrite) {
        orow_next += ostride;
        owait = odec - 1;
      } else {
        --owait;
      }
    }
    duo_meet();
  }
  if (CPL && live) a.state[(int64_t)RS_ST_CPL_RESUME * a.np_pad + p] = (double)next_i;
  if (live) {
    double *st = a.state;
    const int64_t np = a.np_pad;
    /* LATE: the point's row formed again from the lane, which the loop keeps anyway, instead of a 64-bit index
     * held across the time loop for these stores alone */
    uint32_t le = ml;
    if (LATE) asm volatile("" : "+v"(le));
    const int64_t p = LATE ? row0 + le : row0 + lane;
    st[(int64_t)(RS_ST_TMP0 + 0) * np + p] = T.get(1);
    st[(int64_t)(RS_ST_TMP0 + 1) * np + p] = T.get(2);
    st[(int64_t)RS_ST_TNW1 * np + p] = s.tnw1;
    st[(int64_t)RS_ST_TNW2 * np + p] = s.tnw2;
    st[(int64_t)RS_ST_TSURF * np + p] = s.tsurf;
    st[(int64_t)RS_ST_WAT * np + p] = s.wat;
    st[(int64_t)RS_ST_SNOW * np + p] = s.snow;
    st[(int64_t)RS_ST_ICE * np + p] = s.ice;
    st[(int64_t)RS_ST_ICE2 * np + p] = s.ice2;
    st[(int64_t)RS_ST_DEP * np + p] = s.dep;
    st[(int64_t)RS_ST_Q2MELT * np + p] = s.q2melt;
    st[(int64_t)RS_ST_T4MELT * np + p] = s.t4melt;
    st[(int64_t)RS_ST_ALBEDO * np + p] = s.albedo;
    st[(int64_t)RS_ST_VERYCOLD * np + p] = s.verycold ? 1.0 : 0.0;
    st[(int64_t)RS_ST_BLSCORE * np + p] = SCORE ? bl_score_key(score, s) : (double)score;
  }
}

/* The forcing of (1-based) index i from the hourly knots: expand_kernel's arithmetic, value for value -
 * v0 + (secs * (k1 - k0)) / span with the difference taken once per knot interval and the division by
 * the uniform span as rs_div_u; PrecPhase from the later knot between knots; the hour of rs_sy_hour.
 * (The LEAN feature set reads neither Tdew nor, after the initialization, TsurfObs.)  Knot columns are
 * per point: gathered through the plan's order row, once per interval.
 * Unlike expand_kernel this has no IEEE path: it equals the rule only inside knot_interval_fast's domain
 * (include/roadsurf.h states it for rs_hip_step_knots) - a guard here, one uniform branch per index, cost the
 * headline 1.9 % (profiles/knot_domain_guard.txt). */
template <bool FULL>
struct KnotLerp {
  double v0[FULL ? 7 : 6], dv[FULL ? 7 : 6]; /* tair, vz, rhz, prec, sw, lw [, tdew] */
  int32_t ph1; /* (PrecPhase of the earlier knot is used where it is loaded only: knot_forcing) */
  /* The time bookkeeping, launch-uniform and carried from index to index (knot_begin, knot_forcing): the knot
   * interval k and the position r in it of the index knot_forcing makes next - one division per launch, for its
   * first index; the span, its double and its reciprocal, read once per launch; the hour of the interval and
   * forcing_prep_tail's verdict on it, made where the interval's knots are loaded.  (The time loop launders its
   * kernel-argument pointer at every index and the build disables machine LICM: the compiler hoists none of it.) */
  int32_t spk, k, r, hour, night;
  double span, r_spk;
};
/* The launch's first index i0 (1-based; on a knot or between two): where the carried position starts. */
template <bool FULL>
__device__ __forceinline__ void knot_begin(KernArgs ka, KnotLerp<FULL> &K, int32_t i0) {
  K.spk = ka->spk;
  { /* the conversion is the vector unit's: its result goes back to scalar registers for the launch */
    const uint64_t u = (uint64_t)__double_as_longlong((double)K.spk);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    K.span = __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
  }
  K.r_spk = ka->r_spk;
  const int32_t t = i0 - 1;
  K.k = __builtin_amdgcn_readfirstlane(t / K.spk);
  K.r = t - K.k * K.spk;
  K.hour = 0;
  K.night = 0;
}
/* The forcing of index i = k * spk + r + 1, (k, r) as carried; leaves them at index i + 1.  The calls must follow
 * knot_begin(i0) with i = i0, i0 + 1, ... without a gap: i itself only tells index 1 (the observation) from the rest. */
template <bool FULL>
__device__ __forceinline__ Forcing knot_forcing(KernArgs ka, int64_t col, bool live, KnotLerp<FULL> &K,
                                                int32_t &kcur, int32_t i) {
  const int32_t k = K.k, r = K.r;
  /* PrecPhase of the earlier knot: the index on a knot (r == 0) is the first of its interval, or of the launch - the
   * call that loads the interval's knots, and the only one to read it */
  int32_t ph0 = 0;
  if (k != kcur) { /* uniform: a new knot interval */
    kcur = k;
    /* rs_sy_hour's expression on the interval, forcing_prep_tail's comparison on the hour: both change here only */
    const ConstsAS &c = consts_of(ka);
    K.hour = (k + ka->start_hour) % 24;
    const bool night = ((double)K.hour >= c.NightOn) || ((double)K.hour <= c.NightOff);
    K.night = __builtin_amdgcn_readfirstlane(night ? 1 : 0);
    const int fld[7] = {0, 2, 3, 4, 5, 6, 1};
    const int64_t np = ka->np_pad;
    const double *ka_ = ka->knots + ((int64_t)(k - ka->knot_k0) * RS_KNOT_FIELDS) * np + col;
    const bool has_b = (k + 1 - ka->knot_k0) < ka->knot_n;
    const double *kb_ = ka_ + (int64_t)RS_KNOT_FIELDS * np;
#pragma unroll
    for (int q = 0; q < (FULL ? 7 : 6); ++q) {
      K.v0[q] = live ? ka_[(int64_t)fld[q] * np] : 0.0;
      const double v1 = (live && has_b) ? kb_[(int64_t)fld[q] * np] : K.v0[q];
      K.dv[q] = v1 - K.v0[q];
    }
    ph0 = live ? (int32_t)ka_[8 * np] : 0;
    K.ph1 = (live && has_b) ? (int32_t)kb_[8 * np] : ph0;
  }
  /* FULL: beside seven knot pairs and thirteen layers the span, its double and its reciprocal cost the instance two
   * vector registers when they stay resident (120 -> 122): that feature set reads them again at every index */
  const int32_t spk = FULL ? ka->spk : K.spk;
  const double secs = (double)r, span = FULL ? (double)spk : K.span, r_spk = FULL ? ka->r_spk : K.r_spk;
  Forcing f;
  f.tair = K.v0[0] + rs_div_u(secs * K.dv[0], span, r_spk);
  f.vz = K.v0[1] + rs_div_u(secs * K.dv[1], span, r_spk);
  f.rhz = K.v0[2] + rs_div_u(secs * K.dv[2], span, r_spk);
  f.prec = K.v0[3] + rs_div_u(secs * K.dv[3], span, r_spk);
  f.sw = K.v0[4] + rs_div_u(secs * K.dv[4], span, r_spk);
  f.lw = K.v0[5] + rs_div_u(secs * K.dv[5], span, r_spk);
  f.phase = (r == 0) ? ph0 : K.ph1;
  f.hour = K.hour;
  f.tdew = 0.0;
  f.tsurfobs = R4(-9999.9);
  if (FULL) { /* expand_kernel<TDEW, OBS>: the dew point like the others, the observation at index 1 only */
    f.tdew = K.v0[6] + rs_div_u(secs * K.dv[6], span, r_spk);
    if (i == 1 && live) f.tsurfobs = (ka->knots + ((int64_t)(k - ka->knot_k0) * RS_KNOT_FIELDS + 7) * ka->np_pad)[col];
  }
  f.depth = R4(-9999.9);
  K.r = r + 1;
  if (K.r == spk) {
    K.r = 0;
    K.k = k + 1;
  }
  return f;
}

/* ---- the forcing from the RAW series (rs_driver_run's blocks, rs_step_raw) ---------------------------
 * What the driver path's expansion kernel wrote into forcing windows, the ground wave now forms in
 * registers, one index ahead of the surface wave: per variable JsonSource::interpolate's value of every
 * source (examples/example1/src/JsonSource.cpp:86-170), GetWeather's own test of it (:337-356) and the
 * overlay in source order (DataHandler.cpp:75-84), value for value as rs_raw.hpp raw_source_value has them.
 * The sources share their time axes, so which raw interval an index falls into and whether it copies or
 * interpolates there is the same for every point: a SEGMENT (RawSeg) is a run of indices over which every
 * source keeps its (kind, rawPos).  At the first index of a segment the wavefront RESOLVES each variable:
 * every lane loads its two raw ends of every source that has the variable (its column of the series, through
 * the plan's order row), applies the supply test (a copy: raw > threshold; an interpolation: both ends >
 * threshold - the value then lies between them, RawPlanStep::rden) and keeps the ends of the LAST source that
 * supplies.  Where all 64 lanes agree on that source - the rule, not the exception: whether a source has a
 * variable at a time is a property of the data set - the variable costs five instructions per index,
 * v0 + RN(num (v1 - v0) / den) with the source's uniform (num, den, 1/den) on the scalar unit; a copy, or a
 * variable nobody supplies, is v0 + 0.  Anything else - lanes that disagree, a non-finite end, a difference
 * so large or so small that the division by reciprocal is not the IEEE one, a raw -0.0 to be copied, a plan
 * entry with rden = 0 - is evaluated index by index with raw_source_value itself (RAW_SLOW). */
/* Who evaluates which variables: the ground wave alone {tair, vz, rhz, prec, tdew, tsurfobs, sw, lw}
 * (FSET_ALL); with per-point sky view the ground wave the first six of them (FSET_GROUND) and the sky wave
 * {sw, lw, sw_dir, lw_net} (FSET_SKY, duo_sky). */
enum { FSET_ALL = 0, FSET_GROUND = 1, FSET_SKY = 2 };
__device__ __forceinline__ constexpr int raw_nfields(int fset) { return fset == FSET_ALL ? 8 : fset == FSET_GROUND ? 6 : 4; }
__device__ __forceinline__ constexpr int raw_field_of(int fset, int q) {
  return fset == FSET_SKY ? (q == 0 ? RAW_SW : q == 1 ? RAW_LW : q == 2 ? RAW_SWDIR : RAW_LWNET)
                          : (q == 0 ? RAW_TAIR : q == 1 ? RAW_VZ : q == 2 ? RAW_RHZ : q == 3 ? RAW_PREC
                             : q == 4 ? RAW_TDEW : q == 5 ? RAW_OBS : q == 6 ? RAW_SW : RAW_LW);
}
constexpr int kRawObs = 5; /* tsurfobs in FSET_ALL / FSET_GROUND */
template <int NF>
struct RawLerp {
  double v0[NF], dv[NF];
  /* uniform: bit 10 s + q: variable q is interpolated from source s in this segment (s = 4: copied, or
   * missing: v0 + 0); bit 50 + q: index by index (RAW_SLOW) */
  uint64_t mode;
  /* uniform: >= 0: nothing is evaluated index by index in this segment and at most ONE source interpolates
   * (that one; 4: none - every variable is copied or missing): the whole set is one straight line of
   * v0 + RN(num dv / den) with that source's scalars - for a copied or missing variable dv = 0 and the term is
   * +0, as in the general form.  The rule outside the hours in which observations overlay the forecast. */
  int32_t single;
  int32_t seg, seg_end; /* current segment and its end (0-based, exclusive) */
  /* MIXED variables (uniform mask): the lanes disagree on the supplying source - stations without a sensor, gaps
   * in an observation series - but every lane's ends allow the short form: each interpolating source's line is
   * evaluated with that source's scalars and the lane keeps its own (`wsel`, per lane: three bits per variable,
   * the source or 4).  `imask`: the sources that interpolate in this segment. */
  uint32_t mixed, imask;
  uint32_t wsel;
};

/* one variable of one point at 0-based index i, the long way: every source, every test */
__device__ __forceinline__ double raw_slow_value(KernArgs ka, int fld, int64_t col, int32_t i) {
  const double thr = raw_threshold(fld);
  double v = raw_miss();
  const int nsrc = ka->raw.nsrc;
  const int64_t np = ka->raw.np_pad;
  for (int s = 0; s < nsrc; ++s) {
    const double *x = ka->raw.src[s].fld[fld];
    if (!x) continue;
    const RawPlanStep st = raw_plan_at(ka->raw.src[s].plan, i);
    if (st.kind == RAW_NONE) continue;
    const double a = x[(int64_t)st.rp * np + col], b = x[(int64_t)(st.rp + 1) * np + col];
    double vs;
    if (raw_source_value(st, a, b, thr, vs)) v = vs;
  }
  return v;
}

template <int FSET>
__device__ __forceinline__ void raw_resolve(KernArgs ka, int64_t col, bool live, RawLerp<raw_nfields(FSET)> &R) {
  constexpr int NF = raw_nfields(FSET);
  const RawSeg __attribute__((address_space(4))) *sg =
      (const RawSeg __attribute__((address_space(4))) *)ka->raw.segs + R.seg;
  R.seg_end = sg->i1;
  const int32_t i0 = sg->i0;
  const int nsrc = ka->raw.nsrc;
  const int64_t np = ka->raw.np_pad;
  uint64_t mode = 0;
  uint32_t mixed = 0u, imask = 0u, wsel = 0u;
  for (int s = 0; s < nsrc; ++s)
    if (sg->kind[s] == RAW_INTERP) imask |= 1u << s;
#pragma unroll
  for (int q = 0; q < NF; ++q) {
    const int fld = raw_field_of(FSET, q);
    const double thr = raw_threshold(fld);
    int32_t wl = 4;  /* the lane's winner: a source that interpolates, or 4 (copy / nobody) */
    bool okl = true; /* ... and its ends allow the short form */
    double a_w = raw_miss(), d_w = 0.0;
    for (int s = 0; s < nsrc; ++s) {
      const double *x = ka->raw.src[s].fld[fld];
      const int32_t kind = sg->kind[s], rp = sg->rp[s];
      if (!x || kind == RAW_NONE) continue; /* uniform */
      const double *xa = x + (int64_t)rp * np + col;
      const double a = *xa; /* (a dead lane reads column 0) */
      if (kind == RAW_COPY) {
        if (a > thr) {
          wl = 4;
          a_w = a;
          d_w = 0.0;
          okl = !rs_is_neg_zero(a); /* v0 + 0 would lose the sign */
        }
      } else {
        const double b = xa[np];
        if (a > thr && b > thr) {
          const double d = b - a;
          const double den = raw_plan_at(ka->raw.src[s].plan, i0).den;
          const double ad = __builtin_fabs(d);
          wl = s;
          a_w = a;
          d_w = d;
          /* |num d| stays inside the range in which the division by reciprocal is the IEEE one for every
           * 1 <= num < den of the segment (raw_source_value's own test, once per segment) */
          okl = (__builtin_fabs(a) < __builtin_inf()) && (__builtin_fabs(b) < __builtin_inf()) &&
                (den * ad < 1e290) && (d == 0.0 || ad >= 1e-290);
        }
      }
    }
    const int32_t w0 = __builtin_amdgcn_readfirstlane(wl); /* lane 0 is never a dead lane */
    const bool all_ok = __builtin_amdgcn_ballot_w64(live && !okl) == 0ull;
    const bool same = __builtin_amdgcn_ballot_w64(live && wl != w0) == 0ull;
    if (all_ok && same) mode |= 1ull << (10 * w0 + q);
    else if (all_ok) mixed |= 1u << q;
    else mode |= 1ull << (50 + q);
    wsel |= (uint32_t)wl << (3 * q);
    R.v0[q] = a_w;
    R.dv[q] = d_w;
  }
  R.mode = mode;
  R.mixed = mixed;
  R.imask = imask;
  R.wsel = wsel;
  int32_t single = (((mode >> 50) & 1023ull) || mixed) ? -1 : 4;
  for (int s = 0; s < RS_MAX_SOURCES; ++s)
    if ((mode >> (10 * s)) & 1023ull) single = (single == 4) ? s : -1;
  R.single = single;
}

/* The merged raw values of the set's variables at (1-based) index i, in val[].  `need_obs` (FSET_ALL /
 * FSET_GROUND): the step can use the road-temperature observation (initialization phase or force_tsurf),
 * else val[kRawObs] is left unset. */
template <int FSET>
__device__ __forceinline__ void raw_values(KernArgs ka, int64_t col, bool live, RawLerp<raw_nfields(FSET)> &R,
                                           int32_t i, bool need_obs, double (&val)[raw_nfields(FSET)]) {
  constexpr int NF = raw_nfields(FSET);
  const int32_t t = i - 1;
  if (t >= R.seg_end) { /* uniform: a new segment (a segment is never empty) */
    R.seg += 1;
    raw_resolve<FSET>(ka, col, live, R);
  }
  if (R.single >= 0) { /* uniform */
    double num = 0.0, den = 1.0, rden = 1.0;
    if (R.single < RS_MAX_SOURCES) {
      const RawPlanStep st = raw_plan_at(ka->raw.src[R.single].plan, t);
      num = st.num;
      den = st.den;
      rden = st.rden;
    }
    if (rden != 0.0) {
#pragma unroll
      for (int q = 0; q < NF; ++q) val[q] = R.v0[q] + raw_quot(num * R.dv[q], den, rden);
      return;
    }
  }
#pragma unroll
  for (int q = 0; q < NF; ++q) asm volatile("" : "=v"(val[q])); /* each is written by exactly one block below */
  const uint32_t keep = (FSET != FSET_SKY && !need_obs) ? ~(1u << kRawObs) : ~0u;
  uint32_t slow = (uint32_t)(R.mode >> 50) & 1023u & keep;
#pragma nounroll
  for (int s = 0; s < RS_MAX_SOURCES; ++s) {
    const uint32_t m = (uint32_t)(R.mode >> (10 * s)) & 1023u & keep;
    if (m == 0u) continue;
    const RawPlanStep st = raw_plan_at(ka->raw.src[s].plan, t);
    if (st.rden == 0.0) { /* this entry promises nothing (rs_raw.hpp): the long way for this index */
      slow |= m;
      continue;
    }
#pragma unroll
    for (int q = 0; q < NF; ++q)
      if (m & (1u << q)) val[q] = R.v0[q] + raw_quot(st.num * R.dv[q], st.den, st.rden);
  }
  {
    const uint32_t m = (uint32_t)(R.mode >> 40) & 1023u & keep;
#pragma unroll
    for (int q = 0; q < NF; ++q)
      if (m & (1u << q)) val[q] = R.v0[q] + 0.0; /* a copy, or missing: what the short form gives for dv = 0 */
  }
  uint32_t mix = R.mixed & keep;
  if (mix) { /* uniform */
    for (int s = 0; s < RS_MAX_SOURCES; ++s) /* an entry that promises nothing: the long way for this index */
      if ((R.imask & (1u << s)) && raw_plan_at(ka->raw.src[s].plan, t).rden == 0.0) {
        slow |= mix;
        mix = 0u;
      }
  }
  if (mix) {
#pragma unroll
    for (int q = 0; q < NF; ++q)
      if (mix & (1u << q)) val[q] = R.v0[q] + 0.0; /* the lanes that copy, or have nobody: dv = 0 */
#pragma nounroll
    for (int s = 0; s < RS_MAX_SOURCES; ++s) {
      if (!(R.imask & (1u << s))) continue;
      const RawPlanStep st = raw_plan_at(ka->raw.src[s].plan, t);
#pragma unroll
      for (int q = 0; q < NF; ++q)
        if (mix & (1u << q)) {
          const double cand = R.v0[q] + raw_quot(st.num * R.dv[q], st.den, st.rden);
          if (((R.wsel >> (3 * q)) & 7u) == (uint32_t)s) val[q] = cand;
        }
    }
  }
  if (slow) {
#pragma unroll
    for (int q = 0; q < NF; ++q)
      if (slow & (1u << q)) val[q] = raw_slow_value(ka, raw_field_of(FSET, q), col, t);
  }
}

/* The forcing of index i for the ground wave.  FSET_GROUND: the short- and long-wave radiation are the
 * sky wave's (duo_sky: it tests them and hands them on); here they read 0, inside every bound of CheckValues. */
template <int FSET>
__device__ __forceinline__ Forcing raw_forcing(KernArgs ka, int64_t col, bool live, bool rejected,
                                               RawLerp<raw_nfields(FSET)> &R, int32_t i, bool need_obs) {
  double val[raw_nfields(FSET)];
  raw_values<FSET>(ka, col, live, R, i, need_obs, val);
  Forcing f;
  f.tair = rejected ? raw_miss() : val[0];
  f.vz = val[1];
  f.rhz = val[2];
  f.prec = val[3];
  f.tdew = val[4];
  f.tsurfobs = need_obs ? val[kRawObs] : raw_miss();
  f.sw = FSET == FSET_ALL ? val[FSET == FSET_ALL ? 6 : 0] : 0.0;
  f.lw = FSET == FSET_ALL ? val[FSET == FSET_ALL ? 7 : 0] : 0.0;
  f.phase = -9999; /* InputData.cpp:16: the driver never hands PrecPhase on */
  f.hour = ((const int32_t __attribute__((address_space(4))) *)ka->raw.hour)[i - 1]; /* uniform: a scalar load */
  f.depth = raw_miss(); /* InputData.cpp:18 */
  return f;
}

/* FULL: the FULL feature set without sky view, coupling, a depth stream or tsurfOutputDepth (what the
 * launcher checks): the optional streams, the initialization phase and relaxation.  The ground wave owns
 * what they add to the forcing's share of a step - CheckValues' dew-point test, whether the observation
 * is forced on Tmp(1:2) at an index (it needs the forced Tmp(2) itself, for the flux into layer 3), and
 * RelaxationOperations (src/Relaxation.f90:10-47: the anchors at the end of the initialization, which go
 * to the state block there and then, and the decaying correction behind it). */
enum { SRC_WINDOW = 0, SRC_KNOTS = 1, SRC_RAW = 2 }; /* where the ground wave's forcing comes from */
/* SKYG (with SRC_RAW): the launch has per-point sky view and a THIRD wavefront for it (duo_sky): the short- and
 * long-wave radiation, their share of CheckValues and ModRadiationBySurroundings are that wave's; this one
 * makes the other six variables. */
/* REPLAY (with CPL, SRC_RAW): see duo_surface - this wave restores layers 3..N at the rewind and computes the
 * flux and heat capacities of that step from the restored profile and the end-of-window one (the stale TmpNw),
 * and hands over CheckValues' verdict on the forcing of the index behind the window (ForcingPrep::bad_rw). */
template <int NL, int SRC = SRC_WINDOW, bool FULL = false, bool SKYG = false, bool CPL = false, bool REPLAY = false>
__device__ __forceinline__ void duo_ground(const MathTab &mt, DuoMailT<FULL ? PR_FULL : PR_LEAN> &mail, const StepArgs &a) {
  constexpr bool KNOTS = SRC == SRC_KNOTS, RAW = SRC == SRC_RAW;
  static_assert(FULL || !CPL, "coupling belongs to the FULL feature set");
  static_assert(!RAW || FULL, "the driver's series carry the FULL feature set");
  static_assert(!SKYG || RAW, "a sky wave exists only where the forcing is made from the raw series");
  static_assert(!REPLAY || (CPL && RAW && !SKYG), "replay rounds in this flavour: raw series, no sky view");
  /* knot_forcing walks the launch's indices one by one from knot_begin's: it carries its position and takes no index
   * to look one up - a flavour that rewinds or skips indices cannot read knots this way */
  static_assert(!KNOTS || (!CPL && !REPLAY), "the knot-reading source steps every index of the launch in order");
  KernArgs ka = kernargs();
  const uint32_t ml = threadIdx.x & 63u; /* lane of the mailbox; `lane` + row0 = the point (REPLAY: through the list) */
  const int64_t listed = REPLAY ? (int64_t)blockIdx.x * 64 + ml : 0;
  const int64_t row0 = REPLAY ? 0 : a.wave_start ? (int64_t)a.wave_start[blockIdx.x] : (int64_t)blockIdx.x * 64;
  const uint32_t lane = REPLAY ? (listed < a.cpl_nlist ? (uint32_t)a.cpl_list[listed] : 0u) : ml;
  const int64_t p = row0 + lane;
  const bool live = REPLAY ? listed < a.cpl_nlist
                           : a.wave_start ? (int32_t)lane < a.wave_cnt[blockIdx.x] : p < a.npoints;
  double Tg[NL - 2]; /* Tmp(3..NL) */
#pragma unroll
  for (int j = 3; j <= NL; ++j) Tg[j - 3] = live ? a.state[(int64_t)(RS_ST_TMP0 + j - 1) * a.np_pad + p] : 0.0;
  /* LATE (the LEAN instances): what the time loop uses once per index or once per knot interval is not held across
   * it - the bottom temperature is read again at every index (one coalesced load from the scalar base), the knot
   * column is a 32-bit lane value beside a scalar base, the point's row is formed again for the final stores */
  constexpr bool LATE = !FULL;
  const double tbot = (live && !LATE) ? ka->pp.tbottom[p] : 0.0;
  mail.v[0][1][ml] = Tg[0];
  const int32_t nsteps = ka->nsteps, t0 = ka->t0;
  /* FULL: as time_loop sets them up */
  int32_t initlen = 0;
  bool relax = false;
  double relax_dt = 0, relax_dv = 0, relax_dr = 0;
  auto relax_targets = [&](double &tairR, double &vzR, double &rhR) { /* through REAL(4): src/InputOutput.f90:19-26 */
    tairR = (double)(float)ka->pp.tair_relax[p];
    vzR = (double)(float)ka->pp.vz_relax[p];
    rhR = (double)(float)ka->pp.rh_relax[p];
  };
  if (FULL && live) {
    initlen = ka->pp.initlen ? ka->pp.initlen[p] : 0;
    if (consts_of(ka).use_relaxation && ka->pp.tair_relax) {
      double tairR, vzR, rhR;
      relax_targets(tairR, vzR, rhR);
      relax = !(tairR < R4(-100.0) || tairR > R4(100.0) || vzR < R4(0.0) || vzR > R4(100.0) ||
                rhR < R4(0.0) || rhR > 110);
      relax_dt = tairR - a.state[(int64_t)RS_ST_TAIR_END * a.np_pad + p];
      relax_dv = vzR - a.state[(int64_t)RS_ST_VZ_END * a.np_pad + p];
      relax_dr = rhR - a.state[(int64_t)RS_ST_RH_END * a.np_pad + p];
    }
  }
  /* CPL: where the point's coupling window starts - from there on the observation is no longer forced on the
   * two top layers (src/InputOutput.f90:120-121), and at that index the layers are saved (src/Coupling.f90:172-210) */
  int32_t cpl_cs = 0x7fffffff, cpl_ce = 0x7ffffff0;
  if (CPL && live) {
    const int32_t cidx = ka->pp.coupling_index ? ka->pp.coupling_index[p] : 0;
    if (consts_of(ka).use_coupling && ka->pp.coupling_index && !(ka->pp.coupling_tsurf[p] < -100 || cidx < 1)) {
      cpl_cs = ((double)cidx <= consts_of(ka).cplLenR) ? 1 : cidx - consts_of(ka).cplLenI;
      cpl_ce = cidx;
    }
  }
  const int64_t rcol_ = (RAW && live) ? (ka->raw.col ? (int64_t)ka->raw.col[p] : p) : 0; /* the point's column of the raw series */
  /* the anchors of an index are stored at the START of that index's step, when the surface wave's
   * verdict on the index before is in the mailbox (a point that has failed never reaches it) */
  bool anchor_due = false;
  double anchor_t = 0, anchor_v = 0, anchor_r = 0;
  double obs_cur = R4(-9999.9); /* the observation forced on Tmp(1:2) at the current index, or missing */
  KnotLerp<FULL> klerp; /* KNOTS: the knots of the current interval, where the next index lies in it, its day/night verdict */
  klerp.night = 0;
  /* the forcing's share of index `in`, from the forcing in `f` */
  auto prep = [&](const ConstsAS &c, const Forcing &f, int32_t in, double &obs) -> ForcingPrep {
    if (!FULL) return forcing_prep<KNOTS>(c, mt, f, in, in < c.SimLen, klerp.night != 0);
    bool bad;
    const bool has_tdew = RAW ? true : KNOTS ? (ka->knots_tdew & 2) != 0 : ka->f.tdew != nullptr;
    double vz = forcing_prep_head(c, f, in, in < c.SimLen, has_tdew, bad);
    double tair = f.tair, rhz = f.rhz;
    obs = R4(-9999.9);
    if (in < c.SimLen) {
      if ((in <= initlen || c.force_tsurf) && f.tsurfobs > R4(-100.0) && (!CPL || in < cpl_cs)) obs = f.tsurfobs;
      if (relax) {
        if (in == initlen) { /* the anchors: once per point */
          double tairR, vzR, rhR;
          relax_targets(tairR, vzR, rhR);
          relax_dt = tairR - tair;
          relax_dv = vzR - vz;
          relax_dr = rhR - rhz;
          anchor_due = true;
          anchor_t = tair;
          anchor_v = vz;
          anchor_r = rhz;
        }
        if (in > initlen) {
          double e;
          const uint32_t d = (uint32_t)(in - initlen);
          if (c.relax_tab && d <= (uint32_t)c.SimLen) {
            e = ((const double *)c.relax_tab)[d];
          } else {
            const double den = (double)(4.f * 3600.f);
            e = rs_exp(mt, rs_div(-((c.DTSecs * in) - (c.DTSecs * initlen)), den));
          }
          tair = tair - relax_dt * e;
          vz = vz - relax_dv * e;
          rhz = rhz - relax_dr * e;
          if (rhz > R4(100.)) rhz = R4(100.0);
        }
      }
    }
    ForcingPrep q = forcing_prep_tail<KNOTS>(c, mt, f, tair, vz, rhz, bad, klerp.night != 0);
    q.tsurfobs = obs;
    if (REPLAY && live && in == cpl_cs && in < c.SimLen) {
      /* the rewind: CheckValues has just seen the index behind the window end (0-based: cpl_ce) - its forcing
       * the long way, once per replay */
      Forcing g = Forcing();
      const int32_t tb = cpl_ce;
      g.tair = ka->raw.status && ka->raw.status[rcol_] != 0 ? raw_miss() : raw_slow_value(ka, RAW_TAIR, rcol_, tb);
      g.vz = raw_slow_value(ka, RAW_VZ, rcol_, tb);
      g.rhz = raw_slow_value(ka, RAW_RHZ, rcol_, tb);
      g.prec = raw_slow_value(ka, RAW_PREC, rcol_, tb);
      g.sw = raw_slow_value(ka, RAW_SW, rcol_, tb);
      g.lw = raw_slow_value(ka, RAW_LW, rcol_, tb);
      g.tdew = raw_slow_value(ka, RAW_TDEW, rcol_, tb);
      q.bad_rw = check_values_forcing(c, g) | (g.tdew < -90) | (g.tdew > R4(100.0));
    }
    return q;
  };
  /* the forcing of the launch's first index, prepared before the first meeting (a lane beyond npoints
   * reads nothing: the windows need only span npoints columns) */
  Forcing nxt = Forcing();
  int32_t kcur = -1;
  /* (LATE: gathered, the 32-bit entry of the order row; else the lane beside the workgroup's first row) */
  const int32_t kcol32 = (KNOTS && LATE && live) ? (ka->knot_gather ? ka->knot_gather[p] : (int32_t)lane) : 0;
  const int64_t kcol0 = (KNOTS && LATE && !ka->knot_gather) ? row0 : 0;
  const int64_t kcol = LATE ? 0 : (KNOTS && live) ? (ka->knot_gather ? (int64_t)ka->knot_gather[p] : p) : 0;
  /* RAW: the point's column of the raw series, read_input's verdict on it, the segment of the first index */
  constexpr int FSET = SKYG ? FSET_GROUND : FSET_ALL;
  RawLerp<raw_nfields(FSET)> rlerp;
  const int64_t rcol = rcol_;
  const bool rejected = RAW && live && ka->raw.status && ka->raw.status[rcol] != 0;
  /* the observation can act at index `in`: SetCurrentValues' own condition (src/InputOutput.f90:116-121),
   * for the whole wavefront */
  auto obs_wanted = [&](const ConstsAS &c, int32_t in) -> bool {
    return c.force_tsurf || __builtin_amdgcn_ballot_w64(live && in <= initlen) != 0ull;
  };
  if (RAW) {
    rlerp.seg = ka->raw.seg0;
    raw_resolve<FSET>(ka, rcol, live, rlerp);
  }
  {
    const ConstsAS &c0 = consts_of(ka);
    if (KNOTS) {
      knot_begin<FULL>(ka, klerp, t0);
      nxt = knot_forcing<FULL>(ka, LATE ? kcol0 + kcol32 : kcol, live, klerp, kcur, t0);
    } else if (RAW) nxt = raw_forcing<FSET>(ka, rcol, live, rejected, rlerp, t0, obs_wanted(c0, t0));
    else if (live) nxt = load_forcing<FULL, true>(ka, row0, lane, 0);
    duo_put_prep<FULL, SKYG>(mail, 0, ml, prep(c0, nxt, t0, obs_cur));
  }
  duo_meet();
  for (int32_t kv = 0; kv < nsteps; ++kv) {
    asm volatile("" : "+s"(ka));
    const ConstsAS &c = consts_of(ka);
    const int32_t k = __builtin_amdgcn_readfirstlane(kv);
    /* next index's forcing: fetched here, used behind the layers */
    if (!KNOTS && !RAW && k + 1 < nsteps && live) nxt = load_forcing<FULL, true>(ka, row0, lane, k + 1);
    double t2 = mail.v[k & 1][0][ml]; /* Tmp(2) as the last step left it (melting included) */
    const double tbot_k = !LATE ? tbot : live ? LaneOff(lane).ld(ka->pp.tbottom + row0) : 0.0;
    /* a failed point takes no further step in any flavour: its Tmp(3..N) stay as the failing index left
     * them (the flag was raised before the barrier that ended that index) */
    if (REPLAY && !mail.failed[k & 1][ml] && t0 + k == cpl_cs && t0 + k < c.SimLen && live) {
      /* the rewind (uploadDataForCoupling, src/Coupling.f90:245-247): Tmp is restored, TmpNw is not - this
       * step's heat capacities see the end-of-window profile (Tg as it stands), its fluxes the restored one */
      const double *sv = ka->state + (int64_t)RS_ST_CPL_SAVE_TMP0 * ka->np_pad + p;
      const int64_t np = ka->np_pad;
      double cur = sv[(int64_t)2 * np]; /* restored Tmp(3) */
      double Gprev = c.lk[2].condDZ * (cur - sv[np]); /* ... against the restored Tmp(2) */
#pragma unroll
      for (int j = 3; j <= NL; ++j) {
        const double tnext = (j == NL) ? tbot : sv[(int64_t)j * np];
        const double stale = Tg[j - 3];
        Tg[j - 3] = layer_step(c, j, cur, stale, tnext, Gprev, nullptr);
        cur = tnext;
      }
    } else
    if (!mail.failed[k & 1][ml]) {
      if (CPL && !REPLAY && t0 + k == cpl_cs && t0 + k < c.SimLen && live) { /* saveDataForCoupling: layers 3..N as they stand */
#pragma unroll
        for (int j = 3; j <= NL; ++j) ka->state[(int64_t)(RS_ST_CPL_SAVE_TMP0 + j - 1) * ka->np_pad + p] = Tg[j - 3];
      }
      if (FULL) {
        if (obs_cur > R4(-100.0)) t2 = obs_cur; /* SetCurrentValues has forced Tmp(1:2) at this index */
        if (anchor_due && live) {
          double *st = ka->state;
          st[(int64_t)RS_ST_TAIR_END * ka->np_pad + p] = anchor_t;
          st[(int64_t)RS_ST_VZ_END * ka->np_pad + p] = anchor_v;
          st[(int64_t)RS_ST_RH_END * ka->np_pad + p] = anchor_r;
        }
      }
      double Gprev = c.lk[2].condDZ * (Tg[0] - t2); /* G(2), the expression layer 2 itself evaluates */
#pragma unroll
      for (int j = 3; j <= NL; ++j) {
        const double tj = Tg[j - 3];
        const double tnext = (j == NL) ? tbot_k : Tg[j - 2];
        Tg[j - 3] = layer_step(c, j, tj, tj, tnext, Gprev, nullptr);
      }
    }
    if (FULL) anchor_due = false;
    mail.v[(k & 1) ^ 1][1][ml] = Tg[0];
    if (k + 1 < nsteps) {
      const int32_t in = t0 + k + 1;
      if (KNOTS) nxt = knot_forcing<FULL>(ka, LATE ? kcol0 + kcol32 : kcol, live, klerp, kcur, in);
      if (RAW) nxt = raw_forcing<FSET>(ka, rcol, live, rejected, rlerp, in, obs_wanted(c, in));
      duo_put_prep<FULL, SKYG>(mail, (k & 1) ^ 1, ml, prep(c, nxt, in, obs_cur));
    }
    duo_meet();
  }
  if (live) {
    uint32_t le = ml; /* (LATE: as in duo_surface) */
    if (LATE) asm volatile("" : "+v"(le));
    const int64_t pe = LATE ? row0 + le : p;
#pragma unroll
    for (int j = 3; j <= NL; ++j) a.state[(int64_t)(RS_ST_TMP0 + j - 1) * a.np_pad + pe] = Tg[j - 3];
  }
}

/* The sky wave: third wavefront of the workgroup in launches with per-point sky view whose forcing comes from
 * the raw series.  CheckValues' tests of the radiation, the SW_dir clamp and ModRadiationBySurroundings with the
 * sun's position (src/InputOutput.f90:45-84, src/ModRadiation.f90:7-73, src/SunPosition.f90:123-193; examples/
 * example1/src/Simulation.f90:151-162) depend on the forcing and the point's geometry alone: like the rest of
 * the forcing's share of a step they are worked out one index AHEAD, here - four variables from the raw series
 * (global and direct short wave, long wave, net long wave), the tests, the sky view - and the surface wave
 * receives the radiation as the sky view leaves it (mailbox values 9 and 10) plus this wave's flags.  Done on
 * the ground wave, beside thirteen layers and the other six variables, the sky view spilled 86-106 registers;
 * on the surface wave it lengthens the step's serial chain. */
__device__ __forceinline__ void duo_sky(DuoMailT<PR_FULL> &mail, uint32_t *skyfl, const StepArgs &a) {
  KernArgs ka = kernargs();
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t row0 = a.wave_start ? (int64_t)a.wave_start[blockIdx.x] : (int64_t)blockIdx.x * 64;
  const int64_t p = row0 + lane;
  const bool live = a.wave_start ? (int32_t)lane < a.wave_cnt[blockIdx.x] : p < a.npoints;
  SkyPoint sky;
  if (live) sky = sky_point(ka, p);
  const bool sky_on = sky.on;
  const int64_t rcol = live ? (ka->raw.col ? (int64_t)ka->raw.col[p] : p) : 0;
  RawLerp<4> R;
  R.seg = ka->raw.seg0;
  raw_resolve<FSET_SKY>(ka, rcol, live, R);
  const int32_t nsteps = ka->nsteps, t0 = ka->t0;
  auto put = [&](int buf, int32_t in) {
    const ConstsAS &c = consts_of(ka);
    double val[4];
    raw_values<FSET_SKY>(ka, rcol, live, R, in, false, val);
    double sw = val[0], lw = val[1], sw_dir = val[2], lw_net = val[3];
    bool bad = false, stop = false;
    if (in < c.SimLen) {
      /* check_values_forcing's tests of SW and LW (the ground wave runs the others with 0 in their place) */
      bad = (sw < c.chk[1]) | (lw < c.chk[1]) | (sw > c.chk[5]) | (lw > c.chk[6]);
      if (sky_on && sky_limits_bad(sw_dir, lw_net)) bad = true;
      sw_dir = sky_clamp_direct(sw_dir, sw);
    }
    if (sky_on) {
      const double *sunrow = ka->f.sun + (int64_t)(in - t0) * RS_SUN_COLS;
      int64_t hstride;
      const double *hrow = horizon_row(ka, sky.hcol, hstride);
      if (!sky_view_radiation(sunrow, sky.sinlat, sky.coslat, sky.lonrad, sky.coslon, sky.sinlon, sky.skyv,
                              ka->pp.albedo_surroundings, hrow, hstride, sw, sw_dir, lw, lw_net))
        stop = true; /* the reference would `stop` the process here: the point is failed at this index, checked or not */
    }
    mail.prep[buf][PR_SW][lane] = sw;
    mail.prep[buf][PR_LW][lane] = lw;
    skyfl[buf * 64 + lane] = (bad ? 1u : 0u) | (stop ? 4u : 0u);
  };
  put(0, t0);
  duo_meet();
  for (int32_t kv = 0; kv < nsteps; ++kv) {
    asm volatile("" : "+s"(ka));
    const int32_t k = __builtin_amdgcn_readfirstlane(kv);
    if (k + 1 < nsteps) put((k & 1) ^ 1, t0 + k + 1);
    duo_meet();
  }
}

/* SRC: SRC_WINDOW / SRC_KNOTS / SRC_RAW.  SKY: per-point sky view - on the surface wave (forcing windows)
 * or, with SRC_RAW, on a third wavefront (duo_sky). */
template <int NL, bool SCORE, int SRC = SRC_WINDOW, bool FULL = false, bool SKY = false, bool CPL = false,
          bool REPLAY = false>
#ifndef RS_DUO_LEAN_WAVES
/* Five wavefronts per SIMD for the LEAN instances: 96 registers without a spill (the mailbox values a step first needs
 * behind the boundary-layer loop are read there, the ground wave keeps no per-point constant it uses once per index:
 * LATE in duo_surface / duo_ground; tests/test_duo_lean_resources.py holds the figures), 15 424 B of LDS - ten
 * workgroups to a CU.  Measured against four (profiles/r11_five_waves.txt): the step launches of a pass sum to 15 %
 * less, and the headline gains - but only with EVERY kernel of the re-sort chain inside the 32 registers per lane
 * that five step wavefronts leave on a SIMD (forecast_key_kernel, cs_hist, cs_binscan, cs_scatter, apply_kernel):
 * with the forecast key at 46 registers it queued behind the step wavefronts for half a millisecond per launch and the
 * headline LOST 6 %.  (Round 6 had forced five wavefronts on code that then spilled 9-14 registers into the time
 * loop, - 1.7 %: profiles/r06_lean_waves_per_simd.txt.)  A new value held across the time loop, or a chain kernel that
 * grows past 32 registers, undoes it. */
#define RS_DUO_LEAN_WAVES 5
#endif
__global__ void __launch_bounds__((SKY && SRC == SRC_RAW) ? 192 : 128, REPLAY ? 3 : FULL ? 4 : RS_DUO_LEAN_WAVES) step_kernel_duo(const StepArgs a) {
  /* (REPLAY at three waves per SIMD: with the rewind's code the instance spilled 50 registers at four) */
  static_assert(!CPL || SRC == SRC_RAW, "coupling in the two-wavefront flavour: the driver path's lock-step chunks");
  constexpr bool SKYG = SKY && SRC == SRC_RAW;
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  __shared__ DuoMailT<FULL ? PR_FULL : PR_LEAN> mail;
  __shared__ uint32_t skyfl[SKYG ? 2 * 64 : 1]; /* duo_sky's flags, [buffer][lane] */
  const MathTab mt = fill_math_tables(math_lds);
  __syncthreads();
  /* no early return: the wavefronts walk to every barrier, lanes beyond npoints are dead weight.
   * (Dealing the roles by the parity of the hardware wave slot or of the workgroup index, so that every
   * SIMD hosts both kinds, was measured: 1.08e10 and 1.13e10 against 1.12e10 with fixed roles at
   * 125 000 points - nothing to gain.) */
  if (a.wave_start && a.wave_cnt[blockIdx.x] == 0) return; /* a spare workgroup of the wave table: all wavefronts leave */
  if (threadIdx.x < 64) {
    if (a.surface_prio) __builtin_amdgcn_s_setprio(1); /* the longer chain of the two issues first (StepArgs::surface_prio) */
    duo_surface<NL, SCORE, FULL, SKY && !SKYG, SKYG, SRC == SRC_RAW, CPL, REPLAY>(mt, mail, a, skyfl);
  } else if (!SKYG || threadIdx.x < 128) {
    duo_ground<NL, SRC, FULL, SKYG, CPL, REPLAY>(mt, mail, a);
  } else {
    if constexpr (SKYG) duo_sky(mail, skyfl, a);
  }
}

/* FULL feature set + sky view in lock step, LDS profile (any NLayers). */
template <bool DIAG = false>
__global__ void __launch_bounds__(kBlock, 3) step_kernel_sky(const StepArgs a) {
  extern __shared__ double lds[]; /* [NLayers][kBlock] */
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  step_lanes<LdsProfile, true, true, true, false, false, false, DIAG>(a, math_lds, lds);
}

/* The same for NLayers = 15 with the hybrid profile at W waves per SIMD (rs_step_select.hpp). */
template <int W>
__global__ void __launch_bounds__(kBlock, W) step_kernel_sky_h(const StepArgs a) {
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  __shared__ double prof_lds[(15 - RS_HYBRID_REG) * kBlock];
  step_lanes<HybridProfile<15, RS_HYBRID_REG>, true, true>(a, math_lds, prof_lds);
}

/* FULL feature set + coupling in lock step (time_loop<CPL>): everything of a coupled run except
 * the replays.  LDS profile (any NLayers).  SKY: with the sky-view radiation of the points that have
 * one (src/ModRadiation.f90:7-73) - the forcing windows are read-only here, so what the reference
 * saves and restores of SW / SW_dir / LW around a window (src/Coupling.f90:204-208,249-253) is simply
 * the window as it stands.  (The history score of a parked lane is cheap.) */
template <bool SKY>
__global__ void __launch_bounds__(kBlock, 3) step_kernel_cpl(const StepArgs a) {
  extern __shared__ double lds[]; /* [NLayers][kBlock] */
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  step_lanes<LdsProfile, true, SKY, true, true>(a, math_lds, lds);
}

/* The same for NLayers = 15 with the hybrid profile at W waves per SIMD. */
template <int W, bool SKY = false>
__global__ void __launch_bounds__(kBlock, W) step_kernel_cpl_h(const StepArgs a) {
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  __shared__ double prof_lds[(15 - RS_HYBRID_REG) * kBlock];
  step_lanes<HybridProfile<15, RS_HYBRID_REG>, true, SKY, true, true>(a, math_lds, prof_lds);
}

/* One replay round in lock step over the compacted list (time_loop<REPLAY>): NLayers = 15 with the hybrid profile
 * at W waves per SIMD, ... */
template <int W, bool SKY = false>
__global__ void __launch_bounds__(kBlock, W) step_kernel_cpl_replay_h(const StepArgs a) {
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  __shared__ double prof_lds[(15 - RS_HYBRID_REG) * kBlock];
  step_lanes<HybridProfile<15, RS_HYBRID_REG>, true, SKY, false, true, true>(a, math_lds, prof_lds);
}

/* ... and with the LDS profile (any NLayers).  The one kernel that keeps its own copy of step_lanes<REPLAY>: through
 * the shared body the compiler spills two more VGPRs in step_kernel_cpl_replay<false> (23 -> 25, scratch 112 ->
 * 128 B; tools/compare_device_code.py), whatever form the replay loop takes there. */
template <bool SKY>
__global__ void __launch_bounds__(kBlock, 3) step_kernel_cpl_replay(const StepArgs a) {
  extern __shared__ double lds[]; /* [NLayers][kBlock] */
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  const MathTab mt = fill_math_tables(math_lds);
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= (int64_t)a.cpl_nlist) return;
  const int64_t p = (int64_t)a.cpl_list[g];
  if (a.cpl_prio) __builtin_amdgcn_s_setprio(2);
  LdsProfile T{lds + threadIdx.x, consts_of(&a).NLayers};
  Scalars s;
  int32_t score = 0;
  for (int32_t rnd = 0;; ++rnd) {
    load_state<true>(a.state, a.np_pad, p, T, s);
    time_loop<true, LdsProfile, SKY, false, true, true>(mt, T, s, score, (uint32_t)p);
    store_state<true>(a.state, a.np_pad, p, T, s);
    if (rnd + 1 >= a.cpl_inner) break;
    if ((((int32_t)a.state[(int64_t)RS_ST_CPL_FLAGS * a.np_pad + p]) & 1) == 0) break;
  }
}

/* Coupled variant: LDS profile (any NLayers), FULL feature set + coupling. */
template <bool DIAG = false>
__global__ void __launch_bounds__(kBlock, RS_CPL_WAVES) step_kernel_coupled(const StepArgs a) {
  extern __shared__ double lds[]; /* [NLayers][kBlock] */
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  const MathTab mt = fill_math_tables(math_lds);
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= (a.cpl_list ? (int64_t)a.cpl_nlist : a.npoints)) return;
  const int64_t p = a.cpl_list ? (int64_t)a.cpl_list[g] : g;
  if (a.cpl_prio) __builtin_amdgcn_s_setprio(2);
  const int NLc = consts_of(&a).NLayers;
  LdsProfile T{lds + threadIdx.x, NLc};
  Scalars s;
  Coupling q;
  load_state<true>(a.state, a.np_pad, p, T, s);
  load_coupling(a.state, a.np_pad, p, q);
  time_loop_coupled<LdsProfile, DIAG>(mt, T, s, q, a.state, a.np_pad, p);
  store_state<true, LdsProfile, true>(a.state, a.np_pad, p, T, s);
  store_coupling(a.state, a.np_pad, p, q);
}

/* Hourly knots of the synthetic workload, [knot][RS_KNOT_FIELDS][np_pad]. */
__global__ void __launch_bounds__(kBlock) synth_knots_kernel(const KnotArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.npoints) return;
  /* with a plan order (rs_hip_plan_order) slot p holds point order[p] */
  const int64_t gid = a.spec.point_offset + (a.spec.order ? (int64_t)a.spec.order[p] : p);
  /* one thread makes all the knots of its point: the 17 draws the knots share are hashed once */
  const RsSynthPoint pc = rs_sy_point(a.spec.seed, gid);
  for (int32_t y = 0; y < a.nknots; ++y) {
    const RsSynthKnot q = rs_sy_knot_of(&pc, a.spec.seed, gid, a.k0 + y, a.spec.start_hour);
    double *base = a.knots + ((int64_t)y * RS_KNOT_FIELDS) * a.np_pad + p;
    base[0 * a.np_pad] = q.tair;
    base[1 * a.np_pad] = q.tdew;
    base[2 * a.np_pad] = q.vz;
    base[3 * a.np_pad] = q.rhz;
    base[4 * a.np_pad] = q.prec;
    base[5 * a.np_pad] = q.sw;
    base[6 * a.np_pad] = q.lw;
    base[7 * a.np_pad] = q.tsurf0;
    base[8 * a.np_pad] = (double)q.phase;
  }
}

/* The knot buffers are the caller's (include/roadsurf.h): a knot may be -0.0, infinite or NaN, and two knots
 * may differ by anything.  rs_div_u is the IEEE quotient of secs * dv by the span only while that quotient is a
 * normal number and the numerator finite: for 1 <= secs < span <= 2^7 that is 2^-1015 <= |dv| < 2^1017 (derived
 * in tests/test_knot_reference.py: below, the quotient is subnormal and an exact tie rounds the other way; above,
 * secs * dv overflows and the remainder is inf - inf); dv = 0 gives +-0, which leaves every v0 but -0.0 as it
 * is.  An interval with anything else - a non-finite end makes dv non-finite - and every interval of a span
 * beyond 2^7 divides the IEEE way and takes the knot itself at secs = 0 (0 * inf is NaN), as raw_resolve decides it
 * for the raw series: once per interval. */
__device__ __forceinline__ bool knot_interval_fast(double v0, double dv) {
  const double ad = __builtin_fabs(dv);
  return (dv == 0.0 || (ad >= 0x1p-1015 && ad < 0x1p1017)) && !(v0 == 0.0 && __builtin_signbit(v0));
}
__device__ __forceinline__ double knot_value_ieee(double v0, double dv, int32_t r, double secs, double span) {
  return r == 0 ? v0 : v0 + (secs * dv) / span;
}

/* Knots -> step resolution, the device twin of the reference driver's
 * interpolation (examples/example1/src/JsonSource.cpp:115-172): linear between
 * knots, PrecPhase from the later knot.  One thread = one point over one knot
 * interval (blockIdx.y): the two knot rows are read once, then up to
 * steps_per_knot rows are streamed out, each a coalesced 2-KiB store per block
 * and field. */
/* TDEW/OBS/DEPTH: which optional streams the window has (the stores take the scalar row base + 32-bit lane
 * offset form, LaneOff; the tests inside the loop over the time indices are all uniform).  At r = 0 the interpolation adds +-0.0 to the knot value, which returns it
 * unchanged unless the knot is -0.0 - one of the intervals that divide the IEEE way (knot_interval_fast). */
/* (the optional streams - dew point, surface observation, output depth - are there or not for the whole launch:
 * uniform tests of the window's pointers; they were three template parameters, eight instances, until round 6) */
__global__ void __launch_bounds__(kBlock) expand_kernel(const ExpandArgs a) {
  const bool TDEW = a.f.tdew != nullptr, OBS = a.f.tsurfobs != nullptr, DEPTH = a.f.depth != nullptr;
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a block: all of it is waited for */
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.npoints) return;
  const int32_t k = a.kfirst + (int32_t)blockIdx.y;        /* knot interval [k, k+1) */
  int32_t tlo = k * a.spk, thi = tlo + a.spk;              /* 0-based time range */
  if (tlo < a.t0 - 1) tlo = a.t0 - 1;
  if (thi > a.t0 - 1 + a.nsteps) thi = a.t0 - 1 + a.nsteps;
  if (tlo >= thi) return;
  const int64_t kcol = a.gather ? (int64_t)a.gather[p] : p; /* knots kept in point order: gather */
  const double *ka = a.knots + ((int64_t)(k - a.k0) * RS_KNOT_FIELDS) * a.np_pad + kcol;
  const double *kb = ka + (int64_t)RS_KNOT_FIELDS * a.np_pad;
  const bool need_b = (thi - 1) > k * a.spk; /* some r > 0 in range */
  double v0[7], dv[7];
  /* rs_sy_lerp, k0 + (secs * (k1 - k0)) / span, with the difference taken once per interval and
   * the division by the uniform span as rs_div_u (rs_math.hpp: exact for a denominator whose
   * reciprocal is correctly rounded) where every lane's interval allows it (knot_interval_fast) */
  bool fast = true;
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    v0[q] = ka[(int64_t)q * a.np_pad];
    const double v1 = need_b ? kb[(int64_t)q * a.np_pad] : v0[q];
    dv[q] = v1 - v0[q];
    fast = fast && knot_interval_fast(v0[q], dv[q]);
  }
  const bool ieee = a.spk > 128 || __builtin_amdgcn_ballot_w64(!fast) != 0ull; /* uniform per wavefront */
  const double ts0 = ka[7 * a.np_pad];
  const int32_t ph0 = (int32_t)ka[8 * a.np_pad];
  const int32_t ph1 = need_b ? (int32_t)kb[8 * a.np_pad] : ph0;
  const double span = (double)a.spk;
  const int64_t col0 = (int64_t)blockIdx.x * kBlock; /* the workgroup's first column: uniform */
  for (int32_t t = tlo; t < thi; ++t) {
    const int32_t r = t - k * a.spk;
    const double secs = (double)r;
    const int64_t row = (int64_t)(t - (a.t0 - 1)) * a.f.t_stride + col0;
    const LaneOff L(threadIdx.x);
    double v[7];
    if (!ieee) { /* uniform, and the same for every index of the interval */
#pragma unroll
      for (int q = 0; q < 7; ++q) v[q] = v0[q] + rs_div_u(secs * dv[q], span, a.r_spk);
    } else {
#pragma unroll
      for (int q = 0; q < 7; ++q) v[q] = knot_value_ieee(v0[q], dv[q], r, secs, span);
    }
    L.st((double *)a.f.tair + row, v[0]);
    if (TDEW) L.st((double *)a.f.tdew + row, v[1]);
    L.st((double *)a.f.vz + row, v[2]);
    L.st((double *)a.f.rhz + row, v[3]);
    L.st((double *)a.f.prec + row, v[4]);
    L.st((double *)a.f.sw + row, v[5]);
    L.st((double *)a.f.lw + row, v[6]);
    if (OBS) L.st((double *)a.f.tsurfobs + row, (t == 0) ? ts0 : -9999.9);
    if (DEPTH) L.st((double *)a.f.depth + row, -9999.9);
    L.st((int32_t *)a.f.precphase + row, (r == 0) ? ph0 : ph1);
  }
  if (p == 0 && !a.f.hour_pstride)
    for (int32_t t = tlo; t < thi; ++t)
      ((int32_t *)a.f.hour)[t - (a.t0 - 1)] = rs_sy_hour(t + 1, a.spk, a.start_hour);
}

/* Unit-test kernel for rs_math.hpp (tests/test_hip_math.py). fn: 0 exp, 1 log, 2 the bare division
 * x[i] / x[n + i], 3 the bare square root. */
__global__ void __launch_bounds__(kBlock) math_test_kernel(int fn, int64_t n, const double *x,
                                                           double *y) {
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  const MathTab mt = fill_math_tables(math_lds);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (fn == 2) y[i] = rs_div(x[i], x[n + i]);
  else if (fn == 3) y[i] = rs_sqrt(x[i]);
  else y[i] = fn == 0 ? rs_exp(mt, x[i]) : rs_log(mt, x[i]);
}

/* Tdew <-> RH completion of a raw series, examples/example1/src/JsonSource.cpp:288-295 with
 * CalcTdewOrRH of MeteorologyTools.cpp:12-51.  C++ source: the literals are true doubles here
 * (unlike the Fortran side's REAL(4) ones).  exp/log are the glibc-exact ones; the divisions
 * are the compiler's IEEE expansion (denominators can approach 0 on the RH branch). */
__device__ __forceinline__ double calc_tdew_or_rh(const MathTab &mt, double t, double tdew,
                                                  double rh) {
  const double Alphaw = 17.269, Alphai = 21.875, Betaw = 237.3, Betai = 265.5, AFact = 0.61078;
  const double Alpha = (t >= 0.0) ? Alphaw : Alphai;
  const double Beta = (t >= 0.0) ? Betaw : Betai;
  const double EsatT = AFact * rs_exp(mt, Alpha * t / (t + Beta));
  if (!(tdew != tdew) && tdew > -1000) {
    const double EsatTD = AFact * rs_exp(mt, Alpha * tdew / (tdew + Beta));
    const double x = (EsatTD / EsatT) * 100.0;
    return (100.0 < x) ? 100.0 : x; /* std::min(x, 100.0) */
  }
  if (!(rh != rh) && rh > -1) {
    const double Epr = 0.01 * rh * EsatT;
    const double XX = rs_log(mt, Epr / AFact);
    return Beta * XX / (Alpha - XX);
  }
  return __builtin_nan("");
}

__global__ void __launch_bounds__(kBlock) humidity_fill_kernel(const double *__restrict__ tair,
                                                               double *tdew, double *rhz,
                                                               int64_t n) {
  __shared__ double math_lds[RS_MATH_LDS_DOUBLES];
  const MathTab mt = fill_math_tables(math_lds);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double t = tair[i];
  double td = tdew[i], rh = rhz[i];
  if (td < -100 && rh > -100 && t > -100) td = calc_tdew_or_rh(mt, t, -9999.9, rh);
  if (rh < -100 && td > -100 && t > -100) rh = calc_tdew_or_rh(mt, t, td, -9999.9);
  tdew[i] = td;
  rhz[i] = rh;
}

__global__ void __launch_bounds__(kBlock) count_failed_kernel(const double *st, int64_t np_pad,
                                                              int64_t npoints,
                                                              unsigned long long *out) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool bad = p < npoints && st[(int64_t)RS_ST_FAILED * np_pad + p] != 0.0;
  const unsigned long long m = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(out, (unsigned long long)__popcll(m));
}

/* Engine clock as the shader sees it: one wavefront reads the shader-clock counter (s_memtime) and
 * the constant 100 MHz counter (s_memrealtime) `spin_us` apart; out[0..1] = the two deltas.  Enqueued
 * beside the step kernels, it measures the clock the chip holds UNDER that load (bench.py). */
__global__ void __launch_bounds__(64) clock_probe_kernel(uint64_t *out, uint32_t spin_us) {
  const uint64_t c0 = __builtin_readcyclecounter();
  const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  uint64_t r1 = r0;
  /* bounded: at most RS_CLOCK_PROBE_MAX_US (the launcher clamps spin_us) and at most 1 << 16 naps of
   * ~0.9 us - on a part whose real-time counter stands still the wave leaves with out[1] = 0, which
   * bench.py reads as "clock not readable" */
  bool ok = false;
  for (int it = 0; it < (1 << 16); ++it) {
    if (r1 - r0 >= (uint64_t)spin_us * 100ull) {
      ok = true;
      break;
    }
    __builtin_amdgcn_s_sleep(32);
    r1 = __builtin_amdgcn_s_memrealtime();
  }
  const uint64_t c1 = __builtin_readcyclecounter();
  if (threadIdx.x == 0) {
    out[0] = c1 - c0;
    out[1] = ok ? r1 - r0 : 0;
  }
}

/* Coupling windows of the points that ask for a replay (start_coupling_again): out[0] = min
 * couplingStartI, out[1] = max couplingEndI (initialised by the caller to INT_MAX / 0).  What
 * rs_hip_cpl_replay checks the caller's window against. */
__global__ void __launch_bounds__(kBlock) cpl_window_bounds_kernel(const StepArgs a, int32_t *out) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.npoints) return;
  const ConstsAS &c = consts_of(&a);
  if ((((int32_t)a.state[(int64_t)RS_ST_CPL_FLAGS * a.np_pad + p]) & 1) == 0) return;
  /* (cpl_window's rule, kept in this form: see there) */
  const int32_t cidx = a.pp.coupling_index[p];
  if (a.pp.coupling_tsurf[p] < -100 || cidx < 1) return;
  const int32_t cs = ((double)cidx <= c.cplLenR) ? 1 : cidx - c.cplLenI;
  atomicMin(&out[0], cs);
  atomicMax(&out[1], cidx);
}

/* Sort key of rs_hip_recluster_forecast (include/roadsurf.h): CalcBLCondAndLE's fixed point
 * (src/BoundaryLayer.f90:64-96) run at the preview times of the NEXT window, with the carried
 * surface temperature moved along with the air temperature.  A predictor: single precision,
 * hardware reciprocal/sqrt/log - it only orders the slots, no model value depends on it. */
__global__ void __launch_bounds__(kBlock) forecast_key_kernel(const ForecastArgs a) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a plan: little work, all of it waited for */
  /* (the slot and the preview column are 32-bit values - the slots are, rs_cluster.hip - and the carried surface
   * temperature and the air temperature of `now` are read again at every preview instead of being held across the
   * loops: registers, see the scheduling barrier below) */
  const uint32_t s = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if ((int64_t)s >= a.npoints) return;
  const ConstsAS &c = consts_of(&a);
  const int64_t np = a.np_pad;
  auto st_at = [&](int row, uint32_t slot) -> double {
    return a.f32 ? (double)((const float *)a.state)[(int64_t)row * np + slot]
                 : ((const double *)a.state)[(int64_t)row * np + slot];
  };
  auto st = [&](int row) -> double { return st_at(row, s); };
  const uint32_t pq = a.pv.index ? (uint32_t)a.pv.index[s] : s; /* preview rows in point order */
  auto preview_at = [&](const double *const *row, const double *const *row_b, int q, uint32_t col) -> double {
    const double v = row[q][col];
    return row_b[q] ? v + a.pv.w[q] * (row_b[q][col] - v) : v; /* RsPreview::tair_b: between two rows */
  };
  auto preview = [&](const double *const *row, const double *const *row_b, int q) -> double {
    return preview_at(row, row_b, q, pq);
  };
  const double stab_num = -c.VK_Const * c.ZRefT * c.Grav;
  int32_t unst = 0, farc = 0, extra = 0, maxtrip = 5;
  float stab_lo = 2.f, stab_hi = -2.f; /* the converged stability parameter of the previews, after its clamp */
  for (int q = 0; q < a.pv.n; ++q) {
    const double ta = preview(a.pv.tair, a.pv.tair_b, q);
    double vz = preview(a.pv.vz, a.pv.vz_b, q);
    const double hour = (double)a.pv.hour[q];
    const double calm = (hour >= c.NightOn || hour <= c.NightOff) ? c.CalmLimNgt : c.CalmLimDay;
    if (vz < calm) vz = calm;
    uint32_t sl = s, pl = pq; /* (opaque copies: the two loads stay inside the loop) */
    asm volatile("" : "+v"(sl), "+v"(pl));
    const double ts_now = st_at(RS_ST_TSURF, sl);
    const double ta_now = a.pv.tair_now ? a.pv.tair_now[pl] : preview_at(a.pv.tair, a.pv.tair_b, 0, pl);
    const double ts = ts_now + a.pv.alpha * (ta - ta_now);
    const double TaK = ta + R4(273.15);
    const double dens = R4(100000.0) / (R4(287.05) * TaK);
    /* (one IEEE division after the other: interleaved by the scheduler the two expansions held 40 registers, and
     * the kernel has to fit in the 32 that five step wavefronts leave on a SIMD) */
    __builtin_amdgcn_sched_barrier(0);
    const double hcap = R4(1005.0) + (TaK - R4(250.0)) * (TaK - R4(250.0)) / R4(3364.);
    const double avc = hcap * dens;
    /* the iteration itself in single precision with the hardware's reciprocal, square root and
     * logarithm: a predictor needs the regime and the pass count, not the last bit (the exit test
     * is 1e-3 on a conductance of order 1..50) */
    const float dT = (float)(ts - ta), den0 = (float)(avc * TaK), vkvz = (float)(c.VK_Const * vz),
                avk = (float)(avc * c.VK_Const), snum = (float)stab_num, lU = (float)c.logUstar,
                lC = (float)c.logCond;
    float psim = 0.f, psih = 0.f, bl = 0.f, stab_last = 0.f;
    int32_t nnear = 0, nfar = 0, j = 1;
#pragma nounroll /* (unrolled by two it carried six registers more) */
    for (; j <= RS_BL_MAXIT; ++j) {
      const float old = bl;
      const float us = vkvz * __builtin_amdgcn_rcpf(lU + psim);
      bl = avk * us * __builtin_amdgcn_rcpf(lC + psih);
      float stab = snum * bl * dT * __builtin_amdgcn_rcpf(den0 * (us * us * us));
      if (stab > 1.f) stab = 1.f;
      stab_last = stab;
      if (stab > 0.f) {
        psih = 4.7f * stab;
        psim = psih;
      } else {
        const float arg = (1.f + __builtin_amdgcn_sqrtf(1.f - 16.f * stab)) * 0.5f;
        /* glibc's log takes its polynomial path for 1 - 2^-4 <= x < 1 + 0x1.09p-4, the table
         * path otherwise (rs_math.hpp): a wavefront with both kinds of lanes pays for both */
        if (arg < 1.064453125f) ++nnear; else ++nfar;
        psih = -2.f * __logf(arg);
        psim = 0.6f * psih;
      }
      if (j >= 5 && __builtin_fabsf(bl - old) < 0.001f) break;
    }
    if (j > RS_BL_MAXIT) j = RS_BL_MAXIT;
    extra += j - 5;
    maxtrip = j > maxtrip ? j : maxtrip;
    stab_lo = stab_last < stab_lo ? stab_last : stab_lo;
    stab_hi = stab_last > stab_hi ? stab_last : stab_hi;
    if (nnear + nfar > 0) {
      ++unst;
      if (nfar >= nnear) ++farc;
    }
  }
  /* Field 0 in classes (ForecastArgs::extra_log): the LONGEST loop the point is expected to run in the window.
   * The loop's slow band is a narrow curve in the stable regime (Tsurf - Tair about -2.6 VZ^2 for the default
   * heights: the fixed point's slope goes through 1 there, 20-39 passes; profiles/r05_wave_stats.txt: 0.2 % of
   * the lane-steps, but a wavefront runs as many passes as its slowest lane).  On one side of it the stability
   * parameter sits at its clamp (PSI = 4.7, two passes and it stands), on the other below: a point whose
   * previews lie on both sides passes through the band inside the window ... */
  if (a.extra_log && stab_hi >= 1.f && stab_lo < 1.f) maxtrip = 31;
  /* (the storages are read here, behind the previews: nothing of them is held across the loops above) */
  const bool has_snow = st(RS_ST_SNOW) > 0.0, has_ice = st(RS_ST_ICE) > 0.0 || st(RS_ST_ICE2) > 0.0,
             has_wet = st(RS_ST_WAT) > 0.0 || st(RS_ST_DEP) > 0.0;
  const int32_t cover = (has_snow || has_ice || has_wet) ? 1 : 0;
  /* which storage branches the point will take (src/Storage.f90): snow is the longest chain */
  const int32_t sclass = has_snow ? 3 : has_ice ? 2 : has_wet ? 1 : 0;
  if (a.extra_log) { /* ... and the pass count of the last index stepped is one more preview (the two-wavefront
                        flavour without the history score leaves it in the score's slot; other flavours leave 0
                        or a score there: ignored unless 5..RS_BL_MAXIT) */
    const double last = st(RS_ST_BLSCORE);
    if (last >= 5.0 && last <= (double)RS_BL_MAXIT) {
      const int32_t lt = (int32_t)last;
      maxtrip = lt > maxtrip ? lt : maxtrip;
    }
  }
  if (extra > 4095) extra = 4095;
  /* field 9, the ground digit: which layers are frozen.  The heat capacity of a layer is a constant below
   * 0 C and two polynomials above (src/BalanceModel.f90:215-236), and a wavefront whose 64 points all have
   * layer j frozen takes that layer's capDZ from a table (layer_step, rs_physics_body.inc).  The frozen
   * layers of a point are nearly always one run: 4 bits for its deepest layer, 3 for the thawed layers on
   * top of it (the daily thaw reaches a handful of the thin upper layers).  Sorted as a digit of its own BELOW the others (rs_cluster_count_sort, low_bits): the
   * classes of the boundary-layer fields stay as they are, their points line up by frost depth. */
  uint32_t ground = 0u;
  {
    if (a.mode_ground) {
      const int NL = c.NLayers;
      int32_t deepest = 0, first = 0;
      for (int j = NL; j >= 1; --j)
        if (st(RS_ST_TMP0 + j - 1) < 0.0) {
          if (!deepest) deepest = j;
          first = j;
        }
      if (NL > 15) deepest = (deepest * 15) / NL;
      const int32_t top = first > 0 ? first - 1 : 0;
      ground = ((uint32_t)deepest << 3) | (uint32_t)(top > 7 ? 7 : top);
    }
  }
  /* key fields, most significant first, named by the decimal digits of `mode`:
   * 1 unstable previews (4 bits), 2 of which on the table path of log (4 bits), 3 cover (1 bit),
   * 4 predicted extra passes (12 bits), 5 storage class snow > ice > wet > bare (2 bits).  Modes 0..3 are shorthands for 14, 124, 134, 1234. */
  uint32_t key = 0;
  int bits = 0;
  for (int t = a.mode_ndigits - 1; t >= 0; --t) { /* (the digits come from the host: ForecastArgs::mode_digits) */
    const int d = (int)((a.mode_digits >> (4 * t)) & 15u);
    if (d == 1) { key = (key << 4) | (uint32_t)unst; bits += 4; }
    else if (d == 2) { key = (key << 4) | (uint32_t)farc; bits += 4; }
    else if (d == 3) { key = (key << 1) | (uint32_t)cover; bits += 1; }
    else if (d == 4) { key = (key << 12) | (uint32_t)extra; bits += 12; }
    else if (d == 5) { key = (key << 2) | (uint32_t)sclass; bits += 2; }
    /* compact forms: extra passes saturating at 31 (5 bits), the two preview counts at 3 (2 bits) */
    else if (d == 6) { key = (key << 5) | (uint32_t)(extra > 31 ? 31 : extra); bits += 5; }
    else if (d == 0) { /* (inside a list) extra passes saturating at 7, or the longest preview in classes */
      const int32_t t = maxtrip;
      const uint32_t cls = (uint32_t)(t <= 8 ? t - 5 : t <= 12 ? 4 : t <= 20 ? 5 : t <= 30 ? 6 : 7);
      key = (key << 3) | (a.extra_log ? cls : (uint32_t)(extra > 7 ? 7 : extra));
      bits += 3;
    }
    /* (more than three previews: the counts scaled to 0..3) */
    else if (d == 7) { key = (key << 2) | (uint32_t)(a.pv.n > 3 ? (unst * 3 + a.pv.n / 2) / a.pv.n : unst > 3 ? 3 : unst); bits += 2; }
    else if (d == 8) { key = (key << 2) | (uint32_t)(a.pv.n > 3 ? (farc * 3 + a.pv.n / 2) / a.pv.n : farc > 3 ? 3 : farc); bits += 2; }
  }
  /* RsPreview::prec (ABI 8): the most significant bit - some preview has precipitation.  Points with
   * precipitation are a few per cent of a batch at any time, but in an order that ignores it they sit in four
   * wavefronts out of five, and every such wavefront runs PrecipitationToStorage / CalcPrecType (the logistic
   * exp where the phase is missing) for all of its lanes; gathered, they fill one wavefront in thirty. */
  if (a.pv.prec[0]) {
    uint32_t wet = 0u;
    for (int q = 0; q < RS_PREVIEW_MAX; ++q)
      if (a.pv.prec[q] && a.pv.prec[q][pq] > 0.0) wet = 1u;
    key |= wet << bits;
    bits += 1;
  }
  /* descending: the expensive points get the low slots (longest job first, rs_cluster.hip) */
  if (a.compact) { /* right-aligned in its own bits: the plan's counting sort */
    const int low = a.low_bits; /* the ground digit below them, if the mode has one */
    a.keys[s] = ((((1u << bits) - 1u) - key) << low) | (low ? ground : 0u);
  } else if (a.low_bits && bits + a.low_bits <= RS_SORT_KEY_BITS) { /* the same order from the library sort */
    const int low = a.low_bits;
    a.keys[s] = (((((1u << bits) - 1u) - key) << low) | ground) << (RS_SORT_KEY_BITS - bits - low);
  } else {
    if (bits < RS_SORT_KEY_BITS) key <<= (RS_SORT_KEY_BITS - bits); /* left-aligned in the sorted bits */
    else key >>= (bits - RS_SORT_KEY_BITS);
    a.keys[s] = ((1u << RS_SORT_KEY_BITS) - 1u) - key;
  }
  a.slots[s] = (uint32_t)s;
}

}  // namespace rs

/* ---- launchers (host) --------------------------------------------------- */

static inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + RS_BLOCK - 1) / RS_BLOCK)); }

hipError_t rs_read_div_mismatch(unsigned long long *out /*[3]*/, hipStream_t stream) {
  hipError_t e = hipMemcpyFromSymbolAsync(out, HIP_SYMBOL(rs::g_div_mismatch), 3 * sizeof(*out), 0,
                                          hipMemcpyDeviceToHost, stream);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(stream);
}

hipError_t rs_read_bl_stats(unsigned long long *out /*[RS_BL_NSTATS]*/, hipStream_t stream) {
  hipError_t e = hipMemcpyFromSymbolAsync(out, HIP_SYMBOL(rs::g_bl_stats), RS_BL_NSTATS * sizeof(*out), 0,
                                          hipMemcpyDeviceToHost, stream);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(stream);
}

hipError_t rs_read_div_samples(double *out /*[64][4]*/, hipStream_t stream) {
  hipError_t e = hipMemcpyFromSymbolAsync(out, HIP_SYMBOL(rs::g_div_samples), 64 * 4 * sizeof(double), 0,
                                          hipMemcpyDeviceToHost, stream);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(stream);
}

hipError_t rs_launch_math_test(int fn, int64_t n, const double *x, double *y, hipStream_t stream) {
  hipLaunchKernelGGL(rs::math_test_kernel, grid_for(n), dim3(RS_BLOCK), 0, stream, fn, n, x, y);
  return hipGetLastError();
}

hipError_t rs_launch_humidity_fill(const double *tair, double *tdew, double *rhz, int64_t n,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(rs::humidity_fill_kernel, grid_for(n), dim3(RS_BLOCK), 0, stream, tair, tdew,
                     rhz, n);
  return hipGetLastError();
}

hipError_t rs_upload_math_tables(hipStream_t stream) {
  hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(rs::c_gl_exp_tab), rs_gl_exp_tab,
                                        sizeof(rs_gl_exp_tab), 0, hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) return e;
  return hipMemcpyToSymbolAsync(HIP_SYMBOL(rs::c_gl_log_tab), rs_gl_log_tab, sizeof(rs_gl_log_tab), 0,
                                hipMemcpyHostToDevice, stream);
}

int rs_forecast_key_low_bits(int32_t m) {
  for (; m > 0; m /= 10)
    if (m % 10 == 9) return 7;
  return 0;
}

/* the same field widths as forecast_key_kernel */
int rs_forecast_key_bits(int32_t m) {
  m = (m == 0) ? 14 : (m == 1) ? 124 : (m == 2) ? 134 : (m == 3) ? 1234 : m;
  int bits = 0;
  for (; m > 0; m /= 10) {
    const int d = m % 10;
    bits += d == 1 ? 4 : d == 2 ? 4 : d == 3 ? 1 : d == 4 ? 12 : d == 5 ? 2 : d == 6 ? 5 : d == 7 ? 2 : d == 8 ? 2 : d == 0 ? 3 : 0;
  }
  return bits;
}

hipError_t rs_launch_forecast_keys(const rs::ForecastArgs &a_, hipStream_t stream) {
  rs::ForecastArgs a = a_;
  { /* the mode's digits, as forecast_key_kernel used to take them apart itself */
    int32_t m = a.pv.mode;
    a.mode_ground = 0;
    for (int32_t m9 = m; m9 > 0; m9 /= 10) a.mode_ground |= (m9 % 10) == 9;
    m = (m == 0) ? 14 : (m == 1) ? 124 : (m == 2) ? 134 : (m == 3) ? 1234 : m;
    a.mode_digits = 0;
    a.mode_ndigits = 0;
    for (; m > 0; m /= 10) { /* (a negative mode has no digit that names a field: no field, as before) */
      a.mode_digits |= (uint64_t)(m % 10) << (4 * a.mode_ndigits);
      ++a.mode_ndigits;
    }
  }
  hipLaunchKernelGGL(rs::forecast_key_kernel, grid_for(a.npoints), dim3(RS_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t rs_launch_step(const rs::StepArgs &a, const rs::StepLaunch &l, hipStream_t stream) {
  switch (l.kernel) {
#define RS_STEP_CASE(id, ...) \
  case rs::StepKernel::id: hipLaunchKernelGGL((__VA_ARGS__), dim3(l.grid), dim3(l.block), l.lds, stream, a); break;
    RS_STEP_KERNELS_F64(RS_STEP_CASE)
#undef RS_STEP_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t rs_launch_init(const rs::InitArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(rs::init_kernel, grid_for(a.npoints), dim3(RS_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t rs_launch_knots(const rs::KnotArgs &a, int32_t nknots, hipStream_t stream) {
  rs::KnotArgs b = a;
  b.nknots = nknots;
  hipLaunchKernelGGL(rs::synth_knots_kernel, grid_for(a.npoints), dim3(RS_BLOCK), 0, stream, b);
  return hipGetLastError();
}

hipError_t rs_launch_expand(const rs::ExpandArgs &a, int32_t nintervals, hipStream_t stream) {
  dim3 g = grid_for(a.npoints);
  g.y = (unsigned)nintervals;
  hipLaunchKernelGGL(rs::expand_kernel, g, dim3(RS_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t rs_launch_clock_probe(uint64_t *out, uint32_t spin_us, hipStream_t stream) {
  if (spin_us > RS_CLOCK_PROBE_MAX_US) spin_us = RS_CLOCK_PROBE_MAX_US; /* a probe, not a way to park a wave */
  hipLaunchKernelGGL(rs::clock_probe_kernel, dim3(1), dim3(64), 0, stream, out, spin_us);
  return hipGetLastError();
}

hipError_t rs_launch_cpl_window_bounds(const rs::StepArgs &a, int32_t *out, hipStream_t stream) {
  hipLaunchKernelGGL(rs::cpl_window_bounds_kernel, grid_for(a.npoints), dim3(RS_BLOCK), 0, stream, a, out);
  return hipGetLastError();
}

hipError_t rs_launch_count_failed(const double *st, int64_t np_pad, int64_t npoints,
                                  unsigned long long *out, hipStream_t stream) {
  hipLaunchKernelGGL(rs::count_failed_kernel, grid_for(npoints), dim3(RS_BLOCK), 0, stream, st,
                     np_pad, npoints, out);
  return hipGetLastError();
}
