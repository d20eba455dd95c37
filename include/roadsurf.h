/*
 * roadsurf.h — C-ABI of the MI355X-native RoadSurf hot path.
 *
 * Everything here is plain C: pointers, sizes, PODs.  No torch types, no C++.
 * Citations are file:line into the reference tree (fmidev/RoadSurf v1.6.1).
 *
 * Three layers, bottom up:
 *   1. rs_hip_*   device-resident SoA API (HIP kernels, streams).  This is what
 *                 the Fortran host orchestration binds through ISO_C_BINDING
 *                 and what bench.py drives through ctypes.
 *   2. rs_host_*  host-array convenience entry (pack -> H2D -> kernels -> D2H),
 *                 used by the Fortran `runsimulation_batch`.
 *   3. runsimulation / runsimulation_batch   the reference's own BIND(C) entry
 *                 (examples/example1/src/Simulation.f90:4-6, declared on the
 *                 C++ side at examples/example1/src/roadrunner.cpp:22-29) and
 *                 its batched extension.  Implemented in Fortran
 *                 (roadsurf_amd/fortran/RoadSurfHip.f90) on top of layers 1-2.
 */
#ifndef ROADSURF_H
#define ROADSURF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * The five Bind(C) structs of the reference boundary, byte-identical.
 * ---------------------------------------------------------------------- */

/* src/InputPointers.f90.inc:4-27 == examples/example1/src/InputPointers.h:7-30
 * sizeof == 160.  The reference declares the arrays `const` but mutates VZ[0]
 * (src/Initialization.f90:121-123) and SW_dir[i] (src/InputOutput.f90:75-77);
 * so do we, hence no const here. */
typedef struct InputPointers {
  int32_t inputLen;
  double *c_tair;
  double *c_tdew;
  double *c_VZ;
  double *c_Rhz;
  double *c_prec;
  double *c_SW;
  double *c_LW;
  double *c_SW_dir;
  double *c_LW_net;
  double *c_TSurfObs;
  int32_t *c_PrecPhase;
  double *c_local_horizons; /* [360] */
  double *c_Depth;
  int32_t *c_year;
  int32_t *c_month;
  int32_t *c_day;
  int32_t *c_hour;
  int32_t *c_minute;
  int32_t *c_second;
} InputPointers;

/* src/OutputPointers.f90.inc:4-17 == examples/example1/src/OutputPointers.h:5-16
 * sizeof == 56 */
typedef struct OutputPointers {
  int32_t outputLen;
  double *c_TsurfOut;
  double *c_SnowOut;
  double *c_WaterOut;
  double *c_IceOut;
  double *c_DepositOut;
  double *c_Ice2Out;
} OutputPointers;

/* Fortran view: src/InputSettings.f90.inc:4-18.  The C++ struct
 * (examples/example1/src/InputSettings.h:13-26) has no force_tsurf member; the
 * Fortran side reads the padding at offset 12.  We expose the Fortran view
 * (the one that is actually read) and keep the C++ tail out of it. */
typedef struct InputSettings {
  int32_t SimLen;
  int32_t use_coupling;
  int32_t use_relaxation;
  int32_t force_tsurf;
  double DTSecs;
  double tsurfOutputDepth;
  int32_t NLayers;
  int32_t coupling_minutes;
  double couplingEffectReduction;
  int32_t outputStep;
} InputSettings;

/* src/InputParameters.f90.inc:4-91 == examples/example1/src/InputParameters.h:18-110
 * 69 consecutive doubles (552 B). */
typedef struct InputParameters {
  double NightOn, NightOff, CalmLimDay, CalmLimNgt, TrfFricNgt, TrFfricDay;
  double Grav, SB_Const, VK_Const, LVap, LFus, WatDens, SnowDens, IceDens,
      DepDens, WatMHeat, PorEvaF;
  double ZRefW, ZRefT, ZeroDisp, ZMom, ZHeat, Emiss, Albedo,
      Albedo_surroundings, MaxPormms, TClimG, DampDpth, Omega, AZ, DampWearF,
      AlbDry, AlbSnow, vsh1, vsh2, Poro1, Poro2, RhoB1, RhoB2, Silt1, Silt2;
  double freezing_limit_normal, snow_melting_limit_normal,
      ice_melting_limit_normal, frost_melting_limit_normal,
      frost_formation_limit_normal, T4Melt_normal;
  double TLimColdH, TLimColdL, WetSnowFormR, WetSnowMeltR;
  double PLimSnow, PLimRain, MaxSnowmms, MaxDepmms, MaxIcemms, MaxExtmms;
  double MissValI, MissValR;
  double Snow2IceFac;
  double MinPrecmm, MinWatmms, MinSnowmms;
  double MaxWatmms;
  double WDampLim, WWetLim;
  double WWearLim;
  double MinDepmms, MinIcemms;
} InputParameters;

/* src/LocalParameters.f90.inc:4-15 == examples/example1/src/LocalParameters.h:17-25
 * sizeof == 72 */
typedef struct LocalParameters {
  double tair_relax;
  double VZ_relax;
  double RH_relax;
  int32_t couplingIndexI;
  double couplingTsurf;
  double lat;
  double lon;
  double sky_view;
  int32_t InitLenI;
} LocalParameters;

/* Fill *p with the reference defaults (examples/example1/src/InputParameters.h:18-94)
 * and the DTSecs-derived limits (examples/example1/src/InputParameters.cpp:13-21). */
void rs_default_parameters(InputParameters *p, double DTSecs);
/* examples/example1/src/InputSettings.h:13-23 defaults, force_tsurf = 0. */
void rs_default_settings(InputSettings *s, int32_t SimLen);
/* examples/example1/src/LocalParameters.h:17-25 defaults. */
void rs_default_local(LocalParameters *l);

/* ------------------------------------------------------------------------
 * Layer 3: the reference entry point and its batched extension (Fortran).
 * ---------------------------------------------------------------------- */

/* Drop-in for examples/example1/src/Simulation.f90:4-117.  One point, whole
 * time series, synchronous, no return value; failure leaves -9999.0 in the
 * unwritten outputs (src/Initialization.f90:404-411).  Runs on the GPU. */
void runsimulation(OutputPointers *outPointers, const InputPointers *inPointers,
                   const InputSettings *inSettings,
                   const InputParameters *inputParam,
                   const LocalParameters *localParam);

/* Callers of runsimulation on several threads at once (the reference driver's worker pool,
 * examples/example1/src/roadrunner.cpp:454-497): with the environment variable
 * ROADSURF_HIP_COALESCE_US = w > 0 their points are gathered - the first caller waits up to w
 * microseconds (or for ROADSURF_HIP_COALESCE_MAX callers, default 4096) and runs everything queued with
 * its settings and parameters as ONE batch; the others sleep until their point is done.  Same bits as
 * calls of their own.  rs_coalesce_run is what runsimulation calls (returns the batch status),
 * rs_coalesce_stats the batches run and points served so far. */
int32_t rs_coalesce_run(OutputPointers *outPointers, const InputPointers *inPointers,
                        const InputSettings *inSettings, const InputParameters *inputParam,
                        const LocalParameters *localParam);
void rs_coalesce_stats(int64_t *batches, int64_t *points);
/* What rs_coalesce_run hands its gathered points to: runsimulation_batch with the reference's in-place input
 * edits written back by default (below).  Exported for that caller only. */
void rs_runsimulation_gathered(int32_t n, OutputPointers *outPointers, const InputPointers *inPointers,
                               const InputSettings *inSettings, const InputParameters *inputParam,
                               const LocalParameters *localParam, int32_t *status);

/* Extension: n independent points with shared settings/parameters, one
 * OutputPointers/InputPointers/LocalParameters per point (exactly what the
 * reference driver builds per point, examples/example1/src/roadrunner.cpp:404-406).
 * status: 0 ok, <0 error (rs_last_error() has the text). */
void runsimulation_batch(int32_t n, OutputPointers *outPointers,
                         const InputPointers *inPointers,
                         const InputSettings *inSettings,
                         const InputParameters *inputParam,
                         const LocalParameters *localParam, int32_t *status);
/* Same, plus what the reference only prints: first_failed[n] (or NULL) receives per point 0, or the
 * 1-based time index at which CheckValues failed it ("BAD input value!" / "Abnormal surface
 * temperature", src/InputOutput.f90:63-65,80-81); outputs after that index read -9999.0.
 * In-place edits of the INPUT arrays (Ownership): the reference clamps SW_dir to SW at
 * every checked index (src/InputOutput.f90:75-77) and, with sky view, rewrites SW / SW_dir / LW
 * (src/ModRadiation.f90:57-71) in the CALLER's arrays.  Who writes them back:
 *   runsimulation                      by default (it is the reference's entry and leaves the caller's
 *                                      arrays as the reference does); ROADSURF_HIP_WRITEBACK=0 opts out
 *   runsimulation_batch / _batch_ex    only with ROADSURF_HIP_WRITEBACK=1: three more arrays per point
 *                                      back over PCIe, which a batch caller rarely reads
 * The VZ(1) >= 0.4 edit of src/Initialization.f90:121-123 is always written, by every entry. */
void runsimulation_batch_ex(int32_t n, OutputPointers *outPointers,
                            const InputPointers *inPointers,
                            const InputSettings *inSettings,
                            const InputParameters *inputParam,
                            const LocalParameters *localParam, int32_t *status,
                            int32_t *first_failed);

/* ------------------------------------------------------------------------
 * Model constants: everything that is uniform over points once settings and
 * parameters are shared.  Built on the HOST by Fortran (same compiler, same
 * REAL(4)-literal semantics as the reference's init code) and uploaded once.
 * Restates src/Initialization.f90:181-235,310-358,479-557,
 * src/BalanceModel.f90:132-186,254-279 and the REAL(4) folds of
 * src/Cond.f90:78-102.
 * ---------------------------------------------------------------------- */
#define RS_MAX_LAYERS 32

typedef struct RsConstants {
  int32_t NLayers;
  int32_t SimLen;
  int32_t use_relaxation;
  int32_t force_tsurf;
  int32_t use_coupling;    /* settings%use_coupling; per point it is switched off without a
                              usable observation (src/InputOutput.f90:34-36) */
  int32_t cplLenI;         /* int(coupling_minutes*60/DTs)   src/Coupling.f90:516-517 */
  double cplLenR;          /* coupling_minutes*60/DTs        src/Coupling.f90:512 */
  double cplReduction;     /* couplingEffectReduction        src/Coupling.f90:84-87 */
  double DTSecs;
  double Tph;              /* DTSecs/3600.0  src/Initialization.f90:92 */
  double tsurfOutputDepth; /* <0: use depth(i) */
  double twoDT;            /* 2.0*DTSecs, divisor of HS  src/BalanceModel.f90:241 */
  /* layer tables, 1-based like the reference (index 0 unused) */
  double ZDpth[RS_MAX_LAYERS + 2];  /* 1..NLayers+1  src/Initialization.f90:217-235 */
  double DyC[RS_MAX_LAYERS + 2];    /* 1..NLayers    src/Initialization.f90:193-196 */
  double condDZ[RS_MAX_LAYERS + 2]; /* 1..NLayers  -(CC/DyK): constant in time because
                                       CC and DyK never change (src/BalanceModel.f90:145,150) */
  double WCont[RS_MAX_LAYERS + 2];  /* 1..NLayers    src/Initialization.f90:207-213 */
  double dryCap[RS_MAX_LAYERS + 2]; /* 1..NLayers  (1.0-Poro)*vsh of the layer
                                       (src/BalanceModel.f90:233,235) */
  double HSfac1;                    /* ZDpth(2)-ZDpth(1), HS(1)  src/BalanceModel.f90:240 */
  /* boundary layer  src/Initialization.f90:330-337 */
  double logMom, logHeat, logCond, logUstar;
  double VK_Const, ZRefT, Grav, LVap, LFus;
  /* radiation */
  double Emiss, SB_Const, Albedo0;
  /* day/night  src/Initialization.f90:461-467 */
  double NightOn, NightOff, CalmLimDay, CalmLimNgt, TrfFricNgt, TrFfricDay;
  /* storage parameters: the RoadCondParameters members the path reads
   * (src/Initialization.f90:479-557) */
  double MaxPormms, MissValI, MinPrecmm, MinWatmms, MinSnowmms, MinDepmms,
      MinIcemms, MaxSnowmms, MaxDepmms, MaxIcemms, MaxWatmms, AlbDry, AlbSnow,
      WatDens, WatMHeat, PorEvaF, DampWearF, TLimFreeze, TLimMeltSnow,
      TLimMeltIce, TLimMeltDep, TLimDew, TLimColdH, TLimColdL, WetSnowFormR,
      WetSnowMeltR, PLimSnow, PLimRain, WWetLim, WWearLim, T4Melt0;
  /* REAL(4)-folded wear constants  src/Cond.f90:78-102:
   * (0.2+0.25), 0.25/(0.2+0.25), 1.1*2.0*0.145, 1.1*2.0*(4.0*0.290),
   * 0.5*2.0*(4.0*0.290), 0.145 */
  double wSnowTran, wSnow2Ice, wIce, wIce2, wDep, wWat;
} RsConstants;

/* Fortran (roadsurf_amd/fortran/RoadSurfHip.f90).  status 0 ok. */
void rs_build_constants(const InputSettings *inSettings,
                        const InputParameters *inputParam, RsConstants *out,
                        int32_t *status);
/* Time-only part of the solar position (src/SunPosition.f90:196-260 and :70-121,124-125):
 * for n time stamps writes table[k*RS_SUN_COLS + {0,1,2,3}] = apparent right ascension (rad, in
 * [0,2pi]), mean sidereal time at Greenwich (rad), sin and cos of the declination, and (ABI 5)
 * {4,5} = cos and sin of (sidereal time - right ascension): the device forms the cosine of the hour
 * angle of a point from them and the point's longitude by the addition theorem instead of a cosine
 * per point-step.  Fortran, host libm. */
#define RS_SUN_COLS 6
void rs_sun_table(int32_t n, const int32_t *year, const int32_t *month,
                  const int32_t *day, const int32_t *hour, const int32_t *minute,
                  const int32_t *second, double *table);
/* Per-point geometry (src/SunPosition.f90:126-128,133): sin/cos of the latitude and the
 * longitude in radians, evaluated as the reference does.  Fortran, host libm. */
void rs_point_geometry(int32_t n, const LocalParameters *localParam,
                       double *sin_lat, double *cos_lat, double *lon_rad);

/* Bottom boundary temperature Tmp(NLayers+1) for a start date
 * (src/Initialization.f90:266-268, src/BalanceModel.f90:325-351). Fortran. */
double rs_bottom_temperature(const InputParameters *inputParam,
                             const RsConstants *consts, int32_t year,
                             int32_t month, int32_t day);

/* ------------------------------------------------------------------------
 * Layer 1: device-resident SoA API.
 *
 * Layout in HBM.  Points are the fastest axis everywhere:
 *   forcing / outputs:  field[t * t_stride + p],  t_stride >= npoints
 *   carried state:      state[v * npoints_padded + p]
 * so a wavefront (64 consecutive points) reads/writes 512 contiguous bytes
 * per field per time step.
 *
 * Columns beyond npoints.  The kernels launch whole wavefronts over npoints_padded columns; the arrays are
 * the caller's.  Arrays that need `npoints` elements: every array of RsPointParams and every row of a
 * forcing or output window (t_stride >= npoints; the last row needs no more than npoints either).  Arrays
 * whose rows have `npoints_padded` columns: the knots ([knot][RS_KNOT_FIELDS][npoints_padded]), the
 * [360][npoints_padded] layout of `horizons`, the preview rows of RsPreview, a kept order row, a summary
 * accumulator.  The CONTENT of columns beyond npoints is never interpreted, whatever it is (NaN, a
 * neighbour's values, values CheckValues would reject), and nothing is ever written there - with the one
 * exception of the pad columns of the plan's own state block (tests/test_hip_padding.py).
 * ---------------------------------------------------------------------- */

typedef struct RsPlan RsPlan; /* opaque */

/* One step-resolution forcing window resident on the device (device pointers): rows of t_stride >= npoints
 * elements, of which the first npoints are read (never written; rs_hip_expand_forcing writes those and no others).
 * Index t_local = 0 corresponds to absolute (1-based, reference) time index
 * `t0`.  Optional streams may be NULL:
 *   tsurfobs NULL -> all missing (-9999.9);  depth NULL -> all missing;
 *   tdew NULL -> not range-checked (treated as in range).
 * hour: int32, either shared [t] (hour_pstride = 0) or per point
 * [t*t_stride + p] (hour_pstride = 1). */
typedef struct RsForcing {
  const double *tair, *tdew, *vz, *rhz, *prec, *sw, *lw;
  const double *tsurfobs, *depth;
  const int32_t *precphase;
  const int32_t *hour;
  int64_t t_stride;     /* elements between consecutive time indices */
  int32_t hour_pstride; /* 0 shared axis, 1 per point */
  /* sky view (src/ModRadiation.f90): direct short-wave and net long-wave streams, and the
   * time-only solar quantities of rs_sun_table, [nsteps][RS_SUN_COLS] = {ra, stG, sin decl, cos decl,
   * cos(stG - ra), sin(stG - ra)}
   * on a time axis shared by all points.  NULL when no point has 0 <= sky_view < 1. */
  const double *sw_dir, *lw_net;
  const double *sun;
} RsForcing;

/* Output window: rows of t_stride >= npoints elements; only the first npoints of a row are ever written. */
typedef struct RsOutputs {
  double *tsurf, *snow, *water, *ice, *deposit, *ice2;
  int64_t t_stride;
  int32_t decimate; /* 1: every step (reference SaveOutput, src/InputOutput.f90:151-165);
                       k>1: only indices i with (i-1) % k == 0 are written (what the
                       reference driver keeps, examples/example1/src/roadrunner.cpp:290,303) */
  int64_t row0;     /* absolute output row r = (i-1)/decimate is stored at buffer
                       row r - row0 */
} RsOutputs;

/* Per-point parameters (device pointers, [npoints] each: no kernel reads element npoints or beyond). */
typedef struct RsPointParams {
  const double *tbottom;  /* Tmp(NLayers+1), src/Initialization.f90:267 */
  const int32_t *initlen; /* LocalParameters.InitLenI */
  const double *tair_relax, *vz_relax, *rh_relax; /* may be NULL if !use_relaxation */
  /* LocalParameters.couplingIndexI / couplingTsurf; may be NULL if !use_coupling.  With
   * coupling the step window must be the whole series (t0 = 1, nsteps = SimLen): a point
   * replays its coupling window up to 25 times (src/Coupling.f90:61-78,324), so the window
   * has to stay addressable. */
  const int32_t *coupling_index;
  const double *coupling_tsurf;
  /* sky view: LocalParameters.sky_view, the geometry of rs_point_geometry and the local
   * horizon table [360][npoints_padded] (degree of azimuth is the slow axis; NULL = all 0).
   * NULL sky_view = no point uses the sky-view branch. */
  const double *sky_view, *sin_lat, *cos_lat, *lon_rad;
  const double *horizons;
  double albedo_surroundings; /* InputParameters.Albedo_surroundings */
  /* Column of `horizons` that belongs to slot s: horizons[deg * npoints_padded + horizon_index[s]].
   * NULL = column s.  What a caller that re-sorts the plan's slots (rs_hip_recluster*) passes instead
   * of a re-ordered copy of the 2.9 KB-per-point table: the scalars above are gathered into slot
   * order, the table stays where it is and the kernels read it through this row (the plan's own
   * order row, rs_hip_plan_order, is exactly that). */
  const int32_t *horizon_index;
  /* Layout of `horizons` (ABI 5).  0: [360][npoints_padded], the degree of azimuth is the slow axis (above).
   * 1: [npoints][360], the caller's own layout (LocalParameters' c_local_horizons rows, RsDriverInput::
   * horizons) - element horizons[horizon_index[s] * 360 + deg]: no transpose on the way in, and a point's
   * consecutive degrees share cache lines (the azimuth of the sun moves a degree in four minutes). */
  int32_t horizons_by_point;
} RsPointParams;

const char *rs_last_error(void);
int rs_hip_device_count(void);

/* Create a plan for `npoints` points on HIP device `device`; uploads constants,
 * allocates the carried-state block.  `stream` is a hipStream_t (0 = default),
 * all rs_hip_* work of this plan is enqueued on it.
 * Domain: a set of constants outside the operand range of the kernels' division sequences is refused with the
 * name of the offending quantity (NULL, rs_last_error).  Making the plan an fp32 one narrows the domain once
 * more - MaxSnowmms >= 0 - and is refused there: rs_hip_set_precision below. */
RsPlan *rs_hip_plan_create(int32_t device, int64_t npoints,
                           const RsConstants *consts, void *stream);
void rs_hip_plan_destroy(RsPlan *plan);
int64_t rs_hip_plan_npoints(const RsPlan *plan);
size_t rs_hip_plan_state_bytes(const RsPlan *plan);

/* Initialization (src/Initialization.f90:65-147, device part): builds the
 * initial profile and storages from forcing index 1 (t_local 0 of `f`, which
 * must have t0 == 1).  Also applies the VZ(1) >= 0.4 clamp logically (the
 * kernel clamps at i == 1; device forcing is not modified). */
int rs_hip_init_state(RsPlan *plan, const RsForcing *f, const RsPointParams *pp);

/* Advance all points over absolute time indices [t0, t0+nsteps) using the
 * window `f` (whose t_local 0 is absolute index t0) and write outputs for
 * those indices into `o` (row 0 = index t0, or decimated as described).
 * Handles the reference's final-step semantics when the range includes
 * SimLen (lastValues, src/InputOutput.f90:169-198).
 * Asynchronous on the plan's stream.  Returns 0 or <0. */
int rs_hip_step(RsPlan *plan, const RsForcing *f, const RsOutputs *o,
                const RsPointParams *pp, int32_t t0, int32_t nsteps);

/* Coupling with time-chunked windows.  rs_hip_step with coupling wants the whole series in one
 * window, because a point replays its coupling window (src/Coupling.f90:61-78).  The pair below
 * lets a caller keep windows of a few hundred indices:
 *   rs_hip_step_cpl    like rs_hip_step for a chunk [t0, t0+nsteps) of a coupled plan, in lock step:
 *                      saves the state at a point's couplingStartI, runs the first pass of its
 *                      window, decides at couplingEndI (Coupling_control), applies the decaying
 *                      corrections behind it - but never replays: a point that must replay PARKS
 *                      behind its window (and takes no step in later rs_hip_step_cpl calls) until
 *   rs_hip_cpl_replay  has run its replays: the window `f` must cover every parked point's
 *                      [couplingStartI, couplingEndI + 1] (t0 <= min start, t0+nsteps-1 >= max end + 1 unless that
 *                      is beyond SimLen: the reference runs CheckValues on the index behind the
 *                      window before it rewinds, examples/example1/src/Simulation.f90:59-66);
 *                      rounds of the general kernel over the compacted list of points that still
 *                      ask for a replay, until none does (`rounds` = how many, <= 25).
 * A point only ever steps the index it is due for (it remembers it), so the caller then simply
 * continues - or, if the points' windows end at different indices, re-issues - the chunks from
 * min(couplingEndI) + 1 on: points that are ahead wait.  Sky view (RsPointParams::sky_view with
 * sin_lat, cos_lat, lon_rad, RsForcing::sw_dir, lw_net and sun rows of the window) is honoured by both
 * calls; the write-back of rs_hip_set_writeback is not (it follows whole-series windows: rs_hip_step).
 * Outputs of replayed indices are overwritten, as in the reference. */
/* With plan order (rs_hip_recluster) AND coupling: rs_hip_step_cpl / rs_hip_cpl_replay can write
 * the outputs of slot s into column order[s] of the output window, i.e. in POINT order whatever
 * the slots' order is (a replay rewrites rows of earlier launches, so a per-launch buffer in slot
 * order does not do).  Meant for decimated outputs: the stores are scattered. */
int rs_hip_set_output_by_point(RsPlan *plan, int32_t on);
/* closed = 1: every point's coupling window, replays included, is behind the plan (the caller has
 * run rs_hip_cpl_replay over the last of them).  A re-sort then moves the coupling scalars only, not
 * the state saved at the window start (saveDataForCoupling, src/Coupling.f90:172-210) nor the stale
 * TmpNw profile: 32 instead of 68 rows at NLayers = 15.  Reset to 0 by rs_hip_init_state. */
int rs_hip_coupling_windows_closed(RsPlan *plan, int32_t closed);
int rs_hip_step_cpl(RsPlan *plan, const RsForcing *f, const RsOutputs *o,
                    const RsPointParams *pp, int32_t t0, int32_t nsteps);
int rs_hip_cpl_replay(RsPlan *plan, const RsForcing *f, const RsOutputs *o,
                      const RsPointParams *pp, int32_t t0, int32_t nsteps, int32_t *rounds);

/* The reference edits its INPUT arrays in place (SURVEY.md 8b "Ownership"): CheckValues clamps
 * SW_dir(i) to SW(i) (src/InputOutput.f90:75-77) and the sky-view correction rewrites SW(i),
 * SW_dir(i), LW(i) (src/ModRadiation.f90:57-71).  The device forcing windows are never modified;
 * a caller that wants those edits gives three device streams laid out like the forcing window of
 * the NEXT rs_hip_step calls (row 0 = index t0, `t_stride` elements per row), pre-filled with the
 * original values: the sky-view kernels then store SW_dir (every stepped index) and SW, LW (points
 * with 0 <= sky_view < 1) as the reference leaves them; with coupling the last replay wins, as in
 * the reference.  All NULL switches it off.  Without sky view the only edit is the SW_dir clamp,
 * which needs no device work (rs_host_run_batch does it on the host). */
int rs_hip_set_writeback(RsPlan *plan, double *sw, double *sw_dir, double *lw, int64_t t_stride);

/* Copy the carried state block device->host / host->device (checkpointing,
 * tests).  Layout: [RS_NSTATE][npoints_padded] doubles. */
int rs_hip_state_download(RsPlan *plan, double *host, size_t bytes);
int rs_hip_state_upload(RsPlan *plan, const double *host, size_t bytes);
/* Branching a run on the device (the ABI number stays; a binding detects the call by its symbol): point p of `dst`
 * takes the carried state of point parent[p] of `src` (parent: HOST int32[dst npoints], every entry in
 * [0, src npoints) - checked here, rs_last_error names the first that is not, and uploaded to scratch of dst).  The
 * state block is all a launch inherits - the step calls keep no time bookkeeping in the plan - so dst goes on with
 * rs_hip_step* at the index src was about to step, under the same SimLen, as parent[p] would have: an ensemble
 * forecast steps the analysis its members share once (roadsurf_amd/ensemble.py is the definition and a runner).
 * Copied are the rows a re-sort moves: Tmp(1..NLayers), the named rows TmpNw(1) .. the sort key, with use_coupling
 * the coupling scalars and, unless src's coupling windows are closed, the saved and stale profiles.  Either plan
 * may have been re-sorted: the copy goes from src's slot of parent[p] to dst's slot of p; dst keeps its order row and
 * its padding columns, src is not written.  The two plans are on one device, of one precision, with equal
 * RsConstants, without diagnostics, and not the same plan; anything else is refused.  Asynchronous: enqueued on
 * dst's stream behind what src's stream held at the call, and src's stream goes on behind the copy.  Afterwards dst
 * has src's rs_hip_coupling_windows_closed, and a wave table a forecast re-sort left it is dropped. */
int rs_hip_state_fanout(RsPlan *dst, RsPlan *src, const int32_t *parent);
/* Number of points with the sticky failure flag set (src/InputOutput.f90:66). */
int64_t rs_hip_failed_count(RsPlan *plan);
/* Measurement aid: one wavefront that reads the shader-clock counter and the constant 100 MHz
 * counter about spin_us microseconds apart and leaves the two deltas in out[0], out[1] (device
 * memory, 2 x uint64).  Enqueued on a side stream beside the step kernels it tells the engine clock
 * the chip holds under that load: MHz = 100 * out[0] / out[1].  Asynchronous on `stream`.  spin_us is
 * clamped to 10 ms and the wait is bounded: out[1] = 0 means the 100 MHz counter did not advance. */
int rs_hip_clock_probe(int32_t device, void *out, uint32_t spin_us, void *stream);
/* Per point (host int32[npoints], in local point order whatever the plan order is): 0, or the
 * 1-based time index at which CheckValues raised simulation_failed - the step of that index was
 * still taken and saved, later outputs read -9999.0 (examples/example1/src/Simulation.f90:58,
 * src/InputOutput.f90:55-82).  The reference only prints this ("BAD input value!"). */
int rs_hip_first_failed_index(RsPlan *plan, int32_t *first_failed);
/* The reference's other run-time messages (it prints them and carries on): from CalcBLCondAndLE
 * " ERROR : UStar negative,vz" + the values line inside the boundary-layer loop and " Max number of BLCond
 * iterations (MaxIter,BLCond_Old,BLCond) :" behind it (src/BoundaryLayer.f90:69-74,98-101), from Coupling_control
 * "coupling coefficient too small / too big, coupling failed" (src/Coupling.f90:400-401,451-452).
 * rs_hip_set_diagnostics(plan, 1) - fp64 plans in natural order; launches of such a plan take the one-point-per-
 * lane kernels with the profile in LDS, which re-run the loop of every step out of line for the two tests: a
 * debugging switch, not a production setting - zeroes the plan's record; rs_hip_diagnostics copies it out,
 * out[npoints][RS_DIAG_COLS]: 0 time indices that printed "Max number ...", 1 the first of them, 2-4 its j,
 * BLCond_Old, BLCond; 5 passes that printed "UStar negative", 6 the time index of the first, 7-11 its Tair, VZ,
 * Rhz, BLCond, TSurfAve; 12 the coupling messages (8 = too small, 16 = too big; these are kept by every kernel
 * flavour, with or without the switch). */
#define RS_DIAG_COLS 13
int rs_hip_set_diagnostics(RsPlan *plan, int32_t on);
int rs_hip_diagnostics(RsPlan *plan, double *out);
int rs_hip_sync(RsPlan *plan);

/* Synthetic forcing: hourly knots from a counter-based hash,
 * expanded to step resolution by the same linear rule the reference driver
 * uses (examples/example1/src/JsonSource.cpp:115-170).  Device kernels;
 * host twins with identical arithmetic are in roadsurf_amd/csrc/rs_synth.h. */
typedef struct RsSynthSpec {
  uint64_t seed;
  int64_t point_offset;   /* global id of local point 0 (multi-GPU shards) */
  int32_t steps_per_knot; /* 3600/DTSecs = 120 */
  int32_t start_hour;     /* hour of day at absolute index 1 */
  const int32_t *order;   /* NULL, or rs_hip_plan_order(): knot column p then belongs to local
                             point order[p] (plan-order windows, see rs_hip_recluster) */
} RsSynthSpec;

/* Number of doubles per point and knot in a knot buffer.  A knot buffer is [nknots][RS_KNOT_FIELDS][npoints_padded]:
 * the row stride is the plan's; columns beyond npoints may hold anything and are never written by a consumer
 * (rs_hip_synth_knots itself fills live columns only). */
#define RS_KNOT_FIELDS 9
/* The same generator on the host, in the layout the reference driver hands runsimulation: per-point
 * [n][simlen] series (InputPointers' eleven f64 arrays + PrecPhase) and the hour of every index (the shared
 * calendar; examples/example1/src/InputData.cpp:5-26).  Host code, no device call: bench.py's host-array leg,
 * __graft_entry__.smoke() and the parity tests take their inputs from it, so that the CPU checker and the GPU
 * path see bit-identical forcing (csrc/rs_synth_host.hip). */
void rs_synth_fill_points(uint64_t seed, int64_t point_offset, int32_t n, int32_t simlen,
                          int32_t steps_per_knot, int32_t start_hour, double *tair, double *tdew,
                          double *vz, double *rhz, double *prec, double *sw, double *lw,
                          double *sw_dir, double *lw_net, double *tsurfobs, double *depth,
                          int32_t *precphase, int32_t *hour);

/* Generate hourly knots k0..k0+nknots-1 into `knots` (device,
 * [nknots][RS_KNOT_FIELDS][npoints_padded] doubles; npoints_padded from
 * rs_hip_plan_npoints_padded). */
int rs_hip_synth_knots(RsPlan *plan, const RsSynthSpec *spec, double *knots,
                       int32_t k0, int32_t nknots);
/* Expand knots to step-resolution forcing for absolute indices
 * [t0, t0+nsteps) into the caller's device buffers `f` (written here).  The
 * knot buffer must hold knots (t0-1)/spk .. (t0+nsteps-2)/spk + 1, the first
 * of them being knot k0.  hour is written as a shared [nsteps] axis. */
int rs_hip_expand_forcing(RsPlan *plan, const RsSynthSpec *spec,
                          const double *knots, int32_t k0, int32_t nknots,
                          const RsForcing *f, int32_t t0, int32_t nsteps);
/* Same with the knot buffer in POINT order (generated once, spec->order NULL) and the window produced
 * in the plan's current SLOT order: column p of the window is interpolated from knot column
 * rs_hip_plan_order()[p].  What a plan that is re-sorted between launches uses instead of
 * regenerating the knots in slot order for every window. */
int rs_hip_expand_forcing_ordered(RsPlan *plan, const RsSynthSpec *spec,
                                  const double *knots, int32_t k0, int32_t nknots,
                                  const RsForcing *f, int32_t t0, int32_t nsteps);

/* rs_hip_expand_forcing_ordered + rs_hip_step in one launch, without the window: the ground wave of the
 * two-wavefront flavour (fp64) or every lane of the two-points-per-lane flavour (an fp32 plan) interpolates the
 * forcing of the next index from the knots itself (same arithmetic, same values as the expansion calls above).
 * knots in POINT order (spec->order NULL), read through the plan's order row.  NLayers = 15, no output depth, sky
 * view or coupling (anything else: an error - use the two calls).  The feature set follows pp as in rs_hip_step:
 * LEAN without pp->initlen, force_tsurf and relaxation targets, else FULL - an initialization phase, relaxation,
 * the knots' observation at index 1 (field 7 of knot 0) and CheckValues' test of the dew point.  The LEAN set does
 * not read the dew point of the knots: it has no test of it, where the reference always has one.
 * What a knot block may hold.  The knots are the caller's.  rs_hip_expand_forcing and
 * rs_hip_expand_forcing_ordered give k0 + (r * (k1 - k0)) / steps_per_knot in IEEE double arithmetic bit for
 * bit for EVERY block, r = 0 .. steps_per_knot - 1, and the knot itself at r = 0: a knot of -0.0 stays -0.0, a
 * subnormal step is divided exactly, an infinite knot or a step whose multiple overflows gives the infinite value,
 * a NaN knot gives NaN strictly between the knots around it.  (An fp32 plan rounds k0 and k1 - k0 to single
 * precision and takes one fused multiply-add with the weight float(r) * float(1 / steps_per_knot); where k1 - k0
 * is not finite in single precision the value at r = 0 is the knot's.)  PrecPhase (field 8) is the later knot's
 * between knots and the knot's own at r = 0.
 * rs_hip_step_knots equals that rule on a DOMAIN only - its interpolation is on the headline's critical path and
 * divides by the reciprocal of the span without a test: steps_per_knot <= 128, every knot finite, and every
 * difference of two successive knots of a field either zero or 2^-1015 <= |k1 - k0| < 2^1017.  Inside it the
 * values are the rule's bit for bit, except that a knot of -0.0 reads +0.0 at its own index (the model's
 * results do not depend on the sign of a zero input).  Outside it: an infinite or NaN knot makes every value of
 * the intervals around it NaN, the knot's own index included - a NaN passes every test of CheckValues, so the
 * point is NOT failed where the reference fails it and writes NaN rows; a smaller difference may be off in the
 * last bit.  A caller that cannot vouch for its knots uses the two calls.
 * What a small shard uses: there the window expansion is the longest link of the chain between two step launches
 * of a plan. */
int rs_hip_step_knots(RsPlan *plan, const RsSynthSpec *spec, const double *knots, int32_t k0,
                      int32_t nknots, const RsOutputs *o, const RsPointParams *pp, int32_t t0,
                      int32_t nsteps);

/* Same, enqueued on another HIP stream (hipStream_t) than the plan's: lets a caller
 * overlap the HBM-bound expansion of window c+1 with the VALU-bound stepping of
 * window c (double-buffered windows, dependencies by HIP events on the caller's side). */
int rs_hip_expand_forcing_on(RsPlan *plan, const RsSynthSpec *spec,
                             const double *knots, int32_t k0, int32_t nknots,
                             const RsForcing *f, int32_t t0, int32_t nsteps,
                             void *stream);

/* Test hook: y[i] = device exp (fn 0) / log (fn 1) / bare square root (fn 3) of x[i], or the bare
 * division x[i] / x[n + i] (fn 2; x holds 2n values); device pointers
 * (roadsurf_amd/csrc/rs_math.hpp; tests/test_hip_math.py). */
int rs_hip_test_math(RsPlan *plan, int32_t fn, int64_t n, const double *x, double *y);

/* Arithmetic flavour of a plan: 64 (default; the parity path) or 32 (BASELINE config 5:
 * fp32 state/forcing/outputs/arithmetic, tolerance-gated against fp64).  Every feature of the
 * model runs in either flavour.  Which fp32 kernel a launch takes: NLayers == 15 without an output
 * depth or coupling - two points per lane, two wavefronts per 128 points (LEAN, the FULL set, and
 * through rs_hip_step sky view with local horizons); anything else - coupling (rs_hip_step over
 * the whole series: every point replays its coupling window inside the launch), tsurfOutputDepth
 * or a depth stream, the FULL set or sky view at another layer count - the general kernel with one
 * point per lane and the profile in LDS; LEAN launches at another layer count likewise one point
 * per lane.  Refused on an fp32 plan: rs_hip_step_cpl / rs_hip_cpl_replay (time-chunked coupling),
 * rs_hip_set_diagnostics, the write-back of the in-place input edits (rs_hip_set_writeback).
 * With 32 the `double *` members of RsForcing/RsOutputs point to FLOAT arrays of the same
 * [t][p] layout, depth, sw_dir and lw_net included (precphase/hour stay int32; tbottom, the sun
 * table and the per-point members of RsPointParams - relaxation targets, coupling observation,
 * sky view, latitude / longitude terms, horizons - stay double: the sun's position is worked out
 * in fp64 in either flavour), and the state block holds floats.  Set before rs_hip_init_state.
 * Domain of 32: MaxSnowmms >= 0, else the call is refused.  Under a negative limit SnowStorage lifts every
 * snow-free road to -MaxSnowmms / 2 at every index, and the next index melts exactly that amount: what is left
 * is a rounding residual whose sign decides whether snow is worn into ice.  Single precision takes the other
 * sign than the reference, in either fp32 kernel (ice grows by 4e-4 mm an index where the reference keeps none;
 * tests/test_hip_param_sets.py), so no tolerance against fp64 holds there.  The other upper limits and
 * MinPrecmm may be negative. */
int rs_hip_set_precision(RsPlan *plan, int32_t bits);

/* How this build divides: 0 = compiler's IEEE expansion everywhere (-DRS_IEEE_DIV),
 * 1 = bare Newton sequence for normal-range operands (default, same bits, see
 * rs_math.hpp), 2 = both evaluated and compared (-DRS_DIV_CHECK).  In mode 2
 * rs_hip_div_mismatch_count returns how many call-site evaluations disagreed
 * with two finite results since the library was loaded (0 in the other modes). */
int rs_hip_division_mode(void);
/* Experiment builds (-DRS_BL_STATS): out[57] = {wave-steps, lane-steps, wave-steps in which every active lane's
 * boundary-layer fixed point repeated its bits at pass 2, 3, 4, the same per lane, trip counts and which
 * wave-uniform shortcuts applied (rs_math.hpp g_bl_stats)}; zeros in the product. */
int rs_hip_bl_stats(RsPlan *plan, int64_t *out);
int64_t rs_hip_div_mismatch_count(RsPlan *plan);
/* mode 2: evaluations where one of the two results is inf/NaN (x/0, x/inf, inf/x: the bare
 * sequence gives NaN there) - the operands the boundary-layer guard handles in the shipped build
 * (roadsurf_amd/csrc/rs_physics_body.inc) - plus those that differ only in the sign of a zero
 * result (-0.0/b; harmless, rs_math.hpp); rs_hip_div_mismatch_count counts different VALUES */
int64_t rs_hip_div_special_count(RsPlan *plan);
/* mode 2: the first 64 finite mismatches as {numerator or sqrt argument, denominator (0 for a
 * square root), IEEE result, bare result}; out = host double[64][4] */
int rs_hip_div_samples(RsPlan *plan, double *out);

/* Kernel flavour: 0 auto, 1 register profile (NLayers == 15), 2 LDS profile (any NLayers),
 * 3 two wavefronts per 64 points - one steps the surface (forcing, boundary layer, layers 1-2,
 * storages), the other the layers below, meeting once per time step: the flavour for launches too
 * small to fill the chip with one point per lane (LEAN feature set, NLayers == 15, windows under
 * 4 GiB per stream; any other launch of such a plan runs as 0).  0 picks 3 for launches of at most
 * 65 536 points (the measured break-even), else 1 for NLayers == 15 with the LEAN feature set, 4 with
 * the FULL one, else 2.
 * 4: layers 1-7 in registers, 8-15 in LDS columns - the FULL feature set (NLayers == 15) at four
 * waves per SIMD without scratch spills; a LEAN launch of such a plan runs as 0.
 * (Until round 6 a tens digit bounded the waves per SIMD of flavours 1 and 2; the measured choices -
 * LEAN four, FULL three - are the kernels' launch bounds now.)
 * All flavours return the same bits.  An fp32 plan (rs_hip_set_precision): 0 = two points per lane, two
 * wavefronts per 128 points (NLayers == 15); 1 or 2 = one point per lane with the profile in LDS. */
int rs_hip_set_variant(RsPlan *plan, int32_t variant);

/* ---- plan order: load balancing by regime ----------------------------------------------
 * The boundary-layer fixed point (src/BoundaryLayer.f90:64-96) stops after its 5 mandatory passes
 * for most point-steps but needs up to ~35 for some, and a wavefront runs until its slowest lane
 * is done: with independent points in arbitrary order a wave averages 13.9 passes where a lane
 * averages 5.5.  Slow convergence is a property of the weather regime and persists for hours.
 * rs_hip_recluster sorts the plan's SLOTS by the extra passes each point needed during the last
 * launch and moves the carried state accordingly, so that slow points share wavefronts.  From
 * then on everything indexed by "point" in this API - forcing and output windows, RsPointParams
 * arrays - is indexed by SLOT: slot s holds local point rs_hip_plan_order(plan)[s].  Producers
 * generate their windows in that order (the synthetic generator takes the order in RsSynthSpec;
 * raw series are 130x smaller than the windows, so gathering them is cheap) and consumers map
 * the outputs back with the same array.  Points do not interact: the order changes no value.
 *   rs_hip_plan_order   device pointer to order[npoints_padded] (identity until the first
 *                       recluster; allocated by the first call), valid until the next recluster
 *   rs_hip_recluster    asynchronous on the plan's stream; the order changes for the NEXT launch */
const int32_t *rs_hip_plan_order(RsPlan *plan);
int rs_hip_recluster(RsPlan *plan);
/* Outputs stay attributable to points (SaveOutput is per point, src/InputOutput.f90:151-165):
 *   rs_hip_plan_order_copy   copies the current order (int32[npoints_padded]) to a device buffer of
 *                            the caller, asynchronously on the plan's stream - call it after the
 *                            rs_hip_step of a launch and before rs_hip_recluster, and column s of
 *                            that launch's output window is local point dst[s] (4 bytes per point and
 *                            launch against the 48 bytes per point and time index of the outputs)
 *   rs_hip_plan_reset_order  back to the identity (a new run over the same plan) */
/* rs_hip_recluster_forecast: like rs_hip_recluster, but the sort key is a FORECAST of the next
 * launch instead of the history of the last one.  What a point costs a wavefront is decided by its
 * boundary-layer regime (stable: no sqrt/log; unstable: which path of log) and by how many passes
 * its fixed point needs - functions of (Tsurf - Tair, wind speed) only (src/BoundaryLayer.f90:64-96).
 * The forcing of the next window is known before it is stepped, so the key kernel runs the fixed
 * point for each point at a few PREVIEW times of the next window (surface temperature = the carried
 * one, moved along with the air temperature by `alpha`) and sorts by
 *     (how many previews are unstable, how many of those take the table path of log, [cover],
 *      predicted passes beyond the mandatory five).
 * Rows are device pointers in the plan's CURRENT slot order, [npoints_padded] each. */
#define RS_PREVIEW_MAX 8
typedef struct RsPreview {
  int32_t n;                             /* 1..RS_PREVIEW_MAX preview times */
  const double *tair[RS_PREVIEW_MAX];    /* air temperature at preview time q */
  const double *vz[RS_PREVIEW_MAX];      /* wind speed at preview time q */
  int32_t hour[RS_PREVIEW_MAX];          /* hour of day at preview time q (calm limit day/night) */
  const double *tair_now;                /* air temperature at the first index of the next window */
  double alpha;                          /* Tsurf(preview) = Tsurf + alpha*(Tair(preview) - Tair_now) */
  int32_t mode;                          /* key fields in priority order as decimal digits: 1 unstable
                                            previews, 2 table-path previews, 3 cover, 4 predicted extra
                                            passes (e.g. 1234); 0..3 = 14, 124, 134, 1234; 5 storage
                                            class, 6/7/8 = 4/1/2 in fewer bits, 0 (inside a list) = three
                                            bits for the LONGEST loop expected in the window - over the previews,
                                            the last index stepped and a passage through the loop's slow band -
                                            in classes 5, 6, 7, 8, 9-12, 13-20, 21-30, 31+ passes (round 4, a
                                            device whose live plans hold at most 131 072 points, and
                                            ROADSURF_HIP_EXTRA_CLASSES=0: field 4 saturating at 7); 9 (anywhere in the list)
                                            = the ground digit, which layers are frozen, always the LEAST
                                            significant field, honoured for keys of at most 12 bits without
                                            it (the plan's counting sort; 378059 is what bench.py and
                                            rs_driver_run use) */
  const int32_t *index;                  /* NULL: the preview rows are in SLOT order; else row element
                                            index[slot] belongs to that slot (rows kept in point order,
                                            index = rs_hip_plan_order(): no regeneration after a re-sort) */
  const double *prec[RS_PREVIEW_MAX];    /* ABI 8.  precipitation at preview time q, or all NULL.  With rows: the
                                            key gets one more bit, its MOST significant - "some preview of the
                                            next window has precipitation" - whatever `mode` says.  A wavefront
                                            none of whose points has precipitation at an index skips
                                            PrecipitationToStorage / CalcPrecType there (exact: they add zeros);
                                            precipitating points are a few per cent of a batch at any time but, in
                                            arbitrary order, sit in most wavefronts.  Read for every q < RS_PREVIEW_MAX
                                            with a row, whatever n says (the rows need not be at the preview times) */
  const double *tair_b[RS_PREVIEW_MAX];  /* ABI 9.  Previews BETWEEN two rows: where tair_b[q] is not NULL, preview q is */
  const double *vz_b[RS_PREVIEW_MAX];    /* tair[q] + w[q] * (tair_b[q] - tair[q]), likewise vz - the straight line the */
  double w[RS_PREVIEW_MAX];              /* forcing itself follows between two hourly knots: a caller whose rows are the
                                            knots places its previews AT the first and last index of the next
                                            window instead of at the knots around it (bench.py's workload: a wavefront's
                                            boundary-layer passes per step 6.50 -> 6.21).  tair_now may then be NULL: the
                                            air temperature of preview 0 */
} RsPreview;
int rs_hip_recluster_forecast(RsPlan *plan, const RsPreview *preview);
/* A plan that is only ever sorted by forecast can tell the step kernels not to keep the history
 * score (a few vector instructions per boundary-layer pass); rs_hip_recluster then refuses. */
int rs_hip_set_history_score(RsPlan *plan, int32_t on);
int rs_hip_plan_order_copy(RsPlan *plan, int32_t *dst_device);
/* ABI 10.  The output rows of a launch in POINT order at every index, for a consumer that keeps one series per
 * point (SaveOutput fills a point's arrays, src/InputOutput.f90:151-165; OutputData.cpp:5-13): the first
 * `nrows` rows of the window `src` ([row][slot], fp64) are written into point-major arrays
 *     dst[stream][point * dst_rows + dst_row0 + row],   stream = Tsurf, Snow, Water, Ice, Deposit, Ice2,
 * point = order[slot] (`order`: a device row kept with rs_hip_plan_order_copy, or NULL = the plan's current
 * order: then call it between the step launch and the next re-sort).  Asynchronous on the plan's stream, or - with
 * a kept order row - on `stream` (a hipStream_t of the caller's, who orders it behind the launch and in front of
 * the window's next use: with two windows in turn the pass overlaps the next launch).  One
 * pass over the rows (read once, written once in whole lines), and not a cheap one - the outputs are most of
 * the bytes this path moves: at 1 M points the pass with it after every launch runs at 1.4-1.5e10 point-timesteps/s
 * against 2.5e10 without; natural order, whose rows are [row][point], not per-point series, runs at 1.46e10
 * (tools/bench_point_order_outputs.py). */
int rs_hip_outputs_by_point(RsPlan *plan, const RsOutputs *src, int32_t nrows, const int32_t *order_device,
                            double *const *dst_device, int64_t dst_rows, int64_t dst_row0, void *stream);
int rs_hip_plan_reset_order(RsPlan *plan);

/* Per-point forecast summaries, reduced from the output rows on the device (the ABI number stays: every name here
 * is new, a binding detects them with rs_hip_summary_cols).  What a road-weather consumer derives from a
 * point's six series is small - the lowest surface temperature and when, whether and when the surface first drops
 * below freezing and for how long, how much snow, water, ice there is at most and for how long - and none of it
 * needs the series off the device, or transposed there.  rs_hip_outputs_summary reads the first `nrows` rows of
 * a window `src` ([row][slot], of any launch and any flavour; on an fp32 plan the members of `src` are float arrays
 * as everywhere else, widened exactly) and merges them into the accumulator of the caller,
 *     acc_device[col * npoints_padded + point],   point = order[slot],   double, RS_SUM_COLS columns:
 *   0       number of valid rows - a row of a point is VALID iff its Tsurf is not exactly -9999.0 (what failed and
 *           rejected points carry behind their last saved index); only valid rows count below
 *   1, 2    min Tsurf, time index of it (the smallest index among equals)
 *   3, 4    max Tsurf, time index of it (the smallest index among equals)
 *   5       smallest time index with Tsurf < spec.tsurf_below (0 = none)
 *   6       number of rows with Tsurf < spec.tsurf_below
 *   7..11   max of Snow, Water, Ice, Deposit, Ice2
 *   12..16  number of rows with that storage > spec.storage_above[k]
 * Row r of `src` is the absolute 1-based time index index0 + r*index_step.  A point without valid rows has count 0,
 * min +inf, max -inf, indices 0, storage maxima -inf, counts 0: that is what rs_hip_summary_reset writes into all
 * npoints_padded columns.  Every comparison is strict; NaN compares false everywhere and still counts as a valid row.
 * The accumulator is in POINT order, so re-sorts between the calls do not matter, and the merge - ties to the smaller
 * index, counts added - makes the result independent of the order in which disjoint row ranges are fed.  Feeding a row
 * twice counts it twice: documented, not detected.  The definition, in numpy: roadsurf_amd/summary.py.
 * `order_device` and `stream` as for rs_hip_outputs_by_point: NULL = the plan's current order, on the plan's stream;
 * a stream of the caller's only with a kept order row.  All six streams are required; t_stride >= npoints.  Columns
 * of points >= npoints are never touched.  It reads 48 B per point and row (24 B of an fp32 window) and reads and writes
 * 136 B per point and call: measured cost in profiles/summary_outputs.txt (tools/bench_summary_outputs.py). */
#define RS_SUM_COLS 17
typedef struct RsSummarySpec {
  double tsurf_below;       /* Tsurf strictly below this counts as "below" (0.0: freezing) */
  double storage_above[5];  /* Snow, Water, Ice, Deposit, Ice2 strictly above this count */
} RsSummarySpec;
int32_t rs_hip_summary_cols(void); /* RS_SUM_COLS of the library */
int rs_hip_summary_reset(RsPlan *plan, double *acc_device, void *stream);
int rs_hip_outputs_summary(RsPlan *plan, const RsOutputs *src, int32_t nrows, int32_t index0, int32_t index_step,
                           const int32_t *order_device, const RsSummarySpec *spec, double *acc_device, void *stream);

/* Per-group time series, reduced from the output rows on the device: the other axis - per row, over a set of points
 * (the ABI number stays: every name here is new, a binding detects them with rs_hip_group_cols).  Every point has a
 * group id, group_device[point] (int32, POINT order): a district of a road network, or the station whose ensemble
 * members the points are.  An id outside [0, ngroups) belongs to no group and is ignored.  rs_hip_outputs_groups
 * reads the first `nrows` rows of a window `src` ([row][slot], of any launch and any flavour; float arrays on an fp32
 * plan, widened exactly) and merges row r into row acc_row0 + r of the accumulator of the caller,
 *     acc_device[((acc_row0 + r) * ngroups + g) * cols + col],   g = group[order[slot]],   double,
 * cols = rs_hip_group_cols(spec) = RS_GRP_COLS + (nedges ? nedges + 1 : 0):
 *   0       number of VALID points of g at that row - valid iff Tsurf is not exactly -9999.0; only these count below
 *   1, 2    min Tsurf, max Tsurf (+inf / -inf when there is none; a NaN never wins)
 *   3       number of points with Tsurf < spec.thresholds.tsurf_below
 *   4..8    number of points with Snow, Water, Ice, Deposit, Ice2 > spec.thresholds.storage_above[k]
 *   9..13   max of Snow, Water, Ice, Deposit, Ice2 (-inf when none; a NaN never wins)
 *   14..    histogram of Tsurf over spec.edges[nedges] (strictly increasing, nedges <= RS_GRP_MAX_EDGES): nedges + 1
 *           bins, a valid non-NaN Tsurf falls into bin j = number of edges <= Tsurf (a value equal to an edge lies in
 *           the upper bin, a NaN in no bin).  nedges = 0: no bins.
 * Every comparison is strict; NaN compares false everywhere and still counts in column 0.  There are no sums and no
 * means, on purpose: every column is a count (exact in fp64), a minimum or a maximum, so the merge of two cells is
 * exact, commutative and associative, and the result does not depend on the order in which points, launches, tiles,
 * plans or devices contribute - which is what lets the device use atomics and still equal the definition
 * (roadsurf_amd/groups.py, reduce_groups) bit for bit.  Medians and percentiles come from the histogram.  Several
 * plans may merge into one accumulator on the same device; feeding a point twice counts it twice (documented, not
 * detected).  rs_hip_group_reset writes the empty cell (counts 0, min +inf, maxima -inf) into all acc_rows rows.
 * A call is refused unless 0 <= acc_row0 and acc_row0 + nrows <= acc_rows; nothing outside rows [acc_row0, acc_row0 +
 * nrows) is written.  `order_device` and `stream` as for rs_hip_outputs_summary: NULL = the plan's current order, on
 * the plan's stream; a stream of the caller's only with a kept order row.  All six streams are required; t_stride >=
 * npoints; columns of `src` at or beyond npoints are never read as points, and group_device is read at [0, npoints)
 * only.  The call changes no value and not how the plan steps.
 * Two kernels, chosen by the host from ngroups * cols alone (rs_hip_group_path): up to RS_GRP_LDS_CELLS doubles per row
 * (districts) a workgroup keeps the cells of a block of rows in LDS, updates them with LDS atomics over many blocks of
 * slots and flushes its non-empty cells with one global atomic each; beyond that (ensembles) lanes update the global
 * cells directly.  fp64 add, min and max atomics are single instructions on gfx950 in LDS and in device memory; the
 * accumulator must be ordinary (coarse-grained) device memory.  It reads 48 B per point and row (24 B of an fp32
 * window); tools/bench_group_outputs.py measures the cost (its output is kept as profiles/group_outputs.txt). */
#define RS_GRP_COLS 14
#define RS_GRP_MAX_EDGES 31
#define RS_GRP_LDS_CELLS 8192 /* ngroups * cols up to this: the LDS kernel (64 KiB of a CU's 160 KiB per workgroup) */
typedef struct RsGroupSpec {
  RsSummarySpec thresholds;
  int32_t ngroups, nedges;
  double edges[RS_GRP_MAX_EDGES];
} RsGroupSpec;
int32_t rs_hip_group_cols(const RsGroupSpec *spec); /* RS_GRP_COLS + (nedges ? nedges + 1 : 0); <0: bad spec */
int32_t rs_hip_group_path(const RsGroupSpec *spec); /* 1: cells in LDS; 2: global cells directly; <0: bad spec */
int rs_hip_group_reset(RsPlan *plan, double *acc_device, int64_t acc_rows, const RsGroupSpec *spec, void *stream);
int rs_hip_outputs_groups(RsPlan *plan, const RsOutputs *src, int32_t nrows, const int32_t *group_device,
                          const int32_t *order_device, const RsGroupSpec *spec, double *acc_device, int64_t acc_rows,
                          int64_t acc_row0, void *stream);

/* Per-station ensemble statistics, reduced from the member rows on the device (the ABI number stays: every name here
 * is new, a binding detects them with rs_hip_ens_cols).  The group series above hold counts and extremes only, so that
 * atomics stay exact; a mean, a spread and percentiles equal a definition bit for bit only if the members of a station
 * are visited in ONE fixed order and every operation is rounded on its own.  That order is a table of the caller's:
 * rs_ens_member_table (host only, no device) turns group_host[npoints] (int32, POINT order; an id outside [0, ngroups)
 * belongs to no station) into table_host[rs_ens_table_ints = ngroups + 1 + npoints]:
 *     table[0 .. ngroups]            start[g]: station g's members are the entries start[g] .. start[g + 1] - 1 of
 *     table[ngroups + 1 + e]         the member list, e in [0, npoints): the points of station 0, of station 1, ...,
 *                                    each station's in ascending point index; the unused tail is -1
 * and returns -1, rs_last_error naming the first such station, where a station has more than spec.max_members members.
 * The caller uploads the table.  rs_hip_outputs_ens reads the first `nrows` rows of a window `src` ([row][slot], of
 * any launch and any flavour; float arrays on an fp32 plan, widened exactly; all arithmetic is fp64) and WRITES
 *     acc_device[((acc_row0 + r) * ngroups + g) * cols + col],   double,   cols = rs_hip_ens_cols = RS_ENS_COLS + nquant
 * A member is VALID at a row iff its Tsurf is not exactly -9999.0 and USED iff it is valid and its Tsurf is not NaN;
 * with the k used members of g in table order, x_0 .. x_{k-1} their Tsurf:
 *   0       number of valid members
 *   1       k
 *   2       mean Tsurf (((x_0 + x_1) + x_2) + ...) / k: every addition rounded on its own, one division
 *   3       spread sqrt(((d_0*d_0 + d_1*d_1) + ...) / k), d_j = x_j - mean: the population form, every product, sum,
 *           the division and the root rounded on their own
 *   4..8    mean of Snow, Water, Ice, Deposit, Ice2 over the USED members, summed the same way; a NaN storage of a used
 *           member makes that one mean NaN and nothing else
 *   9 + j   quantile spec.quant[j] (each in [0, 1], strictly increasing, nquant <= RS_ENS_MAX_QUANT) of the used Tsurf
 *           sorted ascending to y: h = q * (k - 1), lo = floor(h), hi = min(lo + 1, k - 1), t = h - lo, the value
 *           y[lo] + t * (y[hi] - y[lo]), every operation rounded on its own
 * k = 0: columns 2 and above are -9999.0.  roadsurf_amd/ensstats.py (reduce_members) is the definition in numpy, and
 * the tests hold the device to it exactly.  A cell is complete in one call - every member of a station lives in THIS
 * plan - so the call writes and never merges: every station's cell of every fed row is written, the empty one
 * included, rows outside [acc_row0, acc_row0 + nrows) are not touched, and there is no reset.  A station whose members
 * are spread over several plans or devices is not supported (documented, not detected).
 * `order_device` and `stream` as for rs_hip_outputs_groups.  `work_device`: int32[npoints_padded] of the caller's; the
 * call fills it, on the same stream, with the inverse of the order row it resolved (point -> slot) and leaves its
 * contents unspecified.  No state is hidden in the plan, so calls on different streams (with a work row each) cannot
 * race.  Refused, with nothing launched: null arguments or nrows < 1; a bad spec; rows outside acc_rows; a missing
 * stream of the six; t_stride below the plan's points; a stream of the caller's without a kept order row; no
 * work_device.  A table that rs_ens_member_table did not make may give unspecified cells, never an access out of
 * bounds: the kernel reads the table's ngroups + 1 + npoints ints and the window's columns [0, npoints) only, clamps a
 * segment to max_members and to the table, and an entry or an inverse outside [0, npoints) contributes nothing.
 * The kernel uses no atomics: a workgroup takes 64 consecutive stations, brings their members' values of one row and
 * variable together in LDS (65 * max_members doubles per wavefront, each wavefront rows of its own), and lane g owns
 * station g.  tools/bench_ensemble_stats.py measures the cost (its output is kept as profiles/ensemble_stats.txt). */
#define RS_ENS_MAX_MEMBERS 64
#define RS_ENS_MAX_QUANT 8
#define RS_ENS_COLS 9
typedef struct RsEnsSpec {
  int32_t ngroups, max_members, nquant;
  double quant[RS_ENS_MAX_QUANT];
} RsEnsSpec;
int32_t rs_hip_ens_cols(const RsEnsSpec *spec); /* RS_ENS_COLS + nquant; <0: bad spec (host only) */
int64_t rs_ens_table_ints(int32_t npoints, const RsEnsSpec *spec); /* ngroups + 1 + npoints; <0: bad spec */
int rs_ens_member_table(int32_t npoints, const int32_t *group_host, const RsEnsSpec *spec, int32_t *table_host);
int rs_hip_outputs_ens(RsPlan *plan, const RsOutputs *src, int32_t nrows, const int32_t *table_device,
                       const int32_t *order_device, const RsEnsSpec *spec, double *acc_device, int64_t acc_rows,
                       int64_t acc_row0, int32_t *work_device, void *stream);

/* Per-point threshold episodes, reduced from the output rows on the device (the ABI number stays: every name here is
 * new, a binding detects them with rs_hip_episode_cols).  The summaries say how cold, when first below a threshold and
 * for how many rows; a surface that thaws at midday and refreezes at night has several intervals, and only the series
 * themselves told from when to when.  An EPISODE is a maximal run of consecutive output rows of one point on which a
 * condition of the caller's holds - a conjunction of strict bounds on any of RS_EPI_VARS variables: Tsurf, Snow,
 * Water, Ice, Deposit, Ice2 and the dew-point deficit Tsurf - tdew (RsDriverKept::deficit), in this order.
 *   use               bit k set: variable k is tested, and passes iff above[k] < x and x < below[k] - both strict,
 *                     -inf / +inf make a bound one-sided, a NaN compares false
 *   peak              0..6: the variable whose maximum a record keeps
 *   min_rows          >= 1: a run of fewer rows is dropped and counted nowhere
 *   max_episodes      K in 1..RS_EPI_MAX: the first K episodes of a point are kept as records, later ones only counted
 * A spec is refused if use is 0 or has a bit at RS_EPI_VARS or above, if a bound is NaN, and outside these ranges.
 * A row of a point HOLDS iff its Tsurf is not exactly -9999.0 (the validity rule of the summaries), every used
 * variable passes and - if the deficit is used - the deficit is not exactly -9999.0 (what a deficit without both
 * operands reads).  A -9999.0 in a peak variable that is not used in the condition is an ordinary number.
 * The accumulator of the caller is
 *     acc_device[col * npoints_padded + point],   point = order[slot],   double,
 * cols = rs_hip_episode_cols(spec) = RS_EPI_HEAD + K * RS_EPI_REC columns:
 *   0         episodes committed, those beyond K included
 *   1         rows in committed episodes
 *   2         rows of the longest committed episode
 *   3         the time index the next row must have to continue the open run (0 = nothing expected)
 *   4..9      the open run, as a record (rows 0 = none)
 *   10+6j ..  record j = 0..K-1: first time index, last time index, rows, min Tsurf, time index of it (the smallest
 *             among equals), max of the peak variable
 * Extremes use strict comparisons and a NaN never wins; the empty record is {0, 0, 0, +inf, 0, -inf}.
 * Unlike the summaries this reduction is ORDER DEPENDENT: rs_hip_outputs_episodes feeds the first `nrows` rows of a
 * window `src` ([row][slot], of any launch and any flavour) to every point's automaton in sequence, row r being the
 * absolute 1-based time index i = index0 + r*index_step.  Per row: if column 3 is non-zero and differs from i, the
 * open run is closed; column 3 becomes i + index_step; if the row holds it extends the open run (whose first index is
 * set when its rows go from 0 to 1), otherwise the open run is closed.  Closing: a run of at least min_rows rows is
 * copied into record number [column 0] if that is below K, then column 0 grows by one, column 1 by the run's rows and
 * column 2 rises to them; in every case the run is cleared.  So the calls of a pass feed consecutive rows in time
 * order - cut anywhere, the result is that of one call -, and a call whose index0 is not the expected index starts
 * afresh behind a gap.  rs_hip_episodes_finish closes every point's open run and sets column 3 to 0: what a consumer
 * reads; it is idempotent.  rs_hip_episodes_reset writes the accumulator of no rows into all npoints_padded columns
 * of the cols rows.  The definition, in numpy: roadsurf_amd/episodes.py.
 * `deficit_device` holds the deficit of the same rows in the layout of the window, [row][slot] with src->t_stride; it
 * is required iff bit 6 is used or peak is 6, and the call is refused without it then.  On an fp32 plan the members of
 * `src` and the deficit rows are float arrays, widened exactly.  `order_device` and `stream` as for
 * rs_hip_outputs_summary: NULL = the plan's current order, on the plan's stream; a stream of the caller's only with a
 * kept order row; an order entry outside [0, npoints) writes nothing.  All six streams are required; t_stride >=
 * npoints.  Columns of points >= npoints are never touched by the feed and the finish, rows at or beyond cols by none
 * of the three.  The accumulator is in POINT order, so re-sorts between the calls do not matter.  One lane owns a
 * slot and walks its rows in order (they are not split over wavefronts as the summary's are: the automaton is
 * sequential); it reads 48 B per point and row, 56 B with the deficit (half of that from an fp32 window), and reads and
 * writes 80 B per point and call plus 48 B per committed episode: measured cost in profiles/episode_outputs.txt
 * (tools/bench_episode_outputs.py). */
#define RS_EPI_VARS 7
#define RS_EPI_MAX 8
#define RS_EPI_HEAD 10
#define RS_EPI_REC 6
typedef struct RsEpisodeSpec {
  int32_t use;                /* bit k: variable k is tested (Tsurf, Snow, Water, Ice, Deposit, Ice2, deficit) */
  int32_t peak;               /* 0..6: the variable whose maximum a record keeps */
  int32_t min_rows;           /* >= 1 */
  int32_t max_episodes;       /* K: 1..RS_EPI_MAX */
  double above[RS_EPI_VARS];  /* variable k passes iff above[k] < x ... */
  double below[RS_EPI_VARS];  /* ... and x < below[k] */
} RsEpisodeSpec;
int32_t rs_hip_episode_cols(const RsEpisodeSpec *spec); /* RS_EPI_HEAD + K * RS_EPI_REC; <0: bad spec (host only) */
int rs_hip_episodes_reset(RsPlan *plan, const RsEpisodeSpec *spec, double *acc_device, void *stream);
int rs_hip_outputs_episodes(RsPlan *plan, const RsOutputs *src, const void *deficit_device, int32_t nrows,
                            int32_t index0, int32_t index_step, const int32_t *order_device, const RsEpisodeSpec *spec,
                            double *acc_device, void *stream);
int rs_hip_episodes_finish(RsPlan *plan, const RsEpisodeSpec *spec, double *acc_device, void *stream);

/* Per-station probabilities of a road condition over the ensemble members, reduced from the member rows on the device
 * (the ABI number stays: every name here is new, a binding detects them with rs_hip_prob_cols).  The number an ensemble
 * is run for is the share of a station's members on which a condition holds - "Tsurf below 0 and water on the road",
 * "ice present", "dew-point deficit below 0" - now, and by now: the monotone curve "probability of ice by 06:00".  A
 * CONDITION is the condition of the episodes above, a conjunction of strict bounds on the RS_EPI_VARS variables Tsurf,
 * Snow, Water, Ice, Deposit, Ice2 and the dew-point deficit:
 *   use               bit k set: variable k is tested, and passes iff above[k] < x and x < below[k] - both strict,
 *                     -inf / +inf make a bound one-sided, a NaN compares false; every bound is compared in fp64
 * and a row of a member HOLDS under it by the episodes' rule: its Tsurf is not exactly -9999.0, every used variable
 * passes and - if the deficit is used - the deficit is not exactly -9999.0.  A spec holds nconds in 1..RS_PROB_MAX_CONDS
 * conditions; it is refused if ngroups < 1, max_members is outside 1..RS_ENS_MAX_MEMBERS, or a condition's use is 0 or
 * has a bit at RS_EPI_VARS or above, or a bound is NaN.  The members of a station are given by the table of
 * rs_ens_member_table for the same ngroups and max_members (an RsEnsSpec without quantiles): the same table serves
 * both reducers.  rs_hip_outputs_prob reads the first `nrows` rows of a window `src` ([row][slot], of any launch and
 * any flavour; float arrays on an fp32 plan, widened exactly) and WRITES
 *     acc_device[((acc_row0 + r) * ngroups + g) * cols + col],   double,   cols = rs_hip_prob_cols = 1 + 2 * nconds
 *   0                the number of VALID members of g at row r (Tsurf not exactly -9999.0)
 *   1 + c            NOW: the number of members whose row r holds under condition c
 *   1 + nconds + c   BY_NOW: the number of members that are valid at r and for which condition c has held at r or at
 *                    any row fed earlier since the carry was reset - so every count is at or below column 0, and a
 *                    member that failed after the condition held leaves numerator and denominator together
 * Every cell is a count, exact in fp64; the probabilities are the counts over column 0, one division of the consumer's.
 * The carry is ever_device[npoints_padded], int32 in POINT order (re-sorts between the calls do not matter): bit c set
 * means that condition c has held at a fed row of the point; an invalid row sets nothing.  rs_hip_prob_reset writes
 * zero into all npoints_padded entries; rs_hip_outputs_prob reads and updates the entries of the points [0, npoints)
 * only.  Columns 0 and NOW do not depend on the order of feeding; BY_NOW does: the calls of a pass feed consecutive
 * rows in time order - cut anywhere, the result is that of one call - and rows fed out of order give the curve of the
 * order fed (documented, not detected).  A cell is complete in one call, as for rs_hip_outputs_ens: every station's
 * cell of every fed row is written, the empty one (all zeros) included, rows outside [acc_row0, acc_row0 + nrows) are
 * not touched, and a station whose members are spread over several plans is not supported.  The definition, in numpy:
 * roadsurf_amd/ensprob.py (reduce_members_prob); the tests hold the device to it exactly.
 * `deficit_device` holds the deficit of the same rows in the layout and type of the window, [row][slot] with
 * src->t_stride; it is required iff rs_hip_prob_needs_deficit, and the call is refused without it then.
 * `order_device` and `stream` as for rs_hip_outputs_summary: NULL = the plan's current order, on the plan's stream; a
 * stream of the caller's only with a kept order row.  `work_device`: int32[work_ints] of the caller's, at least
 * rs_hip_prob_work_ints(plan, nrows) = npoints_padded * (1 + nrows); the call fills it on the same stream - the inverse
 * of the order row it resolved, then one word per row and slot - and leaves its contents unspecified.  No state is
 * hidden in the plan, so calls on different streams (with scratch each) cannot race.  Refused, with nothing launched:
 * null arguments or nrows < 1; a bad spec; rows outside acc_rows; a missing deficit; missing or short scratch; a missing
 * stream of the six; t_stride below the plan's points; a stream of the caller's without a kept order row.  A table
 * that rs_ens_member_table did not make, or an order row that is no permutation, may give unspecified cells and carry
 * for the stations and points it touches, never an access outside the table, the window, the carry, the scratch or the
 * accumulator: the kernels read the table's ngroups + 1 + npoints ints and the window's columns [0, npoints) only, clamp
 * a segment to max_members and to the table, and an entry or an inverse outside [0, npoints) contributes nothing.
 * Two kernels, no atomics: BY_NOW is sequential per member, so one lane owns a slot and walks the call's rows in time
 * order (whole lines, several rows in flight, as the episodes' feed), writing per row one word - bits 0..7 holds now,
 * bits 8..15 counted by now, bit 16 valid - and the carry once; then a workgroup takes 64 consecutive stations,
 * resolves their members to slots once as rs_hip_outputs_ens does, and lane g counts the bits of station g's words.
 * It reads 48 B per member and row (56 B with the deficit, half of that from an fp32 window) and writes and reads 4 B;
 * tools/bench_ensemble_prob.py measures the cost (its output is kept as profiles/ensemble_prob.txt). */
#define RS_PROB_MAX_CONDS 8
typedef struct RsProbCond {
  int32_t use, reserved;      /* bit k: variable k is tested (Tsurf, Snow, Water, Ice, Deposit, Ice2, deficit) */
  double above[RS_EPI_VARS];  /* variable k passes iff above[k] < x ... */
  double below[RS_EPI_VARS];  /* ... and x < below[k] */
} RsProbCond;
typedef struct RsProbSpec {
  int32_t ngroups, max_members, nconds, reserved;
  RsProbCond cond[RS_PROB_MAX_CONDS];
} RsProbSpec;
int32_t rs_hip_prob_cols(const RsProbSpec *spec);          /* 1 + 2 * nconds; <0: bad spec (host only) */
int32_t rs_hip_prob_needs_deficit(const RsProbSpec *spec); /* 1 iff some condition uses bit 6; <0: bad spec */
int64_t rs_hip_prob_spec_bytes(void);                      /* sizeof(RsProbSpec): the binding's size check */
int64_t rs_hip_prob_work_ints(const RsPlan *plan, int32_t nrows); /* int32s of scratch one call over nrows rows needs; <0: no plan or nrows < 1 */
int rs_hip_prob_reset(RsPlan *plan, int32_t *ever_device, void *stream); /* zero into all npoints_padded entries */
int rs_hip_outputs_prob(RsPlan *plan, const RsOutputs *src, const void *deficit_device, int32_t nrows,
                        const int32_t *table_device, const int32_t *order_device, const RsProbSpec *spec,
                        int32_t *ever_device, double *acc_device, int64_t acc_rows, int64_t acc_row0,
                        int32_t *work_device, int64_t work_ints, void *stream);

/* Per-point aggregates over output periods, reduced from the output rows on the device (the ABI number stays: every
 * name here is new, a binding detects them with rs_hip_period_cols).  The model steps every DTSecs and a consumer
 * keeps far fewer rows: a kept row is a SAMPLE, and what it does not show - how cold the surface got within the hour,
 * whether there was ice at any time in it - is what a regular coarse series is wanted for.  A spec cuts the time axis
 * into `nperiods` periods of `length` indices: period w holds the absolute 1-based time indices
 *     first_index + w*length .. first_index + (w+1)*length - 1,   0 <= w < nperiods,
 * and a row outside [first_index, first_index + length*nperiods) belongs to no period and is ignored.  (With
 * first_index = 2 and length = the driver's decimation step, period w ends at the driver's kept row w + 1.)
 * rs_hip_outputs_periods reads the first `nrows` rows of a window `src` ([row][slot], of any launch and any flavour;
 * on an fp32 plan the members of `src` are float arrays, widened exactly), row r being the time index
 * index0 + r*index_step (computed in 64 bits: any index0 is taken, a row before first_index is simply no period's),
 * and continues the accumulator of the caller,
 *     acc_device[(w * RS_PER_COLS + col) * npoints_padded + point],   point = order[slot],   double:
 *   0       number of valid rows of the period - VALID iff Tsurf is not exactly -9999.0, as for the summaries; only
 *           valid rows count below
 *   1, 2    min Tsurf, max Tsurf (+inf / -inf when there is none; a NaN never wins)
 *   3       the sum of Tsurf over the valid rows in ascending time index, ((x0 + x1) + x2) + ..., every addition
 *           rounded on its own (0.0 when there is none); the mean is the consumer's one division by column 0
 *   4       number of rows with Tsurf < spec.th.tsurf_below
 *   5, 6    Tsurf of the valid row with the largest time index, and that index (-9999.0 and 0 when there is none):
 *           the sample, which beside min and max shows what sampling missed
 *   7..11   max of Snow, Water, Ice, Deposit, Ice2 (-inf when there is none; a NaN never wins)
 *   12..16  number of rows with that storage > spec.th.storage_above[k]
 * Every comparison is strict; NaN compares false everywhere and still counts as a valid row - column 3 is NaN from
 * such a row on, column 5 may be one.  rs_hip_periods_reset writes the cell of no rows into all npoints_padded columns
 * of all periods.  THE FEED CONTRACT: every column but 3 is independent of the order in which rows are fed (column 6
 * decides column 5); column 3 equals the definition when the rows of each period are fed in ascending time order, each
 * once, cut into calls anywhere - a call continues the cells it finds.  Rows fed out of order give the sum of the
 * order fed, a row fed twice counts twice: documented, not detected (as BY_NOW of rs_hip_outputs_prob).  The
 * accumulator is in POINT order, so re-sorts between the calls do not matter.  The definition, in numpy:
 * roadsurf_amd/periods.py (reduce_series); the tests hold the device to it bit for bit.
 * `order_device` and `stream` as for rs_hip_outputs_summary: NULL = the plan's current order, on the plan's stream; a
 * stream of the caller's only with a kept order row.  An order entry outside [0, npoints) writes nothing; columns at
 * or beyond npoints are never touched by the feed; the window is read at columns [0, npoints) and rows [0, nrows)
 * only, and a cell only for 0 <= w < nperiods: the accumulator is nperiods * RS_PER_COLS * npoints_padded doubles.
 * Refused, with nothing launched and the argument named in rs_last_error: a NULL plan, src, spec or acc_device;
 * nrows < 1; index_step < 1; a bad spec (first_index < 1, length < 1, nperiods < 1, length * nperiods > 2^31 - 1,
 * reserved != 0, a threshold that is not finite - rs_hip_period_check says which, on the host alone); a missing
 * stream of the six; t_stride below the plan's points; a stream of the caller's without a kept order row.
 * One lane owns a slot and carries the open period's cell in registers over that period's rows in time order, several
 * rows of all six streams in flight, every row load a whole line per wavefront; a period is never split, and the
 * periods of a call that spans several go to different wavefronts.  No atomics.  It reads 48 B per point and row (24 B
 * of an fp32 window) and reads and writes 272 B (2 * RS_PER_COLS * 8) per point and period the call touches;
 * tools/bench_period_outputs.py measures the cost (its output is kept as profiles/period_outputs.txt). */
#define RS_PER_COLS 17
typedef struct RsPeriodSpec {
  int32_t first_index, length, nperiods, reserved /* 0 */;
  RsSummarySpec th; /* Tsurf strictly below, storages strictly above: what columns 4 and 12..16 count */
} RsPeriodSpec;
int32_t rs_hip_period_cols(void);                      /* RS_PER_COLS of the library */
int64_t rs_hip_period_spec_bytes(void);                /* sizeof(RsPeriodSpec): the binding's size check */
int rs_hip_period_check(const RsPeriodSpec *spec);     /* host only; 0, or <0 with rs_last_error naming the member */
int rs_hip_periods_reset(RsPlan *plan, const RsPeriodSpec *spec, double *acc_device, void *stream);
int rs_hip_outputs_periods(RsPlan *plan, const RsOutputs *src, int32_t nrows, int32_t index0, int32_t index_step,
                           const int32_t *order_device, const RsPeriodSpec *spec, double *acc_device, void *stream);

/* Gridded fields gathered to points on the device (the ABI number stays: every name here is new, a binding detects
 * them with rs_hip_grid_max_stencil).  A weather model delivers fields [time][node]; every kernel here reads series
 * [time][point].  Each point has a stencil of `stencil` nodes, node_device[point * stencil + k] (int32) with weights
 * weight_device[point * stencil + k] - bilinear, nearest neighbour, a mask, an unstructured mesh: projections are the
 * caller's business - and rs_hip_gather_nodes writes, for every row r < nrows and slot s < npoints,
 *     dst_device[r * dst_stride + s] = w0 * a0 + w1 * a1 + ...,   ak = src_device[r * src_stride + node k],
 * point = order[s], by these rules (the definition, in numpy: roadsurf_amd/grid.py, gather_nodes):
 *   - a term whose weight is exactly 0.0 does not exist: its node is not looked at, whatever it holds (NaN, a missing
 *     value, an index out of range);
 *   - a value is PRESENT iff it is > present_above (the reference's own test, `> -100.0`; a NaN is absent).  If any
 *     existing term is absent, or its node lies outside [0, n_nodes), or no term exists, the result is missing_value;
 *   - else the existing terms are added in stencil order, every product and every sum rounded on its own (no fused
 *     multiply-add): one node with weight 1.0 gives the node's bits, -0.0 included.
 * An out-of-range node under a non-zero weight yields missing_value: the index is compared before anything is loaded
 * through it, so no argument makes the kernel read outside `src`.  Columns of `dst` at or beyond npoints are never
 * written; node_device and weight_device are read at points [0, npoints) only.  src_stride >= n_nodes, dst_stride >=
 * npoints, 1 <= stencil <= RS_GRID_MAX_STENCIL.  `order_device` and `stream` as for rs_hip_outputs_summary: NULL = the
 * plan's current order (slot = point on a plan that was never re-sorted), on the plan's stream; a stream of the
 * caller's only with a kept order row.  One point per lane, the stencil in registers, rows in the loop: the reads are
 * scattered (neighbours along a road share nodes, the caches serve most of them), the writes whole lines, all offsets
 * 64-bit.  A row of the hourly knots a layer-1 caller keeps resident, [RS_KNOT_FIELDS][npoints_padded], is exactly a
 * `dst`.  rs_driver_run_grid uses it for sources that arrive as fields; tools/bench_grid_source.py measures it (its
 * output is kept as profiles/grid_source.txt). */
#define RS_GRID_MAX_STENCIL 4
int32_t rs_hip_grid_max_stencil(void); /* RS_GRID_MAX_STENCIL of the library */
int rs_hip_gather_nodes(RsPlan *plan, const double *src_device, int32_t nrows, int64_t n_nodes, int64_t src_stride,
                        const int32_t *node_device, const double *weight_device, int32_t stencil,
                        const int32_t *order_device, double present_above, double missing_value,
                        double *dst_device, int64_t dst_stride, void *stream);

/* Device timing of the step kernel with HIP events recorded on the plan's
 * stream around every rs_hip_step launch since the last reset.  Returns the
 * summed milliseconds (synchronises on the last event) and the launch count. */
int rs_hip_timing_reset(RsPlan *plan);
double rs_hip_timing_step_ms(RsPlan *plan, int32_t *nlaunches);
/* The same launches as intervals [start, stop] in milliseconds after `ref_event` (a hipEvent_t
 * with timing enabled that the caller recorded on this device before the launches).  With several
 * plans stepping concurrently on one device (one stream each) their step kernels overlap in time;
 * the union of all plans' intervals is the time during which the device ran step kernels.  Returns
 * the number of launches (at most `cap` are written) or < 0. */
int32_t rs_hip_timing_intervals(RsPlan *plan, void *ref_event, double *start_ms, double *stop_ms,
                                int32_t cap);
int64_t rs_hip_plan_npoints_padded(const RsPlan *plan);

/* ------------------------------------------------------------------------
 * Layer 2: host-array batch (used by the Fortran runsimulation_batch).
 * Inputs are the per-point arrays of the reference boundary; packing to SoA,
 * H2D, kernels and D2H happen inside, tiled over points.  tbottom[n] is
 * computed by the Fortran caller.  Returns 0 or <0.
 * ---------------------------------------------------------------------- */
typedef struct RsHostExtras {
  /* sky view: NULL/0 when no point has 0 <= sky_view < 1 */
  const double *sun;      /* rs_sun_table of the shared time axis, [SimLen][RS_SUN_COLS] */
  const double *sin_lat;  /* rs_point_geometry, [n] each */
  const double *cos_lat;
  const double *lon_rad;
  double albedo_surroundings;
  /* out, [n] or NULL: per point 0, or the 1-based time index at which its run was failed
   * (rs_hip_first_failed_index) */
  int32_t *first_failed;
  /* 1: write the reference's in-place edits of the caller's input arrays back
   * (src/InputOutput.f90:75-77: SW_dir(i) = min(SW_dir(i), SW(i)) at every checked index;
   * src/ModRadiation.f90:57-71: SW, SW_dir, LW as the sky-view correction leaves them) */
  int32_t writeback;
  /* out, [n][RS_DIAG_COLS] or NULL: rs_hip_diagnostics' record of every point (the plans of the call then run
   * with rs_hip_set_diagnostics) */
  double *diagnostics;
} RsHostExtras;

/* `device` >= 0: that device.  `device` < 0 (what runsimulation_batch / runsimulation pass): the
 * batch is cut into contiguous blocks of points over the device list - environment
 * ROADSURF_HIP_DEVICES ("0,1,2,3", a device may repeat; default "all" visible devices), blocks of
 * at least ROADSURF_HIP_MIN_SHARD points (default 4096), batches too small to split take the
 * devices in turn - one host thread + stream + plan per block, no collective: the in-process
 * counterpart of the reference driver's worker pool (examples/example1/src/roadrunner.cpp:423-501).
 * rs_last_fanout(): number of blocks the calling thread's last call used. */
int rs_last_fanout(void);
int rs_host_run_batch(int32_t n, OutputPointers *outPointers,
                      const InputPointers *inPointers,
                      const RsConstants *consts,
                      const LocalParameters *localParam, const double *tbottom,
                      const RsHostExtras *extras, int32_t device);

/* ------------------------------------------------------------------------
 * Layer 4: the reference DRIVER's data path on the device.
 *
 * What examples/example1 does on the host for every point before and after
 * `runsimulation` — and what makes a step-resolution boundary PCIe-bound — happens here
 * on the GPU, so only the RAW series (hourly NWP / observations) cross the bus inbound and
 * only the decimated outputs come back:
 *   JsonSource ctor      Tdew <-> RH completion of the raw series
 *                        (JsonSource.cpp:288-295, MeteorologyTools.cpp:12-51)
 *   JsonSource::interpolate   raw times -> simulation times, per variable, with the
 *                        reference's missing-value rules (JsonSource.cpp:49-176)
 *   DataHandler::GetWeather   later sources overwrite earlier ones where they have data
 *                        (DataHandler.cpp:75-84, JsonSource.cpp:323-373; PrecPhase and
 *                        Depth are NOT carried over there, so they stay missing)
 *   read_input           completeness check, relaxation targets, coupling index/observation
 *                        and the blanking of TSurfObs inside the coupling window
 *                        (roadrunner.cpp:156-278)
 *   runsimulation        the hot path (layers 1-3)
 *   save_output          every (outputStep*60/DTSecs)-th index (roadrunner.cpp:285-315)
 * Out of scope: JSON/text parsing and writing (host work, roadsurf_amd/driver.py has a
 * reader/writer for the reference's schema).
 * A source's points either share one raw time axis or have one each (RsRawSource).
 * ---------------------------------------------------------------------- */
#define RS_MAX_SOURCES 4

/* One data source after parsing (JsonSource.cpp:182-316).  Arrays are HOST pointers,
 * [n_points][n_times] row-major (one contiguous series per point, as the reference's
 * InputData holds them); NULL = the variable is absent from this source (all missing,
 * -9999.9).  PrecipitationForm is not listed: the reference reads it but never hands it
 * on (JsonSource.cpp:323-373 does not copy PrecPhase).
 * Time axis: either one axis shared by all points (times[n_times], lengths NULL: gridded NWP
 * data), or one per point like the reference's per-station "time" arrays
 * (times_per_point = 1: times[n_points][n_times], and lengths[n_points] gives how many leading
 * entries of a point's row are real: rows are padded to the common width n_times). */
typedef struct RsRawSource {
  int32_t n_times;          /* row width of every array below */
  int32_t is_observation;   /* DataHandler.cpp:65-66: counts for GetLatestObsIndex */
  const int64_t *times;     /* epoch seconds, strictly increasing within a series */
  const double *tair, *rhz, *tdew, *vz, *prec, *lw_net, *lw, *sw, *sw_dir, *tsurfobs;
  int32_t times_per_point;  /* 0 shared axis, 1 per-point axes */
  const int32_t *lengths;   /* per-point series lengths (times_per_point = 1), or NULL = n_times */
} RsRawSource;

typedef struct RsDriverInput {
  int32_t n_points;
  int32_t n_sources;            /* 1..RS_MAX_SOURCES, applied in this order */
  const RsRawSource *sources;
  int64_t start_time;           /* InputSettings.start_time; simulation index k (0-based) is at
                                   start_time + k*int(DTSecs)  (JsonSource.cpp:199-205) */
  int64_t forecast_time;        /* InputSettings.forecast_time (roadrunner.cpp:168-169) */
  /* local calendar of the simulation times, [SimLen] each (JsonSource.cpp:297-308) */
  const int32_t *year, *month, *day, *hour, *minute, *second;
  const double *horizons;       /* [n_points][360] local horizon angles, or NULL (all 0) */
} RsDriverInput;

/* Per-point status: 0 simulated; 1..6 a mandatory variable is missing at `missing_index`
 * (tair, Rhz, prec, SW, LW, VZ: the order roadrunner.cpp:188-229 tests them in) and the
 * point is skipped like the reference skips it (outputs stay -9999.0); 7 the relaxation
 * index equals SimLen (the reference reads one past its arrays there, roadrunner.cpp:246-248). */
typedef struct RsDriverOutput {
  int32_t n_out;                /* number of kept indices: ceil(SimLen / step) */
  double *tsurf, *snow, *water, *ice, *deposit, *ice2; /* host [n_points][n_out]; NULL = not wanted */
  int32_t *status;              /* [n_points] */
  int32_t *missing_index;       /* [n_points] 0-based index of the first missing value, else -1 */
} RsDriverOutput;

/* What a call may ask for beside the six series, each an optional member of RsDriverRequest (below).  The ABI number
 * did not move for any of them: every name is new, and a binding detects a call by looking for its symbol.
 *
 * RsDriverSummary: per-point summaries of the kept rows [first_row, last_row] of n_out (the caller passes the forecast
 * part): RS_SUM_COLS doubles per point as rs_hip_outputs_summary defines them, the time index of kept row r being
 * r*step + 1.  They are reduced on the device from the tile's result block, behind the blanking of rejected points
 * (whose summary is the empty one) and behind every coupling replay, and only n_points * RS_SUM_COLS doubles come
 * back for them.  The six series pointers of `out` may all be NULL: a call for the summaries alone transposes and
 * downloads no series. */
typedef struct RsDriverSummary {
  RsSummarySpec spec;
  int32_t first_row, last_row;
  double *summary; /* host [n_points][RS_SUM_COLS] */
} RsDriverSummary;
/* RsDriverGroups: per-group series of the kept rows [first_row, last_row] (rs_hip_outputs_groups defines the cells):
 * group[n_points] gives every point's group, and series[r - first_row][g][col] is the cell of kept row r.  They are
 * reduced where the summaries are - from the tile's result block, behind the blanking of rejected points (whose rows
 * are -9999.0 and count nowhere) and behind every coupling replay.  A block of points keeps one accumulator on its
 * device across its tiles, and a tile's slice of `group` goes up with the tile; with device < 0 every block of the
 * fan-out reduces its own and the host merges them by the rule of the definition.  Only rows x ngroups x cols doubles
 * come home for them; the six series pointers of `out` may all be NULL. */
typedef struct RsDriverGroups {
  RsGroupSpec spec;
  const int32_t *group; /* host [n_points] */
  int32_t first_row, last_row;
  double *series; /* host [last_row - first_row + 1][ngroups][cols] */
} RsDriverGroups;
/* RsGridSource: a source that arrives as the weather model delivers it: fields [n_times][n_nodes] plus one stencil per
 * point (rs_hip_gather_nodes defines the gather; its presence threshold is the reference's own, `> -100.0`, for lw_net
 * `> -1000.0`, and its missing value -9999.9).  grids[s] != NULL makes source s a gridded one: in->sources[s] then
 * supplies n_times, times and is_observation only - a shared time axis, every field pointer and `lengths` NULL - and
 * the call computes exactly what it computes when the caller gathers every field to the points on the host
 * (roadsurf_amd/grid.py, to_raw_source) and passes the result per point.  The fields of a gridded source go to every
 * device of the call ONCE, before its blocks start (the blocks of a fan-out that share a device share the copy; it is
 * freed when the call returns), a tile uploads its slice of `node` and `weight` instead of field rows, and the raw
 * columns [n_times][point] are filled by the gather kernel instead of a transpose; everything behind them runs as it
 * does for per-point sources.  Before any device work the host checks every gridded source - stencil in
 * 1..RS_GRID_MAX_STENCIL, finite weights, every node under a non-zero weight inside [0, n_nodes) - and refuses the
 * call with the first offending point named.  `grids` NULL, or all its entries NULL: every source is per point. */
typedef struct RsGridSource {
  int64_t n_nodes;
  const double *tair, *rhz, *tdew, *vz, *prec, *lw_net, *lw, *sw, *sw_dir, *tsurfobs; /* host [n_times][n_nodes]; NULL = absent */
  int32_t stencil;      /* 1..RS_GRID_MAX_STENCIL */
  const int32_t *node;  /* host [n_points][stencil] */
  const double *weight; /* host [n_points][stencil] */
} RsGridSource;
/* RsDriverKept: the INPUTS the model saw at the kept rows, and the dew-point deficit there (a binding checks the length
 * of `merged` with rs_driver_kept_fields).  The reference's operational program stores,
 * per point and output time, the surface temperature, the air temperature, the dew point and their difference, the
 * hoar-frost and condensation indicator (examples/example2/src/QueryDataTools.cpp:285-296, 323-347); these are the
 * merged, interpolated, Tdew / RH-completed series read_input hands to runsimulation, which no other call returns
 * short of rs_driver_expand's [10][n_points][SimLen] download.  The definition, in numpy: roadsurf_amd/kept.py.
 *   merged[f][p][r]  equals, bit for bit, rs_driver_expand's merged[f][p][r * step] of the same call (step =
 *                    outputStep*60/DTSecs, kept row r = 0-based simulation index r * step, roadrunner.cpp:303): the
 *                    values read_input returns, for EVERY point - a rejected point's rows are not blanked - with
 *                    TSurfObs blanked to -9999.9 inside a point's coupling window (roadrunner.cpp:266-273).  They
 *                    predate runsimulation's in-place edits of its inputs: VZ(1), the clamp of SW_dir to SW, the
 *                    sky-view correction of SW, SW_dir and LW are NOT in them.
 *   deficit[p][r]    = Tsurf[p][r] - tdew[p][r], one fp64 subtraction, where both operands are not NaN and > -9000
 *                    (-9000.0 itself is missing here: calc_difference's rule, not read_input's), else exactly -9999.0.
 *                    Tsurf is the FINAL kept row - behind every coupling replay and behind the blanking of rejected
 *                    points, whose deficit therefore reads -9999.0 throughout; tdew is the kept merged value, whether
 *                    or not merged[1] was asked for.
 * The six outputs, the summaries, the group series, status, missing_index and `local` of a call do not depend on
 * `kept`; the six series pointers of `out` may all be NULL.  A tile makes the wanted variables one at a time from its
 * raw columns and plans, which stay on the device for the whole tile, into ONE extra [n_out][points] buffer (0.2 GB for
 * 524 288 points and 49 rows), on the tile's stream, behind its time loop; columns at or beyond the tile's points are
 * never sent to the host.  With device < 0 every block writes its own points' rows.  All its eleven pointers NULL: as
 * without it.  tools/bench_kept_rows.py measures the cost (profiles/kept_rows.txt). */
typedef struct RsDriverKept {
  double *merged[10]; /* host [n_points][n_out] each, order of rs_driver_expand's `merged`
                         (tair, tdew, VZ, Rhz, prec, SW, LW, SW_dir, LW_net, TSurfObs); NULL = not wanted */
  double *deficit;    /* host [n_points][n_out] or NULL */
} RsDriverKept;
int32_t rs_driver_kept_fields(void); /* 10: the length of RsDriverKept::merged in the library */
/* RsDriverEpisodes: per-point threshold episodes of the kept rows [first_row, last_row] (rs_hip_outputs_episodes defines
 * them; a binding detects them with rs_hip_episode_cols): cols = rs_hip_episode_cols(&spec)
 * doubles per point, FINISHED, the time index of kept row r being r*step + 1.  Every tile resets its accumulator, feeds
 * the rows in one call from its result block - where the summaries are reduced: behind the blanking of rejected points,
 * whose episodes are the empty accumulator, and behind every coupling replay -, finishes, and only n_points * cols
 * doubles come home for them.  A spec that uses the deficit (bit 6, or peak 6) has the tile make it, from the kept dew
 * point and the final Tsurf rows, whether or not `kept` asks for it: the very values RsDriverKept::deficit returns for
 * the same call, made once per tile when both want them, in one further [n_out][points] buffer of the tile (0.2 GB for
 * 524 288 points and 49 rows).  With device < 0 every block writes its own points' rows.  The six series pointers of
 * `out` may all be NULL.  The six outputs, the summaries, the group series, the kept arrays, status, missing_index and
 * `local` of a call do not depend on `episodes`. */
typedef struct RsDriverEpisodes {
  RsEpisodeSpec spec;
  int32_t first_row, last_row;
  double *episodes; /* host [n_points][cols] */
} RsDriverEpisodes;

/* What one call wants beside the six series: any subset, a NULL member = not wanted.  A further product is a further
 * member here, not a further entry. */
typedef struct RsDriverRequest {
  const RsGridSource *const *grids; /* [n_sources] or NULL */
  const RsDriverSummary *summary;   /* or NULL */
  const RsDriverGroups *groups;     /* or NULL */
  const RsDriverKept *kept;         /* or NULL */
  const RsDriverEpisodes *episodes; /* or NULL */
} RsDriverRequest;
/* local[n_points]: in lat, lon, sky_view (others ignored); out InitLenI, tair_relax,
 * VZ_relax, RH_relax, couplingIndexI, couplingTsurf as read_input leaves them.
 * device >= 0: that device; device < 0: fan-out over the device list like rs_host_run_batch.
 * `request` NULL, or all its members NULL: the six series, status, missing_index and `local` alone.
 * Returns 0 or <0 (rs_last_error; a refused member is named by the older entry that introduced it). */
int rs_driver_run_request(const RsDriverInput *in, const InputSettings *settings, const InputParameters *params,
                          LocalParameters *local, const RsDriverOutput *out, const RsDriverRequest *request /* or NULL */,
                          int32_t device);
/* The older entries, one per product as it arrived: each is rs_driver_run_request with the request shown. */
int rs_driver_run(const RsDriverInput *in, const InputSettings *settings,
                  const InputParameters *params, LocalParameters *local,
                  const RsDriverOutput *out, int32_t device); /* request NULL */
int rs_driver_run_summary(const RsDriverInput *in, const InputSettings *settings,
                          const InputParameters *params, LocalParameters *local,
                          const RsDriverOutput *out, const RsDriverSummary *summary, int32_t device); /* {NULL, summary} */
int rs_driver_run_groups(const RsDriverInput *in, const InputSettings *settings,
                         const InputParameters *params, LocalParameters *local,
                         const RsDriverOutput *out, const RsDriverSummary *summary, const RsDriverGroups *groups,
                         int32_t device); /* {NULL, summary, groups} */
int rs_driver_run_grid(const RsDriverInput *in, const RsGridSource *const *grids /* [n_sources] */,
                       const InputSettings *settings, const InputParameters *params, LocalParameters *local,
                       const RsDriverOutput *out, const RsDriverSummary *summary, const RsDriverGroups *groups,
                       int32_t device); /* {grids, summary, groups} */
int rs_driver_run_kept(const RsDriverInput *in, const RsGridSource *const *grids /* [n_sources] or NULL */,
                       const InputSettings *settings, const InputParameters *params, LocalParameters *local,
                       const RsDriverOutput *out, const RsDriverSummary *summary, const RsDriverGroups *groups,
                       const RsDriverKept *kept, int32_t device); /* {grids, summary, groups, kept} */
int rs_driver_run_episodes(const RsDriverInput *in, const RsGridSource *const *grids /* [n_sources] or NULL */,
                           const InputSettings *settings, const InputParameters *params, LocalParameters *local,
                           const RsDriverOutput *out, const RsDriverSummary *summary, const RsDriverGroups *groups,
                           const RsDriverKept *kept, const RsDriverEpisodes *episodes,
                           int32_t device); /* {grids, summary, groups, kept, episodes} */
/* The ensemble form of the driver (the ABI number stays: every name here is new, a binding detects the call by its
 * symbol and checks the struct with rs_driver_ensemble_bytes).  `in` holds the STATIONS and the sources they share;
 * every station has members - parent[q] is member q's station - that see one further source, `member`
 * ([n_members][n_times] per field, a time axis shared by all members), put at `position` of the overlay order: in
 * front of shared source `position`, later sources win.  The DEFINITION is a plain call on replicated input
 * (roadsurf_amd/driver.py, replicate_sources: every shared source row-gathered by parent as bit copies, the member
 * source inserted): the members get exactly what rs_driver_run_request returns for that input - status,
 * missing_index, the decisions in `local` and the six series at the kept rows from first_row on - and the stations
 * what it returns for the shared sources alone at the kept rows before first_row; later station rows read -9999.0, as
 * rows never saved do.
 *   The branch follows from the member source: JsonSource::interpolate writes nothing to a simulation time before a
 * source's first raw time, so with k_b the smallest 0-based simulation index whose time is at or behind
 * member.times[0], every index below k_b is shared.  branch_index = B = k_b is the last shared 1-based time index,
 * first_row = ceil(k_b / step) the first kept row that is a member's own, member_out.n_out = n_out - first_row.
 *   The call steps the stations over [1, B] ONCE, copies every station's carried state into its members on the device
 * (rs_hip_state_fanout) and steps the members over [B + 1, SimLen] alone.  A tile is a run of whole stations whose
 * members fit ROADSURF_HIP_TILE_POINTS; the members are a second tile with a second plan beside the stations': the
 * member source is uploaded as any per-point source, the shared sources' raw columns are filled on the device from the
 * stations' columns through parent (bit copies: values, per-point time axes and lengths; a gridded shared source
 * included, whose columns the stations' tile has gathered), horizons and geometry are the station's.  Every member's
 * decisions are made from its own columns; a station steps with the decisions of its series before index k_b (a hole
 * behind the branch that rejects the station does not keep its members from being accepted).
 *   stats / probs: per-station cells of the members' kept rows first_row .. n_out - 1, [n_tail][n_stations][cols] as
 * rs_hip_outputs_ens and rs_hip_outputs_prob define them for group = parent (spec.ngroups = n_stations), reduced on the
 * device from the members' final, blanked result block; with all six series pointers of member_out NULL nothing else
 * of the members' rows comes home.
 *   Refused before any device work, rs_last_error naming the reason and the first offending member or station: a
 * member source with per-point time axes, flagged as observation, carrying tsurfobs or without times; times[0] <=
 * start_time; B outside [1, SimLen - 1]; a parent row that is not non-decreasing within [0, n_stations); more than
 * RS_MAX_SOURCES sources in all; position outside [0, n_sources]; device < 0 (no fan-out over the device list);
 * member_out.n_out other than n_tail; a station with more members than a tile holds; with stats or probs the limits
 * of rs_ens_member_table, ngroups other than n_stations, and a probs condition that uses the deficit.  Refused per
 * tile, once its decisions are known and before it steps (nothing of that tile has reached the caller's arrays,
 * earlier tiles are complete): with coupling a station whose coupling is on and couplingIndexI + 1 > B (a replay
 * reads the index behind its window, which must be shared), and an accepted member whose InitLenI, couplingIndexI or
 * couplingTsurf differ from its station's, or whose relaxation targets differ while InitLenI < B.
 *   ROADSURF_HIP_DRIVER_TIMING=1 also reports the column copies and the fan-outs.  rs_driver_last_tiles counts the
 * station tiles.  tools/bench_driver_ensemble.py measures the call against the plain one (profiles/driver_ensemble.txt). */
typedef struct RsDriverEnsemble {
  int32_t n_members;
  int32_t position;              /* 0 .. in->n_sources: the member source's place in the overlay order */
  const int32_t *parent;         /* host [n_members], non-decreasing, in [0, in->n_points) */
  RsRawSource member;            /* fields host [n_members][n_times]; times_per_point = 0, no tsurfobs */
  RsDriverOutput member_out;     /* n_out = n_tail; series host [n_members][n_tail] or NULL; status, missing_index
                                    host [n_members] or NULL */
  LocalParameters *member_local; /* host [n_members] out (lat, lon, sky_view the station's), or NULL */
  const RsEnsSpec *stats_spec;   /* or NULL */
  double *stats;                 /* host [n_tail][n_stations][rs_hip_ens_cols] */
  const RsProbSpec *probs_spec;  /* or NULL */
  double *probs;                 /* host [n_tail][n_stations][rs_hip_prob_cols] */
  int32_t branch_index, first_row; /* out: B and the first kept row of the members (also set by a refusal behind them) */
} RsDriverEnsemble;
int64_t rs_driver_ensemble_bytes(void); /* sizeof(RsDriverEnsemble): the binding's size check */
int rs_driver_run_ensemble(const RsDriverInput *in, const RsGridSource *const *grids /* [n_sources] or NULL */,
                           const InputSettings *settings, const InputParameters *params, LocalParameters *local,
                           const RsDriverOutput *out, RsDriverEnsemble *ens, int32_t device);
/* Tiles: a call steps its points in tiles of ROADSURF_HIP_TILE_POINTS (default 524 288).  With
 * coupling the forcing windows of a tile span [first coupling-window start, last window end + 1]
 * of ITS points; a tile whose windows would exceed ROADSURF_HIP_WINDOW_BUDGET_MB (default 24 576)
 * - stations whose observations ended hours apart - is cut in halves, down to 4 096 points.
 * rs_driver_last_tiles(): tiles the calling thread's last call with device >= 0 stepped. */
int rs_driver_last_tiles(void);
/* Since ABI 6 the blocks of rs_driver_run step with a kernel that makes its forcing from the raw series itself
 * (no forcing windows, no expansion kernel) wherever it can: sources on shared time axes, NLayers = 15, no
 * coupling, no output depth; ROADSURF_HIP_DRIVER_WINDOWS=1 keeps the windows.  Step launches of that kind in
 * the calling thread's last call with device >= 0 (tests). */
int rs_driver_last_raw_launches(void);
/* rs_driver_run keeps its forcing-window block (up to 64 GB of HBM with coupling) for the next
 * call, because releasing and re-acquiring that much VRAM costs seconds (the driver wipes it).
 * This frees it. */
void rs_driver_release_cache(void);
/* Test hook: only the input side.  merged = host [10][n_points][SimLen] in the order tair,
 * tdew, VZ, Rhz, prec, SW, LW, SW_dir, LW_net, TSurfObs: what read_input returns. */
int rs_driver_expand(const RsDriverInput *in, const InputSettings *settings,
                     LocalParameters *local, double *merged, int32_t *status,
                     int32_t *missing_index, int32_t device);
/* ... with gridded sources, as rs_driver_run_grid takes them */
int rs_driver_expand_grid(const RsDriverInput *in, const RsGridSource *const *grids, const InputSettings *settings,
                          LocalParameters *local, double *merged, int32_t *status, int32_t *missing_index,
                          int32_t device);

/* ------------------------------------------------------------------------
 * Layer 5: the device side of `module RoadSurf`'s per-step procedures
 * (roadsurf_amd/fortran/RoadSurfCompat.f90 over roadsurf_amd/csrc/rs_compat.hip; reference:
 * src/RoadSurf.f90:6-270, driven by examples/example1/src/Simulation.f90:57-115).  ONE point, ONE time
 * index per call: a compatibility path for callers that own the time loop, not a fast one.
 * ---------------------------------------------------------------------- */
typedef struct RsCompat RsCompat;
/* the caller's series of one point (HOST pointers, [SimLen] each, reference layout; NULL = absent) */
typedef struct RsCompatArrays {
  const double *tair, *tdew, *vz, *rhz, *prec, *sw, *lw, *sw_dir, *lw_net, *tsurfobs, *depth;
  const int32_t *precphase, *hour;
  const double *horizons; /* [360] */
  double *out[6];         /* Tsurf, Snow, Water, Ice, Deposit, Ice2: rows a coupling replay rewrites */
} RsCompatArrays;
/* state_out: the point's state column, RS_COMPAT_NSTATE doubles in the order of roadsurf_amd/csrc/rs_state.h */
#define RS_COMPAT_NSTATE (RS_MAX_LAYERS + 17 + 21 + 2 * RS_MAX_LAYERS)
RsCompat *rs_compat_begin(const RsConstants *consts, const LocalParameters *local, double tbottom,
                          const RsCompatArrays *arrays, const double *sun, const double *geo,
                          double albedo_surroundings, double *state_out);
int rs_compat_step(RsCompat *ctx, int32_t i, double *state_out, double *edits);
int rs_compat_replay(RsCompat *ctx, int32_t i, double *state_out, int32_t *rewritten);
int rs_compat_last_state(const RsCompat *ctx, double *state_out);
int rs_compat_outputs(const RsCompat *ctx, int32_t i, double *out6);
int32_t rs_compat_failed_index(const RsCompat *ctx);
void rs_compat_end(RsCompat *ctx);

/* Hash of the sources this library was built from (16 hex digits; roadsurf_amd/provenance.py build_sha16()):
 * tests/conftest.py rebuilds a prebuilt library whose stamp is not the hash of the sources beside it. */
const char *rs_build_sha16(void);
#define RS_ABI_VERSION 11 /* 2: round 2 additions (forecast re-sort, coupling rounds, fan-out, writeback, failure index); 3: RsPreview::index, rs_hip_expand_forcing_ordered, rs_hip_clock_probe, rs_driver_last_tiles; 4: RsPointParams::horizon_index, rs_hip_step_knots; 5: RS_SUN_COLS 6, RsPointParams::horizons_by_point; 6: rs_driver_last_raw_launches (rs_driver_run without forcing windows); 7: rs_compat_* (module RoadSurf's per-step procedures); 8: RsPreview::prec; 9: RsPreview::tair_b / vz_b / w; 10: rs_hip_outputs_by_point; 11: rs_hip_set_diagnostics / rs_hip_diagnostics, RsHostExtras::diagnostics */
int rs_abi_version(void);
/* sizeof of the boundary structs as the C side / the Fortran side see them
 * (0 InputPointers, 1 OutputPointers, 2 InputSettings, 3 InputParameters,
 * 4 LocalParameters, 5 RsConstants; rs_abi_sizeof alone goes on through the structs of the device API and the
 * driver, to 23 RsDriverRequest); bindings assert that they agree. */
int64_t rs_abi_sizeof(int which);
int64_t rs_fortran_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif /* ROADSURF_H */
