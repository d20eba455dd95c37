/*
 * rs_driver.hip — layer 4 of include/roadsurf.h: the reference DRIVER's data path
 * (examples/example1/src: JsonSource.cpp, DataHandler.cpp, MeteorologyTools.cpp,
 * roadrunner.cpp read_input/save_output) with the per-value work on the device.
 *
 * Data flow per tile of points:
 *   raw host series [point][time] --H2D--> LDS-tiled transpose --> raw[time][point] in HBM
 *   humidity_fill_kernel       Tdew <-> RH completion           (JsonSource.cpp:288-295)
 *   scan_raw_kernel            per variable: first missing index, latest observation,
 *                              latest road-temperature observation (one pass over the series)
 *   finalize_kernel            read_input's decisions per point    (roadrunner.cpp:186-275)
 *   per time chunk:
 *     expand_raw_kernel        JsonSource::interpolate + GetWeather overlay, written as the
 *                              [t][point] windows the step kernels read
 *     step kernel              (layers 1-3), outputs decimated in the kernel
 *   outputs [row][point] --transpose--> [point][row] --D2H--> caller
 *   kept_rows_kernel           on request (rs_driver_run_kept): the merged series at the kept rows, from the raw
 *                              series and plans that are still there, and deficit_kernel over them and the result
 *   episodes                   on request (rs_driver_run_episodes): the result block's rows, and that deficit, fed to
 *                              every point's automaton (rs_cluster.hip), finished, [cols][point] -> [point][cols]
 *
 * JsonSource::interpolate walks the raw and the simulation time axes together; which raw
 * interval a simulation index falls into, and whether it copies or interpolates there,
 * depends on the TIMES only.  All points of a source share its time axis, so the walk is
 * run once per source on the host (build_plan: the reference's loop, statement for
 * statement, quirks included) and the device applies the resulting per-index plan to every
 * point's data with the reference's arithmetic and missing-value tests.
 *
 * The kernels are streaming (HBM-bound): one variable per blockIdx.y, one point per lane,
 * time in the loop, the two raw neighbours cached in registers and re-read only when the
 * plan moves to another raw interval.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <mutex>
#include <vector>

#include "../../include/roadsurf.h"
#include "rs_devutil.hpp"
#include "rs_state.h"
#include "rs_devices.hpp"
#include "rs_driver_ens.hpp"
#include "rs_ens_table.hpp"
#include "rs_group_rule.hpp"
#include "rs_kernels.h"
#include "rs_raw.hpp"

extern "C" void rs_host_set_error(const char *msg);

namespace {

using rsu::Dev;
using rsu::transpose;

#ifndef RS_DRIVER_RAW_CHUNK
#define RS_DRIVER_RAW_CHUNK 120 /* indices per launch of a block whose step kernel reads the raw series (round 5, with the class key: 120 beats 240 by 1 % without coupling, 3-4 % with; 60 and 180 between) */
#endif
constexpr int NFLD = rs::RAW_NFLD;
/* order of `merged` in rs_driver_expand and of the window buffers (rs_raw.hpp) */
enum { R_TAIR = rs::RAW_TAIR, R_TDEW = rs::RAW_TDEW, R_VZ = rs::RAW_VZ, R_RHZ = rs::RAW_RHZ, R_PREC = rs::RAW_PREC,
       R_SW = rs::RAW_SW, R_LW = rs::RAW_LW, R_SWDIR = rs::RAW_SWDIR, R_LWNET = rs::RAW_LWNET, R_OBS = rs::RAW_OBS };
enum { K_NONE = rs::RAW_NONE, K_COPY = rs::RAW_COPY, K_INTERP = rs::RAW_INTERP };
using PlanStep = rs::RawPlanStep; /* one per source and simulation index (rs_raw.hpp) */
__device__ __forceinline__ PlanStep plan_at(const PlanStep *plan, int32_t i) { return rs::raw_plan_at(plan, i); }

struct SrcDev {
  const double *fld[NFLD]; /* [n_times][np_pad], nullptr = variable absent */
  const PlanStep *plan;    /* [SimLen]; shared time axis only */
  /* per-point time axes (RsRawSource.times_per_point): the walk runs per lane */
  const int64_t *ptimes;   /* [n_times][np_pad] or nullptr */
  const int32_t *plen;     /* [np_pad] series lengths */
  int32_t *prp;            /* [np_pad] rawPos of the walk at the start of the current window */
  int32_t n_times;
  int32_t is_obs;
};

struct SrcSet {
  SrcDev src[RS_MAX_SOURCES];
  int32_t nsrc;
  int32_t simlen;
  int64_t np_pad;
  int64_t npoints;
  int64_t sim0; /* simulation index i is at sim0 + i*dt seconds (JsonSource.cpp:199-205) */
  int32_t dt;
};

__device__ __forceinline__ double miss_r() { return rs::raw_miss(); }
__device__ __forceinline__ double threshold(int fld) { return rs::raw_threshold(fld); }
__device__ __forceinline__ bool source_value(const PlanStep &st, double a, double b, double thr, double &v) {
  return rs::raw_source_value(st, a, b, thr, v);
}

/* ---- per-point time axes: JsonSource::interpolate's walk (JsonSource.cpp:57-85,113-114,171)
 * evaluated per lane instead of once per source on the host.  State of the walk = rawPos. */
constexpr int32_t PP_DEAD = 0x3fffffff; /* the while loop can never run (again) for this series */

/* rawPos before the first simulation index (JsonSource.cpp:60-82) */
__device__ __forceinline__ int32_t pp_initial(const SrcDev &sd, int64_t np_pad, int64_t p,
                                              int64_t sim0) {
  const int32_t len = sd.plen[p];
  if (len <= 0) return PP_DEAD; /* JsonSource.cpp:233-237 */
  if (sd.ptimes[p] < sim0) {
    int32_t k = 0;
    for (; k < len; ++k)
      if (sd.ptimes[(int64_t)k * np_pad + p] >= sim0) break;
    return k - 1;
  }
  return 0;
}

struct PpWalk {
  int32_t rp, len, cached; /* cached: the rawPos tr/tr1 belong to, -1 none */
  int64_t tr, tr1;
};

__device__ __forceinline__ void pp_begin(PpWalk &w, const SrcDev &sd, int64_t p, int32_t rp0) {
  w.rp = rp0;
  w.len = sd.plen[p];
  w.cached = -1;
  w.tr = w.tr1 = 0;
}

/* One pass of the reference's while loop for simulation time ts: what happens to this index. */
__device__ __forceinline__ PlanStep pp_step(PpWalk &w, const SrcDev &sd, int64_t np_pad, int64_t p,
                                            int64_t ts) {
  PlanStep st;
  st.kind = K_NONE;
  st.rp = 0;
  st.num = 0.0;
  st.den = 1.0;
  st.rden = 0.0; /* per-lane denominators: IEEE division */
  if (w.rp + 1 >= w.len) return st; /* `while (rawPos+1 < rawLen ...)` is over */
  if (w.cached != w.rp) {
    w.tr = sd.ptimes[(int64_t)w.rp * np_pad + p];
    w.tr1 = sd.ptimes[(int64_t)(w.rp + 1) * np_pad + p];
    w.cached = w.rp;
  }
  if (ts < w.tr) return st; /* simulation starts before the data: the walk has not begun */
  if (ts == w.tr) {
    st.kind = K_COPY;
    st.rp = w.rp;
  } else if (ts == w.tr1) {
    /* rawPos++ and the loop condition is tested again for the same simulation index */
    w.rp += 1;
    if (w.rp + 1 >= w.len) {
      w.rp = PP_DEAD;
      return st;
    }
    w.tr = w.tr1;
    w.tr1 = sd.ptimes[(int64_t)(w.rp + 1) * np_pad + p];
    w.cached = w.rp;
    st.kind = K_COPY;
    st.rp = w.rp;
  } else {
    st.kind = K_INTERP;
    st.rp = w.rp;
    st.num = (double)(ts - w.tr);
    st.den = (double)(w.tr1 - w.tr);
  }
  return st;
}

/* Sequential pass over simulation indices [i0, i1) of one variable of one point.
 * visit(i, merged value, bitmask of the sources that supplied a value).
 * rp0[s]: rawPos at i0 for sources with per-point time axes. */
template <bool PP, class Visit> /* PP: some source has per-point time axes */
__device__ __forceinline__ void walk_field(const SrcSet &S, int fld, int64_t p, int32_t i0,
                                           int32_t i1, const int32_t *rp0, Visit &&visit) {
  const double thr = threshold(fld);
  double a[RS_MAX_SOURCES], b[RS_MAX_SOURCES];
  int32_t cur[RS_MAX_SOURCES];
  PpWalk pw[RS_MAX_SOURCES];
#pragma unroll
  for (int s = 0; s < RS_MAX_SOURCES; ++s) {
    a[s] = b[s] = 0.0;
    cur[s] = -2;
    pw[s].rp = PP_DEAD;
    pw[s].len = 0;
    pw[s].cached = -1;
    pw[s].tr = pw[s].tr1 = 0;
    if (PP && s < S.nsrc && S.src[s].ptimes) pp_begin(pw[s], S.src[s], p, rp0[s]);
  }
  /* the variable's column and the plan of every source, once (fld indexes the kernel arguments
   * dynamically: left inside, that is a scalar load per source and time index) */
  const double *xs[RS_MAX_SOURCES];
  const PlanStep *plans[RS_MAX_SOURCES];
#pragma unroll
  for (int s = 0; s < RS_MAX_SOURCES; ++s) {
    xs[s] = (s < S.nsrc) ? S.src[s].fld[fld] : nullptr;
    plans[s] = (s < S.nsrc) ? S.src[s].plan : nullptr;
  }
  const int64_t np_pad = S.np_pad;
  for (int32_t i = i0; i < i1; ++i) {
    double v = miss_r();
    uint32_t mask = 0;
#pragma unroll
    for (int s = 0; s < RS_MAX_SOURCES; ++s) {
      if (s >= S.nsrc) continue;
      const double *x = xs[s];
      PlanStep st;
      if (PP && S.src[s].ptimes) {
        /* the walk advances whether or not this source has the variable */
        st = pp_step(pw[s], S.src[s], np_pad, p, S.sim0 + (int64_t)i * S.dt);
      } else {
        if (!x) continue;
        st = plan_at(plans[s], i); /* uniform: one scalar load */
      }
      if (!x || st.kind == K_NONE) continue;
      if (st.rp != cur[s]) {
        a[s] = x[(int64_t)st.rp * np_pad + p];
        b[s] = x[(int64_t)(st.rp + 1) * np_pad + p];
        cur[s] = st.rp;
      }
      double vs;
      if (source_value(st, a[s], b[s], thr, vs)) { /* DataHandler.cpp:75-84: later sources win */
        v = vs;
        mask |= 1u << s;
      }
    }
    visit(i, v, mask);
  }
}

/* rawPos at simulation index 0 of every per-point source */
__device__ __forceinline__ void initial_positions(const SrcSet &S, int64_t p, int32_t *rp0) {
#pragma unroll
  for (int s = 0; s < RS_MAX_SOURCES; ++s)
    rp0[s] = (s < S.nsrc && S.src[s].ptimes) ? pp_initial(S.src[s], S.np_pad, p, S.sim0) : 0;
}

/* Random access to the merged value (used for the relaxation targets). */
__device__ __forceinline__ double merged_at(const SrcSet &S, int fld, int64_t p, int32_t i) {
  const double thr = threshold(fld);
  double v = miss_r();
  for (int s = 0; s < S.nsrc; ++s) {
    const double *x = S.src[s].fld[fld];
    if (!x) continue;
    PlanStep st;
    if (S.src[s].ptimes) { /* replay the walk up to i */
      PpWalk w;
      pp_begin(w, S.src[s], p, pp_initial(S.src[s], S.np_pad, p, S.sim0));
      st.kind = K_NONE;
      for (int32_t k = 0; k <= i; ++k) st = pp_step(w, S.src[s], S.np_pad, p, S.sim0 + (int64_t)k * S.dt);
    } else {
      st = plan_at(S.src[s].plan, i);
    }
    if (st.kind == K_NONE) continue;
    const double a = x[(int64_t)st.rp * S.np_pad + p], b = x[(int64_t)(st.rp + 1) * S.np_pad + p];
    double vs;
    if (source_value(st, a, b, thr, vs)) v = vs;
  }
  return v;
}

/* roadrunner.cpp:42-45 */
__device__ __forceinline__ bool is_missing(double v) { return (v != v) || v < -9000; }

struct ScanArgs {
  SrcSet S;
  int32_t *first_missing; /* [6][np_pad]: tair, Rhz, prec, SW, LW, VZ (roadrunner.cpp:188-229) */
  int32_t *last_obs;      /* [np_pad] DataHandler::GetLatestObsIndex, -1 if none */
  int32_t *cpl_i;         /* [np_pad] last index with a road temperature observation, -1 */
  double *cpl_t;          /* [np_pad] that observation */
};

template <bool PP>
__global__ void __launch_bounds__(RS_BLOCK) scan_raw_kernel(const ScanArgs A) {
  __builtin_amdgcn_s_setprio(3); /* before a block's first time step: all of it is waited for */
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= A.S.npoints) return;
  const int y = blockIdx.y;
  const int L = A.S.simlen;
  int32_t rp0[RS_MAX_SOURCES] = {0, 0, 0, 0};
  if (PP) initial_positions(A.S, p, rp0);
  if (y < 6) {
    const int fld = (y == 0) ? R_TAIR : (y == 1) ? R_RHZ : (y == 2) ? R_PREC : (y == 3) ? R_SW
                  : (y == 4) ? R_LW : R_VZ;
    uint32_t obsmask = 0;
    for (int s = 0; s < A.S.nsrc; ++s)
      if (A.S.src[s].is_obs) obsmask |= 1u << s;
    int32_t first = L, last = -1;
    walk_field<PP>(A.S, fld, p, 0, L, rp0, [&](int32_t i, double v, uint32_t mask) {
      if (first == L && is_missing(v)) first = i;
      /* JsonSource.cpp:412-416: `for i = SimLen..1: if tair[i-1] > -100 return i`, on the
       * source's OWN interpolated series; DataHandler.cpp:118-137 takes the max over the
       * observation sources */
      if (mask & obsmask) last = i + 1;
    });
    A.first_missing[(int64_t)y * A.S.np_pad + p] = first;
    if (y == 0) A.last_obs[p] = last;
  } else {
    int32_t ci = -1;
    double ct = miss_r();
    /* roadrunner.cpp:256-261: last index whose TSurfObs is neither missing nor < -100 */
    walk_field<PP>(A.S, R_OBS, p, 0, L, rp0, [&](int32_t i, double v, uint32_t) {
      if (!(is_missing(v) || v < -100)) {
        ci = i;
        ct = v;
      }
    });
    A.cpl_i[p] = ci;
    A.cpl_t[p] = ct;
  }
}

/* Shared time axes: a SEGMENT is a run of simulation indices over which every source keeps its
 * (kind, rawPos).  Whether a source supplies a value is then the same at every index of the run:
 * K_COPY: raw[rawPos] > threshold; K_INTERP: both ends > threshold - the interpolated value lies
 * between them (the weight num/den is at most 1 - 1/den, so the rounded increment is smaller in
 * magnitude than the rounded difference of the ends) and passes GetWeather's own test with them.
 * That holds for finite ends; a run with a non-finite end above the threshold is walked index by
 * index like the general scan.  ~250 segments instead of SimLen = 5 761 indices per point and
 * variable: the scan was 18 ms of a block's 35 ms before its first time step. */
using ScanSeg = rs::RawSeg;

__device__ __forceinline__ bool rs_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

/* merged value at one index, shared axes (walk_field's body for a single i) */
__device__ __forceinline__ double merged_one(const SrcSet &S, int fld, int64_t p, int32_t i, uint32_t &mask) {
  const double thr = threshold(fld);
  double v = miss_r();
  mask = 0;
  for (int s = 0; s < S.nsrc; ++s) {
    const double *x = S.src[s].fld[fld];
    if (!x) continue;
    const PlanStep st = plan_at(S.src[s].plan, i);
    if (st.kind == K_NONE) continue;
    const double a = x[(int64_t)st.rp * S.np_pad + p], b = x[(int64_t)(st.rp + 1) * S.np_pad + p];
    double vs;
    if (source_value(st, a, b, thr, vs)) {
      v = vs;
      mask |= 1u << s;
    }
  }
  return v;
}

__global__ void __launch_bounds__(RS_BLOCK) scan_seg_kernel(const ScanArgs A, const ScanSeg *segs, int32_t nseg) {
  __builtin_amdgcn_s_setprio(3); /* before a block's first time step: all of it is waited for */
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= A.S.npoints) return;
  const int y = blockIdx.y;
  const int L = A.S.simlen;
  const int fld = (y == 0) ? R_TAIR : (y == 1) ? R_RHZ : (y == 2) ? R_PREC : (y == 3) ? R_SW
                : (y == 4) ? R_LW : (y == 5) ? R_VZ : R_OBS;
  const double thr = threshold(fld);
  uint32_t obsmask = 0;
  for (int s = 0; s < A.S.nsrc; ++s)
    if (A.S.src[s].is_obs) obsmask |= 1u << s;
  const double *xs[RS_MAX_SOURCES];
#pragma unroll
  for (int s = 0; s < RS_MAX_SOURCES; ++s) xs[s] = (s < A.S.nsrc) ? A.S.src[s].fld[fld] : nullptr;
  const int64_t np_pad = A.S.np_pad;
  int32_t first = L, last = -1, ci = -1;
  const ScanSeg __attribute__((address_space(4))) *sg = (const ScanSeg __attribute__((address_space(4))) *)segs;
  for (int32_t k = 0; k < nseg; ++k) {
    const int32_t i0 = sg[k].i0, i1 = sg[k].i1;
    uint32_t mask = 0;
    bool slow = false;
#pragma unroll
    for (int s = 0; s < RS_MAX_SOURCES; ++s) {
      if (s >= A.S.nsrc || !xs[s]) continue;
      const int32_t kind = sg[k].kind[s], rp = sg[k].rp[s];
      if (kind == K_NONE) continue;
      const double a = xs[s][(int64_t)rp * np_pad + p];
      if (kind == K_COPY) {
        if (a > thr) mask |= 1u << s;
      } else {
        const double b = xs[s][(int64_t)(rp + 1) * np_pad + p];
        if (a > thr && b > thr) {
          mask |= 1u << s;
          if (!rs_finite(a) || !rs_finite(b)) slow = true;
        }
      }
    }
    if (slow) { /* an infinite end: index by index, as the general scan does */
      for (int32_t i = i0; i < i1; ++i) {
        uint32_t mi;
        const double v = merged_one(A.S, fld, p, i, mi);
        if (y < 6) {
          if (first == L && is_missing(v)) first = i;
          if (mi & obsmask) last = i + 1;
        } else if (!(is_missing(v) || v < -100)) {
          ci = i;
        }
      }
      continue;
    }
    if (y < 6) {
      if (first == L && mask == 0) first = i0; /* nobody supplies a value: the merged series is missing */
      if (mask & obsmask) last = i1;           /* (the run's last index) + 1 */
    } else if (mask != 0) {
      ci = i1 - 1; /* a supplied value is > -100: roadrunner.cpp:256-261 takes it */
    }
  }
  if (y < 6) {
    A.first_missing[(int64_t)y * np_pad + p] = first;
    if (y == 0) A.last_obs[p] = last;
  } else {
    double ct = miss_r();
    if (ci >= 0) {
      uint32_t mi;
      ct = merged_one(A.S, R_OBS, p, ci, mi);
    }
    A.cpl_i[p] = ci;
    A.cpl_t[p] = ct;
  }
}

struct FinalArgs {
  SrcSet S;
  const int32_t *first_missing, *last_obs, *cpl_i;
  const double *cpl_t;
  int32_t use_relaxation, use_coupling, cplLen, default_initlen;
  int32_t ignore_from; /* a missing value at this 0-based index or behind it rejects nobody (INT32_MAX: read_input's own rule) */
  /* out, [np_pad] */
  int32_t *status, *missing_index, *initlen, *cpl_index, *cpl_hi;
  double *tair_relax, *vz_relax, *rh_relax, *cpl_tsurf;
};

/* read_input after GetWeather, roadrunner.cpp:186-275 */
__global__ void __launch_bounds__(RS_BLOCK) finalize_kernel(const FinalArgs A) {
  __builtin_amdgcn_s_setprio(3); /* before a block's first time step: all of it is waited for */
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= A.S.np_pad) return;
  const int L = A.S.simlen;
  int32_t status = 0, mi = L;
  if (p < A.S.npoints) {
    for (int k = 0; k < 6; ++k) {
      const int32_t fm = A.first_missing[(int64_t)k * A.S.np_pad + p];
      if (fm < mi && fm < A.ignore_from) { /* strict: at equal index the earlier test in the reference's order wins */
        mi = fm;
        status = k + 1;
      }
    }
  }
  int32_t initlen = A.default_initlen; /* roadrunner.cpp:168-169 */
  double tr = miss_r(), vr = miss_r(), rr = miss_r();
  int32_t cidx = -9999, chi = -1;
  double ctsurf = miss_r();
  if (p < A.S.npoints && status == 0) {
    if (A.use_relaxation == 1) { /* roadrunner.cpp:235-250 */
      const int32_t idx = A.last_obs[p];
      if (idx > -1) {
        initlen = idx;
        if (idx >= L) {
          status = 7; /* the reference reads data.tair[SimLen] here */
        } else {
          tr = merged_at(A.S, R_TAIR, p, idx);
          vr = merged_at(A.S, R_VZ, p, idx);
          rr = merged_at(A.S, R_RHZ, p, idx);
        }
      }
    }
    if (A.use_coupling == 1 && status == 0) { /* roadrunner.cpp:253-275 */
      const int32_t i = A.cpl_i[p];
      if (i >= A.cplLen) {
        ctsurf = A.cpl_t[p];
        cidx = i;
        chi = i;
      }
    }
  }
  A.status[p] = status;
  A.missing_index[p] = (status >= 1 && status <= 6) ? mi : -1;
  A.initlen[p] = initlen;
  A.tair_relax[p] = tr;
  A.vz_relax[p] = vr;
  A.rh_relax[p] = rr;
  A.cpl_index[p] = cidx;
  A.cpl_tsurf[p] = ctsurf;
  A.cpl_hi[p] = chi;
}

struct ExpandRawArgs {
  SrcSet S;
  double *out[NFLD]; /* [nsteps][stride] windows; nullptr = not wanted */
  const int32_t *status; /* [np_pad] or nullptr */
  const int32_t *cpl_hi; /* [np_pad] or nullptr */
  int32_t cplLen;
  int32_t i0, nsteps; /* 0-based first simulation index of the window */
  int64_t stride;
  const int32_t *order; /* plan order (rs_hip_recluster): window column s holds point order[s];
                           nullptr = natural order */
};

template <bool PP>
__global__ void __launch_bounds__(RS_BLOCK) expand_raw_kernel(const ExpandRawArgs A) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a block: all of it is waited for */
  const int64_t slot = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  const int fld = blockIdx.y;
  double *out = A.out[fld];
  if (slot >= A.S.npoints || !out) return;
  out += slot;
  /* everything per point (raw columns, walk positions, decisions) is read at the point's own
   * index: the raw series are ~100x smaller than the window, gathering them is cheap */
  const int64_t p = A.order ? (int64_t)A.order[slot] : slot;
  /* a point read_input rejects is not simulated by the reference (roadrunner.cpp:393): a
   * missing air temperature makes CheckValues stop its lane at the first index (its output
   * rows are blanked afterwards, blank_rejected_kernel) */
  const bool rejected = A.status && A.status[p] != 0 && fld == R_TAIR;
  /* roadrunner.cpp:266-273: no road temperature input inside the coupling window */
  int32_t clr_lo = 0, clr_hi = -1;
  if (fld == R_OBS && A.cpl_hi) {
    clr_hi = A.cpl_hi[p];
    clr_lo = clr_hi - A.cplLen; /* exclusive */
    if (clr_hi < 0) clr_lo = clr_hi;
  }
  const int32_t i0 = A.i0;
  const int64_t stride = A.stride;
  int32_t rp0[RS_MAX_SOURCES];
#pragma unroll
  for (int s = 0; s < RS_MAX_SOURCES; ++s)
    rp0[s] = (PP && s < A.S.nsrc && A.S.src[s].ptimes) ? A.S.src[s].prp[p] : 0;
  walk_field<PP>(A.S, fld, p, i0, i0 + A.nsteps, rp0, [&](int32_t i, double v, uint32_t) {
    if (rejected) v = miss_r();
    if (i > clr_lo && i <= clr_hi) v = miss_r();
    out[(int64_t)(i - i0) * stride] = v;
  });
}

/* A point read_input rejects is never handed to runsimulation (roadrunner.cpp:393): all its
 * output rows read -9999.0 (OutputData.cpp:5-13).  Its lanes did run - stopped by CheckValues
 * at the first index, which still writes that index's row (src/InputOutput.f90:55-82 sets the
 * flag, examples/example1/src/Simulation.f90:100 leaves the loop after SaveOutput). */
__global__ void __launch_bounds__(RS_BLOCK) blank_rejected_kernel(double *out, int64_t stride,
                                                                  int32_t nrows, int64_t npoints,
                                                                  const int32_t *status) {
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= npoints || status[p] == 0) return;
  for (int f = 0; f < 6; ++f)
    for (int32_t r = 0; r < nrows; ++r) out[((int64_t)f * nrows + r) * stride + p] = -9999.0;
}

/* A few (variable, index) rows of the merged series in slot order - what the driver path still needs as
 * ROWS once the step kernel makes its own forcing from the raw series (rs_step_raw): air temperature and
 * road-temperature observation of index 1 for the initial profile (src/Initialization.f90:256-259), air
 * temperature and wind speed at the three preview indices of the forecast sort key.  Shared time axes. */
constexpr int RAWROWS_MAX = 12;
struct RawRowsArgs {
  SrcSet S;
  const int32_t *status, *order; /* as ExpandRawArgs */
  int32_t nrows;
  int32_t fld[RAWROWS_MAX], idx[RAWROWS_MAX]; /* variable and 0-based simulation index of row y */
  double *out[RAWROWS_MAX];                   /* [np_pad] each */
};
__global__ void __launch_bounds__(RS_BLOCK) raw_rows_kernel(const RawRowsArgs A) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a block: all of it is waited for */
  const int64_t slot = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  const int y = blockIdx.y;
  if (slot >= A.S.npoints || y >= A.nrows) return;
  const int64_t p = A.order ? (int64_t)A.order[slot] : slot;
  const int fld = A.fld[y];
  uint32_t mask;
  double v = merged_one(A.S, fld, p, A.idx[y], mask);
  if (A.status && A.status[p] != 0 && fld == R_TAIR) v = miss_r(); /* a rejected point: as expand_raw_kernel */
  A.out[y][slot] = v;
}

/* The merged series at the KEPT rows - 0-based simulation index r * step for kept row r, save_output's decimation
 * (roadrunner.cpp:303) - as read_input returns them (rs_driver_run_kept): bit for bit what expand_raw_kernel writes at
 * those indices for the test hook, which passes no status - a rejected point keeps its values.  One point per lane,
 * variable y of the launch's list in blockIdx.y, rows in the loop: stores are whole lines of out[row][np_pad].
 * Shared time axes: merged_one at each kept index - the plan entry one scalar load, the two raw ends coalesced across
 * the lanes.  Per-point axes: ONE sequential walk over [0, SimLen) from initial_positions() that stores at the kept
 * indices only; never from SrcDev::prp, which pp_advance_kernel moves during the time loop (the result must not depend
 * on when this runs), and never by merged_at, whose replay from index 0 per row would be quadratic. */
struct KeptRowsArgs {
  SrcSet S;
  int32_t nfld;
  int32_t fld[NFLD];     /* the launch's variables */
  double *out[NFLD];     /* [n_out][stride] each */
  const int32_t *cpl_hi; /* [np_pad] or nullptr, as ExpandRawArgs */
  int32_t cplLen;
  int32_t step, n_out;   /* (n_out - 1) * step < SimLen */
  int64_t stride;
};
template <bool PP>
__global__ void __launch_bounds__(RS_BLOCK) kept_rows_kernel(const KeptRowsArgs A) {
  __builtin_amdgcn_s_setprio(3); /* on a block's way out: waited for, beside other blocks' step kernels */
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  const int y = blockIdx.y;
  if (p >= A.S.npoints || y >= A.nfld) return;
  const int fld = A.fld[y];
  double *out = A.out[y] + p;
  /* roadrunner.cpp:266-273: no road temperature input inside the coupling window (as expand_raw_kernel) */
  int32_t clr_lo = 0, clr_hi = -1;
  if (fld == R_OBS && A.cpl_hi) {
    clr_hi = A.cpl_hi[p];
    clr_lo = clr_hi - A.cplLen; /* exclusive */
    if (clr_hi < 0) clr_lo = clr_hi;
  }
  const int32_t step = A.step;
  const int64_t stride = A.stride;
  if (!PP) {
    for (int32_t r = 0; r < A.n_out; ++r) {
      const int32_t i = r * step;
      uint32_t mask;
      double v = merged_one(A.S, fld, p, i, mask);
      if (i > clr_lo && i <= clr_hi) v = miss_r();
      out[(int64_t)r * stride] = v;
    }
  } else {
    int32_t rp0[RS_MAX_SOURCES];
    initial_positions(A.S, p, rp0);
    int32_t next = 0, r = 0; /* the next kept index and its row */
    walk_field<true>(A.S, fld, p, 0, A.S.simlen, rp0, [&](int32_t i, double v, uint32_t) {
      if (i != next) return;
      if (i > clr_lo && i <= clr_hi) v = miss_r();
      out[(int64_t)r * stride] = v;
      next += step;
      ++r;
    });
  }
}

/* The dew-point deficit of the kept rows, in place over the kept dew point: x[r][p] = tsurf[r][p] - x[r][p] where both
 * are not NaN and > -9000, else -9999.0 (roadsurf_amd/kept.py, dew_point_deficit).  tsurf: the final result rows. */
__global__ void __launch_bounds__(RS_BLOCK) deficit_kernel(const double *__restrict__ tsurf, double *x, int64_t stride,
                                                           int32_t nrows, int64_t npoints) {
  __builtin_amdgcn_s_setprio(3); /* on a block's way out: waited for, beside other blocks' step kernels */
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= npoints) return;
  for (int32_t r = 0; r < nrows; ++r) {
    const int64_t k = (int64_t)r * stride + p;
    const double a = tsurf[k], b = x[k];
    x[k] = (a > -9000.0 && b > -9000.0) ? a - b : -9999.0; /* (a NaN compares false) */
  }
}

/* Per-point walks: position at simulation index 0 ... */
__global__ void __launch_bounds__(RS_BLOCK) pp_init_kernel(const SrcSet S) {
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= S.npoints) return;
  for (int s = 0; s < S.nsrc; ++s)
    if (S.src[s].ptimes) S.src[s].prp[p] = pp_initial(S.src[s], S.np_pad, p, S.sim0);
}
/* ... and moved past the window [i0, i0+nsteps) that has just been expanded. */
__global__ void __launch_bounds__(RS_BLOCK) pp_advance_kernel(const SrcSet S, int32_t i0,
                                                              int32_t nsteps) {
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= S.npoints) return;
  for (int s = 0; s < S.nsrc; ++s) {
    if (!S.src[s].ptimes) continue;
    PpWalk w;
    pp_begin(w, S.src[s], p, S.src[s].prp[p]);
    for (int32_t i = i0; i < i0 + nsteps; ++i)
      (void)pp_step(w, S.src[s], S.np_pad, p, S.sim0 + (int64_t)i * S.dt);
    S.src[s].prp[p] = w.rp;
  }
}

/* per-point parameters into slot order */
__global__ void __launch_bounds__(RS_BLOCK) gather_params_kernel(
    const int32_t *__restrict__ order, int64_t npoints, const int32_t *initlen_p, int32_t *initlen_s,
    const double *tair_p, double *tair_s, const double *vz_p, double *vz_s, const double *rh_p,
    double *rh_s, const int32_t *cidx_p = nullptr, int32_t *cidx_s = nullptr,
    const double *ctsurf_p = nullptr, double *ctsurf_s = nullptr,
    const double *geo_p = nullptr, double *geo_s = nullptr, int64_t geo_stride = 0) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a block: all of it is waited for */
  const int64_t s = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (s >= npoints) return;
  const int64_t p = order[s];
  initlen_s[s] = initlen_p[p];
  tair_s[s] = tair_p[p];
  vz_s[s] = vz_p[p];
  rh_s[s] = rh_p[p];
  if (cidx_s) { /* coupling index and observation travel with the slot too */
    cidx_s[s] = cidx_p[p];
    ctsurf_s[s] = ctsurf_p[p];
  }
  if (geo_s) /* sky view factor, sin/cos of the latitude, longitude: four scalars; the 360-column horizon
                table stays in point order and is read through the order row (RsPointParams::horizon_index) */
    for (int q = 0; q < 4; ++q) geo_s[q * geo_stride + s] = geo_p[q * geo_stride + p];
}

/* output rows of one launch, written in slot order, into the natural-order result */
__global__ void __launch_bounds__(RS_BLOCK) unpermute_rows_kernel(
    const int32_t *__restrict__ order, int64_t npoints, const double *__restrict__ chunk_out,
    int64_t chunk_rows, double *final_out, int64_t final_rows, int64_t row0, int32_t nrows,
    int64_t stride) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a block: all of it is waited for */
  const int64_t s = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (s >= npoints) return;
  const int64_t p = order[s];
  const int f = blockIdx.y;
  for (int32_t r = 0; r < nrows; ++r)
    final_out[((int64_t)f * final_rows + row0 + r) * stride + p] =
        chunk_out[((int64_t)f * chunk_rows + r) * stride + s];
}

__global__ void __launch_bounds__(RS_BLOCK) fill_i32_kernel(int32_t *x, int64_t n, int32_t v) {
  const int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (i < n) x[i] = v;
}
__global__ void __launch_bounds__(RS_BLOCK) fill_f64_kernel(double *x, int64_t n, double v) {
  const int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (i < n) x[i] = v;
}

/* columns [m, mp) of row blockIdx.x of x[rows][mp] */
__global__ void __launch_bounds__(RS_BLOCK) fill_pad_kernel(double *x, int64_t m, int64_t mp, double v) {
  double *row = x + (int64_t)blockIdx.x * mp;
  for (int64_t c = m + threadIdx.x; c < mp; c += RS_BLOCK) row[c] = v;
}

/* The raw columns of one source of a members' tile from the columns of its stations' tile (rs_driver_run_ensemble):
 * column p of every array takes column parent[p] of the stations' - 64-bit words copied as they are, so values, the
 * humidity completion the stations' tile has made, per-point time stamps and their padding arrive bit for bit; the
 * columns [m, mp) read the missing value (time stamps 0, lengths 0).  One array per blockIdx.y - the NFLD variables,
 * then the per-point time axis with the lengths -, one member per lane, rows in the loop: the stores are whole lines,
 * the loads the lines of the (non-decreasing) parents. */
struct ParentCopyArgs {
  const uint64_t *src[NFLD + 1]; /* [n_times][src_stride], nullptr = absent */
  uint64_t *dst[NFLD + 1];       /* [n_times][mp] */
  const int32_t *src_len;        /* [src_stride] or nullptr: with the time axis */
  int32_t *dst_len;              /* [mp] */
  const int32_t *parent;         /* [m], every entry a live column of the stations' tile */
  int32_t n_times;
  int64_t src_stride, mp, m;
};
__global__ void __launch_bounds__(RS_BLOCK) parent_copy_kernel(const ParentCopyArgs A) {
  __builtin_amdgcn_s_setprio(3); /* before a block's first time step: all of it is waited for */
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  const int y = blockIdx.y;
  const uint64_t *src = A.src[y];
  uint64_t *dst = A.dst[y];
  if (p >= A.mp || !src || !dst) return;
  const bool live = p < A.m;
  const int64_t q = live ? (int64_t)A.parent[p] : 0;
  const uint64_t pad = y < NFLD ? (uint64_t)__double_as_longlong(-9999.9) : 0;
  src += q;
  dst += p;
  for (int32_t t = 0; t < A.n_times; ++t) dst[(int64_t)t * A.mp] = live ? src[(int64_t)t * A.src_stride] : pad;
  if (y == NFLD && A.src_len) A.dst_len[p] = live ? A.src_len[q] : 0;
}

/* slot s takes src[order[s]] (a members' tile in plan order: the stations' column of the horizon table per slot) */
__global__ void __launch_bounds__(RS_BLOCK) gather_i32_kernel(const int32_t *__restrict__ order, int64_t npoints,
                                                              const int32_t *__restrict__ src, int32_t *dst) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a block: all of it is waited for */
  const int64_t s = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (s < npoints) dst[s] = src[order[s]];
}

void launch_expand_raw(bool any_pp, int64_t mp, const ExpandRawArgs &ea, hipStream_t stream) {
  const dim3 g((unsigned)(mp / RS_BLOCK), NFLD), b(RS_BLOCK);
  if (any_pp)
    hipLaunchKernelGGL(expand_raw_kernel<true>, g, b, 0, stream, ea);
  else
    hipLaunchKernelGGL(expand_raw_kernel<false>, g, b, 0, stream, ea);
}

inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + RS_BLOCK - 1) / RS_BLOCK)); }

/* ---- host side ------------------------------------------------------------------ */

int fail_msg(const char *msg, int code) {
  rs_host_set_error(msg);
  return code;
}
int fail_hip(const char *what, hipError_t e) {
  char buf[300];
  snprintf(buf, sizeof(buf), "rs_driver: %s: %s", what, hipGetErrorString(e));
  rs_host_set_error(buf);
  return -10;
}
#define HOK(expr)                                     \
  do {                                                \
    hipError_t e_ = (expr);                           \
    if (e_ != hipSuccess) return fail_hip(#expr, e_); \
  } while (0)

/* The time walk of JsonSource::interpolate (JsonSource.cpp:49-85,113-114,171-175) without
 * the data: which raw interval each simulation index uses and how. */
void build_plan(const int64_t *rawtime, int rawLen, const std::vector<int64_t> &simtime,
                std::vector<PlanStep> &plan) {
  const int simLen = (int)simtime.size();
  plan.assign(simLen, PlanStep{K_NONE, 0, 0.0, 1.0, 0.0});
  if (rawLen == 0) return; /* JsonSource.cpp:233-237 */
  int rawPos = 0, simPos = 0;
  if (rawtime[0] < simtime[0]) {
    for (rawPos = 0; rawPos < rawLen; ++rawPos)
      if (rawtime[rawPos] >= simtime[0]) break;
    rawPos = rawPos - 1;
    simPos = 0;
  } else if (simtime[0] < rawtime[0]) {
    for (simPos = 0; simPos < simLen; ++simPos)
      if (simtime[simPos] >= rawtime[0]) break;
    rawPos = 0;
  }
  while (rawPos + 1 < rawLen && simPos < simLen) {
    if (std::llabs(simtime[simPos] - rawtime[rawPos]) < 0.01) {
      plan[simPos] = PlanStep{K_COPY, rawPos, 0.0, 1.0, 0.0};
      simPos++;
    } else if (std::llabs(simtime[simPos] - rawtime[rawPos + 1]) < 0.01) {
      rawPos++;
    } else {
      const double den = (double)(rawtime[rawPos + 1] - rawtime[rawPos]);
      /* a positive whole number of seconds below 2^53: its significand is never all ones, the
       * one case rs_div_u's reciprocal does not cover; anything else divides the IEEE way */
      /* ... and for 0 < num < den < 2^40 (times that increase, as the reference assumes) the interpolated
       * value provably lies between the two raw ends (rs_raw.hpp): what the segment scan and the step
       * kernel's own interpolation (rs_kernels.hip raw_forcing) rely on; an entry outside that is marked
       * by rden = 0 and handled index by index */
      const double num = (double)(simtime[simPos] - rawtime[rawPos]);
      const double rden = (den >= 1.0 && den < 1.0995e12 && num > 0.0 && num < den) ? 1.0 / den : 0.0;
      plan[simPos] = PlanStep{K_INTERP, rawPos, num, den, rden};
      simPos++;
    }
  }
}

const double *raw_field(const RsRawSource &s, int fld) {
  switch (fld) {
    case R_TAIR: return s.tair;
    case R_TDEW: return s.tdew;
    case R_VZ: return s.vz;
    case R_RHZ: return s.rhz;
    case R_PREC: return s.prec;
    case R_SW: return s.sw;
    case R_LW: return s.lw;
    case R_SWDIR: return s.sw_dir;
    case R_LWNET: return s.lw_net;
    default: return s.tsurfobs;
  }
}

const double *grid_field(const RsGridSource &g, int fld) {
  switch (fld) {
    case R_TAIR: return g.tair;
    case R_TDEW: return g.tdew;
    case R_VZ: return g.vz;
    case R_RHZ: return g.rhz;
    case R_PREC: return g.prec;
    case R_SW: return g.sw;
    case R_LW: return g.lw;
    case R_SWDIR: return g.sw_dir;
    case R_LWNET: return g.lw_net;
    default: return g.tsurfobs;
  }
}

/* The fields of a call's gridded sources on one device, [n_times][n_nodes] as the caller holds them: uploaded once
 * before the blocks start, shared by the blocks of a fan-out on that device, freed when the call returns. */
struct GridDevice {
  int device = 0;
  Dev fld[RS_MAX_SOURCES][NFLD];
  ~GridDevice() { (void)hipSetDevice(device); }
};
/* A call's gridded sources as one block of it sees them (NULL: the call has none) */
struct GridView {
  const RsGridSource *const *grids; /* [n_sources], NULL entry = per-point source */
  const GridDevice *dev;            /* the block's device */
};

struct Common {
  const RsGridSource *grid[RS_MAX_SOURCES] = {};         /* non-NULL: source s arrives as fields (RsGridSource) */
  const double *grid_dev[RS_MAX_SOURCES][NFLD] = {};     /* ... and its fields on this block's device */
  int n = 0, nsrc = 0, L = 0, DT = 0;
  int default_initlen = 0, cplLen = 0;
  std::vector<int64_t> simtime;
  std::vector<std::vector<PlanStep>> plans;
  std::vector<ScanSeg> segs; /* shared axes only (scan_seg_kernel); empty: some source has per-point axes */
  std::vector<std::vector<int32_t>> active_prefix; /* [source][i]: plan entries != K_NONE among indices < i */
};

int prepare(const RsDriverInput *in, const InputSettings *st, Common &c, const GridView *gv = nullptr) {
  if (!in || !st || in->n_points < 1 || in->n_sources < 1 || in->n_sources > RS_MAX_SOURCES ||
      !in->sources)
    return fail_msg("rs_driver: bad arguments (n_points >= 1, 1 <= n_sources <= RS_MAX_SOURCES)", -1);
  if (st->SimLen < 1 || !(st->DTSecs >= 1.0))
    return fail_msg("rs_driver: SimLen >= 1 and DTSecs >= 1 required", -1);
  c.n = in->n_points;
  c.nsrc = in->n_sources;
  c.L = st->SimLen;
  c.DT = (int)st->DTSecs; /* JsonSource takes `const int DTSecs` */
  c.simtime.resize(c.L);
  for (int k = 0; k < c.L; ++k) c.simtime[k] = in->start_time + (int64_t)k * c.DT;
  /* roadrunner.cpp:168-169: time_t / double, truncated */
  c.default_initlen = 1 + (int)((double)(in->forecast_time - in->start_time) / st->DTSecs);
  /* roadrunner.cpp:263: static_cast<int>(coupling_minutes * 60 / DTSecs) */
  c.cplLen = (int)((double)(st->coupling_minutes * 60) / st->DTSecs);
  c.plans.resize(c.nsrc);
  for (int s = 0; s < c.nsrc && gv; ++s) {
    if (!(c.grid[s] = gv->grids[s])) continue;
    for (int f = 0; f < NFLD; ++f) c.grid_dev[s][f] = gv->dev->fld[s][f].as<double>();
  }
  for (int s = 0; s < c.nsrc; ++s) {
    const RsRawSource &rs = in->sources[s];
    if (rs.n_times < 0 || (rs.n_times > 0 && !rs.times))
      return fail_msg("rs_driver: source without a time axis", -1);
    if (rs.times_per_point) {
      if (rs.lengths)
        for (int p = 0; p < c.n; ++p)
          if (rs.lengths[p] < 0 || rs.lengths[p] > rs.n_times)
            return fail_msg("rs_driver: lengths[p] outside 0..n_times", -1);
      c.plans[s].assign(c.L, PlanStep{K_NONE, 0, 0.0, 1.0, 0.0}); /* unused: the walk runs on the device */
    } else {
      if (rs.lengths) return fail_msg("rs_driver: lengths given without times_per_point", -1);
      build_plan(rs.times, rs.n_times, c.simtime, c.plans[s]);
    }
  }
  c.active_prefix.assign(c.nsrc, std::vector<int32_t>(c.L + 1, 0));
  for (int s = 0; s < c.nsrc; ++s)
    for (int i = 0; i < c.L; ++i) c.active_prefix[s][i + 1] = c.active_prefix[s][i] + (c.plans[s][i].kind != K_NONE ? 1 : 0);
  bool any_pp = false;
  for (int s = 0; s < c.nsrc; ++s) any_pp = any_pp || (in->sources[s].times_per_point && in->sources[s].n_times > 0);
  c.segs.clear();
  if (!any_pp && !getenv("ROADSURF_HIP_SCAN_FULL")) {
    for (int i = 0; i < c.L; ++i) {
      ScanSeg g{};
      g.i0 = i;
      g.i1 = i + 1;
      for (int s = 0; s < RS_MAX_SOURCES; ++s) {
        g.kind[s] = s < c.nsrc ? c.plans[s][i].kind : K_NONE;
        g.rp[s] = s < c.nsrc ? c.plans[s][i].rp : 0;
      }
      bool same = !c.segs.empty();
      if (same)
        for (int s = 0; s < RS_MAX_SOURCES; ++s)
          same = same && c.segs.back().kind[s] == g.kind[s] && (g.kind[s] == K_NONE || c.segs.back().rp[s] == g.rp[s]);
      if (same) c.segs.back().i1 = i + 1;
      else c.segs.push_back(g);
    }
  }
  return 0;
}

/* Device copies of one tile's raw data + plans. */
struct TileRaw {
  Dev plan[RS_MAX_SOURCES];
  Dev ptimes[RS_MAX_SOURCES], plen[RS_MAX_SOURCES], prp[RS_MAX_SOURCES];
  Dev fld[RS_MAX_SOURCES][NFLD];
  bool any_pp = false;
  Dev stage; /* landing block of the H2D copies ... */
  size_t off[RS_MAX_SOURCES][NFLD + 1] = {}; /* ... byte offset of (source, field) in it; NFLD: the times */
  bool has[RS_MAX_SOURCES][NFLD + 1] = {};
  size_t off_node[RS_MAX_SOURCES] = {}, off_weight[RS_MAX_SOURCES] = {}; /* a gridded source: the tile's stencils */
  Dev segs;  /* Common::segs */
  SrcSet S{};
};

/* A members' tile of rs_driver_run_ensemble: the sources it does not upload, because its stations' tile holds them */
struct ParentFill {
  const TileRaw *T;               /* the stations' tile, raw columns final (humidity completed) */
  const int32_t *parent;          /* device [m]: the column of T behind member p */
  int src_of[RS_MAX_SOURCES];     /* the stations' source behind the members' source s; -1: the member source, uploaded */
  double *copy_ms;                /* ROADSURF_HIP_DRIVER_TIMING: the column copies' time is added here, or nullptr */
};

/* ROADSURF_HIP_DRIVER_TIMING=1: wall time per phase of rs_driver_run on stderr (synchronises) */
struct PhaseTimer {
  bool on;
  hipStream_t s;
  double t0;
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  static double now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
  }
  PhaseTimer(hipStream_t st, bool enabled) : on(enabled), s(st), t0(now()) {}
  void lap(int k) {
    if (!on) return;
    (void)hipStreamSynchronize(s);
    const double t = now();
    acc[k] += t - t0;
    t0 = t;
  }
  void report() const {
    if (!on) return;
    fprintf(stderr,
            "rs_driver_run phases [s]: setup %.3f  upload+transpose %.3f  scan/decide %.3f  alloc/params %.3f  "
            "expand+step %.3f  outputs %.3f  window alloc %.3f  free %.3f\n", acc[0], acc[1], acc[2], acc[3],
            acc[4], acc[5], acc[6], acc[7]);
  }
};

/* The tile's raw series onto the device, in two halves.  `upload_tile` lands every host array of the
 * tile - point-major rows [m][n_times], as the caller holds them - in ONE landing block with back-to-
 * back copies: that is the part that owns the PCIe link, and the part the workers of a device take in
 * turns (rs_devices.hpp: copy_gate).  `upload_finish` turns the rows into the [n_times][mp] columns the
 * kernels read (LDS-tiled transposes), completes Tdew / RH and positions the per-point walks.  (Round 3
 * had one landing buffer per field, so copy and transpose alternated inside the gate and the blocks of a
 * call started ~38 ms apart; the copies alone take less than half of that.)
 * All of it on the worker's one stream.  The copies on a stream of their own, each piece's transpose behind
 * its event, were measured and taken out: a process has four hardware queues, and with two streams per
 * worker two blocks' compute streams can land on one queue, their step kernels then take turns (the call
 * 0.64 s instead of 0.58 s; round 5 again: 0.35 -> 0.43 s, profiles/r05_ab_upload_stream.txt). */
int upload_finish(const RsDriverInput *in, const Common &c, int64_t p0, int m, int64_t mp,
                  TileRaw &T, hipStream_t stream, const ParentFill *pf = nullptr) {
  T.S.nsrc = c.nsrc;
  T.S.simlen = c.L;
  T.S.np_pad = mp;
  T.S.npoints = m;
  T.S.sim0 = in->start_time;
  T.S.dt = c.DT;
  const char *base = T.stage.as<char>();
  for (int s = 0; s < c.nsrc; ++s) {
    const RsRawSource &rs = in->sources[s];
    SrcDev &d = T.S.src[s];
    d = SrcDev{};
    d.n_times = rs.n_times;
    d.is_obs = rs.is_observation;
    if (pf && pf->src_of[s] >= 0) { /* the stations' columns through parent: no landing block, no transpose */
      const SrcDev &ps = pf->T->S.src[pf->src_of[s]];
      ParentCopyArgs pa;
      std::memset(&pa, 0, sizeof(pa));
      if (ps.ptimes) {
        HOK(T.ptimes[s].alloc((size_t)rs.n_times * mp * sizeof(int64_t)));
        HOK(T.plen[s].alloc(mp * sizeof(int32_t)));
        HOK(T.prp[s].alloc(mp * sizeof(int32_t)));
        d.ptimes = T.ptimes[s].as<int64_t>();
        d.plen = T.plen[s].as<int32_t>();
        d.prp = T.prp[s].as<int32_t>();
        pa.src[NFLD] = reinterpret_cast<const uint64_t *>(ps.ptimes);
        pa.dst[NFLD] = reinterpret_cast<uint64_t *>(T.ptimes[s].p);
        pa.src_len = ps.plen;
        pa.dst_len = T.plen[s].as<int32_t>();
        T.any_pp = true;
      } else {
        HOK(T.plan[s].alloc((size_t)c.L * sizeof(PlanStep)));
        HOK(hipMemcpyAsync(T.plan[s].p, c.plans[s].data(), (size_t)c.L * sizeof(PlanStep), hipMemcpyHostToDevice, stream));
        d.plan = T.plan[s].as<PlanStep>();
      }
      for (int f = 0; f < NFLD; ++f) {
        if (!ps.fld[f] || rs.n_times == 0) continue;
        HOK(T.fld[s][f].alloc((size_t)rs.n_times * mp * sizeof(double)));
        d.fld[f] = T.fld[s][f].as<double>();
        pa.src[f] = reinterpret_cast<const uint64_t *>(ps.fld[f]);
        pa.dst[f] = reinterpret_cast<uint64_t *>(T.fld[s][f].p);
      }
      pa.parent = pf->parent;
      pa.n_times = rs.n_times;
      pa.src_stride = pf->T->S.np_pad;
      pa.mp = mp;
      pa.m = m;
      if (rs.n_times > 0) {
        hipLaunchKernelGGL(parent_copy_kernel, dim3((unsigned)(mp / RS_BLOCK), NFLD + 1), dim3(RS_BLOCK), 0, stream, pa);
        HOK(hipGetLastError());
      }
      continue;
    }
    if (rs.times_per_point && rs.n_times > 0) {
      /* per-point axes: times [m][n_times] -> [n_times][mp], lengths, walk positions */
      HOK(T.ptimes[s].alloc((size_t)rs.n_times * mp * sizeof(int64_t)));
      HOK(transpose(reinterpret_cast<const int64_t *>(base + T.off[s][NFLD]), T.ptimes[s].as<int64_t>(), m,
                    rs.n_times, rs.n_times, mp, stream));
      HOK(T.plen[s].alloc(mp * sizeof(int32_t)));
      if (rs.lengths) {
        HOK(hipMemsetAsync(T.plen[s].p, 0, mp * sizeof(int32_t), stream));
        HOK(hipMemcpyAsync(T.plen[s].p, rs.lengths + p0, (size_t)m * sizeof(int32_t),
                           hipMemcpyHostToDevice, stream));
      } else {
        hipLaunchKernelGGL(fill_i32_kernel, grid1(mp), dim3(RS_BLOCK), 0, stream,
                           T.plen[s].as<int32_t>(), mp, (int32_t)rs.n_times);
        HOK(hipGetLastError());
      }
      HOK(T.prp[s].alloc(mp * sizeof(int32_t)));
      d.ptimes = T.ptimes[s].as<int64_t>();
      d.plen = T.plen[s].as<int32_t>();
      d.prp = T.prp[s].as<int32_t>();
      T.any_pp = true;
    } else {
      HOK(T.plan[s].alloc((size_t)c.L * sizeof(PlanStep)));
      HOK(hipMemcpyAsync(T.plan[s].p, c.plans[s].data(), (size_t)c.L * sizeof(PlanStep),
                         hipMemcpyHostToDevice, stream));
      d.plan = T.plan[s].as<PlanStep>();
    }
    for (int f = 0; f < NFLD; ++f) {
      const bool h = T.has[s][f];
      d.fld[f] = nullptr;
      /* Tdew and RH can be completed from each other: both exist if either does */
      const bool derived = (f == R_TDEW && T.has[s][R_RHZ] && T.has[s][R_TAIR]) ||
                           (f == R_RHZ && T.has[s][R_TDEW] && T.has[s][R_TAIR]);
      if ((!h && !derived) || rs.n_times == 0) continue;
      const size_t ne = (size_t)rs.n_times * mp;
      HOK(T.fld[s][f].alloc(ne * sizeof(double)));
      double *dst = T.fld[s][f].as<double>();
      if (h && c.grid[s]) {
        /* the field stays as it arrived, [n_times][n_nodes]: the tile's columns are gathered from it (rs_grid.hip);
         * the live columns hold what grid.py's to_raw_source defines, the pad columns the missing value */
        const RsGridSource &g = *c.grid[s];
        HOK(rs_grid_gather(c.grid_dev[s][f], rs.n_times, g.n_nodes, g.n_nodes,
                           reinterpret_cast<const int32_t *>(base + T.off_node[s]),
                           reinterpret_cast<const double *>(base + T.off_weight[s]), g.stencil, nullptr, rs::raw_threshold(f),
                           -9999.9, dst, mp, m, stream));
        if (mp > m) {
          hipLaunchKernelGGL(fill_pad_kernel, dim3((unsigned)rs.n_times), dim3(RS_BLOCK), 0, stream, dst, (int64_t)m, mp,
                             -9999.9);
          HOK(hipGetLastError());
        }
      } else if (h) {
        HOK(transpose(reinterpret_cast<const double *>(base + T.off[s][f]), dst, m, rs.n_times, rs.n_times,
                      mp, stream));
      } else {
        hipLaunchKernelGGL(fill_f64_kernel, grid1((int64_t)ne), dim3(RS_BLOCK), 0, stream, dst,
                           (int64_t)ne, -9999.9);
        HOK(hipGetLastError());
      }
      d.fld[f] = dst;
    }
    /* JsonSource.cpp:288-295 (needs the math tables: the caller has created a plan) */
    if (d.fld[R_TAIR] && d.fld[R_TDEW] && d.fld[R_RHZ])
      HOK(rs_launch_humidity_fill(d.fld[R_TAIR], const_cast<double *>(d.fld[R_TDEW]),
                                  const_cast<double *>(d.fld[R_RHZ]), (int64_t)rs.n_times * mp,
                                  stream));
  }
  if (T.any_pp) {
    hipLaunchKernelGGL(pp_init_kernel, grid1(mp), dim3(RS_BLOCK), 0, stream, T.S);
    HOK(hipGetLastError());
  }
  if (!c.segs.empty()) {
    HOK(T.segs.alloc(c.segs.size() * sizeof(ScanSeg)));
    HOK(hipMemcpyAsync(T.segs.p, c.segs.data(), c.segs.size() * sizeof(ScanSeg), hipMemcpyHostToDevice, stream));
  }
  return 0;
}

/* one tile's turn on the link: its series and, where `hzpt` is given, its local horizons */
int upload_tile(const RsDriverInput *in, const Common &c, int32_t device, int64_t p0, int m, int64_t mp,
                TileRaw &T, Dev *hzpt, bool timing, hipStream_t stream, const ParentFill *pf = nullptr) {
  const double tg0 = PhaseTimer::now();
  std::lock_guard<std::mutex> turn(rsu::copy_gate(device)); /* rs_devices.hpp: uploads take turns */
  const double tg1 = PhaseTimer::now();
  size_t total = 0;
  for (int s = 0; s < c.nsrc; ++s) {
    const RsRawSource &rs = in->sources[s];
    if (rs.n_times < 1 || (pf && pf->src_of[s] >= 0)) continue; /* (nothing, or its stations' tile has it) */
    const size_t piece = ((size_t)m * rs.n_times * sizeof(double) + 255) & ~(size_t)255;
    if (const RsGridSource *g = c.grid[s]) { /* the fields are on the device already: the tile's slice of the stencils */
      T.off_node[s] = total;
      total += ((size_t)m * g->stencil * sizeof(int32_t) + 255) & ~(size_t)255;
      T.off_weight[s] = total;
      total += ((size_t)m * g->stencil * sizeof(double) + 255) & ~(size_t)255;
      for (int f = 0; f < NFLD; ++f) T.has[s][f] = grid_field(*g, f) != nullptr;
      continue;
    }
    if (rs.times_per_point) {
      T.off[s][NFLD] = total;
      T.has[s][NFLD] = true;
      total += piece;
    }
    for (int f = 0; f < NFLD; ++f)
      if (raw_field(rs, f)) {
        T.off[s][f] = total;
        T.has[s][f] = true;
        total += piece;
      }
  }
  HOK(T.stage.alloc(total ? total : 256)); /* (a members' tile whose own source has no variable lands nothing) */
  char *base = T.stage.as<char>();
  for (int s = 0; s < c.nsrc; ++s) {
    const RsRawSource &rs = in->sources[s];
    if (pf && pf->src_of[s] >= 0) continue;
    if (const RsGridSource *g = c.grid[s]) {
      if (rs.n_times < 1) continue;
      HOK(hipMemcpyAsync(base + T.off_node[s], g->node + (size_t)p0 * g->stencil, (size_t)m * g->stencil * sizeof(int32_t),
                         hipMemcpyHostToDevice, stream));
      HOK(hipMemcpyAsync(base + T.off_weight[s], g->weight + (size_t)p0 * g->stencil,
                         (size_t)m * g->stencil * sizeof(double), hipMemcpyHostToDevice, stream));
      continue;
    }
    if (T.has[s][NFLD])
      HOK(hipMemcpyAsync(base + T.off[s][NFLD], rs.times + (size_t)p0 * rs.n_times,
                         (size_t)m * rs.n_times * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    for (int f = 0; f < NFLD; ++f)
      if (T.has[s][f])
        HOK(hipMemcpyAsync(base + T.off[s][f], raw_field(rs, f) + (size_t)p0 * rs.n_times,
                           (size_t)m * rs.n_times * sizeof(double), hipMemcpyHostToDevice, stream));
  }
  /* the tile's local horizons (2.9 KB per point: as many bytes as all the series together) in the same
   * turn on the link, so that the block's first launch waits for ITS bytes only - enqueued later, the
   * copy shared the link with the next block's series and the first step started 58 ms into the call */
  if (hzpt) {
    HOK(hzpt->alloc((size_t)m * 360 * sizeof(double)));
    HOK(hipMemcpyAsync(hzpt->p, in->horizons + (size_t)p0 * 360, (size_t)m * 360 * sizeof(double),
                       hipMemcpyHostToDevice, stream));
  }
  HOK(hipStreamSynchronize(stream));
  const double tc0 = PhaseTimer::now();
  if (int rc = upload_finish(in, c, p0, m, mp, T, stream, pf)) return rc;
  const double tg2 = PhaseTimer::now();
  HOK(hipStreamSynchronize(stream)); /* the turn on the link ends when the last byte has landed */
  if (pf && pf->copy_ms) *pf->copy_ms += 1e3 * (PhaseTimer::now() - tc0); /* (with the member source's transposes) */
  if (timing)
    fprintf(stderr, "rs_driver_run upload: waited %.1f ms for the link, issued the copies in %.1f ms, "
                    "drained in %.1f ms\n", 1e3 * (tg1 - tg0), 1e3 * (tg2 - tg1), 1e3 * (PhaseTimer::now() - tg2));
  return 0;
}

/* Per-point decisions of read_input for one tile (device arrays, [mp]). */
struct TileDecisions {
  Dev first_missing, last_obs, cpl_i, cpl_t;
  Dev status, missing_index, initlen, cpl_index, cpl_hi, tair_relax, vz_relax, rh_relax, cpl_tsurf;
};

/* read_input's decisions from the scan's results.  ignore_from < SimLen (the stations of rs_driver_run_ensemble): the
 * decisions of the series before that index, as if nothing were missing from it on. */
int finalize_tile(const Common &c, const InputSettings *st, const TileRaw &T, TileDecisions &D, int32_t ignore_from,
                  hipStream_t stream) {
  const int64_t mp = T.S.np_pad;
  FinalArgs fa;
  fa.S = T.S;
  fa.first_missing = D.first_missing.as<int32_t>();
  fa.last_obs = D.last_obs.as<int32_t>();
  fa.cpl_i = D.cpl_i.as<int32_t>();
  fa.cpl_t = D.cpl_t.as<double>();
  fa.ignore_from = ignore_from;
  fa.use_relaxation = st->use_relaxation;
  fa.use_coupling = st->use_coupling;
  fa.cplLen = c.cplLen;
  fa.default_initlen = c.default_initlen;
  fa.status = D.status.as<int32_t>();
  fa.missing_index = D.missing_index.as<int32_t>();
  fa.initlen = D.initlen.as<int32_t>();
  fa.cpl_index = D.cpl_index.as<int32_t>();
  fa.cpl_hi = D.cpl_hi.as<int32_t>();
  fa.tair_relax = D.tair_relax.as<double>();
  fa.vz_relax = D.vz_relax.as<double>();
  fa.rh_relax = D.rh_relax.as<double>();
  fa.cpl_tsurf = D.cpl_tsurf.as<double>();
  hipLaunchKernelGGL(finalize_kernel, grid1(mp), dim3(RS_BLOCK), 0, stream, fa);
  HOK(hipGetLastError());
  return 0;
}

int decide_tile(const Common &c, const InputSettings *st, const TileRaw &T, TileDecisions &D,
                hipStream_t stream) {
  const int64_t mp = T.S.np_pad;
  HOK(D.first_missing.alloc((size_t)6 * mp * sizeof(int32_t)));
  HOK(D.last_obs.alloc(mp * sizeof(int32_t)));
  HOK(D.cpl_i.alloc(mp * sizeof(int32_t)));
  HOK(D.cpl_t.alloc(mp * sizeof(double)));
  for (Dev *d : {&D.status, &D.missing_index, &D.initlen, &D.cpl_index, &D.cpl_hi})
    HOK(d->alloc(mp * sizeof(int32_t)));
  for (Dev *d : {&D.tair_relax, &D.vz_relax, &D.rh_relax, &D.cpl_tsurf})
    HOK(d->alloc(mp * sizeof(double)));
  ScanArgs sa;
  sa.S = T.S;
  sa.first_missing = D.first_missing.as<int32_t>();
  sa.last_obs = D.last_obs.as<int32_t>();
  sa.cpl_i = D.cpl_i.as<int32_t>();
  sa.cpl_t = D.cpl_t.as<double>();
  if (T.any_pp)
    hipLaunchKernelGGL(scan_raw_kernel<true>, dim3((unsigned)(mp / RS_BLOCK), 7), dim3(RS_BLOCK), 0,
                       stream, sa);
  else if (!c.segs.empty() && T.segs.p)
    hipLaunchKernelGGL(scan_seg_kernel, dim3((unsigned)(mp / RS_BLOCK), 7), dim3(RS_BLOCK), 0, stream, sa,
                       (const ScanSeg *)T.segs.as<ScanSeg>(), (int32_t)c.segs.size());
  else
    hipLaunchKernelGGL(scan_raw_kernel<false>, dim3((unsigned)(mp / RS_BLOCK), 7), dim3(RS_BLOCK), 0,
                       stream, sa);
  HOK(hipGetLastError());
  return finalize_tile(c, st, T, D, INT32_MAX, stream);
}

/* Copy the decisions back into the caller's LocalParameters / status arrays the way
 * read_input leaves them.  In two halves: `issue` enqueues the device-to-host copies (into page-locked
 * memory the worker thread keeps) behind the decision kernels and returns; `finish` waits for them and
 * writes the caller's arrays.  A run without coupling finishes after it has enqueued the whole
 * simulation - nothing on the host needs the decisions before - so the time loop starts without
 * waiting for the upload and the scan to drain. */
struct TileReport {
  int m = 0;
  int64_t p0 = 0;
  hipEvent_t ev = nullptr;
  char *h = nullptr; /* [4][m] int32 status, missing_index, initlen, cpl_index; [4][m] double relax x 3, cpl_tsurf */
  bool pending = false;
  ~TileReport() {
    if (ev) (void)hipEventDestroy(ev);
  }
};

inline char *report_staging(size_t bytes) {
  static thread_local rsu::Pinned buf;
  static thread_local size_t cap = 0;
  if (cap < bytes) {
    if (buf.p) (void)hipHostFree(buf.p);
    buf.p = nullptr;
    cap = 0;
    if (buf.alloc(bytes) != hipSuccess) return nullptr;
    cap = bytes;
  }
  return static_cast<char *>(buf.p);
}

int report_issue(const TileDecisions &D, int64_t p0, int m, TileReport &R, hipStream_t stream) {
  R.m = m;
  R.p0 = p0;
  R.h = report_staging((size_t)m * (4 * sizeof(int32_t) + 4 * sizeof(double)));
  if (!R.h) return fail_msg("rs_driver_run: no page-locked memory for the decisions", -10);
  int32_t *hi = reinterpret_cast<int32_t *>(R.h);
  double *hd = reinterpret_cast<double *>(R.h + (size_t)4 * m * sizeof(int32_t));
  const void *si[4] = {D.status.p, D.missing_index.p, D.initlen.p, D.cpl_index.p};
  const void *sd[4] = {D.tair_relax.p, D.vz_relax.p, D.rh_relax.p, D.cpl_tsurf.p};
  for (int k = 0; k < 4; ++k) {
    HOK(hipMemcpyAsync(hi + (size_t)k * m, si[k], (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HOK(hipMemcpyAsync(hd + (size_t)k * m, sd[k], (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream));
  }
  if (!R.ev) HOK(hipEventCreateWithFlags(&R.ev, hipEventDisableTiming));
  HOK(hipEventRecord(R.ev, stream));
  R.pending = true;
  return 0;
}

int report_finish(const Common &c, const InputSettings *st, TileReport &R, LocalParameters *local,
                  int32_t *status, int32_t *missing_index) {
  if (!R.pending) return 0;
  HOK(hipEventSynchronize(R.ev));
  R.pending = false;
  const int m = R.m;
  const int64_t p0 = R.p0;
  const int32_t *hs = reinterpret_cast<const int32_t *>(R.h), *hm = hs + m, *hi = hs + 2 * (size_t)m,
                *hc = hs + 3 * (size_t)m;
  const double *tr = reinterpret_cast<const double *>(R.h + (size_t)4 * m * sizeof(int32_t)), *vr = tr + m,
               *rr = tr + 2 * (size_t)m, *ct = tr + 3 * (size_t)m;
  for (int p = 0; p < m; ++p) {
    if (status) status[p0 + p] = hs[p];
    if (missing_index) missing_index[p0 + p] = hm[p];
    if (!local) continue;
    LocalParameters &l = local[p0 + p];
    l.InitLenI = c.default_initlen; /* roadrunner.cpp:169, before anything can fail */
    if (hs[p] >= 1 && hs[p] <= 6) continue; /* read_input returned early */
    if (st->use_relaxation == 1) {
      l.tair_relax = tr[p];
      l.VZ_relax = vr[p];
      l.RH_relax = rr[p];
      l.InitLenI = hi[p];
    }
    if (st->use_coupling == 1 && hs[p] == 0) {
      l.couplingTsurf = ct[p];
      l.couplingIndexI = hc[p];
    }
  }
  return 0;
}

int check_device(int32_t device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail_msg("rs_driver: no HIP device visible - this library has no CPU path", -9);
  if (device < 0 || device >= ndev) return fail_msg("rs_driver: device index out of range", -9);
  return 0;
}

struct StreamGuard {
  hipStream_t s = nullptr;
  ~StreamGuard() {
    if (s) (void)hipStreamDestroy(s);
  }
};
struct PlanGuard {
  RsPlan *p = nullptr;
  ~PlanGuard() {
    if (p) rs_hip_plan_destroy(p);
  }
};

/* What rs_driver_expand and rs_driver_run hand to every tile of a call. */
struct Call {
  const RsDriverInput *in;
  const InputSettings *st;
  const Common &c;
  const RsConstants &consts;
  int32_t device;
  hipStream_t stream;
  LocalParameters *local;
  int32_t *status, *missing_index; /* the decisions go to these two and to `local` (each may be null) */
};

/* A tile's plan, its raw series on the device and read_input's decisions about its points. */
struct TileHead {
  PlanGuard pg;
  int64_t mp = 0; /* the plan's padded point count: the stride of every [row][point] array of the tile */
  TileRaw T;
  Dev d_hzpt; /* local horizons [m][360], with `horizons` */
  TileDecisions D;
  TileReport rep;
};

/* Plan, upload, decide, report for points [p0, p0+m).  The decisions are enqueued for the caller's arrays; they
 * are there on return with `report_now` (or with the timer on, whose laps drain the stream anyway), else
 * after the caller's own report_finish. */
int tile_prologue(const Call &k, int64_t p0, int m, bool horizons, bool report_now, PhaseTimer &pt, TileHead &H,
                  const ParentFill *pf = nullptr) {
  H.pg.p = rs_hip_plan_create(k.device, m, &k.consts, k.stream);
  if (!H.pg.p) return -11;
  H.mp = rs_hip_plan_npoints_padded(H.pg.p);
  if (int rc = upload_tile(k.in, k.c, k.device, p0, m, H.mp, H.T, horizons ? &H.d_hzpt : nullptr, pt.on, k.stream, pf))
    return rc;
  pt.lap(1);
  if (int rc = decide_tile(k.c, k.st, H.T, H.D, k.stream)) return rc;
  if (int rc = report_issue(H.D, p0, m, H.rep, k.stream)) return rc;
  if (report_now || pt.on)
    if (int rc = report_finish(k.c, k.st, H.rep, k.local, k.status, k.missing_index)) return rc;
  pt.lap(2);
  return 0;
}

/* The forcing windows are the one large allocation (up to 64 GB with coupling).  The amdgpu
 * driver wipes VRAM when it is released, and a hipMalloc that lands on pages still being
 * wiped waits for them: measured here, a 60 GB hipMalloc right after a 60 GB hipFree takes
 * 3-6 s, against 0.6 s for the whole simulation.  So the window block is kept per process and
 * reused by the next call (rs_driver_release_cache frees it); a concurrent second caller gets a
 * private allocation. */
constexpr int WINCACHE_SLOTS = 8; /* concurrent rs_driver_run workers per device that keep a block */
struct WindowCache {
  std::mutex m;
  void *p[WINCACHE_SLOTS] = {};
  size_t bytes[WINCACHE_SLOTS] = {};
  bool busy[WINCACHE_SLOTS] = {};
} g_wincache[64], /* per device: the fan-out of rs_driver_run has several workers on each */
    g_arenacache[64]; /* the same for the workers' arenas (rs_devutil.hpp): every other buffer of a tile */

struct WindowLease {
  void *p = nullptr;
  bool cached = false;
  hipStream_t stream = nullptr; /* the stream whose kernels use the block */
  ~WindowLease() { release(); }
  int device = 0, slot = -1;
  WindowCache *cache = g_wincache;
  hipError_t acquire(size_t bytes, int dev) {
    device = dev & 63;
    WindowCache &c = cache[device];
    std::lock_guard<std::mutex> lk(c.m);
    /* a free slot that is large enough, else a free slot to (re)allocate */
    int pick = -1;
    for (int k = 0; k < WINCACHE_SLOTS && pick < 0; ++k)
      if (!c.busy[k] && c.p[k] && c.bytes[k] >= bytes) pick = k;
    for (int k = 0; k < WINCACHE_SLOTS && pick < 0; ++k)
      if (!c.busy[k] && !c.p[k]) pick = k;
    for (int k = 0; k < WINCACHE_SLOTS && pick < 0; ++k)
      if (!c.busy[k]) pick = k;
    if (pick >= 0) {
      if (c.p[pick] && c.bytes[pick] < bytes) {
        (void)hipFree(c.p[pick]);
        c.p[pick] = nullptr;
        c.bytes[pick] = 0;
      }
      if (!c.p[pick]) {
        hipError_t e = hipMalloc(&c.p[pick], bytes);
        if (e != hipSuccess) {
          c.p[pick] = nullptr;
          return e;
        }
        c.bytes[pick] = bytes;
      }
      c.busy[pick] = true;
      cached = true;
      slot = pick;
      p = c.p[pick];
      return hipSuccess;
    }
    cached = false;
    return hipMalloc(&p, bytes);
  }
  void release() {
    if (!p) return;
    /* error returns leave kernels in flight on the call's stream: nobody else may get the
     * block before they have drained (the lease is declared after the stream guard, so the
     * stream is still alive here) */
    if (stream) (void)hipStreamSynchronize(stream);
    if (cached) {
      std::lock_guard<std::mutex> lk(cache[device].m);
      cache[device].busy[slot] = false;
    } else {
      (void)hipFree(p);
    }
    p = nullptr;
  }
};

struct ArenaScope {
  rsu::Arena *prev;
  explicit ArenaScope(rsu::Arena *a) : prev(rsu::tls_arena()) { rsu::tls_arena() = a; }
  ~ArenaScope() { rsu::tls_arena() = prev; }
};

/* Decided once per call (one device's share of it), from the arguments and the environment: every getenv
 * of the run path is in make_run_policy (ROADSURF_HIP_SCAN_FULL, which rs_driver_expand shares: prepare). */
struct RunPolicy {
  int step = 0, n_out = 0; /* output decimation and rows (check_run_arguments) */
  bool coupled = false;
  bool cpl_chunked = false;  /* coupling in time chunks: lock step, replay rounds, lock step */
  bool use_raw = false;      /* the step kernel makes its forcing from the raw series: no windows */
  bool skyview = false;
  bool small_block = false;
  bool want_cluster = false; /* plan order, if the tile has more than one launch (TilePolicy::cluster) */
  bool timing = false;       /* ROADSURF_HIP_DRIVER_TIMING */
  bool kept = false;         /* the call wants kept input rows or the deficit (rs_driver_run_kept): one more [n_out][mp] */
  int epi_cols = 0;          /* the call wants threshold episodes (rs_driver_run_episodes): columns per point, else 0 */
  bool epi_deficit = false;  /* ... whose spec uses the deficit: one more [n_out][mp] that holds it */
  int P = 0;                 /* points per tile */
  int TC = 0;                /* indices per launch */
  int nwin = 0;              /* forcing windows of a tile (SW_dir / LW_net only with sky view) */
  size_t win_budget = 0;     /* bytes of forcing windows one worker may hold */
};

void make_run_policy(const InputSettings *st, const RsConstants &consts, const Common &c,
                     const LocalParameters *local, int64_t pbeg, int64_t pend, RunPolicy &R) {
  const int L = c.L;
  R.timing = getenv("ROADSURF_HIP_DRIVER_TIMING") != nullptr;
  R.coupled = st->use_coupling == 1;
  for (int p = 0; p < c.n; ++p)
    if (local[p].sky_view < 1.0 && local[p].sky_view > (double)-0.01f) R.skyview = true;
  R.nwin = R.skyview ? NFLD : NFLD - 2;
  /* Coupling runs time-chunked too (rs_hip_step_cpl / rs_hip_cpl_replay): lock-step
   * chunks that park a point behind its coupling window, replay rounds over a window-sized block,
   * lock-step chunks again - with sky view too (in natural order: the per-point geometry is not
   * gathered into a plan order). */
  R.cpl_chunked = R.coupled && !getenv("ROADSURF_HIP_CPL_WHOLE");
  /* The blocks' step kernel makes its forcing from the raw series itself (rs_step_raw: the two-wavefront
   * flavour, ground wave = JsonSource::interpolate + overlay one index ahead) wherever it can: sources on
   * shared time axes (the segment table exists), NLayers = 15, no output depth.  No forcing window, no
   * expansion kernel - with coupling for the lock-step chunks; the replay rounds keep a window over the
   * coupling windows of the tile (rs_hip_cpl_replay).  ROADSURF_HIP_DRIVER_WINDOWS=1: the windows and the one-point-per-lane
   * kernels as before (tests compare the two). */
  R.use_raw = !c.segs.empty() && (!R.coupled || R.cpl_chunked) && consts.NLayers == 15 &&
              !(st->tsurfOutputDepth >= 0.0) && !getenv("ROADSURF_HIP_DRIVER_WINDOWS");
  /* Tile of points: large enough to fill the chip (256 CUs x 4 workgroups of 256 points is
   * 262144 points per round).  With coupling the windows hold the whole series (a point
   * replays its coupling window), so the tile follows from a 64 GB window budget. */
  const char *ep = getenv("ROADSURF_HIP_TILE_POINTS"), *et = getenv("ROADSURF_HIP_CHUNK_STEPS");
  int64_t Pdef = 524288;
  if (R.coupled && !R.cpl_chunked) {
    Pdef = (int64_t)(64e9 / ((double)L * NFLD * sizeof(double)));
    Pdef = std::max<int64_t>(4096, std::min<int64_t>(262144, Pdef / 4096 * 4096));
  }
  int64_t Pcap = INT64_MAX;
  if (R.use_raw) {
    /* the raw-series step kernels address a tile's whole output window (every decimated row of the series,
     * padded stride) with 32-bit offsets: rs_step_raw / rs_cpl_replay_raw refuse a window of rs_a32_limit()
     * elements per stream or more (e.g. 250 000 points x 48 h with outputStep = 1 min: 7.2e8), so the tile is
     * cut to fit - whatever ROADSURF_HIP_TILE_POINTS asks for */
    Pcap = std::max<int64_t>(RS_BLOCK, (int64_t)((rs_a32_limit() - 1) / (uint64_t)R.n_out) / RS_BLOCK * RS_BLOCK);
  }
  R.P = (int)std::min<int64_t>(std::min<int64_t>(pend - pbeg, Pcap), ep ? std::max(1, atoi(ep)) : Pdef);
  /* A block of a few wavefronts (the reference's operational example: 401 stations) is the latency of its
   * dependent steps whatever the order of its points: no re-sorts, and launches of eight hours (154 against 165 ms
   * per call of that example, profiles/r05_operational_shape.txt) */
  R.small_block = pend - pbeg < 4096;
  const char *ec = getenv("ROADSURF_HIP_CLUSTER"); /* 0 / 1: natural / plan order whatever the size */
  R.want_cluster = ec ? atoi(ec) != 0 : !R.small_block;
  R.TC = (R.coupled && !R.cpl_chunked) ? L : std::min(L, et ? std::max(1, atoi(et)) : R.use_raw ? (R.want_cluster ? RS_DRIVER_RAW_CHUNK : 960) : 256);
  /* Budget of one worker's forcing windows.  Chunked coupling sizes its replay block from the
   * tile's couplingIndexI values (known only after read_input has run on the device): one station
   * that stopped reporting hours before the others stretches the block towards SimLen, and at the
   * default tile that is > 100 GB per worker.  Such a tile is cut in halves until it fits. */
  const char *eb = getenv("ROADSURF_HIP_WINDOW_BUDGET_MB");
  R.win_budget = eb ? (size_t)std::max(1, atoi(eb)) << 20 : (size_t)24 << 30;
}

/* Decided per tile, once read_input's decisions about its points are back in `local`: where the coupling
 * windows lie, what the replay rounds read, how many window rows that takes - and whether the tile fits. */
struct TilePolicy {
  bool any_on = false;                    /* some point of the tile has a coupling window */
  int cs_min = 0, ce_min = 0, ce_max = 0; /* first window start, first and last window end */
  int r_lo = 0, r_hi = 0;                 /* replay block, 1-based inclusive */
  bool replay_raw = false;                /* the replay rounds read the raw series too (rs_cpl_replay_raw) */
  bool need_win = false;                  /* the tile expands forcing windows at all */
  int WR = 0;                             /* rows of a window */
  bool cluster = false;                   /* plan order: the slots are re-sorted between launches */
  bool forecast_key = false;              /* ... by a forecast of the next launch (else by the last one's history) */
  int halve_to = 0;                       /* > 0: the windows would pass the budget - start again with so many points */
};

TilePolicy make_tile_policy(const RunPolicy &R, const Common &c, const InputSettings *st,
                            const LocalParameters *local, int64_t p0, int m, int64_t mp, bool any_pp,
                            bool no_replay = false) {
  const int L = c.L, TC = R.TC;
  TilePolicy t;
  /* chunked coupling: where the tile's coupling windows lie (no_replay: the members of rs_driver_run_ensemble, whose
   * windows their stations have closed - lock-step chunks alone, no replay block) */
  if (R.cpl_chunked && !no_replay) {
    for (int p = 0; p < m; ++p) {
      const LocalParameters &lp = local[p0 + p];
      if (lp.couplingTsurf < -100 || lp.couplingIndexI < 1) continue; /* src/InputOutput.f90:34-36 */
      const int ce = lp.couplingIndexI;
      /* initCouplingTimes, src/Coupling.f90:512-517 */
      const int cs = ((double)ce <= (double)(st->coupling_minutes * 60) / st->DTSecs) ? 1 : ce - c.cplLen;
      if (!t.any_on) { t.cs_min = cs; t.ce_min = t.ce_max = ce; t.any_on = true; }
      t.cs_min = std::min(t.cs_min, cs); t.ce_min = std::min(t.ce_min, ce); t.ce_max = std::max(t.ce_max, ce);
    }
  }
  t.r_lo = t.cs_min;
  t.r_hi = std::min(t.ce_max + 1, L);
  const int rlen = t.r_hi - t.r_lo + 1;
  /* the replay rounds read the raw series too (rs_cpl_replay_raw) where the block ends before SimLen and
   * there is no sky view */
  /* ... and is COMPACT - not much longer than one coupling window, rs_hip_cpl_replay's own rule: stations whose
   * observations end hours apart (the reference's operational example) make a block in which a lock-step
   * replay would step every listed point through all of it, round after round - those keep the forcing window
   * and the per-lane replay kernel */
  t.replay_raw = R.use_raw && R.cpl_chunked && t.any_on && !R.skyview && std::min(t.ce_max + 1, L) < L &&
                 (int64_t)rlen * 4 <= ((int64_t)c.cplLen + 2) * 5;
  t.need_win = !R.use_raw || (R.cpl_chunked && t.any_on && !t.replay_raw); /* raw-series stepping: windows for such replays only */
  t.WR = (R.cpl_chunked && t.any_on) ? (R.use_raw ? rlen : std::max(TC, rlen)) : TC;
  if (R.cpl_chunked && t.WR > TC && (size_t)R.nwin * mp * t.WR * sizeof(double) > R.win_budget && m > 4096)
    t.halve_to = std::max(4096, (m / 2 + 4095) / 4096 * 4096);
  /* Plan order (rs_hip_recluster): with more than one launch per tile the slots
   * are re-sorted by regime after every launch; windows and per-point parameters are then
   * produced in slot order and each launch's output rows are mapped back.  Time-chunked
   * coupling runs that way too: the lock-step chunks are re-sorted like the uncoupled launches,
   * and the coupling kernels' outputs - the replays' included - go straight to their point's
   * column (rs_hip_set_output_by_point).  Measured at 1 M points, four plans: 0.90 s against
   * 0.96 s in natural order with the history key (-12 % vector instructions in the lock-step
   * kernel), see DESIGN.md 6 for the forecast key.  ROADSURF_HIP_CLUSTER=0 switches the order
   * off.  Sky view (round 4): the four geometry scalars are gathered like the other per-point
   * parameters, the local-horizon table is read through the order row. */
  t.cluster = (!R.coupled || R.cpl_chunked) && TC < L && R.want_cluster;
  /* Re-sort of the slots for the window [t_next, t_next+len_next): by a FORECAST of that window
   * (rs_hip_recluster_forecast) - air temperature and wind speed at three of its
   * indices, produced from the raw series in the CURRENT slot order by the expansion kernel
   * itself (only those two fields, one index each) - or, where the raw series have per-point time
   * axes (their walks would have to be re-positioned for every preview), by the history of the
   * last launch. */
  t.forecast_key = !any_pp;
  return t;
}

/* Hour and sun position per simulation index on the device, the points' geometry on the host: shared by the tiles. */
struct SharedAxes {
  Dev d_hour, d_sun;
  std::vector<double> sun, slat, clat, lrad; /* (this worker's points only: index q of the last three is point pbeg + q) */
};

/* One device's share of a call, points [pbeg, pend): what its tiles are given. */
struct Run : Call {
  const InputParameters *params;
  const RsDriverOutput *out;
  const RunPolicy &R;
  int64_t pbeg, pend;
  double tbottom;
  const SharedAxes &ax;
  PhaseTimer &pt;
  WindowLease &win;
  size_t win_bytes; /* of the block `win` holds */
  const RsDriverRequest &q; /* what the call wants beside the series, normalised (driver_run); NULL member: not that */
  double *grp_acc;          /* device [rows][ngroups][cols]: this block's group cells, merged into by every tile */
};

/* tiles the calling thread's last single-device rs_driver_run stepped (tests: the window budget), and how many
 * of its step launches made their forcing from the raw series (rs_step_raw) */
thread_local int g_last_tiles = 0, g_last_raw_launches = 0;

void outputs_at(RsOutputs &o, double *b, size_t os) { /* six output blocks of `os` elements each */
  o.tsurf = b; o.snow = b + os; o.water = b + 2 * os; o.ice = b + 3 * os;
  o.deposit = b + 4 * os; o.ice2 = b + 5 * os;
}
void geometry_at(RsPointParams &p, const double *g, int64_t mp) { /* four rows of `mp`: d_geo, d_geo_s */
  p.sky_view = g; p.sin_lat = g + mp; p.cos_lat = g + 2 * mp; p.lon_rad = g + 3 * mp;
}

/* A tile's device buffers and the argument blocks that point into them, from the per-point parameters to
 * the outputs' way home.  The stages are called in this order by driver_run_range. */
struct Tile : TileHead {
  Run &r;
  const RunPolicy &R;
  const Common &c;
  const hipStream_t stream;
  const int64_t p0;
  const int m;
  TilePolicy tp;
  /* (in the order they are allocated) */
  Dev d_tb, d_geo;                /* bottom temperature; sky view, sin / cos latitude, longitude in point order */
  Dev d_phase, d_out, d_outpt;    /* PrecPhase window; the six outputs [n_out][mp]; one of them [m][n_out] */
  Dev d_outc, d_pp_s, d_geo_s;    /* slot order: one launch's output rows, per-point parameters, geometry */
  Dev d_prev, d_row1;             /* preview rows of the forecast key; index 1's rows for the initial profile */
  Dev d_sum, d_sumpt;             /* the summaries [RS_SUM_COLS][mp], and as the caller holds them [m][RS_SUM_COLS] */
  Dev d_gid;                      /* the tile's slice of RsDriverGroups::group */
  Dev d_kept;                     /* one variable's kept rows [n_out][mp], then the deficit (rs_driver_run_kept) */
  Dev d_epidef;                   /* the kept dew point, then the deficit [n_out][mp], where the episodes read it */
  Dev d_epi, d_epipt;             /* the episodes [cols][mp], and as the caller holds them [m][cols] */
  RsPointParams pp, pps;          /* in point order, in slot order */
  RsOutputs oo, oc;               /* the result [n_out][mp]; one launch's rows in slot order (rows_c) */
  size_t os = 0;                  /* mp * n_out */
  int rows_c = 0;                 /* output rows one launch can produce */
  ExpandRawArgs ea;
  rs::RawForcing rf;
  int walk_at = 0;                /* 0-based index the per-point raw walks are positioned at */
  size_t seg = 0;                 /* segment of the index the raw-series kernels start at (seek_seg) */
  /* rs_driver_run_ensemble.  A members' tile: its stations' horizon table [stations][360] and every member's column of
   * it, device [m] - and that row in slot order.  A stations' tile: the status read_input gives, where the tile steps
   * with the decisions of the series before the branch (finalize_tile) - what the result is blanked by */
  const double *hz_table = nullptr;
  const int32_t *hz_col = nullptr;
  Dev d_hzcol_s, d_status_rep;
  Dev d_etable, d_einv, d_eacc, d_ever, d_words; /* the members' reducers: table, identity row, cells, carry, words */

  Tile(Run &run, int64_t p0_, int m_) : r(run), R(run.R), c(run.c), stream(run.stream), p0(p0_), m(m_) {}
  const RsPointParams &ppx() const { return tp.cluster ? pps : pp; }
  const int32_t *col() const { return tp.cluster ? ea.order : nullptr; }

  /* per-point parameters in point order */
  int point_params() {
    HOK(d_tb.alloc(mp * sizeof(double)));
    hipLaunchKernelGGL(fill_f64_kernel, grid1(mp), dim3(RS_BLOCK), 0, stream, d_tb.as<double>(), mp, r.tbottom);
    HOK(hipGetLastError());
    std::memset(&pp, 0, sizeof(pp));
    pp.tbottom = d_tb.as<double>();
    pp.initlen = D.initlen.as<int32_t>();
    if (r.st->use_relaxation == 1) {
      pp.tair_relax = D.tair_relax.as<double>();
      pp.vz_relax = D.vz_relax.as<double>();
      pp.rh_relax = D.rh_relax.as<double>();
    }
    if (R.coupled) {
      pp.coupling_index = D.cpl_index.as<int32_t>();
      pp.coupling_tsurf = D.cpl_tsurf.as<double>();
    }
    if (R.skyview) {
      HOK(d_geo.alloc((size_t)4 * mp * sizeof(double)));
      std::vector<double> g((size_t)4 * mp, 1.0);
      for (int p = 0; p < m; ++p) {
        g[p] = r.local[p0 + p].sky_view;
        g[(size_t)mp + p] = r.ax.slat[p0 - r.pbeg + p];
        g[(size_t)2 * mp + p] = r.ax.clat[p0 - r.pbeg + p];
        g[(size_t)3 * mp + p] = r.ax.lrad[p0 - r.pbeg + p];
      }
      HOK(hipMemcpyAsync(d_geo.p, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, stream));
      HOK(hipStreamSynchronize(stream)); /* g goes out of scope */
      geometry_at(pp, d_geo.as<double>(), mp);
      pp.albedo_surroundings = r.params->Albedo_surroundings;
      /* the horizon table as the caller holds it, [point][360] (RsPointParams::horizons_by_point): no
       * transpose, half the device memory, and a point's neighbouring degrees in one cache line; no table
       * at all where the caller has none (the kernels read a missing table as 0) */
      pp.horizons = r.in->horizons ? d_hzpt.as<double>() : nullptr; /* (uploaded with the series, tile_prologue) */
      pp.horizons_by_point = 1;
      if (hz_table) { /* a member reads its station's row */
        pp.horizons = hz_table;
        pp.horizon_index = hz_col;
      }
    }
    return 0;
  }
  /* the forcing windows (where the tile has any), the outputs, the slot-order copies, and the argument blocks over them */
  int buffers() {
    if (tp.need_win && (size_t)R.nwin * mp * tp.WR * sizeof(double) > r.win_bytes) {
      r.win.release();
      r.win_bytes = (size_t)R.nwin * mp * tp.WR * sizeof(double);
      HOK(r.win.acquire(r.win_bytes, r.device));
    }
    const size_t fs = (size_t)mp * tp.WR;
    if (tp.need_win) {
      HOK(d_phase.alloc(fs * sizeof(int32_t)));
      hipLaunchKernelGGL(fill_i32_kernel, grid1((int64_t)fs), dim3(RS_BLOCK), 0, stream,
                         d_phase.as<int32_t>(), (int64_t)fs, -9999); /* InputData.cpp:16 */
      HOK(hipGetLastError());
    }
    os = (size_t)mp * R.n_out;
    HOK(d_out.alloc((size_t)6 * os * sizeof(double)));
    /* OutputData.cpp:5-13: rows the simulation never saves read -9999.0 */
    hipLaunchKernelGGL(fill_f64_kernel, grid1((int64_t)(6 * os)), dim3(RS_BLOCK), 0, stream,
                       d_out.as<double>(), (int64_t)(6 * os), -9999.0);
    HOK(hipGetLastError());
    HOK(d_outpt.alloc((size_t)m * R.n_out * sizeof(double)));

    ea.S = T.S; /* (expand_window: the sources of the current window) */
    /* window f lives at slot k of the leased block (SW_dir / LW_net only with sky view) */
    double *wb = static_cast<double *>(r.win.p);
    for (int f = 0, k = 0; f < NFLD; ++f) {
      const bool used = tp.need_win && (R.skyview || (f != R_SWDIR && f != R_LWNET));
      ea.out[f] = used ? wb + (size_t)(k++) * fs : nullptr;
    }
    ea.status = D.status.as<int32_t>();
    ea.cpl_hi = R.coupled ? D.cpl_hi.as<int32_t>() : nullptr;
    ea.cplLen = c.cplLen;
    ea.stride = mp;
    ea.order = nullptr;

    outputs_at(oo, d_out.as<double>(), os);
    oo.t_stride = mp;
    oo.decimate = R.step;
    oo.row0 = 0;

    std::memset(&rf, 0, sizeof(rf));
    if (R.use_raw) { /* the step kernel's view of the raw series (rs_step_raw, rs_cpl_replay_raw) */
      rf.nsrc = T.S.nsrc;
      for (int k = 0; k < T.S.nsrc; ++k) {
        for (int f = 0; f < NFLD; ++f) rf.src[k].fld[f] = T.S.src[k].fld[f];
        rf.src[k].plan = T.S.src[k].plan;
      }
      rf.nseg = (int32_t)c.segs.size();
      rf.segs = T.segs.as<ScanSeg>();
      rf.np_pad = mp;
      rf.status = D.status.as<int32_t>();
      rf.hour = r.ax.d_hour.as<int32_t>();
    }

    /* plan order (TilePolicy::cluster): the slot-order copies of what the launches read and write per point */
    rows_c = R.TC / R.step + 2;
    oc = oo;
    pps = pp;
    if (tp.cluster && R.skyview) { /* the four geometry scalars in slot order (padding: sky view 1.0 = off) */
      HOK(d_geo_s.alloc((size_t)4 * mp * sizeof(double)));
      hipLaunchKernelGGL(fill_f64_kernel, grid1((int64_t)(4 * mp)), dim3(RS_BLOCK), 0, stream,
                         d_geo_s.as<double>(), (int64_t)(4 * mp), 1.0);
      HOK(hipGetLastError());
      geometry_at(pps, d_geo_s.as<double>(), mp);
    }
    if (tp.cluster) {
      if (!R.use_raw) { /* (the raw-series step kernel writes its rows straight into point order) */
        HOK(d_outc.alloc((size_t)6 * rows_c * mp * sizeof(double)));
        outputs_at(oc, d_outc.as<double>(), (size_t)rows_c * mp);
      }
      /* slot-order copies: 4 doubles (3 relaxation targets, coupling observation), 2 int32 */
      HOK(d_pp_s.alloc((size_t)mp * (2 * sizeof(int32_t) + 4 * sizeof(double))));
      double *pd = d_pp_s.as<double>();
      const bool relax = r.st->use_relaxation == 1;
      pps.tair_relax = relax ? pd : nullptr;
      pps.vz_relax = relax ? pd + mp : nullptr;
      pps.rh_relax = relax ? pd + 2 * mp : nullptr;
      pps.initlen = reinterpret_cast<int32_t *>(pd + 4 * mp);
      if (R.coupled) {
        pps.coupling_tsurf = pd + 3 * mp;
        pps.coupling_index = reinterpret_cast<int32_t *>(pd + 4 * mp) + mp;
      }
      HOK(hipMemsetAsync(d_pp_s.p, 0, (size_t)mp * (2 * sizeof(int32_t) + 4 * sizeof(double)), stream));
      if (int rc = gather_params()) return rc;
    }
    return 0;
  }
  /* per-point parameters into the plan's current slot order */
  int gather_params() {
    ea.order = rs_hip_plan_order(pg.p); /* identity until the first recluster */
    if (!ea.order) return -14;
    double *pd = d_pp_s.as<double>();
    const bool coupled = R.coupled, skyview = R.skyview;
    hipLaunchKernelGGL(gather_params_kernel, grid1(m), dim3(RS_BLOCK), 0, stream, ea.order, (int64_t)m,
                       pp.initlen, const_cast<int32_t *>(pps.initlen), D.tair_relax.as<double>(), pd,
                       D.vz_relax.as<double>(), pd + mp, D.rh_relax.as<double>(), pd + 2 * mp,
                       coupled ? pp.coupling_index : nullptr,
                       coupled ? const_cast<int32_t *>(pps.coupling_index) : nullptr,
                       coupled ? pp.coupling_tsurf : nullptr,
                       coupled ? const_cast<double *>(pps.coupling_tsurf) : nullptr,
                       skyview ? pp.sky_view : nullptr, skyview ? d_geo_s.as<double>() : nullptr, (int64_t)mp);
    HOK(hipGetLastError());
    if (skyview) pps.horizon_index = ea.order; /* slot -> column of the horizon table */
    if (skyview && hz_table) {
      if (!d_hzcol_s.p) HOK(d_hzcol_s.alloc(mp * sizeof(int32_t)));
      hipLaunchKernelGGL(gather_i32_kernel, grid1(m), dim3(RS_BLOCK), 0, stream, ea.order, (int64_t)m, hz_col,
                         d_hzcol_s.as<int32_t>());
      HOK(hipGetLastError());
      pps.horizon_index = d_hzcol_s.as<int32_t>();
    }
    return 0;
  }
  /* The sources that can supply a value somewhere in [i0, i0+n): a shared-axis source whose plan is
   * K_NONE over the whole range - the observations behind their last report, i.e. for seven windows
   * out of eight of a 48 h run - is left out of the launch (it would cost a plan load and a branch
   * per index and variable for nothing).  Order kept: later sources win. */
  SrcSet sources_for(int i0, int n) const {
    SrcSet s = T.S;
    if (T.any_pp) return s;
    s.nsrc = 0;
    for (int k = 0; k < T.S.nsrc; ++k) {
      const std::vector<int32_t> &act = c.active_prefix[k];
      if (act[std::min(i0 + n, c.L)] - act[std::min(i0, c.L)] > 0) s.src[s.nsrc++] = T.S.src[k];
    }
    for (int k = s.nsrc; k < RS_MAX_SOURCES; ++k) s.src[k] = SrcDev{};
    return s;
  }
  /* one window [t0, t0+len): raw series -> step-resolution forcing on the device */
  int expand_window(int t0, int len, RsForcing &fo) {
    if (T.any_pp && walk_at != t0 - 1) { /* not the continuation of the last window: re-position */
      hipLaunchKernelGGL(pp_init_kernel, grid1(mp), dim3(RS_BLOCK), 0, stream, T.S);
      HOK(hipGetLastError());
      if (t0 > 1) {
        hipLaunchKernelGGL(pp_advance_kernel, grid1(mp), dim3(RS_BLOCK), 0, stream, T.S, (int32_t)0,
                           (int32_t)(t0 - 1));
        HOK(hipGetLastError());
      }
      walk_at = t0 - 1;
    }
    ea.i0 = t0 - 1;
    ea.nsteps = len;
    ea.S = sources_for(t0 - 1, len);
    launch_expand_raw(T.any_pp, mp, ea, stream);
    HOK(hipGetLastError());
    if (T.any_pp && t0 + len <= c.L) { /* per-point walks: move to the start of the next window */
      hipLaunchKernelGGL(pp_advance_kernel, grid1(mp), dim3(RS_BLOCK), 0, stream, T.S,
                         (int32_t)(t0 - 1), (int32_t)len);
      HOK(hipGetLastError());
      walk_at = t0 - 1 + len;
    }
    std::memset(&fo, 0, sizeof(fo));
    fo.tair = ea.out[R_TAIR]; fo.tdew = ea.out[R_TDEW]; fo.vz = ea.out[R_VZ];
    fo.rhz = ea.out[R_RHZ]; fo.prec = ea.out[R_PREC]; fo.sw = ea.out[R_SW]; fo.lw = ea.out[R_LW];
    fo.tsurfobs = ea.out[R_OBS];
    fo.depth = nullptr; /* InputData.cpp:18: Depth is never filled by the driver */
    fo.precphase = d_phase.as<int32_t>();
    fo.hour = r.ax.d_hour.as<int32_t>() + (t0 - 1);
    fo.t_stride = mp;
    fo.hour_pstride = 0;
    if (R.skyview) {
      fo.sw_dir = ea.out[R_SWDIR];
      fo.lw_net = ea.out[R_LWNET];
      fo.sun = r.ax.d_sun.as<double>() + (size_t)(t0 - 1) * RS_SUN_COLS;
    }
    return 0;
  }
  /* Plan order: re-sort of the slots for the launch that starts at t_next (TilePolicy::forecast_key), and the
   * per-point parameters into the new order. */
  int resort(int t_next) {
    if (!tp.cluster) return 0;
    const int len_next = std::min(R.TC, c.L - t_next + 1);
    if (!tp.forecast_key) {
      if (rs_hip_recluster(pg.p) != 0) return -14;
      return gather_params();
    }
    if (!d_prev.p) HOK(d_prev.alloc((size_t)9 * mp * sizeof(double)));
    double *prev = d_prev.as<double>();
    const int idx[3] = {t_next, t_next + len_next / 2, t_next + len_next - 1};
    RsPreview pv;
    std::memset(&pv, 0, sizeof(pv));
    if (R.use_raw) { /* air temperature and wind speed of the three indices in one launch ... */
      RawRowsArgs ra;
      std::memset(&ra, 0, sizeof(ra));
      ra.S = T.S;
      ra.status = ea.status;
      ra.order = ea.order;
      /* ... with their precipitation: nine rows (RsPreview::prec, the key's precipitation bit: +1.7 % / +4 %,
       * profiles/r05_ab_precip_bit.txt) */
      ra.nrows = 9;
      for (int q = 0; q < 3; ++q) {
        const int row[3] = {2 * q, 2 * q + 1, 6 + q}, fld[3] = {R_TAIR, R_VZ, R_PREC};
        for (int k = 0; k < 3; ++k) {
          ra.fld[row[k]] = fld[k];
          ra.idx[row[k]] = idx[q] - 1;
          ra.out[row[k]] = prev + (size_t)row[k] * mp;
        }
        pv.tair[q] = ra.out[2 * q];
        pv.vz[q] = ra.out[2 * q + 1];
        pv.prec[q] = ra.out[6 + q];
        pv.hour[q] = r.in->hour[idx[q] - 1];
      }
      hipLaunchKernelGGL(raw_rows_kernel, dim3((unsigned)(mp / RS_BLOCK), (unsigned)ra.nrows), dim3(RS_BLOCK), 0, stream, ra);
      HOK(hipGetLastError());
    } else {
      ExpandRawArgs pe = ea; /* current order, same decisions */
      for (int q = 0; q < 3; ++q) {
        for (int f = 0; f < NFLD; ++f) pe.out[f] = nullptr;
        pe.out[R_TAIR] = prev + (size_t)(2 * q) * mp;
        pe.out[R_VZ] = prev + (size_t)(2 * q + 1) * mp;
        pe.i0 = idx[q] - 1;
        pe.nsteps = 1;
        pe.S = sources_for(idx[q] - 1, 1);
        launch_expand_raw(false, mp, pe, stream);
        HOK(hipGetLastError());
        pv.tair[q] = pe.out[R_TAIR];
        pv.vz[q] = pe.out[R_VZ];
        pv.hour[q] = r.in->hour[idx[q] - 1];
      }
    }
    /* the boundary-layer regime at the window's first and last index; the middle one makes the key's count
     * fields finer and the order no better (relaxation 0.346 -> 0.343 s without it, as bench.py's FULL leg with
     * its windows of whole hours: profiles/r05_ab_driver_previews.txt).
     * Its precipitation row stays: the key's precipitation bit reads every row it is given. */
    pv.n = 2;
    pv.tair[1] = pv.tair[2];
    pv.vz[1] = pv.vz[2];
    pv.hour[1] = pv.hour[2];
    pv.tair_now = pv.tair[0];
    pv.alpha = 0.5;
    pv.mode = 378059; /* 10 bits + the ground digit: the plan's own counting sort (rs_cluster.hip) */
    if (rs_hip_recluster_forecast(pg.p, &pv) != 0) return -14;
    return gather_params();
  }
  /* The initial profile where there is no forcing window: index 1's air temperature and observation
   * (src/Initialization.f90:256-259) as two rows of the raw series */
  int init_state_from_raw() {
    HOK(d_row1.alloc((size_t)2 * mp * sizeof(double)));
    RawRowsArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    ra.S = T.S;
    ra.status = ea.status;
    ra.order = col();
    ra.nrows = 2;
    ra.fld[0] = R_TAIR;
    ra.fld[1] = R_OBS;
    ra.out[0] = d_row1.as<double>();
    ra.out[1] = d_row1.as<double>() + mp;
    hipLaunchKernelGGL(raw_rows_kernel, dim3((unsigned)(mp / RS_BLOCK), 2), dim3(RS_BLOCK), 0, stream, ra);
    HOK(hipGetLastError());
    RsForcing f1;
    std::memset(&f1, 0, sizeof(f1));
    f1.tair = f1.vz = f1.rhz = f1.prec = f1.sw = f1.lw = ra.out[0]; /* (only tair and tsurfobs are read) */
    f1.tsurfobs = ra.out[1];
    f1.precphase = reinterpret_cast<const int32_t *>(ra.out[0]);
    f1.hour = r.ax.d_hour.as<int32_t>();
    f1.t_stride = mp;
    return rs_hip_init_state(pg.p, &f1, &ppx()) != 0 ? -12 : 0;
  }
  /* `seg` and rf.seg0 to the segment that holds the 0-based index i (stage 3 of chunked coupling starts behind the
   * first window end: back) */
  void seek_seg(int i) {
    while (seg > 0 && c.segs[seg].i0 > i) --seg;
    while (seg + 1 < c.segs.size() && c.segs[seg].i1 <= i) ++seg;
    rf.seg0 = (int32_t)seg;
  }
  /* one launch over [t0, t0+len) from the raw series; its (decimated) rows go straight to their point's column
   * of the result */
  int step_raw(int t0, int len) {
    if (t0 == 1)
      if (int rc = init_state_from_raw()) return rc;
    seek_seg(t0 - 1);
    rf.col = col();
    const double *sunrows = R.skyview ? r.ax.d_sun.as<double>() + (size_t)(t0 - 1) * RS_SUN_COLS : nullptr;
    if (rs_step_raw(pg.p, &rf, sunrows, &oo, &ppx(), t0, len, tp.cluster) != 0) return -13;
    ++g_last_raw_launches;
    return 0;
  }
  /* a lock-step chunk of chunked coupling: from the raw series (rs_step_raw: no window) where the block steps that way */
  int lockstep(int t0, int len, RsForcing &fo) {
    if (R.use_raw) return step_raw(t0, len);
    if (int rc = expand_window(t0, len, fo)) return rc;
    if (t0 == 1 && rs_hip_init_state(pg.p, &fo, &ppx()) != 0) return -12;
    if (rs_hip_step_cpl(pg.p, &fo, &oo, &ppx(), t0, len) != 0) return -13;
    return 0;
  }
  /* Chunked coupling.  Stage 1: lock step to the last window end; stage 2: the replay rounds over the block
   * [first window start, last window end + 1]; stage 3: lock step from behind the first
   * window end (points whose window ends later wait there: they step only the index they
   * are due for).  Plan order: the slots are re-sorted after every lock-step chunk; windows and per-point
   * parameters are produced in slot order, outputs go to their point's column. */
  int loop_cpl_chunked(int last) { /* `last`: the last index stepped (SimLen; B for the stations of an ensemble call) */
    const int L = last, TC = R.TC;
    RsForcing fo;
    if (tp.cluster && rs_hip_set_output_by_point(pg.p, 1) != 0) return -14;
    const int s1_hi = tp.any_on ? std::min(tp.ce_max, L) : L;
    for (int t0 = 1; t0 <= s1_hi; t0 += TC) {
      const int len = std::min(TC, s1_hi - t0 + 1);
      if (int rc = lockstep(t0, len, fo)) return rc;
      /* the next lock-step chunk: the one behind this, or stage 3's first */
      const int t_next = (t0 + len <= s1_hi) ? t0 + len : (tp.any_on && tp.ce_min + 1 <= L) ? tp.ce_min + 1 : 0;
      if (t_next > 0)
        if (int rc = resort(t_next)) return rc;
    }
    if (!tp.any_on) return 0;
    int32_t rounds = 0;
    const int rlen = tp.r_hi - tp.r_lo + 1;
    if (tp.replay_raw) {
      seek_seg(tp.r_lo - 1);
      rf.col = col();
      if (rs_cpl_replay_raw(pg.p, &rf, &oo, &ppx(), tp.r_lo, rlen, tp.cluster, &rounds) != 0) return -13;
    } else {
      if (int rc = expand_window(tp.r_lo, rlen, fo)) return rc;
      if (rs_hip_cpl_replay(pg.p, &fo, &oo, &ppx(), tp.r_lo, rlen, &rounds) != 0) return -13;
    }
    /* every window is behind the plan: stage 3's re-sorts need not move the saved state */
    if (rs_hip_coupling_windows_closed(pg.p, 1) != 0) return -14;
    for (int t0 = tp.ce_min + 1; t0 <= L; t0 += TC) {
      const int len = std::min(TC, L - t0 + 1);
      if (int rc = lockstep(t0, len, fo)) return rc;
      if (t0 + len <= L)
        if (int rc = resort(t0 + len)) return rc;
    }
    return 0;
  }
  /* the members of an ensemble call with coupling: lock-step chunks over [first, SimLen] - every window is closed */
  int loop_lockstep(int first) {
    const int L = c.L, TC = R.TC;
    RsForcing fo;
    if (tp.cluster && rs_hip_set_output_by_point(pg.p, 1) != 0) return -14;
    for (int t0 = first; t0 <= L; t0 += TC) {
      const int len = std::min(TC, L - t0 + 1);
      if (int rc = lockstep(t0, len, fo)) return rc;
      if (t0 + len <= L)
        if (int rc = resort(t0 + len)) return rc;
    }
    return 0;
  }
  /* no windows: the step kernel's ground wave reads the raw series (rs_step_raw) */
  int loop_raw(int first, int last) {
    const int L = last, TC = R.TC;
    for (int t0 = first; t0 <= L; t0 += TC) {
      const int len = std::min(TC, L - t0 + 1);
      if (int rc = step_raw(t0, len)) return rc;
      if (t0 + len <= L)
        if (int rc = resort(t0 + len)) return rc;
    }
    return 0;
  }
  /* forcing windows for the one-point-per-lane kernels (rs_hip_step) */
  int loop_windows(int first, int last) {
    const int L = last, TC = R.TC, step = R.step;
    for (int t0 = first; t0 <= L; t0 += TC) {
      const int len = std::min(TC, L - t0 + 1);
      RsForcing fo;
      if (int rc = expand_window(t0, len, fo)) return rc;
      /* in plan order this launch's rows go to the launch buffer in slot order, then home */
      const int64_t r_first = ((int64_t)t0 - 1 + step - 1) / step;
      const int64_t r_last = ((int64_t)t0 + len - 2) / step;
      oc.row0 = r_first;
      if (t0 == 1 && rs_hip_init_state(pg.p, &fo, &ppx()) != 0) return -12;
      if (rs_hip_step(pg.p, &fo, tp.cluster ? &oc : &oo, &ppx(), t0, len) != 0) return -13;
      if (!tp.cluster) continue;
      if (r_last >= r_first) {
        hipLaunchKernelGGL(unpermute_rows_kernel, dim3((unsigned)(mp / RS_BLOCK), 6), dim3(RS_BLOCK), 0,
                           stream, ea.order, (int64_t)m, (const double *)d_outc.as<double>(),
                           (int64_t)rows_c, d_out.as<double>(), (int64_t)R.n_out, r_first,
                           (int32_t)(r_last - r_first + 1), (int64_t)mp);
        HOK(hipGetLastError());
      }
      if (t0 + len <= L)
        if (int rc = resort(t0 + len)) return rc;
    }
    return 0;
  }
  /* the six row pointers of the result block at kept row first_row: what the reducers of rs_cluster.hip read */
  void result_rows(const void *in[6], int first_row) const {
    for (int f = 0; f < 6; ++f) in[f] = d_out.as<double>() + (size_t)f * os + (size_t)first_row * mp;
  }
  /* a block [rows][mp] on the device -> [point][rows] in `pt` -> the tile's rows, from p0, of a host array
   * [n_points][rows] */
  int block_home(const double *block, double *pt, int rows, double *host) {
    HOK(transpose(block, pt, rows, m, mp, rows, stream));
    HOK(hipMemcpyAsync(host + (size_t)p0 * rows, pt, (size_t)m * rows * sizeof(double), hipMemcpyDeviceToHost, stream));
    return 0;
  }
  /* The summaries of the kept rows [first_row, last_row] (rs_driver_run_summary): reduced from the result block, which
   * is in point order, final (every coupling replay has rewritten its rows) and blanked where read_input rejected the
   * point; RS_SUM_COLS doubles per point come home for them. */
  int summaries_home() {
    const RsDriverSummary &q = *r.q.summary;
    HOK(d_sum.alloc((size_t)RS_SUM_COLS * mp * sizeof(double)));
    HOK(d_sumpt.alloc((size_t)m * RS_SUM_COLS * sizeof(double)));
    HOK(rs_cluster_summary_reset(d_sum.as<double>(), mp, stream));
    const void *in[6];
    result_rows(in, q.first_row);
    HOK(rs_cluster_outputs_summary(in, false, nullptr, m, mp, q.last_row - q.first_row + 1, q.first_row * R.step + 1,
                                   R.step, q.spec, d_sum.as<double>(), mp, stream));
    return block_home(d_sum.as<double>(), d_sumpt.as<double>(), RS_SUM_COLS, q.summary);
  }
  /* The group series of the kept rows [first_row, last_row] (rs_driver_run_groups), from the same final, blanked
   * result block: the tile's points merge into the block's accumulator, which comes home behind the last tile. */
  int groups_home() {
    const RsDriverGroups &q = *r.q.groups;
    HOK(d_gid.alloc((size_t)m * sizeof(int32_t)));
    HOK(hipMemcpyAsync(d_gid.p, q.group + p0, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    const void *in[6];
    result_rows(in, q.first_row);
    HOK(rs_cluster_outputs_groups(in, false, nullptr, d_gid.as<int32_t>(), m, mp, q.last_row - q.first_row + 1, q.spec,
                                  r.grp_acc, stream));
    return 0;
  }
  /* a block [n_out][mp] -> the tile's rows of a host array [n_points][n_out] */
  int rows_home(const double *block, double *host) { return block_home(block, d_outpt.as<double>(), R.n_out, host); }
  /* The inputs at the kept rows and the dew-point deficit (rs_driver_run_kept): the wanted variables one at a time from
   * the tile's raw columns and plans through the one buffer - the dew point first, which the deficit then replaces in
   * place, reading the final, blanked surface temperature rows of the result block.  Where the episodes read the
   * deficit (rs_driver_run_episodes) the dew point's turn goes through a buffer of its own, which keeps the deficit
   * for episodes_home: it is made once, whoever wants it. */
  int kept_home() {
    const RsDriverKept *q = r.q.kept;
    if (q) HOK(d_kept.alloc(os * sizeof(double)));
    if (R.epi_deficit) HOK(d_epidef.alloc(os * sizeof(double)));
    KeptRowsArgs ka;
    std::memset(&ka, 0, sizeof(ka));
    ka.S = T.S;
    ka.nfld = 1;
    ka.cpl_hi = R.coupled ? D.cpl_hi.as<int32_t>() : nullptr;
    ka.cplLen = c.cplLen;
    ka.step = R.step;
    ka.n_out = R.n_out;
    ka.stride = mp;
    const int turn[NFLD] = {R_TDEW, R_TAIR, R_VZ, R_RHZ, R_PREC, R_SW, R_LW, R_SWDIR, R_LWNET, R_OBS};
    for (int k = 0; k < NFLD; ++k) {
      const int f = turn[k];
      double *host = q ? q->merged[f] : nullptr;
      const bool deficit = f == R_TDEW && ((q && q->deficit) || R.epi_deficit);
      if (!host && !deficit) continue;
      double *block = f == R_TDEW && R.epi_deficit ? d_epidef.as<double>() : d_kept.as<double>();
      ka.fld[0] = f;
      ka.out[0] = block;
      const dim3 g((unsigned)(mp / RS_BLOCK), 1), b(RS_BLOCK);
      if (T.any_pp)
        hipLaunchKernelGGL(kept_rows_kernel<true>, g, b, 0, stream, ka);
      else
        hipLaunchKernelGGL(kept_rows_kernel<false>, g, b, 0, stream, ka);
      HOK(hipGetLastError());
      if (host)
        if (int rc = rows_home(block, host)) return rc;
      if (deficit) {
        hipLaunchKernelGGL(deficit_kernel, grid1(m), dim3(RS_BLOCK), 0, stream, (const double *)d_out.as<double>(), block,
                           (int64_t)mp, (int32_t)R.n_out, (int64_t)m);
        HOK(hipGetLastError());
        if (q && q->deficit)
          if (int rc = rows_home(block, q->deficit)) return rc;
      }
    }
    return 0;
  }
  /* The threshold episodes of the kept rows [first_row, last_row] (rs_driver_run_episodes), from the same final, blanked
   * result block as the summaries and - where the spec uses it - the deficit kept_home left in d_epidef: reset, one feed
   * of the rows in order, finish; cols doubles per point come home for them. */
  int episodes_home() {
    const RsDriverEpisodes &q = *r.q.episodes;
    const int cols = R.epi_cols;
    HOK(d_epi.alloc((size_t)cols * mp * sizeof(double)));
    HOK(d_epipt.alloc((size_t)m * cols * sizeof(double)));
    HOK(rs_cluster_episodes_reset(d_epi.as<double>(), mp, q.spec, stream));
    const void *in[6];
    result_rows(in, q.first_row);
    const void *def = R.epi_deficit ? d_epidef.as<double>() + (size_t)q.first_row * mp : nullptr;
    HOK(rs_cluster_outputs_episodes(in, def, false, nullptr, m, mp, q.last_row - q.first_row + 1,
                                    q.first_row * R.step + 1, R.step, q.spec, d_epi.as<double>(), mp, stream));
    HOK(rs_cluster_episodes_finish(d_epi.as<double>(), m, mp, q.spec, stream));
    return block_home(d_epi.as<double>(), d_epipt.as<double>(), cols, q.episodes);
  }
  /* The members of an ensemble call (rs_driver_run_ensemble), stations [s0, s0 + ms) of n_stations: blank what
   * read_input rejected, reduce the kept rows from first_row on per station - the member table of the tile's members,
   * the cells of the tile's stations into their columns of the caller's [n_tail][n_stations][cols] - and bring the
   * wanted series' rows from first_row on home. */
  int members_home(const RsDriverEnsemble &e, int first_row, const int32_t *parent_local, int64_t s0, int ms,
                   int64_t n_stations) {
    double *ob = d_out.as<double>();
    hipLaunchKernelGGL(blank_rejected_kernel, grid1(m), dim3(RS_BLOCK), 0, stream, ob, (int64_t)mp,
                       (int32_t)R.n_out, (int64_t)m, (const int32_t *)D.status.as<int32_t>());
    HOK(hipGetLastError());
    const int n_tail = R.n_out - first_row;
    std::vector<int32_t> table; /* (alive until the stream has drained) */
    std::vector<double> cells;
    if (n_tail > 0 && (e.stats_spec || e.probs_spec)) {
      const void *in[6];
      result_rows(in, first_row);
      HOK(d_einv.alloc(mp * sizeof(int32_t)));
      HOK(rs_cluster_identity(d_einv.as<int32_t>(), mp, stream)); /* the result block is in point order */
      RsEnsSpec ts;
      std::memset(&ts, 0, sizeof(ts));
      ts.ngroups = ms;
      char err[300];
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 ? !e.stats_spec : !e.probs_spec) continue;
        const int32_t mm = pass == 0 ? e.stats_spec->max_members : e.probs_spec->max_members;
        if (table.empty() || ts.max_members != mm) { /* one table serves both reducers under one max_members */
          HOK(hipStreamSynchronize(stream)); /* (the upload of the last one) */
          ts.max_members = mm;
          table.assign((size_t)ms + 1 + m, 0);
          if (rs_ens::member_table(m, parent_local, &ts, table.data(), err, sizeof(err)) != 0) return fail_msg(err, -1);
          HOK(d_etable.alloc(table.size() * sizeof(int32_t)));
          HOK(hipMemcpyAsync(d_etable.p, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        }
        int cols;
        double *host;
        if (pass == 0) {
          RsEnsSpec sp = *e.stats_spec;
          sp.ngroups = ms;
          cols = rs_ens::cols(&sp);
          HOK(d_eacc.alloc((size_t)n_tail * ms * cols * sizeof(double)));
          HOK(rs_cluster_outputs_ens(in, false, d_etable.as<int32_t>(), d_einv.as<int32_t>(), m, mp, n_tail, sp,
                                     d_eacc.as<double>(), stream));
          host = e.stats;
        } else {
          RsProbSpec sp = *e.probs_spec;
          sp.ngroups = ms;
          cols = rs_cluster_prob_cols(&sp);
          HOK(d_ever.alloc(mp * sizeof(int32_t)));
          HOK(hipMemsetAsync(d_ever.p, 0, mp * sizeof(int32_t), stream)); /* one carry per tile, reset once */
          HOK(d_words.alloc((size_t)n_tail * mp * sizeof(uint32_t)));
          HOK(d_eacc.alloc((size_t)n_tail * ms * cols * sizeof(double)));
          HOK(rs_cluster_outputs_prob(in, nullptr, false, nullptr, d_etable.as<int32_t>(), d_einv.as<int32_t>(), m, mp, n_tail,
                                      sp, d_ever.as<int32_t>(), d_words.as<uint32_t>(), mp, d_eacc.as<double>(), stream));
          host = e.probs;
        }
        cells.resize((size_t)n_tail * ms * cols);
        HOK(hipMemcpyAsync(cells.data(), d_eacc.p, cells.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
        HOK(hipStreamSynchronize(stream)); /* (d_eacc is the next pass's too) */
        for (int r = 0; r < n_tail; ++r) /* the tile's stations' columns of every row */
          std::memcpy(host + ((size_t)r * n_stations + s0) * cols, cells.data() + (size_t)r * ms * cols,
                      (size_t)ms * cols * sizeof(double));
      }
    }
    const RsDriverOutput &o = e.member_out;
    double *dst[6] = {o.tsurf, o.snow, o.water, o.ice, o.deposit, o.ice2};
    for (int f = 0; f < 6 && n_tail > 0; ++f)
      if (dst[f])
        if (int rc = block_home(ob + (size_t)f * os + (size_t)first_row * mp, d_outpt.as<double>(), n_tail, dst[f])) return rc;
    HOK(hipStreamSynchronize(stream));
    r.pt.lap(5);
    return 0;
  }
  /* blank what read_input rejected, then [row][point] -> [point][row] -> the caller's arrays */
  int outputs_home() {
    double *ob = d_out.as<double>();
    hipLaunchKernelGGL(blank_rejected_kernel, grid1(m), dim3(RS_BLOCK), 0, stream, ob, (int64_t)mp,
                       (int32_t)R.n_out, (int64_t)m,
                       (const int32_t *)(d_status_rep.p ? d_status_rep.as<int32_t>() : D.status.as<int32_t>()));
    HOK(hipGetLastError());
    if (r.q.summary)
      if (int rc = summaries_home()) return rc;
    if (r.q.groups)
      if (int rc = groups_home()) return rc;
    if (r.q.kept || R.epi_deficit)
      if (int rc = kept_home()) return rc;
    if (r.q.episodes)
      if (int rc = episodes_home()) return rc;
    double *dst[6] = {r.out->tsurf, r.out->snow, r.out->water, r.out->ice, r.out->deposit, r.out->ice2};
    for (int f = 0; f < 6; ++f)
      if (dst[f])
        if (int rc = rows_home(ob + (size_t)f * os, dst[f])) return rc;
    HOK(hipStreamSynchronize(stream));
    r.pt.lap(5);
    for (Dev *d : {&d_phase, &d_outc, &d_pp_s, &d_geo_s, &d_out, &d_outpt, &d_prev, &d_sum, &d_sumpt, &d_gid, &d_kept, &d_epidef, &d_epi, &d_epipt}) d->release();
    r.pt.lap(7);
    return 0;
  }
};

int check_run_arguments(const RsDriverInput *in, const InputSettings *st, const InputParameters *params,
                        const LocalParameters *local, const RsDriverOutput *out, const Common &c, RunPolicy &R,
                        RsConstants &consts) {
  if (!params || !local || !out) return fail_msg("rs_driver_run: params, local and out are required", -1);
  if (!in->year || !in->month || !in->day || !in->hour || !in->minute || !in->second)
    return fail_msg("rs_driver_run: the calendar arrays of the simulation times are required", -1);
  /* roadrunner.cpp:290: int step = outputStep*60/DTSecs */
  R.step = (int)((double)(st->outputStep * 60) / st->DTSecs);
  if (R.step < 1) return fail_msg("rs_driver_run: outputStep*60/DTSecs < 1", -1);
  R.n_out = (c.L + R.step - 1) / R.step;
  if (out->n_out != R.n_out) {
    char b[160];
    snprintf(b, sizeof(b), "rs_driver_run: n_out must be ceil(SimLen/step) = %d (step %d)", R.n_out, R.step);
    return fail_msg(b, -1);
  }
  int32_t rc32 = 0;
  rs_build_constants(st, params, &consts, &rc32);
  if (rc32 != 0)
    return fail_msg("rs_driver_run: bad settings (NLayers in 5..32, SimLen >= 1, DTSecs > 0)", -1);
  return 0;
}

/* Every buffer of a tile other than the forcing windows comes out of one block this worker keeps
 * across calls (rs_devutil.hpp: Arena): no hipMalloc / hipFree inside the tile loop.  The size is
 * an estimate from the tile's shape; what does not fit is allocated the old way. */
size_t arena_estimate(const RsDriverInput *in, const Common &c, const RunPolicy &R) {
  const size_t mpx = ((size_t)R.P + RS_BLOCK - 1) / RS_BLOCK * RS_BLOCK, L = (size_t)c.L, TC = (size_t)R.TC;
  size_t raw = 0;
  for (int k = 0; k < c.nsrc; ++k) {
    const size_t nt = (size_t)std::max(in->sources[k].n_times, 1);
    raw += nt * mpx * 8 * (NFLD + 1) + L * sizeof(PlanStep) + 3 * mpx * 8;
  }
  const size_t rows = R.cpl_chunked ? (size_t)std::max(R.TC, std::min(c.L, c.cplLen + 2)) : TC;
  size_t need = 2 * raw                                /* raw series + their landing block */
                + mpx * 160                            /* decisions, bottom temperature, slot-order copies */
                + mpx * rows * 4                       /* PrecPhase window */
                + 7 * mpx * (size_t)R.n_out * 8        /* outputs + their point-major copy */
                + 6 * mpx * (TC / R.step + 2) * 8      /* one launch's rows in slot order */
                + 6 * mpx * 8 + L * 40;                /* previews, hour, sun */
  if (R.skyview) need += 2 * (size_t)360 * mpx * 8 + 8 * mpx * 8;
  if (R.kept) need += mpx * (size_t)R.n_out * 8; /* one variable's kept rows */
  if (R.epi_deficit) need += mpx * (size_t)R.n_out * 8; /* the deficit the episodes read */
  need += 2 * mpx * (size_t)R.epi_cols * 8;             /* the episodes, twice */
  need += mpx * ((size_t)2 * RS_NSTATE * 8 + 64) + ((size_t)16 << 20); /* the tile's plan: two state blocks, order rows, sort scratch */
  need += need / 16 + ((size_t)64 << 10) * 64; /* alignment of ~60 pieces, slack */
  return need;
}

int upload_shared_axes(const Call &k, const RunPolicy &R, int64_t pbeg, int64_t pend, SharedAxes &A) {
  const RsDriverInput *in = k.in;
  const int L = k.c.L;
  HOK(A.d_hour.alloc((size_t)L * sizeof(int32_t)));
  HOK(hipMemcpyAsync(A.d_hour.p, in->hour, (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, k.stream));
  if (!R.skyview) return 0;
  A.sun.resize((size_t)L * RS_SUN_COLS);
  rs_sun_table(L, in->year, in->month, in->day, in->hour, in->minute, in->second, A.sun.data());
  HOK(A.d_sun.alloc(A.sun.size() * sizeof(double)));
  HOK(hipMemcpyAsync(A.d_sun.p, A.sun.data(), A.sun.size() * sizeof(double), hipMemcpyHostToDevice, k.stream));
  A.slat.resize(pend - pbeg);
  A.clat.resize(pend - pbeg);
  A.lrad.resize(pend - pbeg);
  rs_point_geometry((int32_t)(pend - pbeg), k.local + pbeg, A.slat.data(), A.clat.data(), A.lrad.data());
  return 0;
}

/* a and b merged into a, cells of `cols` numbers each: counts add, extremes are the extremes of the two
 * (roadsurf_amd/groups.py, merge) */
void merge_group_cells(double *a, const double *b, size_t ncells, int cols) {
  for (size_t i = 0; i < ncells; ++i, a += cols, b += cols)
    for (int c = 0; c < cols; ++c) a[c] = rs_grp::merge(c, a[c], b[c]);
}
std::mutex g_group_merge; /* the blocks of a fan-out merge into the caller's one array */

/* ---- the request's argument checks.  A message names the entry that introduced the member, whichever entry the call
 * came in through.  What a caller can observe fixes their order: the episodes, then the groups, before anything else
 * of the call (check_request, once, on the calling thread); the summary's rows behind the checks of the run's own
 * arguments (check_summary, in every worker: n_out is only known to be the run's there). */
bool rows_in(int first_row, int last_row, int n_out) { return first_row >= 0 && last_row >= first_row && last_row < n_out; }

int check_request(RsDriverRequest &q, const RsDriverOutput *out) {
  if ((q.episodes || q.groups) && !out) return fail_msg("rs_driver_run: bad arguments", -1);
  if (const RsDriverEpisodes *e = q.episodes) {
    if (rs_cluster_episode_cols(&e->spec) < 0)
      return fail_msg("rs_driver_run_episodes: bad spec (use: bits 0..6, at least one; no NaN bound; peak 0..6; min_rows >= 1; max_episodes 1..RS_EPI_MAX)", -1);
    if (!e->episodes || !rows_in(e->first_row, e->last_row, out->n_out))
      return fail_msg("rs_driver_run_episodes: episodes is required, with 0 <= first_row <= last_row < n_out", -1);
  }
  if (const RsDriverKept *k = q.kept) { /* nothing wanted: as without */
    bool any = k->deficit != nullptr;
    for (int f = 0; f < NFLD; ++f) any = any || k->merged[f];
    if (!any) q.kept = nullptr;
  }
  if (const RsDriverGroups *g = q.groups) {
    if (rs_cluster_group_cols(&g->spec) < 0)
      return fail_msg("rs_driver_run_groups: bad spec (ngroups >= 1, nedges <= RS_GRP_MAX_EDGES, edges strictly increasing)", -1);
    if (!g->group || !g->series || !rows_in(g->first_row, g->last_row, out->n_out))
      return fail_msg("rs_driver_run_groups: group and series are required, with 0 <= first_row <= last_row < n_out", -1);
  }
  return 0;
}

int check_summary(const RsDriverSummary *sum, int n_out) {
  if (sum && (!sum->summary || !rows_in(sum->first_row, sum->last_row, n_out)))
    return fail_msg("rs_driver_run_summary: summary is required, with 0 <= first_row <= last_row < n_out", -1);
  return 0;
}

/* ---- gridded sources (RsGridSource): checked on the host, their fields resident once per device of the call */

bool any_grid(const RsDriverInput *in, const RsGridSource *const *grids) {
  if (!grids || !in || !in->sources || in->n_sources < 1 || in->n_sources > RS_MAX_SOURCES) return false;
  for (int s = 0; s < in->n_sources; ++s)
    if (grids[s]) return true;
  return false;
}

/* before any device work: what a gridded source must be, and a scan of its n_points x stencil nodes and weights */
int check_grids(const RsDriverInput *in, const RsGridSource *const *grids) {
  char b[200];
  for (int s = 0; s < in->n_sources; ++s) {
    const RsGridSource *g = grids[s];
    if (!g) continue;
    const RsRawSource &rs = in->sources[s];
    if (rs.times_per_point || rs.lengths) {
      snprintf(b, sizeof(b), "rs_driver: gridded source %d needs a time axis shared by all points (times_per_point = 0, lengths NULL)", s);
      return fail_msg(b, -1);
    }
    for (int f = 0; f < NFLD; ++f)
      if (raw_field(rs, f)) {
        snprintf(b, sizeof(b), "rs_driver: gridded source %d: the field pointers of its RsRawSource must be NULL (the fields are the RsGridSource's)", s);
        return fail_msg(b, -1);
      }
    if (g->stencil < 1 || g->stencil > RS_GRID_MAX_STENCIL) {
      snprintf(b, sizeof(b), "rs_driver: gridded source %d: stencil %d outside 1..%d", s, g->stencil, RS_GRID_MAX_STENCIL);
      return fail_msg(b, -1);
    }
    if (g->n_nodes < 1 || !g->node || !g->weight) {
      snprintf(b, sizeof(b), "rs_driver: gridded source %d: n_nodes >= 1, node and weight are required", s);
      return fail_msg(b, -1);
    }
    const int st = g->stencil;
    for (int64_t p = 0; p < in->n_points; ++p)
      for (int k = 0; k < st; ++k) {
        const double w = g->weight[p * st + k];
        const int64_t nd = g->node[p * st + k];
        if (!std::isfinite(w)) {
          snprintf(b, sizeof(b), "rs_driver: gridded source %d: weight %d of point %lld is not finite", s, k, (long long)p);
          return fail_msg(b, -1);
        }
        if (w != 0.0 && (nd < 0 || nd >= g->n_nodes)) {
          snprintf(b, sizeof(b), "rs_driver: gridded source %d: node %d of point %lld (%lld) outside [0, n_nodes = %lld) under a non-zero weight",
                   s, k, (long long)p, (long long)nd, (long long)g->n_nodes);
          return fail_msg(b, -1);
        }
      }
  }
  return 0;
}

/* The calling thread's part: every gridded source's fields to every distinct device of the call, each device's in
 * its turn on the link (copy_gate), before the blocks start. */
struct GridUploads {
  std::vector<GridDevice *> devs;
  ~GridUploads() {
    for (GridDevice *d : devs) delete d;
  }
  const GridDevice *find(int device) const {
    for (const GridDevice *d : devs)
      if (d->device == device) return d;
    return nullptr;
  }
};

int upload_grids(const RsDriverInput *in, const RsGridSource *const *grids, const std::vector<int> &devices,
                 GridUploads &G) {
  for (int device : devices) {
    if (G.find(device)) continue;
    if (int rc = check_device(device)) return rc;
    HOK(hipSetDevice(device));
    GridDevice *d = new GridDevice;
    d->device = device;
    G.devs.push_back(d);
    StreamGuard sg;
    HOK(hipStreamCreate(&sg.s));
    const double tg0 = PhaseTimer::now();
    std::lock_guard<std::mutex> turn(rsu::copy_gate(device));
    size_t bytes = 0;
    for (int s = 0; s < in->n_sources; ++s) {
      const RsGridSource *g = grids[s];
      if (!g || in->sources[s].n_times < 1) continue;
      const size_t nb = (size_t)in->sources[s].n_times * (size_t)g->n_nodes * sizeof(double);
      for (int f = 0; f < NFLD; ++f) {
        const double *h = grid_field(*g, f);
        if (!h) continue;
        HOK(d->fld[s][f].alloc(nb));
        HOK(hipMemcpyAsync(d->fld[s][f].p, h, nb, hipMemcpyHostToDevice, sg.s));
        bytes += nb;
      }
    }
    HOK(hipStreamSynchronize(sg.s));
    if (getenv("ROADSURF_HIP_DRIVER_TIMING"))
      fprintf(stderr, "rs_driver_run grid fields: %.1f MB to device %d in %.1f ms\n", 1e-6 * (double)bytes, device,
              1e3 * (PhaseTimer::now() - tg0));
  }
  return 0;
}

/* points [pbeg, pend) of the input on one device */
int driver_run_range(const RsDriverInput *in, const InputSettings *st, const InputParameters *params,
                     LocalParameters *local, const RsDriverOutput *out, const RsDriverRequest &q, int32_t device,
                     int64_t pbeg, int64_t pend, const GridView *gv = nullptr) {
  Common c;
  RunPolicy R;
  RsConstants consts;
  if (int rc = prepare(in, st, c, gv)) return rc;
  if (int rc = check_run_arguments(in, st, params, local, out, c, R, consts)) return rc;
  if (int rc = check_summary(q.summary, R.n_out)) return rc;
  if (int rc = check_device(device)) return rc;
  HOK(hipSetDevice(device));
  StreamGuard sg; /* the worker's one stream: uploads, kernels and downloads of its tiles (upload_tile) */
  HOK(hipStreamCreate(&sg.s));
  const hipStream_t stream = sg.s;
  Dev d_grp; /* this block's group cells, kept across its tiles (its own allocation: the arena is the tiles') */
  const RsDriverGroups *grp = q.groups;
  const RsDriverEpisodes *epi = q.episodes;
  const size_t grp_cells = grp ? (size_t)(grp->last_row - grp->first_row + 1) * grp->spec.ngroups : 0;
  const int grp_cols = grp ? rs_cluster_group_cols(&grp->spec) : 0;
  if (grp) {
    HOK(d_grp.alloc(grp_cells * grp_cols * sizeof(double)));
    HOK(rs_cluster_group_reset(d_grp.as<double>(), grp->last_row - grp->first_row + 1, grp->spec, stream));
  }
  make_run_policy(st, consts, c, local, pbeg, pend, R);
  R.kept = q.kept != nullptr;
  R.epi_cols = epi ? rs_cluster_episode_cols(&epi->spec) : 0;
  R.epi_deficit = epi && (((epi->spec.use >> 6) & 1) || epi->spec.peak == 6);
  const Call call{in, st, c, consts, device, stream, local, out->status, out->missing_index};

  WindowLease arena_lease; /* (declared behind the stream guard: WindowLease::release) */
  arena_lease.stream = stream;
  arena_lease.cache = g_arenacache;
  rsu::Arena arena;
  const size_t arena_bytes = arena_estimate(in, c, R);
  if (arena_lease.acquire(arena_bytes, device) == hipSuccess) {
    arena.base = static_cast<char *>(arena_lease.p);
    arena.cap = arena_bytes;
  }
  ArenaScope arena_scope(arena.base ? &arena : nullptr);
  SharedAxes ax;
  if (int rc = upload_shared_axes(call, R, pbeg, pend, ax)) return rc;

  PhaseTimer pt(stream, R.timing);
  pt.lap(0);
  WindowLease win;
  win.stream = stream;
  /* chunked coupling: the replay block spans a coupling window plus the index behind it
   * (usually more rows than a chunk); a tile whose windows are spread further re-leases (Tile::buffers).
   * A block that steps from the raw series needs windows for the replay rounds of coupling only: sized per tile. */
  const int64_t Ppad = ((int64_t)R.P + RS_BLOCK - 1) / RS_BLOCK * RS_BLOCK;
  const int rows0 = R.cpl_chunked ? std::max(R.TC, std::min(c.L, c.cplLen + 2)) : R.TC;
  Run run{call, params, out, R, pbeg, pend,
          rs_bottom_temperature(params, &consts, in->year[0], in->month[0], in->day[0]), ax, pt, win,
          R.use_raw ? 0 : (size_t)R.nwin * Ppad * rows0 * sizeof(double), q, d_grp.as<double>()};
  if (run.win_bytes) HOK(win.acquire(run.win_bytes, device));
  pt.lap(6);

  int Pcur = R.P;
  g_last_tiles = 0;
  g_last_raw_launches = 0;
  const size_t arena_mark = arena.off; /* the shared axes stay; a tile's buffers go when it is done */
  for (int64_t p0 = pbeg; p0 < pend;) {
    arena.rewind(arena_mark); /* the last tile's buffers are gone (same stream: what still runs there runs first) */
    const int m = (int)std::min<int64_t>(Pcur, pend - p0);
    Tile X(run, p0, m);
    /* (chunked coupling sizes its replay block from the decisions: it needs them at once) */
    if (int rc = tile_prologue(run, p0, m, R.skyview && in->horizons, R.cpl_chunked, pt, X)) return rc;
    if (int rc = X.point_params()) return rc;
    X.tp = make_tile_policy(R, c, st, local, p0, m, X.mp, X.T.any_pp);
    if (X.tp.halve_to) { /* started again at the same p0 */
      Pcur = X.tp.halve_to;
      continue;
    }
    if (int rc = X.buffers()) return rc;
    pt.lap(3);
    /* The three organisations of the time loop share one cycle - the forcing for [t0, t0+len), the initial state at
     * t0 = 1, the step, the re-sort for the next chunk - and differ in the rs_* entries they call.  (With the
     * forecast key nobody reads the step kernels' history score: the instances run without it.) */
    if (rs_hip_set_history_score(X.pg.p, (X.tp.cluster && X.tp.forecast_key && !R.cpl_chunked) ? 0 : 1) != 0) return -14;
    if (int rc = R.cpl_chunked ? X.loop_cpl_chunked(c.L) : R.use_raw ? X.loop_raw(1, c.L) : X.loop_windows(1, c.L)) return rc;
    X.d_row1.release();
    /* everything is enqueued: the decisions go to the caller's arrays while the device works */
    if (int rc = report_finish(c, st, X.rep, local, out->status, out->missing_index)) return rc;
    pt.lap(4);
    if (int rc = X.outputs_home()) return rc;
    p0 += m;
    ++g_last_tiles;
    Pcur = R.P; /* the next tile starts at full size again */
  }
  if (grp) { /* (every tile ended with a synchronisation: the accumulator is final) */
    std::vector<double> part(grp_cells * grp_cols);
    HOK(hipMemcpyAsync(part.data(), d_grp.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HOK(hipStreamSynchronize(stream));
    std::lock_guard<std::mutex> lk(g_group_merge);
    merge_group_cells(grp->series, part.data(), grp_cells, grp_cols);
  }
  pt.report();
  return 0;
}

/* the input side alone (rs_driver_expand, rs_driver_expand_grid) */
int driver_expand(const RsDriverInput *in, const RsGridSource *const *grids, const InputSettings *st,
                  LocalParameters *local, double *merged, int32_t *status, int32_t *missing_index, int32_t device) {
  GridUploads G; /* (declared first: freed when every stream of the call is gone) */
  GridView gv{grids, nullptr};
  const bool gridded = any_grid(in, grids);
  if (gridded) {
    if (int rc = check_grids(in, grids)) return rc;
    if (int rc = upload_grids(in, grids, std::vector<int>{device}, G)) return rc;
    gv.dev = G.find(device);
  }
  Common c;
  if (int rc = prepare(in, st, c, gridded ? &gv : nullptr)) return rc;
  if (!merged) return fail_msg("rs_driver_expand: merged is required", -1);
  if (int rc = check_device(device)) return rc;
  HOK(hipSetDevice(device));
  StreamGuard sg;
  HOK(hipStreamCreate(&sg.s));
  /* the math tables live with the plans' constants: make one (any valid constants do) */
  InputSettings s15 = *st;
  InputParameters prm;
  rs_default_parameters(&prm, st->DTSecs);
  RsConstants consts;
  int32_t rc32 = 0;
  rs_build_constants(&s15, &prm, &consts, &rc32);
  if (rc32 != 0) return fail_msg("rs_driver_expand: bad settings", -1);
  const Call call{in, st, c, consts, device, sg.s, local, status, missing_index};
  PhaseTimer pt(sg.s, false);
  const int P = std::min(c.n, 4096);
  for (int64_t p0 = 0; p0 < c.n; p0 += P) {
    const int m = (int)std::min<int64_t>(P, c.n - p0);
    TileHead H;
    if (int rc = tile_prologue(call, p0, m, false, true, pt, H)) return rc;
    const int64_t mp = H.mp;
    Dev win, pt_out;
    HOK(win.alloc((size_t)NFLD * c.L * mp * sizeof(double)));
    HOK(pt_out.alloc((size_t)m * c.L * sizeof(double)));
    ExpandRawArgs ea;
    ea.S = H.T.S;
    for (int f = 0; f < NFLD; ++f) ea.out[f] = win.as<double>() + (size_t)f * c.L * mp;
    ea.status = nullptr; /* the test hook shows what read_input returns, rejected or not */
    ea.order = nullptr;
    ea.cpl_hi = st->use_coupling == 1 ? H.D.cpl_hi.as<int32_t>() : nullptr;
    ea.cplLen = c.cplLen;
    ea.i0 = 0;
    ea.nsteps = c.L;
    ea.stride = mp;
    launch_expand_raw(H.T.any_pp, mp, ea, sg.s);
    HOK(hipGetLastError());
    for (int f = 0; f < NFLD; ++f) {
      HOK(transpose((const double *)ea.out[f], pt_out.as<double>(), c.L, m, mp, c.L, sg.s));
      HOK(hipMemcpyAsync(merged + ((size_t)f * c.n + p0) * c.L, pt_out.p, (size_t)m * c.L * sizeof(double),
                         hipMemcpyDeviceToHost, sg.s));
    }
    HOK(hipStreamSynchronize(sg.s));
  }
  return 0;
}

/* rs_driver_run_request and the older entries: one device, or the fan-out.  `q` is the call's own copy of the request:
 * check_request normalises it (kept with nothing wanted becomes NULL), and the workers read nothing else. */
int driver_run(const RsDriverInput *in, const InputSettings *st, const InputParameters *params, LocalParameters *local,
               const RsDriverOutput *out, RsDriverRequest q, int32_t device) {
  if (!in || in->n_points < 1) return fail_msg("rs_driver_run: bad arguments", -1);
  if (int rc = check_request(q, out)) return rc;
  if (const RsDriverGroups *grp = q.groups) { /* the empty cells: what merge_group_cells starts from */
    const int cols = rs_cluster_group_cols(&grp->spec);
    const size_t ncells = (size_t)(grp->last_row - grp->first_row + 1) * grp->spec.ngroups;
    for (size_t i = 0; i < ncells; ++i)
      for (int c = 0; c < cols; ++c) grp->series[i * cols + c] = rs_grp::empty(c);
  }
  const RsGridSource *const *grids = q.grids;
  const bool gridded = any_grid(in, grids);
  if (gridded)
    if (int rc = check_grids(in, grids)) return rc;
  GridUploads G;
  GridView gv{grids, nullptr};
  if (device >= 0) {
    if (gridded) {
      if (int rc = upload_grids(in, grids, std::vector<int>{device}, G)) return rc;
      gv.dev = G.find(device);
    }
    rsu::g_last_fanout = 1;
    return driver_run_range(in, st, params, local, out, q, device, 0, in->n_points, gridded ? &gv : nullptr);
  }
  /* four blocks per device.  (Six for batches with local horizons were 4 % faster while the horizon table
   * was transposed on the device, tools/experiments/r4_blocks.sh; with the table left in the caller's layout
   * - RsPointParams::horizons_by_point - four and six are level: 1.047e10 / 1.046e10 over three alternating
   * runs each.) */
  /* With local horizons a block uploads twice the bytes, the blocks start 38 instead of 19 ms apart and - of equal
   * size - end that far apart too: there the blocks shrink, the last to 70 % of the first (+1.4 % over three
   * tapers, profiles/r05_ab_block_taper.txt; without horizons equal blocks are as good). */
  const std::vector<rsu::Shard> shards =
      rsu::make_shards(in->n_points, rsu::device_list(), in->horizons ? 30 : RS_BLOCK_TAPER_PCT_DEFAULT);
  if (gridded) {
    std::vector<int> devices;
    for (const rsu::Shard &sh : shards) devices.push_back(sh.device);
    if (int rc = upload_grids(in, grids, devices, G)) return rc;
  }
  return rsu::fan_out(shards, [&](const rsu::Shard &sh, int) {
    const GridView v{grids, G.find(sh.device)};
    return driver_run_range(in, st, params, local, out, q, sh.device, sh.off, sh.off + sh.cnt, gridded ? &v : nullptr);
  });
}

/* ---- the ensemble form (include/roadsurf.h, rs_driver_run_ensemble; the host rules: rs_driver_ens.hpp) */

/* the decisions report_finish writes, of the points [p0, p0 + m), from one array into another */
void copy_decisions(LocalParameters *dst, const LocalParameters *src, int64_t p0, int m) {
  for (int64_t p = p0; p < p0 + m; ++p) dst[p] = src[p];
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int driver_run_ensemble(const RsDriverInput *in, const RsGridSource *const *grids, const InputSettings *st,
                        const InputParameters *params, LocalParameters *local, const RsDriverOutput *out,
                        RsDriverEnsemble *ens, int32_t device) {
  char b[400];
  if (!in || !st || !ens || !in->sources || in->n_points < 1 || in->n_sources < 1)
    return fail_msg("rs_driver_run_ensemble: bad arguments (the stations' input, settings and the ensemble struct are required)", -1);
  if (device < 0)
    return fail_msg("rs_driver_run_ensemble: device < 0: the ensemble form has no fan-out over the device list", -1);
  const int nsh = in->n_sources, S = in->n_points, nmem = ens->n_members;
  if (nsh + 1 > RS_MAX_SOURCES) {
    snprintf(b, sizeof(b), "rs_driver_run_ensemble: %d shared sources and the member source are more than RS_MAX_SOURCES = %d", nsh,
             RS_MAX_SOURCES);
    return fail_msg(b, -1);
  }
  if (ens->position < 0 || ens->position > nsh) {
    snprintf(b, sizeof(b), "rs_driver_run_ensemble: position = %d outside [0, n_sources = %d]", (int)ens->position, nsh);
    return fail_msg(b, -1);
  }
  const RsRawSource &msrc = ens->member;
  if (msrc.times_per_point || msrc.lengths)
    return fail_msg("rs_driver_run_ensemble: the member source needs a time axis shared by all members (times_per_point = 0, lengths NULL)", -1);
  if (msrc.is_observation)
    return fail_msg("rs_driver_run_ensemble: the member source must not be an observation source (is_observation = 0): the "
                    "relaxation index would be a member's own", -1);
  if (msrc.tsurfobs)
    return fail_msg("rs_driver_run_ensemble: the member source must carry no tsurfobs: the coupling decisions would be a member's own", -1);
  if (msrc.n_times < 1 || !msrc.times)
    return fail_msg("rs_driver_run_ensemble: the member source needs a time axis (n_times >= 1): the branch follows from times[0]", -1);
  Common chk; /* (SimLen, DTSecs and the shared sources' axes; the call's own Common follows the grids' upload) */
  if (int rc = prepare(in, st, chk)) return rc;
  const int L = chk.L;
  const int step0 = (int)((double)(st->outputStep * 60) / st->DTSecs);
  if (step0 < 1) return fail_msg("rs_driver_run: outputStep*60/DTSecs < 1", -1);
  int32_t B = 0, first_row = 0;
  if (rs_dens::branch(in->start_time, chk.DT, L, step0, msrc.times[0], &B, &first_row, b, sizeof(b)) != 0) return fail_msg(b, -1);
  ens->branch_index = B;
  ens->first_row = first_row;
  std::vector<int32_t> starts;
  if (rs_dens::check_parent(nmem, ens->parent, S, starts, b, sizeof(b)) != 0) return fail_msg(b, -1);
  const bool gridded = any_grid(in, grids);
  if (gridded)
    if (int rc = check_grids(in, grids)) return rc;

  /* the members' input: the shared sources' axes (their rows come from the stations' tile), the member source in its place */
  RsRawSource msources[RS_MAX_SOURCES];
  ParentFill pf{};
  for (int s = 0, k = 0; s <= nsh; ++s) {
    if (s == ens->position) {
      msources[s] = msrc;
      pf.src_of[s] = -1;
    } else {
      msources[s] = in->sources[k];
      msources[s].lengths = nullptr; /* (the stations': copied on the device) */
      pf.src_of[s] = k++;
    }
  }
  for (int s = nsh + 1; s < RS_MAX_SOURCES; ++s) pf.src_of[s] = -1;
  RsDriverInput min = *in;
  min.n_points = nmem;
  min.n_sources = nsh + 1;
  min.sources = msources;
  min.horizons = nullptr; /* (the stations' table, read through parent) */
  Common cM;
  if (int rc = prepare(&min, st, cM)) return rc;
  /* private decisions: what a tile steps with, and what reaches the caller once the tile's checks have passed */
  if (!local) return fail_msg("rs_driver_run: params, local and out are required", -1);
  std::vector<LocalParameters> slocal(local, local + S), rlocal(local, local + S), mlocal((size_t)nmem), mlocal0;
  for (int q = 0; q < nmem; ++q) mlocal[q] = local[ens->parent[q]];
  mlocal0 = mlocal;
  std::vector<int32_t> sstatus(S), smi(S), rstatus(S), rmi(S), mstatus(nmem), mmi(nmem);
  RunPolicy RS, RM;
  RsConstants consts;
  if (int rc = check_run_arguments(in, st, params, slocal.data(), out, chk, RS, consts)) return rc;
  RM.step = RS.step;
  RM.n_out = RS.n_out;
  const int n_tail = RS.n_out - first_row;
  if (ens->member_out.n_out != n_tail) {
    snprintf(b, sizeof(b), "rs_driver_run_ensemble: member_out.n_out must be n_out - first_row = %d (B = %d, first_row = %d)", n_tail,
             (int)B, (int)first_row);
    return fail_msg(b, -1);
  }
  if (ens->stats_spec) {
    const RsEnsSpec &sp = *ens->stats_spec;
    if (rs_ens::cols(&sp) < 0 || !ens->stats || sp.ngroups != S) {
      snprintf(b, sizeof(b), "rs_driver_run_ensemble: stats: a good spec with ngroups = n_stations = %d and the stats array are required", S);
      return fail_msg(b, -1);
    }
    std::vector<int32_t> table((size_t)S + 1 + nmem);
    if (rs_ens::member_table(nmem, ens->parent, &sp, table.data(), b, sizeof(b)) != 0) return fail_msg(b, -1);
  }
  if (ens->probs_spec) {
    const RsProbSpec &sp = *ens->probs_spec;
    if (rs_cluster_prob_cols(&sp) < 0 || !ens->probs || sp.ngroups != S) {
      snprintf(b, sizeof(b), "rs_driver_run_ensemble: probs: a good spec with ngroups = n_stations = %d and the probs array are required", S);
      return fail_msg(b, -1);
    }
    if (rs_cluster_prob_needs_deficit(&sp) == 1)
      return fail_msg("rs_driver_run_ensemble: probs: a condition uses the deficit, and the call has no deficit rows for the members", -1);
    RsEnsSpec ts;
    std::memset(&ts, 0, sizeof(ts));
    ts.ngroups = S;
    ts.max_members = sp.max_members;
    std::vector<int32_t> table((size_t)S + 1 + nmem);
    if (rs_ens::member_table(nmem, ens->parent, &ts, table.data(), b, sizeof(b)) != 0) return fail_msg(b, -1);
  }
  make_run_policy(st, consts, chk, slocal.data(), 0, S, RS);
  make_run_policy(st, consts, cM, mlocal.data(), 0, nmem, RM);
  if (RS.coupled && !RS.cpl_chunked)
    return fail_msg("rs_driver_run_ensemble: coupling over the whole series (ROADSURF_HIP_CPL_WHOLE) cannot stop at the branch", -1);
  if (const int32_t crowded = rs_dens::first_crowded(starts, RM.P); crowded >= 0) {
    snprintf(b, sizeof(b), "rs_driver_run_ensemble: station %d has %d members, more than a tile of %d points holds", (int)crowded,
             (int)(starts[crowded + 1] - starts[crowded]), RM.P);
    return fail_msg(b, -1);
  }

  /* ---- device work from here on */
  if (int rc = check_device(device)) return rc;
  HOK(hipSetDevice(device));
  GridUploads G; /* (declared before the stream: freed when it is gone) */
  GridView gv{grids, nullptr};
  if (gridded) {
    if (int rc = upload_grids(in, grids, std::vector<int>{device}, G)) return rc;
    gv.dev = G.find(device);
  }
  Common cS;
  if (int rc = prepare(in, st, cS, gridded ? &gv : nullptr)) return rc;
  StreamGuard sg;
  HOK(hipStreamCreate(&sg.s));
  const hipStream_t stream = sg.s;
  const Call callS{in, st, cS, consts, device, stream, slocal.data(), sstatus.data(), smi.data()};
  const Call callM{&min, st, cM, consts, device, stream, mlocal.data(), mstatus.data(), mmi.data()};
  WindowLease arena_lease; /* (declared behind the stream guard: WindowLease::release) */
  arena_lease.stream = stream;
  arena_lease.cache = g_arenacache;
  rsu::Arena arena;
  const size_t arena_bytes = arena_estimate(in, cS, RS) + arena_estimate(&min, cM, RM);
  if (arena_lease.acquire(arena_bytes, device) == hipSuccess) {
    arena.base = static_cast<char *>(arena_lease.p);
    arena.cap = arena_bytes;
  }
  ArenaScope arena_scope(arena.base ? &arena : nullptr);
  SharedAxes axS, axM;
  if (int rc = upload_shared_axes(callS, RS, 0, S, axS)) return rc;
  if (int rc = upload_shared_axes(callM, RM, 0, nmem, axM)) return rc;
  PhaseTimer pt(stream, RS.timing);
  pt.lap(0);
  WindowLease winS, winM;
  winS.stream = winM.stream = stream;
  const RsDriverRequest none{};
  const double tbottom = rs_bottom_temperature(params, &consts, in->year[0], in->month[0], in->day[0]);
  Run runS{callS, params, out, RS, 0, S, tbottom, axS, pt, winS, 0, none, nullptr};
  Run runM{callM, params, &ens->member_out, RM, 0, nmem, tbottom, axM, pt, winM, 0, none, nullptr};
  pt.lap(6);

  double copy_ms = 0.0, fanout_ms = 0.0;
  pf.copy_ms = RS.timing ? &copy_ms : nullptr;
  int64_t Scap = RS.P;
  g_last_tiles = 0;
  g_last_raw_launches = 0;
  const size_t arena_mark = arena.off;
  for (int32_t s0 = 0; s0 < S;) {
    arena.rewind(arena_mark);
    const int ms = rs_dens::tile_stations(starts, s0, Scap, RM.P);
    if (ms < 1) return fail_msg("rs_driver_run_ensemble: a station's members do not fit a tile", -1); /* (first_crowded has passed) */
    const int64_t q0 = starts[s0];
    const int mm = starts[(size_t)s0 + ms] - starts[s0];
    /* the stations: an ordinary tile, its decisions at once */
    Tile XS(runS, s0, ms);
    copy_decisions(slocal.data(), local, s0, ms);
    if (int rc = tile_prologue(runS, s0, ms, RS.skyview && in->horizons, true, pt, XS)) return rc;
    copy_decisions(rlocal.data(), slocal.data(), s0, ms);
    bool behind = false; /* some station is rejected by a hole at or behind the branch alone */
    for (int p = s0; p < s0 + ms; ++p) {
      rstatus[p] = sstatus[p];
      rmi[p] = smi[p];
      behind = behind || (sstatus[p] >= 1 && sstatus[p] <= 6 && smi[p] >= B);
    }
    if (behind) { /* ... and steps, with the decisions of the series before the branch: its members may be accepted */
      HOK(XS.d_status_rep.alloc(XS.mp * sizeof(int32_t)));
      HOK(hipMemcpyAsync(XS.d_status_rep.p, XS.D.status.p, XS.mp * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
      if (int rc = finalize_tile(cS, st, XS.T, XS.D, B, stream)) return rc;
      copy_decisions(slocal.data(), local, s0, ms);
      if (int rc = report_issue(XS.D, s0, ms, XS.rep, stream)) return rc;
      if (int rc = report_finish(cS, st, XS.rep, slocal.data(), sstatus.data(), smi.data())) return rc;
    }
    if (RS.coupled)
      for (int p = s0; p < s0 + ms; ++p) {
        const LocalParameters &l = slocal[p];
        const bool on = sstatus[p] == 0 && !(l.couplingTsurf < -100 || l.couplingIndexI < 1);
        if (on && l.couplingIndexI + 1 > B) {
          snprintf(b, sizeof(b), "rs_driver_run_ensemble: station %d: couplingIndexI + 1 = %d > B = %d: a coupling replay reads the "
                                 "index behind its window, which must be shared", p, l.couplingIndexI + 1, (int)B);
          return fail_msg(b, -1);
        }
      }
    if (int rc = XS.point_params()) return rc;
    XS.tp = make_tile_policy(RS, cS, st, slocal.data(), s0, ms, XS.mp, XS.T.any_pp);
    if (XS.tp.halve_to) { /* started again at the same station */
      Scap = XS.tp.halve_to;
      continue;
    }
    /* the members: a second tile, a second plan */
    Tile XM(runM, q0, std::max(mm, 1));
    Dev d_parent;
    std::vector<int32_t> parent_local((size_t)std::max(mm, 1));
    if (mm > 0) {
      for (int q = 0; q < mm; ++q) parent_local[q] = ens->parent[q0 + q] - s0;
      HOK(d_parent.alloc((size_t)mm * sizeof(int32_t)));
      HOK(hipMemcpyAsync(d_parent.p, parent_local.data(), (size_t)mm * sizeof(int32_t), hipMemcpyHostToDevice, stream));
      pf.T = &XS.T;
      pf.parent = d_parent.as<int32_t>();
      copy_decisions(mlocal.data(), mlocal0.data(), q0, mm);
      if (int rc = tile_prologue(runM, q0, mm, false, true, pt, XM, &pf)) return rc;
      /* the sharing argument, held to the decisions themselves */
      for (int q = (int)q0; q < q0 + mm; ++q) {
        if (mstatus[q] != 0) continue;
        const int p = ens->parent[q];
        const LocalParameters &a = mlocal[q], &l = slocal[p];
        const char *what = nullptr;
        if (sstatus[p] != 0) what = "status";
        else if (a.InitLenI != l.InitLenI) what = "InitLenI";
        else if (RS.coupled && a.couplingIndexI != l.couplingIndexI) what = "couplingIndexI";
        else if (RS.coupled && !same_bits(a.couplingTsurf, l.couplingTsurf)) what = "couplingTsurf";
        else if (st->use_relaxation == 1 && l.InitLenI < B &&
                 !(same_bits(a.tair_relax, l.tair_relax) && same_bits(a.VZ_relax, l.VZ_relax) && same_bits(a.RH_relax, l.RH_relax)))
          what = "relaxation targets (with InitLenI < B)";
        if (what) {
          snprintf(b, sizeof(b), "rs_driver_run_ensemble: member %d differs from its station %d in %s: the analysis would not be shared "
                                 "(B = %d)", q, p, what, (int)B);
          return fail_msg(b, -1);
        }
      }
      if (RM.skyview && in->horizons && XS.d_hzpt.p) {
        XM.hz_table = XS.d_hzpt.as<double>();
        XM.hz_col = d_parent.as<int32_t>();
      }
      if (int rc = XM.point_params()) return rc;
      XM.tp = make_tile_policy(RM, cM, st, mlocal.data(), q0, mm, XM.mp, XM.T.any_pp, true);
    }
    /* the tile's checks have passed: its decisions reach the caller */
    for (int p = s0; p < s0 + ms; ++p) {
      local[p] = rlocal[p];
      if (out->status) out->status[p] = rstatus[p];
      if (out->missing_index) out->missing_index[p] = rmi[p];
    }
    for (int64_t q = q0; q < q0 + mm; ++q) {
      if (ens->member_local) ens->member_local[q] = mlocal[q];
      if (ens->member_out.status) ens->member_out.status[q] = mstatus[q];
      if (ens->member_out.missing_index) ens->member_out.missing_index[q] = mmi[q];
    }
    if (int rc = XS.buffers()) return rc;
    if (mm > 0)
      if (int rc = XM.buffers()) return rc;
    pt.lap(3);
    /* the stations' leg: [1, B] */
    if (rs_hip_set_history_score(XS.pg.p, (XS.tp.cluster && XS.tp.forecast_key && !RS.cpl_chunked) ? 0 : 1) != 0) return -14;
    if (int rc = RS.cpl_chunked ? XS.loop_cpl_chunked(B) : RS.use_raw ? XS.loop_raw(1, B) : XS.loop_windows(1, B)) return rc;
    XS.d_row1.release();
    if (RS.cpl_chunked && rs_hip_coupling_windows_closed(XS.pg.p, 1) != 0) return -14;
    if (mm > 0) {
      /* the members' leg: the stations' carried state, then [B + 1, SimLen] */
      if (RS.timing) HOK(hipStreamSynchronize(stream));
      const double tf0 = PhaseTimer::now();
      if (rs_hip_state_fanout(XM.pg.p, XS.pg.p, parent_local.data()) != 0) return -15;
      if (RS.timing) {
        HOK(hipStreamSynchronize(stream));
        fanout_ms += 1e3 * (PhaseTimer::now() - tf0);
      }
      if (rs_hip_set_history_score(XM.pg.p, (XM.tp.cluster && XM.tp.forecast_key && !RM.cpl_chunked) ? 0 : 1) != 0) return -14;
      if (int rc = RM.cpl_chunked ? XM.loop_lockstep(B + 1) : RM.use_raw ? XM.loop_raw(B + 1, L) : XM.loop_windows(B + 1, L))
        return rc;
    }
    pt.lap(4);
    if (int rc = XS.outputs_home()) return rc;
    if (mm > 0) {
      if (int rc = XM.members_home(*ens, first_row, parent_local.data(), s0, ms, S)) return rc;
    } else if (n_tail > 0) { /* stations without a member: the empty cells */
      for (int r = 0; r < n_tail; ++r)
        for (int p = s0; p < s0 + ms; ++p) {
          if (ens->stats_spec) {
            const int cols = rs_ens::cols(ens->stats_spec);
            double *cell = ens->stats + ((size_t)r * S + p) * cols;
            for (int k = 0; k < cols; ++k) cell[k] = k < 2 ? 0.0 : -9999.0;
          }
          if (ens->probs_spec) {
            const int cols = rs_cluster_prob_cols(ens->probs_spec);
            double *cell = ens->probs + ((size_t)r * S + p) * cols;
            for (int k = 0; k < cols; ++k) cell[k] = 0.0;
          }
        }
    }
    s0 += ms;
    ++g_last_tiles;
    Scap = RS.P;
  }
  if (RS.timing)
    fprintf(stderr, "rs_driver_run_ensemble: B = %d, first_row = %d, %d tiles: column copies %.3f ms, fan-outs %.3f ms\n", (int)B,
            (int)first_row, g_last_tiles, copy_ms, fanout_ms);
  pt.report();
  return 0;
}

}  // namespace

extern "C" {

int64_t rs_driver_ensemble_bytes(void) { return (int64_t)sizeof(RsDriverEnsemble); }

int rs_driver_run_ensemble(const RsDriverInput *in, const RsGridSource *const *grids, const InputSettings *st,
                           const InputParameters *params, LocalParameters *local, const RsDriverOutput *out,
                           RsDriverEnsemble *ens, int32_t device) {
  return driver_run_ensemble(in, grids, st, params, local, out, ens, device);
}

int rs_driver_expand(const RsDriverInput *in, const InputSettings *st, LocalParameters *local,
                     double *merged, int32_t *status, int32_t *missing_index, int32_t device) {
  return driver_expand(in, nullptr, st, local, merged, status, missing_index, device);
}

int rs_driver_expand_grid(const RsDriverInput *in, const RsGridSource *const *grids, const InputSettings *st,
                          LocalParameters *local, double *merged, int32_t *status, int32_t *missing_index,
                          int32_t device) {
  return driver_expand(in, grids, st, local, merged, status, missing_index, device);
}

void rs_driver_release_cache(void) {
  for (int d = 0; d < 128; ++d) {
    WindowCache &c = d < 64 ? g_wincache[d] : g_arenacache[d - 64];
    std::lock_guard<std::mutex> lk(c.m);
    for (int k = 0; k < WINCACHE_SLOTS; ++k) {
      if (c.busy[k] || !c.p[k]) continue;
      if (hipSetDevice(d & 63) != hipSuccess) break;
      (void)hipFree(c.p[k]);
      c.p[k] = nullptr;
      c.bytes[k] = 0;
    }
  }
}

int rs_driver_last_tiles(void) { return g_last_tiles; }
int rs_driver_last_raw_launches(void) { return g_last_raw_launches; }

/* device >= 0: that device.  device < 0: the points are cut into contiguous blocks over the
 * device list (rs_devices.hpp: ROADSURF_HIP_DEVICES, default every visible device), one host
 * thread + stream + plans per device, no collective - the in-process counterpart of the
 * reference driver's worker pool (examples/example1/src/roadrunner.cpp:423-501).  What a request adds to it:
 *   summary   every block fills its points' rows of the one host array
 *   groups    every block reduces its points into cells of its own on its device, and merges them into the caller's
 *             array when its last tile is home
 *   grids     the calling thread checks them and puts their fields on every device of the call before the blocks start
 *   kept      every tile makes them from its raw columns behind its time loop, every block fills its points' rows of the
 *             host arrays
 *   episodes  every tile feeds its result block's rows - and the deficit, where the spec uses it - to its points'
 *             automata, every block fills its points' rows of the one host array */
int rs_driver_run_request(const RsDriverInput *in, const InputSettings *st, const InputParameters *params,
                          LocalParameters *local, const RsDriverOutput *out, const RsDriverRequest *request,
                          int32_t device) {
  return driver_run(in, st, params, local, out, request ? *request : RsDriverRequest{}, device);
}

/* the older entries: the request each of them can express */
int rs_driver_run(const RsDriverInput *in, const InputSettings *st, const InputParameters *params,
                  LocalParameters *local, const RsDriverOutput *out, int32_t device) {
  return driver_run(in, st, params, local, out, RsDriverRequest{}, device);
}
int rs_driver_run_summary(const RsDriverInput *in, const InputSettings *st, const InputParameters *params,
                          LocalParameters *local, const RsDriverOutput *out, const RsDriverSummary *sum,
                          int32_t device) {
  return driver_run(in, st, params, local, out, RsDriverRequest{nullptr, sum}, device);
}
int rs_driver_run_groups(const RsDriverInput *in, const InputSettings *st, const InputParameters *params,
                         LocalParameters *local, const RsDriverOutput *out, const RsDriverSummary *sum,
                         const RsDriverGroups *grp, int32_t device) {
  return driver_run(in, st, params, local, out, RsDriverRequest{nullptr, sum, grp}, device);
}
int rs_driver_run_grid(const RsDriverInput *in, const RsGridSource *const *grids, const InputSettings *st,
                       const InputParameters *params, LocalParameters *local, const RsDriverOutput *out,
                       const RsDriverSummary *sum, const RsDriverGroups *grp, int32_t device) {
  return driver_run(in, st, params, local, out, RsDriverRequest{grids, sum, grp}, device);
}
int32_t rs_driver_kept_fields(void) { return NFLD; }
int rs_driver_run_kept(const RsDriverInput *in, const RsGridSource *const *grids, const InputSettings *st,
                       const InputParameters *params, LocalParameters *local, const RsDriverOutput *out,
                       const RsDriverSummary *sum, const RsDriverGroups *grp, const RsDriverKept *kept, int32_t device) {
  return driver_run(in, st, params, local, out, RsDriverRequest{grids, sum, grp, kept}, device);
}
int rs_driver_run_episodes(const RsDriverInput *in, const RsGridSource *const *grids, const InputSettings *st,
                           const InputParameters *params, LocalParameters *local, const RsDriverOutput *out,
                           const RsDriverSummary *sum, const RsDriverGroups *grp, const RsDriverKept *kept,
                           const RsDriverEpisodes *epi, int32_t device) {
  return driver_run(in, st, params, local, out, RsDriverRequest{grids, sum, grp, kept, epi}, device);
}

} /* extern "C" */
