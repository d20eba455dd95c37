/*
 * rs_cluster.hip — plan order (include/roadsurf.h, rs_hip_recluster): sort the slots of a plan
 * by the boundary-layer passes their points needed during the last launch and move the carried
 * state along.  Device-wide radix sort from hipCUB; everything else is streaming copies.
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "rs_ens_table.hpp"
#include "rs_group_rule.hpp"
#include "rs_kernels.h"
#include "rs_period_rule.hpp"
#include "rs_state.h"

namespace {

constexpr int KEY_BITS = RS_SORT_KEY_BITS; /* rs_kernels.hip, bl_score_key: 19 bits of passes + regime + cover */

template <typename T> /* element type of the state block: double, or float for fp32 plans */
__global__ void __launch_bounds__(RS_BLOCK) keys_kernel(const T *__restrict__ state,
                                                        int64_t np_pad, int64_t npoints,
                                                        uint32_t *keys, uint32_t *slots) {
  const int64_t s = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (s >= npoints) return;
  double v = (double)state[(int64_t)RS_ST_BLSCORE * np_pad + s];
  if (!(v >= 0.0)) v = 0.0;
  const double top = (double)((1u << KEY_BITS) - 1u);
  /* descending: the expensive points get the low slots, so their workgroups are dispatched
   * first and the cheap ones fill the end of the grid (longest job first) */
  keys[s] = (uint32_t)top - (uint32_t)(v > top ? top : v);
  slots[s] = (uint32_t)s;
}

/* Which state rows a re-sort has to move (rs_state.h).  blockIdx.y counts the rows in use:
 * the profile Tmp(1..NLayers), the scalars TmpNw(1)..BLSCORE, then - with coupling - the coupling
 * scalars ITER..RESUME, and while coupling windows are still open also the saved state of
 * saveDataForCoupling (6 scalars, TmpSave(1..NLayers)) and the stale TmpNw profile. */
struct RowMap {
  int32_t nlayers, nscal, ncpl, nsave; /* rows of each group; nsave counts the 6 scalars only */
  __host__ __device__ int32_t total() const {
    return nlayers + nscal + ncpl + nsave + (nsave ? 2 * nlayers : 0);
  }
  __device__ int64_t row(int32_t y) const {
    if (y < nlayers) return y;
    y -= nlayers;
    if (y < nscal) return RS_ST_TNW1 + y;
    y -= nscal;
    if (y < ncpl) return RS_ST_CPL_ITER + y;
    y -= ncpl;
    if (y < nsave) return RS_ST_CPL_SAVE_TSURF + y;
    y -= nsave;
    if (y < nlayers) return RS_ST_CPL_SAVE_TMP0 + y;
    return RS_ST_CPL_STALE_TMP0 + (y - nlayers);
  }
};

/* dst[row][s] = src[row][perm[s]] for the carried state, order_dst[s] = order_src[perm[s]];
 * slots beyond npoints (padding) stay where they are */
template <typename T>
__global__ void __launch_bounds__(RS_BLOCK) apply_kernel(const T *__restrict__ src,
                                                         T *__restrict__ dst,
                                                         const int32_t *__restrict__ order_src,
                                                         int32_t *__restrict__ order_dst,
                                                         const uint32_t *__restrict__ perm,
                                                         int64_t np_pad, int64_t npoints,
                                                         const RowMap rows) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a plan: little work, all of it waited for */
  const int64_t s = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (s >= np_pad) return;
  const int64_t from = (s < npoints) ? (int64_t)perm[s] : s;
  if (blockIdx.y == 0) order_dst[s] = order_src[from];
  const int64_t row = rows.row((int32_t)blockIdx.y);
  dst[row * np_pad + s] = src[row * np_pad + from];
}

/* inv[order[s]] = s: where every point of a re-sorted plan sits (rs_hip_state_fanout) */
__global__ void __launch_bounds__(RS_BLOCK) inverse_kernel(const int32_t *__restrict__ order, int64_t npoints,
                                                           int32_t *__restrict__ inv) {
  const int64_t s = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (s >= npoints) return;
  const int64_t p = order[s];
  if (p >= 0 && p < npoints) inv[p] = (int32_t)s;
}

/* The carried state of another plan's points (rs_hip_state_fanout): dst[row][s] = src[row][slot of parent[point of s]]
 * for the slots s < npoints of dst and the rows of `rows`.  One lane per dst slot, one grid row per state row: the
 * stores are coalesced, the loads gathers - a broadcast within the wavefront where the members of a station sit side
 * by side.  order_dst NULL: slot s holds point s; inv_src NULL: point q sits in slot q.  parent was checked on the
 * host; an index that is no point of its plan (an order row of the caller's making) writes nothing.  Columns beyond
 * dst's npoints and everything of src stay as they are. */
template <typename T>
__global__ void __launch_bounds__(RS_BLOCK) fanout_kernel(const T *__restrict__ src, T *__restrict__ dst,
                                                          const int32_t *__restrict__ order_dst,
                                                          const int32_t *__restrict__ parent,
                                                          const int32_t *__restrict__ inv_src, int64_t np_pad_src,
                                                          int64_t npoints_src, int64_t np_pad_dst, int64_t npoints_dst,
                                                          const RowMap rows) {
  const int64_t s = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (s >= npoints_dst) return;
  const int64_t p = order_dst ? (int64_t)order_dst[s] : s;
  if (p < 0 || p >= npoints_dst) return;
  const int64_t q = parent[p];
  if (q < 0 || q >= npoints_src) return;
  const int64_t from = inv_src ? (int64_t)inv_src[q] : q;
  if (from < 0 || from >= npoints_src) return;
  const int64_t row = rows.row((int32_t)blockIdx.y);
  dst[row * np_pad_dst + s] = src[row * np_pad_src + from];
}

__global__ void __launch_bounds__(RS_BLOCK) iota_kernel(int32_t *x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (i < n) x[i] = (int32_t)i;
}

inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + RS_BLOCK - 1) / RS_BLOCK)); }

}  // namespace

/* The output rows of a launch, [row][slot] per stream, into POINT-MAJOR arrays [point][row] - what a consumer
 * that owns one series per point wants (SaveOutput writes a point's arrays, src/InputOutput.f90:151-165;
 * OutputData.cpp:5-13).  One wavefront per 64 slots and stream: a tile of up to 32 rows is read row by row
 * (coalesced, 512 B each) into LDS, then written point by point - a point's rows of the tile are contiguous in
 * its series, so every store instruction fills whole lines.  (Scattering single values into [row][point] arrays
 * instead would ask the memory for eight times the bytes.) */
struct ByPointArgs {
  const double *src[6];
  double *dst[6];
  const int32_t *order;
  int64_t npoints, src_stride, dst_rows, dst_row0;
  int32_t nrows;
};
__global__ void __launch_bounds__(64) outputs_by_point_kernel(const ByPointArgs a) {
  __shared__ double tile[32][65]; /* 16.6 KB: nine wavefronts to a CU keep enough loads in flight */
  __shared__ int32_t pt[64];
  const int lane = threadIdx.x;
  const int64_t s0 = (int64_t)blockIdx.x * 64;
  const double *src = a.src[blockIdx.y];
  double *dst = a.dst[blockIdx.y];
  const int64_t s = s0 + lane;
  pt[lane] = s < a.npoints ? a.order[s] : -1;
  const int rr = lane & 31, half = lane >> 5;
  for (int32_t r0 = 0; r0 < a.nrows; r0 += 32) {
    const int32_t nr = a.nrows - r0 < 32 ? a.nrows - r0 : 32;
    __syncthreads();
    if (s < a.npoints)
      for (int32_t r = 0; r < nr; ++r) tile[r][lane] = src[(int64_t)(r0 + r) * a.src_stride + s];
    __syncthreads();
    for (int jj = 0; jj < 32; ++jj) { /* two points per instruction: 32 rows = 256 B of each one's series */
      const int j = 2 * jj + half;
      const int32_t p = pt[j];
      if (p >= 0 && rr < nr) dst[(int64_t)p * a.dst_rows + a.dst_row0 + r0 + rr] = tile[rr][j];
    }
  }
}
hipError_t rs_cluster_outputs_by_point(const double *const src[6], double *const dst[6], const int32_t *order,
                                       int64_t npoints, int64_t src_stride, int32_t nrows, int64_t dst_rows,
                                       int64_t dst_row0, hipStream_t stream) {
  ByPointArgs a;
  for (int f = 0; f < 6; ++f) {
    a.src[f] = src[f];
    a.dst[f] = dst[f];
  }
  a.order = order;
  a.npoints = npoints;
  a.src_stride = src_stride;
  a.dst_rows = dst_rows;
  a.dst_row0 = dst_row0;
  a.nrows = nrows;
  /* (a variant without LDS - every lane carrying its slot's values into its point's series, the L2 merging eight
   * rows to a line - was slower: 438 against 388 ms per pass at 1 M points) */
  hipLaunchKernelGGL(outputs_by_point_kernel, dim3((unsigned)((npoints + 63) / 64), 6), dim3(64), 0, stream, a);
  return hipGetLastError();
}

/* Per-point summaries of the output rows (include/roadsurf.h, rs_hip_outputs_summary; the definition is
 * roadsurf_amd/summary.py, reduce_series): a sibling of outputs_by_point_kernel that reads the same [row][slot] windows
 * and keeps RS_SUM_COLS numbers per point instead of the series.  One lane owns a slot and carries its summary in
 * registers over the rows, every row load a coalesced 512 B per wavefront and stream (256 B of an fp32 window),
 * SUM_ROWS rows of all six streams in flight per lane.  The four wavefronts of a workgroup share 64 slots and take a
 * quarter of the rows each - a batch of a few hundred points is a handful of workgroups, and the rows are what
 * there is to spread - then merge through LDS with the rule that also merges across calls (Sum::merge), and the
 * first wavefront ends with one read-merge-write of its points' accumulator columns.  A point sits in one slot:
 * plain loads and stores, no atomics. */
namespace {
constexpr int SUM_WAVES = 4, SUM_ROWS = 4;

struct Sum {
  double v[RS_SUM_COLS]; /* the columns of include/roadsurf.h: everything fp64, indices and counts are exact there */
  __device__ void clear() {
#pragma unroll
    for (int c = 0; c < RS_SUM_COLS; ++c) v[c] = 0.0;
    v[1] = __builtin_huge_val();
    v[3] = -__builtin_huge_val();
#pragma unroll
    for (int k = 0; k < 5; ++k) v[7 + k] = -__builtin_huge_val();
  }
  /* extremes tie to the smaller index; a NaN, and the empty value itself, never wins (every comparison false) */
  __device__ void lower(double t, double i) {
    if (t < v[1] || (t == v[1] && i < v[2])) { v[1] = t; v[2] = i; }
  }
  __device__ void higher(double t, double i) {
    if (t > v[3] || (t == v[3] && i < v[4])) { v[3] = t; v[4] = i; }
  }
  __device__ void first(double i) { /* i > 0 */
    if (v[5] == 0.0 || i < v[5]) v[5] = i;
  }
  /* one row of the point: its time index, Tsurf and the five storages */
  __device__ void row(double i, double t, const double s[5], const RsSummarySpec &sp) {
    if (t == -9999.0) return; /* never saved: behind the last index of a failed point, or a rejected point */
    v[0] += 1.0;
    lower(t, i);
    higher(t, i);
    if (t < sp.tsurf_below) {
      first(i);
      v[6] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      if (s[k] > v[7 + k]) v[7 + k] = s[k];
      if (s[k] > sp.storage_above[k]) v[12 + k] += 1.0;
    }
  }
  /* the summary of this one's rows and o's together (disjoint rows) */
  __device__ void merge(const Sum &o) {
    v[0] += o.v[0];
    lower(o.v[1], o.v[2]);
    higher(o.v[3], o.v[4]);
    if (o.v[5] != 0.0) first(o.v[5]);
    v[6] += o.v[6];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      if (o.v[7 + k] > v[7 + k]) v[7 + k] = o.v[7 + k];
      v[12 + k] += o.v[12 + k];
    }
  }
  __device__ void load(const double *p, int64_t stride) {
#pragma unroll
    for (int c = 0; c < RS_SUM_COLS; ++c) v[c] = p[c * stride];
  }
  __device__ void store(double *p, int64_t stride) const {
#pragma unroll
    for (int c = 0; c < RS_SUM_COLS; ++c) p[c * stride] = v[c];
  }
};

struct SummaryArgs {
  const void *src[6]; /* T[nrows][stride] each: Tsurf, Snow, Water, Ice, Deposit, Ice2 */
  const int32_t *order; /* column s is point order[s]; NULL: point s (rs_driver_run's result block) */
  double *acc;          /* [RS_SUM_COLS][np_pad], point order */
  int64_t npoints, stride, np_pad;
  int32_t nrows, index0, index_step;
  RsSummarySpec spec;
};

template <typename T>
__global__ void __launch_bounds__(64 * SUM_WAVES) outputs_summary_kernel(const SummaryArgs a) {
  __shared__ double part[SUM_WAVES - 1][RS_SUM_COLS][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * 64 + lane;
  const bool live = s < a.npoints;
  Sum sum;
  sum.clear();
  const int32_t per = (a.nrows + SUM_WAVES - 1) / SUM_WAVES, r_lo = wave * per,
                r_hi = a.nrows < r_lo + per ? a.nrows : r_lo + per;
  if (live)
#pragma unroll 1
    for (int32_t r0 = r_lo; r0 < r_hi; r0 += SUM_ROWS) {
      T x[SUM_ROWS][6];
#pragma unroll
      for (int q = 0; q < SUM_ROWS; ++q) {
        const int32_t r = r0 + q < r_hi ? r0 + q : r_hi - 1; /* behind the range: its last row again, not taken */
#pragma unroll
        for (int f = 0; f < 6; ++f) x[q][f] = static_cast<const T *>(a.src[f])[(int64_t)r * a.stride + s];
      }
#pragma unroll
      for (int q = 0; q < SUM_ROWS; ++q) {
        if (r0 + q >= r_hi) break;
        const double st[5] = {(double)x[q][1], (double)x[q][2], (double)x[q][3], (double)x[q][4], (double)x[q][5]};
        sum.row((double)a.index0 + (double)(r0 + q) * (double)a.index_step, (double)x[q][0], st, a.spec);
      }
    }
  if (wave > 0) sum.store(&part[wave - 1][0][lane], 64);
  __syncthreads();
  if (wave > 0 || !live) return;
#pragma unroll 1
  for (int w = 0; w < SUM_WAVES - 1; ++w) {
    Sum o;
    o.load(&part[w][0][lane], 64);
    sum.merge(o);
  }
  const int64_t p = a.order ? (int64_t)a.order[s] : s;
  if (p < 0 || p >= a.npoints) return; /* not an order row of this plan: nothing is written */
  Sum g;
  g.load(a.acc + p, a.np_pad);
  g.merge(sum);
  g.store(a.acc + p, a.np_pad);
}

__global__ void __launch_bounds__(RS_BLOCK) summary_reset_kernel(double *acc, int64_t np_pad) {
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= np_pad) return;
  Sum e;
  e.clear();
  e.store(acc + p, np_pad);
}
}  // namespace

hipError_t rs_cluster_summary_reset(double *acc, int64_t np_pad, hipStream_t stream) {
  hipLaunchKernelGGL(summary_reset_kernel, grid1(np_pad), dim3(RS_BLOCK), 0, stream, acc, np_pad);
  return hipGetLastError();
}

hipError_t rs_cluster_outputs_summary(const void *const src[6], bool f32, const int32_t *order, int64_t npoints,
                                      int64_t src_stride, int32_t nrows, int32_t index0, int32_t index_step,
                                      const RsSummarySpec &spec, double *acc, int64_t np_pad, hipStream_t stream) {
  SummaryArgs a;
  for (int f = 0; f < 6; ++f) a.src[f] = src[f];
  a.order = order;
  a.acc = acc;
  a.npoints = npoints;
  a.stride = src_stride;
  a.np_pad = np_pad;
  a.nrows = nrows;
  a.index0 = index0;
  a.index_step = index_step;
  a.spec = spec;
  const dim3 grid((unsigned)((npoints + 63) / 64)), block(64 * SUM_WAVES);
  if (f32)
    hipLaunchKernelGGL(outputs_summary_kernel<float>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(outputs_summary_kernel<double>, grid, block, 0, stream, a);
  return hipGetLastError();
}

/* Per-point aggregates over output periods (include/roadsurf.h, rs_hip_outputs_periods; the definition is
 * roadsurf_amd/periods.py, reduce_series; which rows a period has: rs_period_rule.hpp): the summaries' sibling with
 * one cell per point AND period, and with a column - the sum of Tsurf - that depends on the order of the additions.
 * So the summary kernel's split of a call's rows over four wavefronts does not carry over: the rows of one period are
 * walked by ONE lane in time order.  What is spread instead is the periods, which are independent: a wavefront is 64
 * slots (blockIdx.x) and every gridDim.y-th period the call touches (blockIdx.y; every gridDim.y-th row where
 * index_step is above the length, when each row is a period of its own) - the headline's launches of 60
 * indices touch one or two hourly periods and fill the device with slots alone, a batch of a few hundred points run
 * in one launch has its hundreds of periods to spread.  The time index is wave-uniform, so a period's rows [lo, hi) of
 * the call are scalars and leaving a period is a uniform branch: a lane reads its point's cell (17 doubles, computed
 * address in POINT order) when the call first touches the period, carries it in registers over the period's rows with
 * PER_ROWS rows of all six streams in flight - every row load a coalesced 512 B per wavefront and stream, 256 B of an
 * fp32 window - and writes it once on leaving.  A point sits in one slot and a (point, period) cell belongs to one
 * lane of one wavefront: plain loads and stores, no atomics; all offsets are 64-bit.  Nothing is indexed by a number
 * of the caller's unchecked: slots and order entries are compared with npoints, rows come from rs_per::rows_of_period
 * (inside [0, nrows)), periods from rs_per::periods_of_call (inside [0, nperiods)). */
namespace {
constexpr int PER_ROWS = 4;

struct Per {
  double v[RS_PER_COLS]; /* the columns of include/roadsurf.h: everything fp64, indices and counts are exact there */
  __device__ void load(const double *p, int64_t stride) {
#pragma unroll
    for (int c = 0; c < RS_PER_COLS; ++c) v[c] = p[c * stride];
  }
  __device__ void store(double *p, int64_t stride) const {
#pragma unroll
    for (int c = 0; c < RS_PER_COLS; ++c) p[c * stride] = v[c];
  }
  /* one row of the point, the next in time of its period: its time index, Tsurf and the five storages */
  __device__ void row(double i, double t, const double s[5], const RsSummarySpec &th) {
    if (t == -9999.0) return; /* never saved: behind the last index of a failed point, or a rejected point */
    /* ((x0 + x1) + x2) + ...: the first valid row is the sum, not 0.0 + it; every addition rounded on its own */
    v[3] = v[0] == 0.0 ? t : __dadd_rn(v[3], t);
    v[0] += 1.0;
    if (t < v[1]) v[1] = t; /* a NaN never wins: every comparison with it is false */
    if (t > v[2]) v[2] = t;
    if (t < th.tsurf_below) v[4] += 1.0;
    if (i > v[6]) { v[5] = t; v[6] = i; } /* the sample: column 6 decides, whatever the order of feeding */
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      if (s[k] > v[7 + k]) v[7 + k] = s[k];
      if (s[k] > th.storage_above[k]) v[12 + k] += 1.0;
    }
  }
};

struct PeriodArgs {
  const void *src[6];   /* T[nrows][stride] each: Tsurf, Snow, Water, Ice, Deposit, Ice2 */
  const int32_t *order; /* column s is point order[s]; NULL: point s */
  double *acc;          /* [nperiods][RS_PER_COLS][np_pad], point order */
  int64_t npoints, stride, np_pad;
  int64_t w_lo, w_hi;   /* the periods the call can touch (rs_per::periods_of_call), w_lo <= w_hi */
  int32_t nrows, index0, index_step;
  RsPeriodSpec spec;
};

template <typename T>
__global__ void __launch_bounds__(64) outputs_periods_kernel(const PeriodArgs a) {
  const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (s >= a.npoints) return;
  const int64_t p = a.order ? (int64_t)a.order[s] : s;
  if (p < 0 || p >= a.npoints) return; /* not an order row of this plan: nothing is written */
  /* a unit is a period of [w_lo, w_hi] - or, where index_step is above length and so no two rows share a period, a
   * row: such a call may span far more periods than it has rows */
  const bool by_row = a.index_step > a.spec.length;
  const int64_t units = by_row ? (int64_t)a.nrows : a.w_hi - a.w_lo + 1;
#pragma unroll 1
  for (int64_t u = blockIdx.y; u < units; u += (int64_t)gridDim.y) {
    int64_t w;
    rs_per::Rows rows;
    if (by_row) {
      w = rs_per::period_of_row(a.spec, a.index0, a.index_step, u);
      rows.lo = u;
      rows.hi = w < 0 ? u : u + 1;
    } else {
      w = a.w_lo + u;
      rows = rs_per::rows_of_period(a.spec, a.index0, a.index_step, a.nrows, w);
    }
    if (rows.lo >= rows.hi) continue; /* a row of no period */
    double *cell = a.acc + w * (int64_t)RS_PER_COLS * a.np_pad + p;
    Per c;
    c.load(cell, a.np_pad);
#pragma unroll 1
    for (int64_t r0 = rows.lo; r0 < rows.hi; r0 += PER_ROWS) {
      T x[PER_ROWS][6];
#pragma unroll
      for (int q = 0; q < PER_ROWS; ++q) {
        const int64_t r = r0 + q < rows.hi ? r0 + q : rows.hi - 1; /* behind the range: its last row again, not taken */
#pragma unroll
        for (int f = 0; f < 6; ++f) x[q][f] = static_cast<const T *>(a.src[f])[r * a.stride + s];
      }
#pragma unroll
      for (int q = 0; q < PER_ROWS; ++q) {
        if (r0 + q >= rows.hi) break;
        const double st[5] = {(double)x[q][1], (double)x[q][2], (double)x[q][3], (double)x[q][4], (double)x[q][5]};
        c.row((double)rs_per::index_of_row(a.index0, a.index_step, r0 + q), (double)x[q][0], st, a.spec.th);
      }
    }
    c.store(cell, a.np_pad);
  }
}

/* the cell of no rows into all np_pad columns of every gridDim.y-th period */
__global__ void __launch_bounds__(RS_BLOCK) periods_reset_kernel(double *acc, int64_t np_pad, int64_t nperiods) {
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= np_pad) return;
  for (int64_t w = blockIdx.y; w < nperiods; w += (int64_t)gridDim.y) {
    double *cell = acc + w * (int64_t)RS_PER_COLS * np_pad + p;
#pragma unroll
    for (int c = 0; c < RS_PER_COLS; ++c) cell[c * np_pad] = rs_per::empty(c);
  }
}

/* blocks along y: enough wavefronts for the device where the x blocks alone are few, never more than there are
 * periods, never above the grid's limit */
inline unsigned periods_grid_y(int64_t blocks_x, int64_t periods) {
  const int64_t want = (8192 + blocks_x - 1) / blocks_x;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>({want, periods, 65535}));
}
}  // namespace

hipError_t rs_cluster_periods_reset(double *acc, int64_t np_pad, const RsPeriodSpec &spec, hipStream_t stream) {
  const dim3 grid = dim3(grid1(np_pad).x, periods_grid_y((np_pad + RS_BLOCK - 1) / RS_BLOCK, spec.nperiods));
  hipLaunchKernelGGL(periods_reset_kernel, grid, dim3(RS_BLOCK), 0, stream, acc, np_pad, (int64_t)spec.nperiods);
  return hipGetLastError();
}

hipError_t rs_cluster_outputs_periods(const void *const src[6], bool f32, const int32_t *order, int64_t npoints,
                                      int64_t src_stride, int32_t nrows, int32_t index0, int32_t index_step,
                                      const RsPeriodSpec &spec, double *acc, int64_t np_pad, hipStream_t stream) {
  const rs_per::Span span = rs_per::periods_of_call(spec, index0, index_step, nrows);
  if (span.lo > span.hi || npoints < 1) return hipSuccess; /* every row lies before the first period or behind the last */
  PeriodArgs a;
  for (int f = 0; f < 6; ++f) a.src[f] = src[f];
  a.order = order;
  a.acc = acc;
  a.npoints = npoints;
  a.stride = src_stride;
  a.np_pad = np_pad;
  a.w_lo = span.lo;
  a.w_hi = span.hi;
  a.nrows = nrows;
  a.index0 = index0;
  a.index_step = index_step;
  a.spec = spec;
  const int64_t blocks_x = (npoints + 63) / 64;
  const int64_t units = index_step > spec.length ? (int64_t)nrows : span.hi - span.lo + 1; /* (the kernel's units) */
  const dim3 grid((unsigned)blocks_x, periods_grid_y(blocks_x, units)), block(64);
  if (f32)
    hipLaunchKernelGGL(outputs_periods_kernel<float>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(outputs_periods_kernel<double>, grid, block, 0, stream, a);
  return hipGetLastError();
}

/* Per-point threshold episodes of the output rows (include/roadsurf.h, rs_hip_outputs_episodes; the definition is
 * roadsurf_amd/episodes.py, feed): the third sibling.  Unlike the summaries this reduction is order dependent - an
 * automaton per point that is fed its rows in sequence - so the rows of a slot are NOT split over wavefronts: one lane
 * owns a slot, loads its head and open run (RS_EPI_HEAD doubles) into registers, walks the rows in order with EPI_ROWS
 * rows of all seven streams in flight (every row load a coalesced 512 B per wavefront and stream, 256 B of an fp32
 * window) and stores the head back at the end.  A few hundred points by tens of rows is microseconds either way, and
 * a million points fill the device with slots alone.  A run that closes with enough rows is committed by storing its
 * six doubles straight to acc[(RS_EPI_HEAD + RS_EPI_REC * j + c) * np_pad + p], a computed address: the K records are
 * never held in registers, where an array indexed by the run-time j would put the kernel into scratch.  A point sits
 * in one slot: plain loads and stores, no atomics; all offsets are 64-bit. */
int32_t rs_cluster_episode_cols(const RsEpisodeSpec *spec) {
  if (!spec) return -1;
  if (spec->use <= 0 || (spec->use >> RS_EPI_VARS) != 0) return -1;
  for (int k = 0; k < RS_EPI_VARS; ++k)
    if (spec->above[k] != spec->above[k] || spec->below[k] != spec->below[k]) return -1;
  if (spec->peak < 0 || spec->peak >= RS_EPI_VARS) return -1;
  if (spec->min_rows < 1) return -1;
  if (spec->max_episodes < 1 || spec->max_episodes > RS_EPI_MAX) return -1;
  return RS_EPI_HEAD + spec->max_episodes * RS_EPI_REC;
}

namespace {
constexpr int EPI_ROWS = 4;

struct Epi {
  double h[RS_EPI_HEAD]; /* the head columns of include/roadsurf.h: everything fp64, indices and counts are exact */
  __device__ void clear_run() {
    h[4] = 0.0; h[5] = 0.0; h[6] = 0.0;
    h[7] = __builtin_huge_val();
    h[8] = 0.0;
    h[9] = -__builtin_huge_val();
  }
  __device__ void load(const double *p, int64_t stride) {
#pragma unroll
    for (int c = 0; c < RS_EPI_HEAD; ++c) h[c] = p[c * stride];
  }
  __device__ void store(double *p, int64_t stride) const {
#pragma unroll
    for (int c = 0; c < RS_EPI_HEAD; ++c) p[c * stride] = h[c];
  }
  /* close the open run: committed if it has min_rows rows - kept as record number h[0] while that is below K -,
   * cleared in every case.  `col` is the point's column of the accumulator. */
  __device__ void close(double *col, int64_t stride, const RsEpisodeSpec &sp) {
    if (h[6] >= (double)sp.min_rows) {
      if (h[0] >= 0.0 && h[0] < (double)sp.max_episodes) { /* (a record number of the caller's making stays inside) */
        double *rec = col + ((int64_t)RS_EPI_HEAD + (int64_t)RS_EPI_REC * (int64_t)h[0]) * stride;
#pragma unroll
        for (int c = 0; c < RS_EPI_REC; ++c) rec[c * stride] = h[4 + c];
      }
      h[0] += 1.0;
      h[1] += h[6];
      if (h[6] > h[2]) h[2] = h[6];
    }
    clear_run();
  }
  /* one row of the point: its time index, the seven variables */
  __device__ void row(double i, double step, const double x[RS_EPI_VARS], double *col, int64_t stride,
                      const RsEpisodeSpec &sp) {
    if (h[3] != 0.0 && h[3] != i) close(col, stride, sp);
    h[3] = i + step;
    bool ok = x[0] != -9999.0; /* never saved: behind the last index of a failed point, or a rejected point */
#pragma unroll
    for (int k = 0; k < RS_EPI_VARS; ++k)
      if ((sp.use >> k) & 1) ok = ok && sp.above[k] < x[k] && x[k] < sp.below[k];
    if ((sp.use >> 6) & 1) ok = ok && x[6] != -9999.0; /* no deficit there (roadsurf_amd/kept.py) */
    if (!ok) {
      close(col, stride, sp);
      return;
    }
    double pk = x[0]; /* a select per variable: x[sp.peak] would index registers with a run-time number */
#pragma unroll
    for (int k = 1; k < RS_EPI_VARS; ++k) pk = sp.peak == k ? x[k] : pk;
    if (h[6] == 0.0) h[4] = i;
    h[5] = i;
    h[6] += 1.0;
    if (x[0] < h[7]) { h[7] = x[0]; h[8] = i; } /* strict, in order: the smallest index among equals; a NaN never wins */
    if (pk > h[9]) h[9] = pk;
  }
};

struct EpisodeArgs {
  const void *src[RS_EPI_VARS]; /* T[nrows][stride] each: Tsurf, Snow, Water, Ice, Deposit, Ice2, deficit (or NULL) */
  const int32_t *order;         /* column s is point order[s]; NULL: point s (rs_driver_run's result block) */
  double *acc;                  /* [cols][np_pad], point order */
  int64_t npoints, stride, np_pad;
  int32_t nrows, index0, index_step;
  RsEpisodeSpec spec;
};

template <typename T>
__global__ void __launch_bounds__(RS_BLOCK) outputs_episodes_kernel(const EpisodeArgs a) {
  const int64_t s = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (s >= a.npoints) return;
  const int64_t p = a.order ? (int64_t)a.order[s] : s;
  if (p < 0 || p >= a.npoints) return; /* not an order row of this plan: nothing is written */
  double *col = a.acc + p;
  Epi e;
  e.load(col, a.np_pad);
  const bool with_deficit = a.src[6] != nullptr;
  const double step = (double)a.index_step;
#pragma unroll 1
  for (int32_t r0 = 0; r0 < a.nrows; r0 += EPI_ROWS) {
    T x[EPI_ROWS][RS_EPI_VARS];
#pragma unroll
    for (int q = 0; q < EPI_ROWS; ++q) {
      const int32_t r = r0 + q < a.nrows ? r0 + q : a.nrows - 1; /* behind the range: its last row again, not taken */
#pragma unroll
      for (int f = 0; f < 6; ++f) x[q][f] = static_cast<const T *>(a.src[f])[(int64_t)r * a.stride + s];
      x[q][6] = with_deficit ? static_cast<const T *>(a.src[6])[(int64_t)r * a.stride + s] : (T)0;
    }
#pragma unroll
    for (int q = 0; q < EPI_ROWS; ++q) {
      if (r0 + q >= a.nrows) break;
      const double v[RS_EPI_VARS] = {(double)x[q][0], (double)x[q][1], (double)x[q][2], (double)x[q][3],
                                     (double)x[q][4], (double)x[q][5], (double)x[q][6]};
      e.row((double)a.index0 + (double)(r0 + q) * step, step, v, col, a.np_pad, a.spec);
    }
  }
  e.store(col, a.np_pad);
}

__global__ void __launch_bounds__(RS_BLOCK) episodes_finish_kernel(double *acc, int64_t npoints, int64_t np_pad,
                                                                   const RsEpisodeSpec spec) {
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= npoints) return;
  Epi e;
  e.load(acc + p, np_pad);
  e.close(acc + p, np_pad, spec);
  e.h[3] = 0.0;
  e.store(acc + p, np_pad);
}

/* the accumulator of no rows into all np_pad columns: the head, then the K empty records */
__global__ void __launch_bounds__(RS_BLOCK) episodes_reset_kernel(double *acc, int64_t np_pad, int32_t nrec) {
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= np_pad) return;
  Epi e;
#pragma unroll
  for (int c = 0; c < 4; ++c) e.h[c] = 0.0;
  e.clear_run();
  e.store(acc + p, np_pad);
  for (int32_t j = 0; j < nrec; ++j) {
    double *rec = acc + p + ((int64_t)RS_EPI_HEAD + (int64_t)RS_EPI_REC * j) * np_pad;
#pragma unroll
    for (int c = 0; c < RS_EPI_REC; ++c) rec[c * np_pad] = e.h[4 + c];
  }
}
}  // namespace

hipError_t rs_cluster_episodes_reset(double *acc, int64_t np_pad, const RsEpisodeSpec &spec, hipStream_t stream) {
  hipLaunchKernelGGL(episodes_reset_kernel, grid1(np_pad), dim3(RS_BLOCK), 0, stream, acc, np_pad,
                     (int32_t)spec.max_episodes);
  return hipGetLastError();
}

hipError_t rs_cluster_outputs_episodes(const void *const src[6], const void *deficit, bool f32, const int32_t *order,
                                       int64_t npoints, int64_t src_stride, int32_t nrows, int32_t index0,
                                       int32_t index_step, const RsEpisodeSpec &spec, double *acc, int64_t np_pad,
                                       hipStream_t stream) {
  EpisodeArgs a;
  for (int f = 0; f < 6; ++f) a.src[f] = src[f];
  a.src[6] = deficit;
  a.order = order;
  a.acc = acc;
  a.npoints = npoints;
  a.stride = src_stride;
  a.np_pad = np_pad;
  a.nrows = nrows;
  a.index0 = index0;
  a.index_step = index_step;
  a.spec = spec;
  if (f32)
    hipLaunchKernelGGL(outputs_episodes_kernel<float>, grid1(npoints), dim3(RS_BLOCK), 0, stream, a);
  else
    hipLaunchKernelGGL(outputs_episodes_kernel<double>, grid1(npoints), dim3(RS_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t rs_cluster_episodes_finish(double *acc, int64_t npoints, int64_t np_pad, const RsEpisodeSpec &spec,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(episodes_finish_kernel, grid1(npoints), dim3(RS_BLOCK), 0, stream, acc, npoints, np_pad, spec);
  return hipGetLastError();
}

/* Per-group time series of the output rows (include/roadsurf.h, rs_hip_outputs_groups; the definition is
 * roadsurf_amd/groups.py, reduce_groups): the second sibling, reducing over the slots of a row instead of the rows of
 * a slot.  Many slots fold into one cell acc[row][group][col], so the cells are updated with atomics - every column is
 * a count, a minimum or a maximum, whose fp64 atomics are exact and order-free, and lanes filter NaN before the
 * atomic.  A lane owns a slot, gathers its group id once and keeps it over the rows it reads, GRP_ROWS rows of the six
 * streams in flight, every row load a coalesced 512 B per wavefront and stream.
 *   groups_lds_kernel     ngroups * cols <= RS_GRP_LDS_CELLS.  A workgroup takes a block of rows_per_block rows
 *                         (blockIdx.y) and every gridDim.x-th block of 256 slots, keeps rows x ngroups x cols cells in
 *                         LDS, updates them with LDS atomics - the extremes behind a plain read of the cell, which can
 *                         only be staler, that is less extreme, than the cell: an update it skips would not have
 *                         changed it - and ends by flushing its non-empty cells with global atomics, consecutive lanes
 *                         on consecutive doubles: a global cell is hit once per workgroup, not once per point.
 *   groups_global_kernel  more cells than that: lanes update the global cells directly. */
namespace {
constexpr int GRP_THREADS = 256, GRP_ROWS = 4;

struct GroupArgs {
  const void *src[6];   /* T[nrows][stride] each: Tsurf, Snow, Water, Ice, Deposit, Ice2 */
  const int32_t *order; /* column s is point order[s]; NULL: point s (rs_driver_run's result block) */
  const int32_t *group; /* [npoints], point order */
  double *acc;          /* [nrows][ngroups][cols]: row acc_row0 of the caller's accumulator */
  int64_t npoints, stride;
  int32_t nrows, ngroups, cols, nedges, rows_per_block;
  RsSummarySpec th;
  double edges[RS_GRP_MAX_EDGES];
};

/* the empty value of column c: counts 0, min +inf, maxima -inf */
__device__ __forceinline__ double grp_empty(int c) {
  return rs_grp::empty(c);
}

/* the group of slot s, or -1: no point, or a point of no group */
__device__ __forceinline__ int32_t grp_of_slot(const GroupArgs &a, int64_t s) {
  if (s >= a.npoints) return -1;
  const int64_t p = a.order ? (int64_t)a.order[s] : s;
  if (p < 0 || p >= a.npoints) return -1; /* not an order row of this plan */
  const int32_t g = a.group[p];
  return g >= 0 && g < a.ngroups ? g : -1;
}

/* One point's row into its cell `c`, in LDS (SCOPE workgroup, PEEK) or in device memory (SCOPE agent). */
template <int SCOPE, bool PEEK>
__device__ __forceinline__ void grp_update(double *c, double t, const double s[5], const GroupArgs &a) {
  if (t == -9999.0) return; /* never saved: behind the last index of a failed point, or a rejected point */
  __hip_atomic_fetch_add(c + 0, 1.0, __ATOMIC_RELAXED, SCOPE);
  /* a NaN fails every comparison here and so never reaches a min or max atomic */
  if (PEEK ? t < __hip_atomic_load(c + 1, __ATOMIC_RELAXED, SCOPE) : t == t)
    __hip_atomic_fetch_min(c + 1, t, __ATOMIC_RELAXED, SCOPE);
  if (PEEK ? t > __hip_atomic_load(c + 2, __ATOMIC_RELAXED, SCOPE) : t == t)
    __hip_atomic_fetch_max(c + 2, t, __ATOMIC_RELAXED, SCOPE);
  if (t < a.th.tsurf_below) __hip_atomic_fetch_add(c + 3, 1.0, __ATOMIC_RELAXED, SCOPE);
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    if (s[k] > a.th.storage_above[k]) __hip_atomic_fetch_add(c + 4 + k, 1.0, __ATOMIC_RELAXED, SCOPE);
    if (PEEK ? s[k] > __hip_atomic_load(c + 9 + k, __ATOMIC_RELAXED, SCOPE) : s[k] == s[k])
      __hip_atomic_fetch_max(c + 9 + k, s[k], __ATOMIC_RELAXED, SCOPE);
  }
  if (a.nedges > 0 && t == t) {
    int j = 0;
    for (int e = 0; e < a.nedges; ++e) j += a.edges[e] <= t ? 1 : 0;
    __hip_atomic_fetch_add(c + RS_GRP_COLS + j, 1.0, __ATOMIC_RELAXED, SCOPE);
  }
}

/* rows [r_lo, r_hi) of slot s into the cells cell0 + (r - r_lo) * row_cells */
template <typename T, int SCOPE, bool PEEK>
__device__ __forceinline__ void grp_rows(const GroupArgs &a, int64_t s, int32_t r_lo, int32_t r_hi, double *cell0,
                                         int64_t row_cells) {
#pragma unroll 1
  for (int32_t r0 = r_lo; r0 < r_hi; r0 += GRP_ROWS) {
    T x[GRP_ROWS][6];
#pragma unroll
    for (int q = 0; q < GRP_ROWS; ++q) {
      const int32_t r = r0 + q < r_hi ? r0 + q : r_hi - 1; /* behind the range: its last row again, not taken */
#pragma unroll
      for (int f = 0; f < 6; ++f) x[q][f] = static_cast<const T *>(a.src[f])[(int64_t)r * a.stride + s];
    }
#pragma unroll
    for (int q = 0; q < GRP_ROWS; ++q) {
      if (r0 + q >= r_hi) break;
      const double st[5] = {(double)x[q][1], (double)x[q][2], (double)x[q][3], (double)x[q][4], (double)x[q][5]};
      grp_update<SCOPE, PEEK>(cell0 + (int64_t)(r0 + q - r_lo) * row_cells, (double)x[q][0], st, a);
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(GRP_THREADS) groups_lds_kernel(const GroupArgs a) {
  extern __shared__ double grp_tab[]; /* [rows of the block][ngroups][cols] */
  const int32_t r_lo = (int32_t)blockIdx.y * a.rows_per_block,
                r_hi = a.nrows < r_lo + a.rows_per_block ? a.nrows : r_lo + a.rows_per_block;
  const int32_t row_cells = a.ngroups * a.cols, n_tab = (r_hi - r_lo) * row_cells;
  for (int32_t i = threadIdx.x; i < n_tab; i += GRP_THREADS) grp_tab[i] = grp_empty(i % a.cols);
  __syncthreads();
#pragma unroll 1
  for (int64_t s = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x; s < a.npoints;
       s += (int64_t)gridDim.x * GRP_THREADS) {
    const int32_t g = grp_of_slot(a, s);
    if (g < 0) continue;
    grp_rows<T, __HIP_MEMORY_SCOPE_WORKGROUP, true>(a, s, r_lo, r_hi, grp_tab + g * a.cols, row_cells);
  }
  __syncthreads();
  /* the flush: cells with a point, and in them only the columns that say something */
  double *dst = a.acc + (int64_t)r_lo * row_cells;
  for (int32_t i = threadIdx.x; i < n_tab; i += GRP_THREADS) {
    const int32_t c = i % a.cols;
    if (grp_tab[i - c] == 0.0) continue;
    const double v = grp_tab[i];
    if (v == grp_empty(c)) continue;
    if (c == 1)
      __hip_atomic_fetch_min(dst + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (c == 2 || (c >= 9 && c < RS_GRP_COLS))
      __hip_atomic_fetch_max(dst + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      __hip_atomic_fetch_add(dst + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <typename T>
__global__ void __launch_bounds__(GRP_THREADS) groups_global_kernel(const GroupArgs a) {
  const int64_t s = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x;
  const int32_t g = grp_of_slot(a, s);
  if (g < 0) return;
  const int64_t row_cells = (int64_t)a.ngroups * a.cols;
  grp_rows<T, __HIP_MEMORY_SCOPE_AGENT, false>(a, s, 0, a.nrows, a.acc + (int64_t)g * a.cols, row_cells);
}

__global__ void __launch_bounds__(RS_BLOCK) group_reset_kernel(double *acc, int64_t n, int32_t cols) {
  const int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (i < n) acc[i] = grp_empty((int)(i % cols));
}
}  // namespace

int32_t rs_cluster_group_cols(const RsGroupSpec *sp) {
  if (!sp || sp->ngroups < 1 || sp->nedges < 0 || sp->nedges > RS_GRP_MAX_EDGES) return -1;
  for (int e = 0; e < sp->nedges; ++e)
    if (sp->edges[e] != sp->edges[e] || (e > 0 && !(sp->edges[e] > sp->edges[e - 1]))) return -1;
  return RS_GRP_COLS + (sp->nedges ? sp->nedges + 1 : 0);
}

/* the one place that chooses the kernel: a row of cells fits the workgroup's LDS, or it does not */
int32_t rs_cluster_group_path(const RsGroupSpec *sp) {
  const int32_t cols = rs_cluster_group_cols(sp);
  if (cols < 0) return -1;
  return (int64_t)sp->ngroups * cols <= RS_GRP_LDS_CELLS ? 1 : 2;
}

hipError_t rs_cluster_group_reset(double *acc, int64_t acc_rows, const RsGroupSpec &spec, hipStream_t stream) {
  const int32_t cols = rs_cluster_group_cols(&spec);
  if (cols < 0 || acc_rows < 1) return hipErrorInvalidValue;
  const int64_t n = acc_rows * spec.ngroups * cols;
  hipLaunchKernelGGL(group_reset_kernel, grid1(n), dim3(RS_BLOCK), 0, stream, acc, n, cols);
  return hipGetLastError();
}

hipError_t rs_cluster_outputs_groups(const void *const src[6], bool f32, const int32_t *order, const int32_t *group,
                                     int64_t npoints, int64_t src_stride, int32_t nrows, const RsGroupSpec &spec,
                                     double *acc_row0, hipStream_t stream) {
  const int32_t path = rs_cluster_group_path(&spec);
  if (path < 0 || nrows < 1 || npoints < 1) return hipErrorInvalidValue;
  GroupArgs a;
  for (int f = 0; f < 6; ++f) a.src[f] = src[f];
  a.order = order;
  a.group = group;
  a.acc = acc_row0;
  a.npoints = npoints;
  a.stride = src_stride;
  a.nrows = nrows;
  a.ngroups = spec.ngroups;
  a.cols = rs_cluster_group_cols(&spec);
  a.nedges = spec.nedges;
  a.th = spec.thresholds;
  for (int e = 0; e < RS_GRP_MAX_EDGES; ++e) a.edges[e] = e < spec.nedges ? spec.edges[e] : 0.0;
  const int64_t slot_blocks = (npoints + GRP_THREADS - 1) / GRP_THREADS;
  if (path == 1) {
    /* as many rows per workgroup as are in flight per lane, fewer where the cells of that many exceed the LDS budget;
     * about a thousand workgroups in all, each looping over its share of the slot blocks */
    const int32_t row_cells = spec.ngroups * a.cols;
    a.rows_per_block = std::max(1, std::min({GRP_ROWS, RS_GRP_LDS_CELLS / row_cells, nrows}));
    const int64_t row_blocks = (nrows + a.rows_per_block - 1) / a.rows_per_block;
    if (row_blocks > 65535) return hipErrorInvalidValue; /* (the callers feed such windows in pieces) */
    const dim3 grid((unsigned)std::min<int64_t>(slot_blocks, std::max<int64_t>(1, 1024 / row_blocks)),
                    (unsigned)row_blocks);
    const size_t lds = (size_t)a.rows_per_block * row_cells * sizeof(double);
    if (f32)
      hipLaunchKernelGGL(groups_lds_kernel<float>, grid, dim3(GRP_THREADS), lds, stream, a);
    else
      hipLaunchKernelGGL(groups_lds_kernel<double>, grid, dim3(GRP_THREADS), lds, stream, a);
  } else {
    a.rows_per_block = nrows;
    const dim3 grid((unsigned)slot_blocks);
    if (f32)
      hipLaunchKernelGGL(groups_global_kernel<float>, grid, dim3(GRP_THREADS), 0, stream, a);
    else
      hipLaunchKernelGGL(groups_global_kernel<double>, grid, dim3(GRP_THREADS), 0, stream, a);
  }
  return hipGetLastError();
}

/* Per-station ensemble statistics of the output rows (include/roadsurf.h, rs_hip_outputs_ens; the definition is
 * roadsurf_amd/ensstats.py, reduce_members): the third reducer over the slots of a row, and of another shape than the
 * group series - a mean, a spread and quantiles equal their definition only if a station's members are summed in one
 * fixed order, which rules atomics out.  A workgroup takes 64 consecutive stations; the member list of the table gives
 * it one contiguous segment of at most 64 * max_members entries, which it resolves ONCE to slots (entry -> point ->
 * inv[point]) and keeps in LDS, each beside its place in a wavefront's row.  Each wavefront then takes rows of its own
 * (only wave-level synchronisation from there on): per row and variable its lanes run over the segment's ENTRIES and
 * load win[row][slot] - whole lines while members sit side by side, gathers after a re-sort - into the wavefront's LDS
 * row, which is MEMBER-major: position j of station g at j * ENS_ROW + g.  Then lane g owns station g and walks its
 * column in table order, the 64 lanes on 64 consecutive doubles; ENS_ROW = 65, one double of padding, keeps the
 * staging's scattered writes - consecutive entries are consecutive members of ONE station - out of each other's
 * banks too.  The Tsurf pass builds the used mask (64 bits: at most 64 members), compacts the used values to the top
 * of the column and sums them on the way, forms mean and squared deviations, sorts the column in place (insertion
 * sort: at most 64 values) and takes the quantiles; the five storage passes re-stage and sum under the mask.  No
 * member value lives in an indexed register array (it would be scratch), every offset is 64 bits, and a damaged table
 * cannot lead outside the table, the window or LDS: a segment is clamped to max_members and to the member list, the
 * workgroup's entries are laid out by a scan of the CLAMPED counts, and an entry or an inverse outside [0, npoints) is
 * a slot of -1, which loads nothing. */
namespace {
constexpr int ENS_MAX_WAVES = 4;          /* rows in flight per workgroup */
constexpr int ENS_LDS_BUDGET = 64 * 1024; /* per workgroup: two or more workgroups to a CU's 160 KiB */
constexpr int ENS_LOADS = 16;             /* loads a lane has in flight while it stages a row */
constexpr int ENS_ROW = 65;               /* doubles per member position of a wavefront's row: 64 stations, one pad */

struct EnsArgs {
  const void *src[6];   /* T[nrows][stride] each: Tsurf, Snow, Water, Ice, Deposit, Ice2 */
  const int32_t *table; /* [ngroups + 1] starts, [npoints] entries (rs_ens_table.hpp) */
  const int32_t *inv;   /* [npoints]: the slot of a point */
  double *acc;          /* [nrows][ngroups][cols]: row acc_row0 of the caller's accumulator */
  int64_t npoints, stride;
  int32_t nrows, ngroups, max_members, nquant, cols, rows_per_block, waves;
  double quant[RS_ENS_MAX_QUANT];
};

/* the lanes of ONE wavefront hand LDS values to each other: its LDS accesses execute in program order, so this orders
 * them for the compiler and waits for nothing another wavefront did */
__device__ __forceinline__ void ens_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* one variable of one row into the wavefront's LDS row, entry by entry, ENS_LOADS loads in flight per lane: the
 * wavefronts of a CU are few (LDS), so the loads a lane keeps in flight are what hides the memory's latency - and
 * with so few wavefronts the registers are there */
template <typename T>
__device__ __forceinline__ void ens_stage(const T *__restrict__ src, const int32_t *slot, const uint16_t *place,
                                          int32_t total, int lane, double *val) {
#pragma unroll 1
  for (int32_t i0 = lane; i0 < total; i0 += 64 * ENS_LOADS) {
    double v[ENS_LOADS];
#pragma unroll
    for (int q = 0; q < ENS_LOADS; ++q) {
      const int32_t i = i0 + 64 * q;
      const int32_t s = i < total ? slot[i] : -1;
      v[q] = s >= 0 ? (double)src[s] : -9999.0; /* no such member: invalid, and under no mask */
    }
#pragma unroll
    for (int q = 0; q < ENS_LOADS; ++q) {
      const int32_t i = i0 + 64 * q;
      if (i < total) val[place[i]] = v[q];
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(64 * ENS_MAX_WAVES) ens_stats_kernel(const EnsArgs a) {
  /* [waves][max_members][ENS_ROW] values; then per entry of the segment, [64 * max_members] each: its slot (int32)
   * and its place in a wavefront's row (uint16) */
  extern __shared__ double ens_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t seg = 64 * a.max_members, row_len = ENS_ROW * a.max_members;
  double *val = ens_lds + (int64_t)wave * row_len;
  int32_t *slot = reinterpret_cast<int32_t *>(ens_lds + (int64_t)a.waves * row_len);
  uint16_t *place = reinterpret_cast<uint16_t *>(slot + seg);
  const int64_t g = (int64_t)blockIdx.x * 64 + lane;
  const bool live = g < a.ngroups;
  /* the station's segment of the member list, clamped to max_members and to the list */
  int32_t first = 0, cnt = 0;
  if (live) {
    const int64_t s0 = a.table[g], s1 = a.table[g + 1];
    if (s0 >= 0 && s0 < a.npoints && s1 > s0) {
      int64_t c = s1 - s0;
      if (c > a.max_members) c = a.max_members;
      if (c > a.npoints - s0) c = a.npoints - s0;
      first = (int32_t)s0;
      cnt = (int32_t)c;
    }
  }
  /* where the station's entries begin in the workgroup's segment: the scan of the clamped counts (every wavefront
   * of the workgroup reads the same table and gets the same layout) */
  int32_t incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t u = __shfl_up(incl, d, 64);
    if (lane >= d) incl += u;
  }
  const int32_t off = incl - cnt, total = __shfl(incl, 63, 64);
  /* entries to slots, once: wavefront w resolves the member positions w, w + waves, ... of every station */
  const int32_t *entry = a.table + ((int64_t)a.ngroups + 1);
  for (int32_t j = wave; j < cnt; j += a.waves) {
    const int64_t p = entry[(int64_t)first + j];
    int32_t s = -1;
    if (p >= 0 && p < a.npoints) {
      const int64_t q = a.inv[p];
      if (q >= 0 && q < a.npoints) s = (int32_t)q;
    }
    slot[off + j] = s;
    place[off + j] = (uint16_t)(j * ENS_ROW + lane);
  }
  __syncthreads();

  const int32_t r_lo = (int32_t)blockIdx.y * a.rows_per_block,
                r_hi = a.nrows - r_lo < a.rows_per_block ? a.nrows : r_lo + a.rows_per_block;
  double *x = val + lane; /* the station's column: position j at x[j * ENS_ROW], cnt of them */
#pragma unroll 1
  for (int32_t r = r_lo + wave; r < r_hi; r += a.waves) {
    double *cell = a.acc + ((int64_t)r * a.ngroups + g) * a.cols;
    ens_wave_sync(); /* (every lane is done with the row before) */
    ens_stage<T>(static_cast<const T *>(a.src[0]) + (int64_t)r * a.stride, slot, place, total, lane, val);
    ens_wave_sync();
    /* Tsurf: the used mask; the used values to the top of the column in table order, and their sum on the way */
    uint64_t used = 0;
    int32_t nvalid = 0, k = 0;
    double sum = 0.0;
    for (int32_t j = 0; j < cnt; ++j) {
      const double t = x[j * ENS_ROW];
      const bool ok = t != -9999.0;
      nvalid += ok ? 1 : 0;
      if (ok && t == t) {
        used |= 1ull << j;
        sum = k ? __dadd_rn(sum, t) : t;
        x[k * ENS_ROW] = t;
        ++k;
      }
    }
    const double kd = (double)k;
    double mean = -9999.0, spread = -9999.0;
    if (k > 0) {
      mean = sum / kd;
      double d = __dsub_rn(x[0], mean);
      double q = __dmul_rn(d, d);
      for (int32_t j = 1; j < k; ++j) {
        d = __dsub_rn(x[j * ENS_ROW], mean);
        q = __dadd_rn(q, __dmul_rn(d, d));
      }
      spread = ::sqrt(q / kd);
      for (int32_t i = 1; i < k; ++i) { /* ascending, in place */
        const double v = x[i * ENS_ROW];
        int32_t j = i;
        while (j > 0 && x[(j - 1) * ENS_ROW] > v) {
          x[j * ENS_ROW] = x[(j - 1) * ENS_ROW];
          --j;
        }
        x[j * ENS_ROW] = v;
      }
    }
    if (live) {
      cell[0] = (double)nvalid;
      cell[1] = kd;
      cell[2] = mean;
      cell[3] = spread;
      for (int32_t c = 0; c < a.nquant; ++c) {
        double v = -9999.0;
        if (k > 0) {
          const double h = __dmul_rn(a.quant[c], (double)(k - 1));
          int32_t lo = (int32_t)h; /* floor: h >= 0 */
          lo = lo < 0 ? 0 : lo > k - 1 ? k - 1 : lo;
          const int32_t hi = lo + 1 < k - 1 ? lo + 1 : k - 1;
          const double t = __dsub_rn(h, (double)lo);
          const double ylo = x[lo * ENS_ROW];
          v = __dadd_rn(ylo, __dmul_rn(t, __dsub_rn(x[hi * ENS_ROW], ylo)));
        }
        cell[RS_ENS_COLS + c] = v;
      }
    }
    /* the storages of the used members, summed in table order */
#pragma unroll 1
    for (int f = 1; f < 6; ++f) {
      ens_wave_sync();
      ens_stage<T>(static_cast<const T *>(a.src[f]) + (int64_t)r * a.stride, slot, place, total, lane, val);
      ens_wave_sync();
      double m = -9999.0;
      if (k > 0) {
        double s = 0.0;
        bool none = true;
        for (int32_t j = 0; j < cnt; ++j) {
          if (!((used >> j) & 1ull)) continue;
          s = none ? x[j * ENS_ROW] : __dadd_rn(s, x[j * ENS_ROW]);
          none = false;
        }
        m = s / kd;
      }
      if (live) cell[3 + f] = m;
    }
  }
}
}  // namespace

int32_t rs_cluster_ens_waves(const RsEnsSpec *sp) {
  if (rs_ens::cols(sp) < 0) return -1;
  /* per entry of the 64 stations an int32 slot and a uint16 place; per wavefront a row of ENS_ROW * max_members */
  const int32_t entries = 64 * sp->max_members * (int32_t)(sizeof(int32_t) + sizeof(uint16_t)),
                row = ENS_ROW * sp->max_members * (int32_t)sizeof(double);
  return std::max(1, std::min(ENS_MAX_WAVES, (ENS_LDS_BUDGET - entries) / row));
}

size_t rs_cluster_ens_lds_bytes(const RsEnsSpec *sp) {
  const int32_t waves = rs_cluster_ens_waves(sp);
  if (waves < 0) return 0;
  return (size_t)sp->max_members * ((size_t)waves * ENS_ROW * sizeof(double) + 64 * (sizeof(int32_t) + sizeof(uint16_t)));
}

hipError_t rs_cluster_outputs_ens(const void *const src[6], bool f32, const int32_t *table, const int32_t *inv,
                                  int64_t npoints, int64_t src_stride, int32_t nrows, const RsEnsSpec &spec,
                                  double *acc_row0, hipStream_t stream) {
  const int32_t waves = rs_cluster_ens_waves(&spec);
  if (waves < 0 || nrows < 1 || npoints < 1) return hipErrorInvalidValue;
  EnsArgs a;
  for (int f = 0; f < 6; ++f) a.src[f] = src[f];
  a.table = table;
  a.inv = inv;
  a.acc = acc_row0;
  a.npoints = npoints;
  a.stride = src_stride;
  a.nrows = nrows;
  a.ngroups = spec.ngroups;
  a.max_members = spec.max_members;
  a.nquant = spec.nquant;
  a.cols = rs_ens::cols(&spec);
  a.waves = waves;
  for (int j = 0; j < RS_ENS_MAX_QUANT; ++j) a.quant[j] = j < spec.nquant ? spec.quant[j] : 0.0;
  /* the stations give the grid's x, blocks of rows its y: about six thousand workgroups in all - several rounds of
   * what the chip holds at once, so that the last round is a small part - each with a whole number of rows per
   * wavefront, since it resolves its segment before its first row */
  const int64_t station_blocks = ((int64_t)spec.ngroups + 63) / 64;
  const int64_t want_row_blocks = std::max<int64_t>(1, 6144 / station_blocks);
  const int64_t rows_each = std::max<int64_t>(1, ((int64_t)nrows + want_row_blocks - 1) / want_row_blocks);
  a.rows_per_block = (int32_t)std::min<int64_t>(INT32_MAX / 2, (rows_each + waves - 1) / waves * waves);
  const int64_t row_blocks = ((int64_t)nrows + a.rows_per_block - 1) / a.rows_per_block;
  const dim3 grid((unsigned)station_blocks, (unsigned)row_blocks);
  const size_t lds = rs_cluster_ens_lds_bytes(&spec);
  if (f32)
    hipLaunchKernelGGL(ens_stats_kernel<float>, grid, dim3(64 * waves), lds, stream, a);
  else
    hipLaunchKernelGGL(ens_stats_kernel<double>, grid, dim3(64 * waves), lds, stream, a);
  return hipGetLastError();
}

/* Per-station probabilities of conditions over the members (include/roadsurf.h, rs_hip_outputs_prob; the definition is
 * roadsurf_amd/ensprob.py, reduce_members_prob): the fourth reducer over the slots of a row, and the first that is also
 * sequential over the rows - "has held by now" is a member's history, a station's cell runs over its members.  Two
 * kernels therefore.  prob_bits_kernel is the episodes' feed with a smaller automaton: one lane owns a slot, reads the
 * carry of its point once, walks the call's rows in time order with PROB_ROWS rows of all streams in flight (every row
 * load a coalesced 512 B per wavefront and stream, 256 B of an fp32 window), stores per row one word at [row][slot] -
 * bits 0..7 holds now per condition, bits 8..15 valid and held by now, bit 16 valid - and the carry once.  The
 * conditions are kernel arguments, tested in loops that unroll over constants under wave-uniform branches: no bound is
 * indexed per lane.  prob_count_kernel takes 64 consecutive stations per workgroup, resolves their segment of the member
 * list ONCE to slots in LDS exactly as ens_stats_kernel does (clamped counts, their scan, -1 for an entry or an inverse
 * outside [0, npoints)), and then lane g walks station g's words of a row - each wavefront rows of its own - and counts
 * their bits into registers.  The words are 4 B against the 48 B the first kernel read for them, and the members of a
 * station sit in a few lines that stay in the caches from one member position to the next, so the walk is not staged
 * through LDS as the statistics' doubles are.  No atomics; every offset is 64 bits. */
int32_t rs_cluster_prob_cols(const RsProbSpec *sp) {
  if (!sp || sp->ngroups < 1 || sp->max_members < 1 || sp->max_members > RS_ENS_MAX_MEMBERS || sp->nconds < 1 ||
      sp->nconds > RS_PROB_MAX_CONDS)
    return -1;
  for (int32_t c = 0; c < sp->nconds; ++c) {
    const RsProbCond &k = sp->cond[c];
    if (k.use <= 0 || (k.use >> RS_EPI_VARS) != 0) return -1;
    for (int v = 0; v < RS_EPI_VARS; ++v)
      if (k.above[v] != k.above[v] || k.below[v] != k.below[v]) return -1;
  }
  return 1 + 2 * sp->nconds;
}

int32_t rs_cluster_prob_needs_deficit(const RsProbSpec *sp) {
  if (rs_cluster_prob_cols(sp) < 0) return -1;
  for (int32_t c = 0; c < sp->nconds; ++c)
    if ((sp->cond[c].use >> 6) & 1) return 1;
  return 0;
}

namespace {
constexpr int PROB_ROWS = 4;  /* rows of all streams a lane of prob_bits_kernel has in flight */
constexpr int PROB_WAVES = 4; /* wavefronts of prob_count_kernel's workgroup: rows in flight */
constexpr int PROB_WORDS = 4; /* words a lane of prob_count_kernel has in flight */

struct ProbBitsArgs {
  const void *src[RS_EPI_VARS]; /* T[nrows][stride] each: Tsurf, Snow, Water, Ice, Deposit, Ice2, deficit (or NULL) */
  const int32_t *order;         /* column s is point order[s] */
  int32_t *ever;                /* [np_pad], point order: bit c = condition c has held */
  uint32_t *words;              /* [nrows][wstride] */
  int64_t npoints, stride, wstride;
  int32_t nrows, nconds;
  RsProbCond cond[RS_PROB_MAX_CONDS];
};

template <typename T>
__global__ void __launch_bounds__(RS_BLOCK) prob_bits_kernel(const ProbBitsArgs a) {
  const int64_t s = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (s >= a.npoints) return;
  const int64_t p = a.order ? (int64_t)a.order[s] : s;
  const bool own = p >= 0 && p < a.npoints; /* not an order row of this plan: no carry is read or written */
  uint32_t ever = own ? (uint32_t)a.ever[p] : 0u;
  const bool with_deficit = a.src[6] != nullptr;
#pragma unroll 1
  for (int32_t r0 = 0; r0 < a.nrows; r0 += PROB_ROWS) {
    T x[PROB_ROWS][RS_EPI_VARS];
#pragma unroll
    for (int q = 0; q < PROB_ROWS; ++q) {
      const int32_t r = r0 + q < a.nrows ? r0 + q : a.nrows - 1; /* behind the range: its last row again, not taken */
#pragma unroll
      for (int f = 0; f < 6; ++f) x[q][f] = static_cast<const T *>(a.src[f])[(int64_t)r * a.stride + s];
      x[q][6] = with_deficit ? static_cast<const T *>(a.src[6])[(int64_t)r * a.stride + s] : (T)0;
    }
#pragma unroll
    for (int q = 0; q < PROB_ROWS; ++q) {
      if (r0 + q >= a.nrows) break;
      const double v[RS_EPI_VARS] = {(double)x[q][0], (double)x[q][1], (double)x[q][2], (double)x[q][3],
                                     (double)x[q][4], (double)x[q][5], (double)x[q][6]};
      const bool valid = v[0] != -9999.0; /* never saved: behind the last index of a failed point, or a rejected point */
      uint32_t now = 0;
#pragma unroll
      for (int c = 0; c < RS_PROB_MAX_CONDS; ++c) {
        if (c >= a.nconds) break;
        const int32_t use = a.cond[c].use;
        bool ok = valid;
#pragma unroll
        for (int k = 0; k < RS_EPI_VARS; ++k)
          if ((use >> k) & 1) ok = ok && a.cond[c].above[k] < v[k] && v[k] < a.cond[c].below[k];
        if ((use >> 6) & 1) ok = ok && v[6] != -9999.0; /* no deficit there (roadsurf_amd/kept.py) */
        now |= (ok ? 1u : 0u) << c;
      }
      ever |= now;
      a.words[(int64_t)(r0 + q) * a.wstride + s] = valid ? (now | ((ever & 0xffu) << 8) | (1u << 16)) : 0u;
    }
  }
  if (own) a.ever[p] = (int32_t)ever;
}

struct ProbCountArgs {
  const uint32_t *words; /* [nrows][wstride] */
  const int32_t *table;  /* [ngroups + 1] starts, [npoints] entries (rs_ens_table.hpp) */
  const int32_t *inv;    /* [npoints]: the slot of a point */
  double *acc;           /* [nrows][ngroups][cols]: row acc_row0 of the caller's accumulator */
  int64_t npoints, wstride;
  int32_t nrows, ngroups, max_members, nconds, cols, rows_per_block;
};

__global__ void __launch_bounds__(64 * PROB_WAVES) prob_count_kernel(const ProbCountArgs a) {
  extern __shared__ int32_t prob_slot[]; /* [64 * max_members]: the slot of every entry of the workgroup's segment */
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = (int64_t)blockIdx.x * 64 + lane;
  const bool live = g < a.ngroups;
  /* the station's segment of the member list, clamped to max_members and to the list */
  int32_t first = 0, cnt = 0;
  if (live) {
    const int64_t s0 = a.table[g], s1 = a.table[g + 1];
    if (s0 >= 0 && s0 < a.npoints && s1 > s0) {
      int64_t c = s1 - s0;
      if (c > a.max_members) c = a.max_members;
      if (c > a.npoints - s0) c = a.npoints - s0;
      first = (int32_t)s0;
      cnt = (int32_t)c;
    }
  }
  /* where the station's entries begin in the workgroup's segment: the scan of the clamped counts */
  int32_t incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t u = __shfl_up(incl, d, 64);
    if (lane >= d) incl += u;
  }
  const int32_t off = incl - cnt; /* off + cnt <= 64 * max_members */
  /* entries to slots, once: wavefront w resolves the member positions w, w + PROB_WAVES, ... of every station */
  const int32_t *entry = a.table + ((int64_t)a.ngroups + 1);
  for (int32_t j = wave; j < cnt; j += PROB_WAVES) {
    const int64_t p = entry[(int64_t)first + j];
    int32_t s = -1;
    if (p >= 0 && p < a.npoints) {
      const int64_t q = a.inv[p];
      if (q >= 0 && q < a.npoints) s = (int32_t)q;
    }
    prob_slot[off + j] = s;
  }
  __syncthreads();

  const int32_t r_lo = (int32_t)blockIdx.y * a.rows_per_block,
                r_hi = a.nrows - r_lo < a.rows_per_block ? a.nrows : r_lo + a.rows_per_block;
  const int32_t *mine = prob_slot + off;
#pragma unroll 1
  for (int32_t r = r_lo + wave; r < r_hi; r += PROB_WAVES) {
    const uint32_t *w = a.words + (int64_t)r * a.wstride;
    int32_t nvalid = 0, now[RS_PROB_MAX_CONDS], by[RS_PROB_MAX_CONDS];
#pragma unroll
    for (int c = 0; c < RS_PROB_MAX_CONDS; ++c) now[c] = by[c] = 0;
    for (int32_t j0 = 0; j0 < cnt; j0 += PROB_WORDS) {
      uint32_t x[PROB_WORDS];
#pragma unroll
      for (int q = 0; q < PROB_WORDS; ++q) {
        const int32_t s = j0 + q < cnt ? mine[j0 + q] : -1;
        x[q] = s >= 0 ? w[s] : 0u; /* no such member: invalid, and under no condition */
      }
#pragma unroll
      for (int q = 0; q < PROB_WORDS; ++q) {
        nvalid += (int32_t)((x[q] >> 16) & 1u);
#pragma unroll
        for (int c = 0; c < RS_PROB_MAX_CONDS; ++c) {
          if (c >= a.nconds) break;
          now[c] += (int32_t)((x[q] >> c) & 1u);
          by[c] += (int32_t)((x[q] >> (8 + c)) & 1u);
        }
      }
    }
    if (live) {
      double *cell = a.acc + ((int64_t)r * a.ngroups + g) * a.cols;
      cell[0] = (double)nvalid;
#pragma unroll
      for (int c = 0; c < RS_PROB_MAX_CONDS; ++c) {
        if (c >= a.nconds) break;
        cell[1 + c] = (double)now[c];
        cell[1 + a.nconds + c] = (double)by[c];
      }
    }
  }
}
}  // namespace

hipError_t rs_cluster_outputs_prob(const void *const src[6], const void *deficit, bool f32, const int32_t *order,
                                   const int32_t *table, const int32_t *inv, int64_t npoints, int64_t src_stride,
                                   int32_t nrows, const RsProbSpec &spec, int32_t *ever, uint32_t *words,
                                   int64_t wstride, double *acc_row0, hipStream_t stream) {
  const int32_t cols = rs_cluster_prob_cols(&spec);
  if (cols < 0 || nrows < 1 || npoints < 1 || wstride < npoints) return hipErrorInvalidValue;
  ProbBitsArgs b;
  for (int f = 0; f < 6; ++f) b.src[f] = src[f];
  b.src[6] = rs_cluster_prob_needs_deficit(&spec) == 1 ? deficit : nullptr;
  b.order = order;
  b.ever = ever;
  b.words = words;
  b.npoints = npoints;
  b.stride = src_stride;
  b.wstride = wstride;
  b.nrows = nrows;
  b.nconds = spec.nconds;
  for (int c = 0; c < RS_PROB_MAX_CONDS; ++c) b.cond[c] = spec.cond[c < spec.nconds ? c : 0];
  if (f32)
    hipLaunchKernelGGL(prob_bits_kernel<float>, grid1(npoints), dim3(RS_BLOCK), 0, stream, b);
  else
    hipLaunchKernelGGL(prob_bits_kernel<double>, grid1(npoints), dim3(RS_BLOCK), 0, stream, b);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  ProbCountArgs a;
  a.words = words;
  a.table = table;
  a.inv = inv;
  a.acc = acc_row0;
  a.npoints = npoints;
  a.wstride = wstride;
  a.nrows = nrows;
  a.ngroups = spec.ngroups;
  a.max_members = spec.max_members;
  a.nconds = spec.nconds;
  a.cols = cols;
  /* the grid of the ensemble statistics: the stations give x, blocks of rows y, several rounds of what the chip holds
   * at once, each workgroup with a whole number of rows per wavefront */
  const int64_t station_blocks = ((int64_t)spec.ngroups + 63) / 64;
  const int64_t want_row_blocks = std::max<int64_t>(1, 6144 / station_blocks);
  const int64_t rows_each = std::max<int64_t>(1, ((int64_t)nrows + want_row_blocks - 1) / want_row_blocks);
  a.rows_per_block = (int32_t)std::min<int64_t>(INT32_MAX / 2, (rows_each + PROB_WAVES - 1) / PROB_WAVES * PROB_WAVES);
  const int64_t row_blocks = ((int64_t)nrows + a.rows_per_block - 1) / a.rows_per_block;
  const dim3 grid((unsigned)station_blocks, (unsigned)row_blocks);
  const size_t lds = (size_t)64 * spec.max_members * sizeof(int32_t);
  hipLaunchKernelGGL(prob_count_kernel, grid, dim3(64 * PROB_WAVES), lds, stream, a);
  return hipGetLastError();
}

hipError_t rs_cluster_identity(int32_t *order, int64_t np_pad, hipStream_t stream) {
  hipLaunchKernelGGL(iota_kernel, grid1(np_pad), dim3(RS_BLOCK), 0, stream, order, np_pad);
  return hipGetLastError();
}

size_t rs_cluster_scratch_bytes(int64_t npoints) {
  size_t bytes = 0;
  uint32_t *k = nullptr;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, k, k, k, k, (int)npoints, 0, KEY_BITS);
  return bytes;
}

/* scratch: [4][np_pad] uint32 (keys in/out, slots in/out) + `tmp` for hipCUB.
 * Leaves the permutation (new slot -> old slot) in scratch + 3*np_pad. */
hipError_t rs_cluster_sort(const double *state, bool f32, int64_t np_pad, int64_t npoints,
                           uint32_t *scratch, void *tmp, size_t tmp_bytes, hipStream_t stream) {
  uint32_t *kin = scratch, *kout = scratch + np_pad, *sin = scratch + 2 * np_pad,
           *sout = scratch + 3 * np_pad;
  if (f32)
    hipLaunchKernelGGL(keys_kernel<float>, grid1(npoints), dim3(RS_BLOCK), 0, stream,
                       reinterpret_cast<const float *>(state), np_pad, npoints, kin, sin);
  else
    hipLaunchKernelGGL(keys_kernel<double>, grid1(npoints), dim3(RS_BLOCK), 0, stream, state, np_pad,
                       npoints, kin, sin);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  /* stable: points with equal scores keep their relative order */
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, kin, kout, sin, sout, (int)npoints, 0,
                                            KEY_BITS, stream);
}

/* ---- the plan's own sort: one stable counting pass -----------------------------------------
 * The forecast key of the default field set is short - something on the road (1 bit), unstable
 * previews and table-path previews (2 bits each for the two or three previews of a window), predicted
 * extra passes saturating at 31 (5 bits), storage class (2 bits): 12 bits - so ONE counting pass
 * sorts it, in three small kernels instead of the 17 of the library's merge sort:
 *   cs_hist     a histogram per tile of CS_TILE keys (LDS atomics): H[tile][bin]
 *   cs_binscan  one lane per bin: exclusive prefix of its counts over the tiles, in place, and the
 *               bin's total (every access a coalesced row of H)
 *   cs_scatter  one wavefront per tile: scans the bins' totals (where every bin starts), start of
 *               (bin, tile) = the bin's start + its tile prefix;
 *               then it walks its keys in order, and the rank of a key among the equal keys of
 *               its 64 is a popcount of ballots - equal keys keep their order (stable, deterministic:
 *               no atomic decides a position, no workgroup waits for another)
 * perm_out[new slot] = old slot, as the library sort's value output. */
namespace {
constexpr int CS_TILE = 1024;

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, off, 64);
    if (lane >= (uint32_t)off) v += u;
  }
  return v;
}

/* via: the permutation an earlier (less significant) pass left - this pass takes its keys in that order
 * (NULL: in slot order); shift: where this pass's digit starts in the key */
__global__ void __launch_bounds__(256) cs_hist_kernel(const uint32_t *__restrict__ keys,
                                                      const uint32_t *__restrict__ via, int64_t n, int shift,
                                                      int nbins, int ntiles, uint32_t *__restrict__ H) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a plan: little work, all of it waited for */
  extern __shared__ uint32_t cs_h[];
  /* (the two loops over the bins stay rolled and the tile's keys are addressed by a 32-bit offset from the tile's
   * uniform base: the kernel has to fit in the 32 registers per lane that five step wavefronts leave on a SIMD) */
#pragma unroll 1
  for (int b = threadIdx.x; b < nbins; b += 256) cs_h[b] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * CS_TILE;
  const int64_t left = n - base;
  const uint32_t cnt = left < CS_TILE ? (uint32_t)left : (uint32_t)CS_TILE; /* (a tile is never empty) */
  const uint32_t *vt = via ? via + base : nullptr;
#pragma unroll
  for (uint32_t i = threadIdx.x; i < (uint32_t)CS_TILE; i += 256)
    if (i < cnt) atomicAdd(&cs_h[(keys[vt ? (int64_t)vt[i] : base + i] >> shift) & (uint32_t)(nbins - 1)], 1u);
  __syncthreads();
  uint32_t *Ht = H + (int64_t)blockIdx.x * nbins;
#pragma unroll 1
  for (int b = threadIdx.x; b < nbins; b += 256) Ht[b] = cs_h[b];
}

/* one lane per bin: walks the tiles in order (coalesced rows of H[tile][bin]), leaves the bin's
 * exclusive prefix over the tiles in place and its total in T[bin] */
__global__ void __launch_bounds__(64) cs_binscan_kernel(uint32_t *H, uint32_t *T, int nbins, int ntiles,
                                                        uint32_t *class_total, int class_shift) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a plan: little work, all of it waited for */
  const int bin = (int)blockIdx.x * 64 + (int)threadIdx.x;
  uint32_t run = 0u;
  if (bin < nbins) {
#pragma unroll 8
    for (int t = 0; t < ntiles; ++t) {
      const uint32_t v = H[(int64_t)t * nbins + bin];
      H[(int64_t)t * nbins + bin] = run;
      run += v;
    }
    T[bin] = run;
  }
  /* for the wave table (cs_wave_table_kernel): the keys per CLASS, class = bin >> class_shift.  A
   * workgroup's 64 bins belong to one class (class_shift >= 6): one atomic per workgroup */
  if (class_total) {
    uint32_t sum = run;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += (uint32_t)__shfl_xor((int)sum, off, 64);
    if (threadIdx.x == 0 && (int)blockIdx.x * 64 < nbins) atomicAdd(&class_total[((int)blockIdx.x * 64) >> class_shift], sum);
  }
}

__global__ void __launch_bounds__(64) cs_scatter_kernel(const uint32_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ via, int64_t n,
                                                        int shift, int nbits, int ntiles,
                                                        const uint32_t *__restrict__ H,
                                                        const uint32_t *__restrict__ T,
                                                        uint32_t *__restrict__ perm_out) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a plan: little work, all of it waited for */
  extern __shared__ uint32_t cs_cur[];
  const int nbins = 1 << nbits;
  const uint32_t lane = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * CS_TILE;
  /* where every bin starts for this tile: the bin's start - the exclusive scan of the bins' totals,
   * which every wavefront forms for itself, a row of 64 bins at a time (64 independent coalesced loads,
   * a wavefront scan per row and the carry of the rows before: cheaper than a launch of its own, and no
   * workgroup waits for another) - plus its prefix over the tiles before this one (cs_binscan) */
  {
    /* the rows' loads are issued a batch at a time (round 3 issued them one row at a time, behind the
     * scan of the row before: 64 L2 round trips in a row, 80 of the kernel's 85 us on a 62 500-point
     * plan, where nothing else hides them) */
    constexpr int ROWS = 8;
    uint32_t carry = 0u;
    for (int r0 = 0; r0 < nbins; r0 += 64 * ROWS) {
      uint32_t tv[ROWS], hv[ROWS];
#pragma unroll
      for (int q = 0; q < ROWS; ++q) {
        const int b = r0 + q * 64 + (int)lane;
        tv[q] = b < nbins ? T[b] : 0u;
        hv[q] = b < nbins ? H[(int64_t)blockIdx.x * nbins + b] : 0u;
      }
#pragma unroll
      for (int q = 0; q < ROWS; ++q) {
        const int b = r0 + q * 64 + (int)lane;
        const uint32_t incl = wave_incl_scan(tv[q], lane);
        if (b < nbins) cs_cur[b] = carry + incl - tv[q] + hv[q];
        carry += (uint32_t)__shfl((int)incl, 63, 64);
      }
    }
  }
  __syncthreads();
  /* the keys of CS_BATCH rounds are fetched together (a load per round would put 64 memory round trips
   * behind one another), but no more: the kernel has to fit beside the step kernels' wavefronts, which
   * leave few vector registers free on a SIMD (64 keys in registers: 193 VGPRs, 0.5 ms per sort) */
  constexpr int CS_BATCH = 4;
  /* (a key's place in the tile as a 32-bit offset beside the tile's uniform base: `cnt` keys, never none) */
  const int64_t left = n - base;
  const uint32_t cnt = left < CS_TILE ? (uint32_t)left : (uint32_t)CS_TILE;
  const uint32_t *vt = via ? via + base : nullptr;
  for (int r0 = 0; r0 < CS_TILE / 64; r0 += CS_BATCH) {
    if ((uint32_t)r0 * 64u >= cnt) break; /* uniform: behind the last key */
    uint32_t kreg[CS_BATCH], sreg[CS_BATCH];
#pragma unroll
    for (int q = 0; q < CS_BATCH; ++q) {
      const uint32_t off = (uint32_t)(r0 + q) * 64u + lane;
      sreg[q] = (off < cnt && vt) ? vt[off] : (uint32_t)base + off;
    }
#pragma unroll
    for (int q = 0; q < CS_BATCH; ++q) {
      const uint32_t off = (uint32_t)(r0 + q) * 64u + lane;
      kreg[q] = off < cnt ? ((keys[sreg[q]] >> shift) & (uint32_t)(nbins - 1)) : 0u;
    }
#pragma unroll
  for (int q = 0; q < CS_BATCH; ++q) {
    const bool valid = (uint32_t)(r0 + q) * 64u + lane < cnt;
    const uint32_t key = kreg[q];
    unsigned long long same = __ballot(valid);
    for (int bit = 0; bit < nbits; ++bit) {
      const bool one = (key >> bit) & 1u;
      const unsigned long long b = __ballot(one);
      same &= one ? b : ~b;
    }
    const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    uint32_t start = 0u;
    if (valid) {
      start = cs_cur[key];
      perm_out[start + rank] = sreg[q];
    }
    /* every lane has read its cursor before the first of its group moves it: the workgroup is ONE
     * wavefront, whose LDS accesses execute in program order - a scheduling fence for the compiler is
     * all it takes (a __syncthreads() here also waits for the scattered store above: 64 memory round
     * trips per tile, measured 0.5 ms per sort) */
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0u) cs_cur[key] = start + (uint32_t)__popcll(same);
    __builtin_amdgcn_wave_barrier();
  }
  }
}
}  // namespace

/* Wave table for the two-wavefront flavour (rs_kernels.hip, step_kernel_duo): wavefront w steps the slots
 * [start[w], start[w] + cnt[w]).  A CLASS = the slots whose sort key shares its class_bits most significant
 * bits (cover, unstable previews, table-path previews for the default key): every class starts a wavefront of
 * its own, so that no wavefront mixes two classes - the slowest wavefront of a small shard's launch is a MIXED
 * one (tools/bl_makespan.py), and the launch is as long as its slowest wavefront.  The slot space is
 * untouched (windows, state, order rows stay dense); only the kernel's wave -> slot mapping changes, at the
 * price of at most one partly filled wavefront per class.  One workgroup of 64 lanes: lane c takes the
 * keys of class c (counted by cs_binscan_kernel), two wavefront scans give every class its first slot and
 * first wavefront. */
__global__ void __launch_bounds__(64) cs_wave_table_kernel(uint32_t *__restrict__ class_total,
                                                           int class_bits, int32_t *__restrict__ wstart,
                                                           int32_t *__restrict__ wcnt, int32_t maxw) {
  __builtin_amdgcn_s_setprio(3); /* a link of the chain between two step launches of a plan: little work, all of it waited for */
  const uint32_t lane = threadIdx.x;
  const int nclasses = 1 << class_bits;
  uint32_t n = 0u;
  if ((int)lane < nclasses) {
    n = class_total[lane]; /* left by cs_binscan_kernel */
    class_total[lane] = 0u; /* ... and zero again for the next sort */
  }
  const uint32_t waves = (n + 63u) >> 6;
  const uint32_t sbase = wave_incl_scan(n, lane) - n, wbase = wave_incl_scan(waves, lane) - waves;
  uint32_t total = 0u;
  for (int c = 0; c < nclasses; ++c) {
    const uint32_t nc = (uint32_t)__shfl((int)n, c, 64), sb = (uint32_t)__shfl((int)sbase, c, 64),
                   wb = (uint32_t)__shfl((int)wbase, c, 64), wc = (nc + 63u) >> 6;
    for (uint32_t k = lane; k < wc; k += 64u) {
      const uint32_t idx = wb + k;
      if ((int32_t)idx < maxw) {
        wstart[idx] = (int32_t)(sb + 64u * k);
        const uint32_t left = nc - 64u * k;
        wcnt[idx] = (int32_t)(left < 64u ? left : 64u);
      }
    }
    total = wb + wc;
  }
  for (uint32_t idx = total + lane; (int32_t)idx < maxw; idx += 64u) { /* the launch's spare wavefronts */
    wstart[idx] = 0;
    wcnt[idx] = 0;
  }
}

/* class_total: the counters rs_cluster_count_sort filled (64 x uint32, zero before the sort; zero again after) */
hipError_t rs_cluster_wave_table(int class_bits, uint32_t *class_total, int32_t *wstart, int32_t *wcnt,
                                 int32_t maxw, hipStream_t stream) {
  if (class_bits < 1 || class_bits > 6 || !class_total) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cs_wave_table_kernel, dim3(1), dim3(64), 0, stream, class_total, class_bits, wstart, wcnt, maxw);
  return hipGetLastError();
}

size_t rs_cluster_count_scratch_bytes(int64_t npoints, int nbits) {
  const int64_t ntiles = (npoints + CS_TILE - 1) / CS_TILE;
  return ((size_t)(1 << nbits) * (size_t)ntiles + (size_t)(1 << nbits)) * sizeof(uint32_t);
}

/* keys in scratch[0..npoints) (values < 2^(nbits + low_bits)), permutation out to scratch + 3*np_pad.
 * low_bits > 0: the key carries a second, less significant digit below its nbits - sorted first, by a pass
 * of its own whose permutation (scratch + np_pad) the main pass reads its keys through: two stable passes,
 * least significant digit first. */
hipError_t rs_cluster_count_sort(int64_t np_pad, int64_t npoints, int nbits, uint32_t *scratch, void *tmp,
                                 size_t tmp_bytes, hipStream_t stream, uint32_t *class_total, int class_bits,
                                 int low_bits) {
  if (nbits < 1 || nbits > 12 || low_bits < 0 || low_bits > 12 ||
      tmp_bytes < rs_cluster_count_scratch_bytes(npoints, nbits > low_bits ? nbits : low_bits))
    return hipErrorInvalidValue;
  const int ntiles = (int)((npoints + CS_TILE - 1) / CS_TILE);
  uint32_t *H = static_cast<uint32_t *>(tmp);
  const uint32_t *via = nullptr;
  if (low_bits > 0) {
    const int nb = 1 << low_bits;
    uint32_t *T = H + (size_t)nb * ntiles;
    hipLaunchKernelGGL(cs_hist_kernel, dim3(ntiles), dim3(256), nb * sizeof(uint32_t), stream, scratch, via,
                       npoints, 0, nb, ntiles, H);
    hipLaunchKernelGGL(cs_binscan_kernel, dim3((nb + 63) / 64), dim3(64), 0, stream, H, T, nb, ntiles,
                       (uint32_t *)nullptr, 0);
    hipLaunchKernelGGL(cs_scatter_kernel, dim3(ntiles), dim3(64), nb * sizeof(uint32_t), stream, scratch, via,
                       npoints, 0, low_bits, ntiles, H, T, scratch + np_pad);
    via = scratch + np_pad;
  }
  const int nbins = 1 << nbits;
  uint32_t *T = H + (size_t)nbins * ntiles;
  hipLaunchKernelGGL(cs_hist_kernel, dim3(ntiles), dim3(256), nbins * sizeof(uint32_t), stream, scratch, via,
                     npoints, low_bits, nbins, ntiles, H);
  /* classes of at least 64 bins only (a workgroup of the bin scan = one class) */
  const bool classes = class_total && class_bits >= 1 && nbits - class_bits >= 6;
  hipLaunchKernelGGL(cs_binscan_kernel, dim3((nbins + 63) / 64), dim3(64), 0, stream, H, T, nbins, ntiles,
                     classes ? class_total : nullptr, nbits - class_bits);
  hipLaunchKernelGGL(cs_scatter_kernel, dim3(ntiles), dim3(64), nbins * sizeof(uint32_t), stream, scratch, via,
                     npoints, low_bits, nbits, ntiles, H, T, scratch + 3 * np_pad);
  return hipGetLastError();
}

hipError_t rs_cluster_sort_keys(int64_t np_pad, int64_t npoints, uint32_t *scratch, void *tmp,
                                size_t tmp_bytes, hipStream_t stream) {
  uint32_t *kin = scratch, *kout = scratch + np_pad, *sin = scratch + 2 * np_pad,
           *sout = scratch + 3 * np_pad;
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, kin, kout, sin, sout, (int)npoints, 0,
                                            KEY_BITS, stream);
}

namespace {
__global__ void __launch_bounds__(RS_BLOCK) again_flags_kernel(const double *__restrict__ state,
                                                               int64_t np_pad, int64_t npoints,
                                                               int32_t *flags, int32_t *iota) {
  const int64_t p = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (p >= npoints) return;
  flags[p] = ((int32_t)state[(int64_t)RS_ST_CPL_FLAGS * np_pad + p]) & 1; /* start_coupling_again */
  iota[p] = (int32_t)p;
}
}  // namespace

size_t rs_cpl_select_scratch_bytes(int64_t npoints) {
  size_t bytes = 0;
  int32_t *x = nullptr;
  (void)hipcub::DeviceSelect::Flagged(nullptr, bytes, x, x, x, x, (int)npoints);
  return bytes;
}

/* flags: scratch int32[2*npoints] (flags, then the identity list to select from) */
hipError_t rs_cpl_select_again(const double *state, int64_t np_pad, int64_t npoints, int32_t *flags,
                               int32_t *list, int32_t *count_dev, void *tmp, size_t tmp_bytes,
                               hipStream_t stream) {
  int32_t *iota = flags + npoints;
  hipLaunchKernelGGL(again_flags_kernel, grid1(npoints), dim3(RS_BLOCK), 0, stream, state, np_pad,
                     npoints, flags, iota);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceSelect::Flagged(tmp, tmp_bytes, iota, flags, list, count_dev, (int)npoints, stream);
}

/* nlayers: NLayers of the plan; cpl_rows: 0 no coupling block, 1 the coupling scalars only (every
 * coupling window is behind the plan: nothing reads the saved state any more), 2 everything */
static RowMap row_map(int nlayers, int cpl_rows) {
  RowMap rows;
  rows.nlayers = nlayers;
  rows.nscal = RS_ST_BLSCORE - RS_ST_TNW1 + 1;
  rows.ncpl = cpl_rows >= 1 ? RS_ST_CPL_RESUME - RS_ST_CPL_ITER + 1 : 0;
  rows.nsave = cpl_rows >= 2 ? RS_ST_CPL_SAVE_ALBEDO - RS_ST_CPL_SAVE_TSURF + 1 : 0;
  return rows;
}

hipError_t rs_cluster_inverse(const int32_t *order, int64_t npoints, int32_t *inv, hipStream_t stream) {
  hipLaunchKernelGGL(inverse_kernel, grid1(npoints), dim3(RS_BLOCK), 0, stream, order, npoints, inv);
  return hipGetLastError();
}

/* the rows a re-sort of src would move (nlayers, cpl_rows as below), from src's slots into dst's */
hipError_t rs_cluster_fanout(const double *state_src, double *state_dst, bool f32, const int32_t *order_dst,
                             const int32_t *parent, const int32_t *inv_src, int64_t np_pad_src, int64_t npoints_src,
                             int64_t np_pad_dst, int64_t npoints_dst, int nlayers, int cpl_rows, hipStream_t stream) {
  dim3 g = grid1(npoints_dst);
  const RowMap rows = row_map(nlayers, cpl_rows);
  g.y = (unsigned)rows.total();
  if (f32)
    hipLaunchKernelGGL(fanout_kernel<float>, g, dim3(RS_BLOCK), 0, stream, reinterpret_cast<const float *>(state_src),
                       reinterpret_cast<float *>(state_dst), order_dst, parent, inv_src, np_pad_src, npoints_src,
                       np_pad_dst, npoints_dst, rows);
  else
    hipLaunchKernelGGL(fanout_kernel<double>, g, dim3(RS_BLOCK), 0, stream, state_src, state_dst, order_dst, parent,
                       inv_src, np_pad_src, npoints_src, np_pad_dst, npoints_dst, rows);
  return hipGetLastError();
}

hipError_t rs_cluster_apply(const double *state_src, double *state_dst, bool f32,
                            const int32_t *order_src, int32_t *order_dst, const uint32_t *perm,
                            int64_t np_pad, int64_t npoints, int nlayers, int cpl_rows,
                            hipStream_t stream) {
  dim3 g = grid1(np_pad);
  const RowMap rows = row_map(nlayers, cpl_rows);
  g.y = (unsigned)rows.total();
  if (f32)
    hipLaunchKernelGGL(apply_kernel<float>, g, dim3(RS_BLOCK), 0, stream,
                       reinterpret_cast<const float *>(state_src), reinterpret_cast<float *>(state_dst),
                       order_src, order_dst, perm, np_pad, npoints, rows);
  else
    hipLaunchKernelGGL(apply_kernel<double>, g, dim3(RS_BLOCK), 0, stream, state_src, state_dst,
                       order_src, order_dst, perm, np_pad, npoints, rows);
  return hipGetLastError();
}
