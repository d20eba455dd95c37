/*
 * rs_grid.hip — gridded forcing gathered to points (include/roadsurf.h: rs_hip_gather_nodes; the definition, in
 * numpy: roadsurf_amd/grid.py gather_nodes).
 *
 * A weather model delivers fields [time][node]; the kernels of the driver path read raw series
 * [time][point].  Every point has a stencil of up to RS_GRID_MAX_STENCIL nodes and weights (bilinear, nearest,
 * a mask, an unstructured mesh: the caller's business), and
 *     dst[r][slot] = w0*src[r][n0] + w1*src[r][n1] + ...      over the terms whose weight is not 0.0,
 * every product and every sum rounded on its own, or `missing` where a term's node value is not > present_above
 * (NaN included), its node lies outside the field, or no term exists.
 *
 * One point per lane: the stencil is loaded once into registers, rows run in the loop and over blockIdx.y.  The
 * reads from `src` are scattered - neighbours along a road share nodes, the caches serve most of them - the
 * writes are whole lines; all offsets are 64-bit (n_times x n_nodes passes 2^31 at real sizes).  A node index is
 * compared with n_nodes before anything is loaded through it.
 */
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/roadsurf.h"
#include "rs_kernels.h"
#include "rs_step_select.hpp"

namespace {

struct GatherArgs {
  const double *src;
  const int32_t *node;
  const double *weight;
  const int32_t *order; /* slot -> point, or nullptr: point = slot */
  double *dst;
  int64_t n_nodes, src_stride, dst_stride, npoints;
  int32_t nrows, rows_per_block;
  double present_above, missing;
};

template <int ST>
__global__ void __launch_bounds__(RS_BLOCK) gather_nodes_kernel(const GatherArgs A) {
  const int64_t slot = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (slot >= A.npoints) return;
  const int64_t p = A.order ? (int64_t)A.order[slot] : slot;
  int64_t idx[ST];
  double w[ST];
  bool any = false, bad = false;
#pragma unroll
  for (int k = 0; k < ST; ++k) {
    w[k] = A.weight[p * ST + k];
    idx[k] = A.node[p * ST + k];
    if (w[k] != 0.0) { /* a term with weight 0.0 does not exist: its node is not looked at */
      any = true;
      bad = bad || idx[k] < 0 || idx[k] >= A.n_nodes;
    }
  }
  bad = bad || !any;
  const int32_t r0 = (int32_t)blockIdx.y * A.rows_per_block;
  const int32_t r1 = r0 + A.rows_per_block < A.nrows ? r0 + A.rows_per_block : A.nrows;
  double *out = A.dst + slot;
#pragma unroll 2
  for (int32_t r = r0; r < r1; ++r) {
    double v = A.missing;
    if (!bad) { /* every existing term's node lies inside [0, n_nodes) */
      const double *row = A.src + (int64_t)r * A.src_stride;
      bool ok = true, started = false;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < ST; ++k) {
        if (w[k] != 0.0) {
          const double a = row[idx[k]];
          ok = ok && a > A.present_above; /* NaN is absent */
          const double t = __dmul_rn(w[k], a);
          acc = started ? __dadd_rn(acc, t) : t; /* the first term as it is: 1.0 * -0.0 stays -0.0 */
          started = true;
        }
      }
      if (ok) v = acc;
    }
    out[(int64_t)r * A.dst_stride] = v;
  }
}

} // namespace

hipError_t rs_grid_gather(const double *src, int32_t nrows, int64_t n_nodes, int64_t src_stride, const int32_t *node,
                          const double *weight, int32_t stencil, const int32_t *order, double present_above,
                          double missing, double *dst, int64_t dst_stride, int64_t npoints, hipStream_t stream) {
  if (nrows < 1 || npoints < 1) return hipSuccess;
  if (stencil < 1 || stencil > RS_GRID_MAX_STENCIL) return hipErrorInvalidValue;
  GatherArgs a;
  a.src = src;
  a.node = node;
  a.weight = weight;
  a.order = order;
  a.dst = dst;
  a.n_nodes = n_nodes;
  a.src_stride = src_stride;
  a.dst_stride = dst_stride;
  a.npoints = npoints;
  a.nrows = nrows;
  a.present_above = present_above;
  a.missing = missing;
  /* blocks of points first; rows are cut over blockIdx.y only as far as it takes to fill the chip */
  const int64_t gx = (npoints + RS_BLOCK - 1) / RS_BLOCK;
  int64_t gy = (2048 + gx - 1) / gx;
  if (gy > nrows) gy = nrows;
  if (gy > 65535) gy = 65535;
  a.rows_per_block = (int32_t)((nrows + gy - 1) / gy);
  gy = (nrows + a.rows_per_block - 1) / a.rows_per_block;
  const dim3 g((unsigned)gx, (unsigned)gy), b(RS_BLOCK);
  switch (stencil) {
    case 1: hipLaunchKernelGGL(gather_nodes_kernel<1>, g, b, 0, stream, a); break;
    case 2: hipLaunchKernelGGL(gather_nodes_kernel<2>, g, b, 0, stream, a); break;
    case 3: hipLaunchKernelGGL(gather_nodes_kernel<3>, g, b, 0, stream, a); break;
    default: hipLaunchKernelGGL(gather_nodes_kernel<4>, g, b, 0, stream, a); break;
  }
  return hipGetLastError();
}
