// The exact distance field of the voxel map, its query and the obstacle penalty of the MINCO objective (include/allocnet_amd.h).
#include <algorithm>

#include "api_internal.h"
#include "minco_core.h"  // with_order
#include "distance_kernels.h"

static_assert(anet::kObsMaxPieces == ANET_MAX_PIECES, "the LDS image of k_minco_obstacle holds ANET_MAX_PIECES pieces");
static_assert(anet::kDistNone == ANET_DIST_NONE, "the sentinel of the kernels is the header's");
static_assert(anet::kDistXCap >= anet::kDistMaxAxis && anet::kDistAxisCap >= 2 * anet::kDistMaxAxis + 2, "a line of the longest axis fits");

namespace {

// oc = origin + 0.5 scale, as voxel_map.hpp's constructor forms it
bool dist_grid_of(const anet_voxel_grid *g, anet::DistGrid *out) {
#pragma clang fp contract(off)
  if (!voxel_grid_ok(g)) return false;
  for (int c = 0; c < 3; ++c) {
    out->size[c] = g->size[c];
    out->oc[c] = g->origin[c] + 0.5 * g->scale;
  }
  out->scale = g->scale;
  return true;
}

int check_obstacle_penalty(anet_ctx *ctx, const anet_obstacle_penalty *q) {
  if (!q) return fail(ctx, ANET_ERR_INVALID, "anet_obstacle_penalty is NULL");
  if (!(q->w >= 0.0) || !(q->w < INFINITY)) return fail(ctx, ANET_ERR_INVALID, "anet_obstacle_penalty.w must be finite and >= 0");
  if (!(q->smooth_mu > 0.0) || !(q->smooth_mu < INFINITY))
    return fail(ctx, ANET_ERR_INVALID, "anet_obstacle_penalty.smooth_mu must be finite and > 0");
  if (!(fabs(q->clearance) < INFINITY)) return fail(ctx, ANET_ERR_INVALID, "anet_obstacle_penalty.clearance must be finite");
  if (q->res < 1) return fail(ctx, ANET_ERR_INVALID, "anet_obstacle_penalty.res must be >= 1");
  return ANET_OK;
}

// the tile width of an axis pass: the largest power of two with tx * L int32 and two flag words in the LDS tile, at most kDistAxisMaxTx and not wider
// than the map needs
int axis_tile_log2(int sx, int L) {
  int lg = 0;
  while ((2 << lg) * (int64_t)L + 2 <= anet::kDistAxisCap && (2 << lg) <= anet::kDistAxisMaxTx && (1 << lg) < sx) ++lg;
  return lg;
}

}  // namespace

extern "C" {

int anet_voxel_distance_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *voxels, int walls, int32_t *sd2,
                            void *stream) {
  ANET_ON_DEVICE(ctx);
  if (!voxel_grid_ok(grid)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_distance_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (!voxels || !sd2) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_distance_dev: NULL pointer");
  const int sx = grid->size[0], sy = grid->size[1], sz = grid->size[2];
  if (sx > anet::kDistMaxAxis || sy > anet::kDistMaxAxis || sz > anet::kDistMaxAxis)
    return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_voxel_distance_dev: an axis longer than 4096 voxels");
  hipStream_t st = (hipStream_t)stream;
  const int w = walls ? 1 : 0;
  const int64_t n_lines = (int64_t)sy * sz;
  const int rows = std::max(1, anet::kDistXRun / sx);  // rows * sx <= kDistXRun, or one line of at most kDistXCap
  hipLaunchKernelGGL(anet::k_vox_dist_x, dim3((unsigned)((n_lines + rows - 1) / rows)), dim3(anet::kDistXBlock), 0, st, voxels, sd2, sx,
                     n_lines, rows, w);
  ANET_HIP(ctx, hipGetLastError());
  const int64_t sxy = (int64_t)sx * sy;
  // y: the lines of plane z, sx apart; z: the lines of row y, sx * sy apart.  A pass over an axis of one voxel still runs when the
  // walls stand next to it.
  if (sy > 1 || w) {
    const int lg = axis_tile_log2(sx, sy);
    hipLaunchKernelGGL(anet::k_vox_dist_axis, dim3((unsigned)((sx + (1 << lg) - 1) >> lg), (unsigned)sz), dim3(anet::kDistAxisBlock), 0,
                       st, sd2, sx, sy, (int64_t)sx, sxy, lg, w);
    ANET_HIP(ctx, hipGetLastError());
  }
  if (sz > 1 || w) {
    const int lg = axis_tile_log2(sx, sz);
    hipLaunchKernelGGL(anet::k_vox_dist_axis, dim3((unsigned)((sx + (1 << lg) - 1) >> lg), (unsigned)sy), dim3(anet::kDistAxisBlock), 0,
                       st, sd2, sx, sz, sxy, (int64_t)sx, lg, w);
    ANET_HIP(ctx, hipGetLastError());
  }
  return ANET_OK;
}

int anet_voxel_distance_query_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const int32_t *sd2, const double *pos, int64_t n,
                                  double *dist, double *grad, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::DistGrid g;
  if (!dist_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_distance_query_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (n < 0) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_distance_query_dev: n < 0");
  if (n == 0) return ANET_OK;
  if (!sd2 || !pos || !dist) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_distance_query_dev: NULL pointer");
  hipLaunchKernelGGL(anet::k_vox_dist_query, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, sd2, pos, n, dist,
                     grad);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_minco_obstacle_partial_grads_dev(anet_ctx *ctx, const anet_obstacle_penalty *pen, int s, int n_pieces, int64_t batch,
                                          int64_t ld, const double *coeffs, const double *T, const anet_voxel_grid *grid,
                                          const int32_t *sd2, int accumulate, double *gdC, double *gdT, double *piece_cost,
                                          void *stream) {
  ANET_ON_DEVICE(ctx);
  if (s < 2 || s > 4) return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_minco_obstacle_partial_grads_dev: order s must be 2, 3 or 4");
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_obstacle_penalty(ctx, pen))) return rc;
  anet::DistGrid g;
  if (!dist_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_minco_obstacle_partial_grads_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (batch > INT32_MAX) return fail(ctx, ANET_ERR_INVALID, "anet_minco_obstacle_partial_grads_dev: batch too large");
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !sd2 || !gdC || !gdT || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_obstacle_partial_grads_dev: NULL pointer or ld < batch");
  anet::ObstacleArgs a{coeffs, T, sd2, gdC, gdT, piece_cost, batch, ld, n_pieces, pen->res, accumulate ? 1 : 0, pen->w, pen->smooth_mu,
                       pen->clearance, g};
  const dim3 grd((unsigned)batch), block(anet::kObsBlock);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_minco_obstacle<decltype(o)::value>, grd, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

}  // extern "C"
