// The log-odds occupancy grid from sensor scans, depth unprojection and the first-hit ray query; exploration goals on that grid:
// frontier mask, connected components of a byte grid, view gain (include/allocnet_amd.h).
#include <algorithm>
#include <cmath>

#include "api_internal.h"
#include "occupancy_kernels.h"
#include "frontier_kernels.h"

extern "C" {

static bool occ_grid_of(const anet_voxel_grid *g, anet::OccGrid *out) {
  if (!voxel_grid_ok(g)) return false;
  out->sx = g->size[0]; out->sy = g->size[1]; out->sz = g->size[2];
  out->scale = g->scale;
  for (int c = 0; c < 3; ++c) out->o[c] = g->origin[c];
  return true;
}
static int64_t occ_count(const anet::OccGrid &g) { return (int64_t)g.sx * g.sy * g.sz; }
// the marks: a byte per voxel, rounded up so that the word form may OR whole 32-bit words
static int64_t occ_mark_bytes(int64_t n) { return round_up(n, 256); }

static bool occ_params_of(const anet_occupancy_params *p, const anet::OccGrid &g, anet::OccParams *out) {
  if (!p) return false;
  if (p->hit <= 0 || p->miss >= 0 || p->lo < -32767 || p->lo >= 0 || p->hi <= 0 || p->hi > 32767) return false;
  if (!(p->min_range >= 0.0) || !(p->min_range < INFINITY)) return false;
  if (!(p->max_range > 0.0) || !(p->max_range < INFINITY) || !(p->max_range / g.scale <= (double)anet::kOccMaxSpan)) return false;
  *out = anet::OccParams{p->hit, p->miss, p->lo, p->hi, p->min_range, p->max_range};
  return true;
}

int64_t anet_occupancy_workspace(const anet_voxel_grid *grid) {
  anet::OccGrid g;
  if (!occ_grid_of(grid, &g)) return -1;
  return occ_mark_bytes(occ_count(g));
}

int anet_occupancy_reset_dev(anet_ctx *ctx, const anet_voxel_grid *grid, int16_t *logodds, void *work, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::OccGrid g;
  if (!occ_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_reset_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (!logodds || !work) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_reset_dev: NULL pointer");
  const int64_t n = occ_count(g), nm = occ_mark_bytes(n);
  hipLaunchKernelGGL(anet::k_occ_reset, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, logodds,
                     (uint8_t *)work, nm);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_occupancy_integrate_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const anet_occupancy_params *params, int16_t *logodds,
                                 const double origin[3], const void *records, int64_t n, int64_t stride, int f64, void *work,
                                 void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::OccScan s;
  if (!occ_grid_of(grid, &s.g)) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_integrate_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (!occ_params_of(params, s.g, &s.prm))
    return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_integrate_dev: hit > 0 > miss, -32767 <= lo < 0 < hi <= 32767, finite min_range >= 0, "
                                       "finite max_range > 0 with max_range / scale <= 65536");
  int oc[3];
  if (!origin) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_integrate_dev: NULL origin");
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(origin[c]) || !anet::occ_cell(s.g, origin[c], c, oc[c]))
      return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_integrate_dev: the sensor origin must be finite and its cell index below 2^30 in magnitude");
    s.o[c] = origin[c];
  }
  const int64_t esz = f64 ? 8 : 4;
  if (n < 0 || (f64 != 0 && f64 != 1) || stride < 3 * esz || stride % esz)
    return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_integrate_dev: n >= 0, f64 in {0, 1}, stride >= 3 elements and a multiple of one");
  if (n == 0) return ANET_OK;
  if (!logodds || !work || !records || (uintptr_t)records % esz) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_integrate_dev: NULL or misaligned pointer");
  s.rec = (const uint8_t *)records;
  s.n = n; s.stride = stride; s.f64 = f64;
  hipStream_t st = (hipStream_t)stream;
  const dim3 rays((unsigned)((n + 255) / 256));
  if (anet::env_set(anet::Tuning::occ_marks_atomic)) {
    hipLaunchKernelGGL(anet::k_occ_mark_atomic, rays, dim3(256), 0, st, s, (uint32_t *)work);
    ANET_HIP(ctx, hipGetLastError());
  } else {
    hipLaunchKernelGGL(anet::k_occ_carve, rays, dim3(256), 0, st, s, (uint8_t *)work);
    ANET_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(anet::k_occ_hit, rays, dim3(256), 0, st, s, (uint8_t *)work);
    ANET_HIP(ctx, hipGetLastError());
  }
  // the cells within ceil(max_range / scale) + 1 of the sensor's cell, cut to the map: every end point is within max_range (1 + a
  // few ulp) of the origin, so its cell is at most that far from the origin's
  const int64_t reach = (int64_t)std::ceil(s.prm.max_range / s.g.scale) + 1;
  const int size[3] = {s.g.sx, s.g.sy, s.g.sz};
  anet::OccBox bx;
  int64_t cells = 1;
  for (int c = 0; c < 3; ++c) {
    const int64_t lo = std::max<int64_t>((int64_t)oc[c] - reach, 0), hi = std::min<int64_t>((int64_t)oc[c] + reach, size[c] - 1);
    if (hi < lo) return ANET_OK;  // the sensor is farther from the map than it sees: nothing was marked
    bx.lo[c] = (int)lo;
    bx.ext[c] = (int)(hi - lo + 1);
    cells *= bx.ext[c];
  }
  hipLaunchKernelGGL(anet::k_occ_update, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, s.g, s.prm, bx, logodds,
                     (uint8_t *)work);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_occupancy_integrate(anet_ctx *ctx, const anet_voxel_grid *grid, const anet_occupancy_params *params, int16_t *logodds,
                             const double origin[3], const void *records, int64_t n, int64_t stride, int f64, void *work) {
  ANET_ON_DEVICE(ctx);
  if (n < 0 || stride < 12 || stride >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31))
    return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_integrate: 0 <= n < 2^31, 12 <= stride < 2^31");
  if (n > 0 && !records) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_integrate: NULL records");
  void *d = nullptr;
  if (n > 0) {
    // (the last record may end with its third coordinate: only what the kernels read is copied)
    const size_t bytes = (size_t)((n - 1) * stride + 3 * (f64 ? 8 : 4));
    const int rc = ensure_scratch(ctx, bytes);
    if (rc != ANET_OK) return rc;
    d = ctx->scratch;
    ANET_HIP(ctx, hipMemcpyAsync(d, records, bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  const int rc = anet_occupancy_integrate_dev(ctx, grid, params, logodds, origin, d ? d : records, n, stride, f64, work, ctx->stream);
  if (rc != ANET_OK) return rc;
  ANET_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANET_OK;
}

int anet_occupancy_to_voxels_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const int16_t *logodds, int32_t occ, int unknown_blocked,
                                 uint8_t *voxels, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::OccGrid g;
  if (!occ_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_to_voxels_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (!logodds || !voxels) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_to_voxels_dev: NULL pointer");
  const int64_t n = occ_count(g);
  hipLaunchKernelGGL(anet::k_occ_to_voxels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, logodds, occ,
                     unknown_blocked, voxels);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_depth_to_points_dev(anet_ctx *ctx, const void *depth, int u16, int width, int height, int step, double depth_scale,
                             const double K[4], const double R[9], const double t[3], double min_depth, double max_depth,
                             double *points, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (width < 1 || height < 1 || step < 1 || (int64_t)width * height >= ((int64_t)1 << 31) || (u16 != 0 && u16 != 1))
    return fail(ctx, ANET_ERR_INVALID, "anet_depth_to_points_dev: width, height, step >= 1, fewer than 2^31 pixels, u16 in {0, 1}");
  if (!depth || !K || !R || !t || !points || (uintptr_t)depth % (u16 ? 2 : 4))
    return fail(ctx, ANET_ERR_INVALID, "anet_depth_to_points_dev: NULL or misaligned pointer");
  if (std::isnan(min_depth) || std::isnan(max_depth) || std::isnan(depth_scale))
    return fail(ctx, ANET_ERR_INVALID, "anet_depth_to_points_dev: NaN depth_scale, min_depth or max_depth");
  anet::DepthCam cam;
  cam.fx = K[0]; cam.fy = K[1]; cam.cx = K[2]; cam.cy = K[3];
  for (int i = 0; i < 9; ++i) cam.R[i] = R[i];
  for (int i = 0; i < 3; ++i) cam.t[i] = t[i];
  cam.depth_scale = depth_scale; cam.min_depth = min_depth; cam.max_depth = max_depth;
  cam.width = width; cam.height = height; cam.step = step;
  cam.nu = (width + step - 1) / step; cam.nv = (height + step - 1) / step;
  cam.u16 = u16;
  const int64_t n = (int64_t)cam.nu * cam.nv;
  hipLaunchKernelGGL(anet::k_depth_to_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cam, depth, points);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_voxel_raycast_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *voxels, const double *origins, const double *ends,
                           int64_t n, int32_t *voxel, double *t, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::OccGrid g;
  if (!occ_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_raycast_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (n < 0) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_raycast_dev: n < 0");
  if (n == 0) return ANET_OK;
  if (!voxels || !origins || !ends || !voxel) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_raycast_dev: NULL pointer");
  hipLaunchKernelGGL(anet::k_voxel_raycast, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, voxels, origins,
                     ends, n, voxel, t);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

// ---- exploration goals: frontier, components, view gain (frontier_kernels.h) -----------------------------------------------------

int anet_occupancy_frontier_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const int16_t *logodds, int32_t occ, const int32_t box_lo[3],
                                const int32_t box_ext[3], uint8_t *mask, int64_t *count_dev, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::OccGrid g;
  if (!occ_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_frontier_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (!logodds || !mask) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_frontier_dev: NULL pointer");
  if ((box_lo == nullptr) != (box_ext == nullptr)) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_frontier_dev: box_lo and box_ext are both NULL or both given");
  anet::OccBox bx{{0, 0, 0}, {g.sx, g.sy, g.sz}};
  if (box_lo) {
    const int size[3] = {g.sx, g.sy, g.sz};
    for (int c = 0; c < 3; ++c) {
      if (box_lo[c] < 0 || box_ext[c] < 1 || (int64_t)box_lo[c] + box_ext[c] > size[c])
        return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_frontier_dev: the box must lie inside the map (lo >= 0, ext >= 1, lo + ext <= size)");
      bx.lo[c] = box_lo[c];
      bx.ext[c] = box_ext[c];
    }
  }
  hipStream_t st = (hipStream_t)stream;
  if (count_dev) ANET_HIP(ctx, hipMemsetAsync(count_dev, 0, sizeof(int64_t), st));
  const int64_t n = occ_count(g);
  hipLaunchKernelGGL(anet::k_occ_frontier, dim3((unsigned)std::min<int64_t>((n + 255) / 256, anet::kFrontierBlocks)), dim3(256), 0, st, g, bx, logodds, occ, mask,
                     (unsigned long long *)count_dev);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

static bool label_grid_of(const anet_voxel_grid *grid, anet::LabelGrid *out) {
  if (!voxel_grid_ok(grid)) return false;
  out->sx = grid->size[0]; out->sy = grid->size[1]; out->sz = grid->size[2];
  out->ntx = (out->sx + anet::kLabelTX - 1) / anet::kLabelTX;
  out->nty = (out->sy + anet::kLabelTY - 1) / anet::kLabelTY;
  out->ntz = (out->sz + anet::kLabelTZ - 1) / anet::kLabelTZ;
  return true;
}

int64_t anet_voxel_components_workspace(const anet_voxel_grid *grid) {
  if (!voxel_grid_ok(grid)) return -1;
  return anet::voxel_components_ws(nullptr, (int64_t)grid->size[0] * grid->size[1] * grid->size[2]).bytes;
}

int anet_voxel_label_components_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *mask, int connectivity, int32_t *labels,
                                    void *work, int32_t *rounds_host, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::LabelGrid g;
  if (!label_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_label_components_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (connectivity != 6 && connectivity != 26) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_label_components_dev: connectivity is 6 or 26");
  if (!mask || !labels || !work || (uintptr_t)work % 8) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_label_components_dev: NULL or misaligned pointer");
  const int rc = ensure_counter(ctx);
  if (rc != ANET_OK) return rc;
  const int64_t n = (int64_t)g.sx * g.sy * g.sz, n_tiles = (int64_t)g.ntx * g.nty * g.ntz;
  const anet::VoxCompWs W = anet::voxel_components_ws(work, n);
  const int n_fwd = connectivity == 6 ? 3 : 13;
  hipStream_t st = (hipStream_t)stream;
  ANET_HIP(ctx, hipMemsetAsync(W.changed, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(anet::k_vox_label_tile, dim3((unsigned)std::min<int64_t>(n_tiles, (int64_t)1 << 22)), dim3(256), 0, st, g, mask,
                     n_fwd, labels);
  ANET_HIP(ctx, hipGetLastError());
  // A round: the unions across tile borders, then every label to its root.  The word holds the last round that linked anything;
  // it is read once per group of rounds, and the labels are settled when the last round issued linked nothing.  Every round that
  // links lowers a label, so n + 1 rounds bound the loop whatever the input (one linking round is what the algorithm needs).
  const dim3 per_voxel((unsigned)((n + 255) / 256));
  int32_t r = 0, last = 0;
  for (;;) {
    for (int k = 0; k < anet::kLabelRoundGroup; ++k) {
      ++r;
      hipLaunchKernelGGL(anet::k_vox_label_merge, per_voxel, dim3(256), 0, st, g, n_fwd, labels, W.changed, r);
      ANET_HIP(ctx, hipGetLastError());
      hipLaunchKernelGGL(anet::k_vox_label_flatten, per_voxel, dim3(256), 0, st, n, labels);
      ANET_HIP(ctx, hipGetLastError());
    }
    ANET_HIP(ctx, hipMemcpyAsync(ctx->h_counter, W.changed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ANET_HIP(ctx, hipStreamSynchronize(st));
    last = ctx->h_counter[0];
    if (last < r) break;
    if ((int64_t)r > n) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_label_components_dev: round cap reached");
  }
  if (rounds_host) *rounds_host = r;  // the rounds that ran (the last linking one was round `last`)
  return ANET_OK;
}

int anet_voxel_component_stats_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const int32_t *labels, int32_t max_components,
                                   int32_t *n_components_dev, int32_t *root, int32_t *count, int64_t *sum_xyz, int32_t *bbox, void *work,
                                   void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::LabelGrid g;
  if (!label_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_component_stats_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (max_components < 0) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_component_stats_dev: max_components < 0");
  if (!labels || !n_components_dev || !work || (uintptr_t)work % 8 || (max_components > 0 && (!root || !count || !sum_xyz || !bbox)))
    return fail(ctx, ANET_ERR_INVALID, "anet_voxel_component_stats_dev: NULL or misaligned pointer");
  const int64_t n = (int64_t)g.sx * g.sy * g.sz;
  const anet::VoxCompWs W = anet::voxel_components_ws(work, n);
  const anet::CompStats s{max_components, root, count, bbox, (unsigned long long *)sum_xyz};
  hipStream_t st = (hipStream_t)stream;
  const dim3 blocks((unsigned)W.n_blocks), threads(anet::kCompScanBlock);
  hipLaunchKernelGGL(anet::k_vox_root_count, blocks, threads, 0, st, n, labels, W.blocks);
  ANET_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(anet::k_vox_root_scan, dim3(1), dim3(256), 0, st, W.n_blocks, W.blocks, n_components_dev);
  ANET_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(anet::k_vox_root_rank, blocks, threads, 0, st, n, labels, W.blocks, W.rank, s);
  ANET_HIP(ctx, hipGetLastError());
  if (max_components > 0) {
    hipLaunchKernelGGL(anet::k_vox_stats, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, labels, W.rank, s);
    ANET_HIP(ctx, hipGetLastError());
  }
  return ANET_OK;
}

// reach of a view: the scan's (the update box of anet_occupancy_integrate_dev)
static int64_t view_reach(const anet::OccParams &prm, const anet::OccGrid &g) { return (int64_t)std::ceil(prm.max_range / g.scale) + 1; }

static int64_t view_gain_bytes(const anet_voxel_grid *grid, const anet_occupancy_params *params, int64_t n_views) {
  anet::OccGrid g;
  anet::OccParams prm;
  if (!occ_grid_of(grid, &g) || !occ_params_of(params, g, &prm) || n_views < 0) return -1;
  return anet::view_gain_ws(nullptr, grid->size, view_reach(prm, g), n_views).bytes;
}
int64_t anet_occupancy_view_gain_workspace(const anet_voxel_grid *grid, const anet_occupancy_params *params, int32_t n_views) {
  return view_gain_bytes(grid, params, n_views);
}
int64_t anet_occupancy_view_gain_workspace_min(const anet_voxel_grid *grid, const anet_occupancy_params *params) {
  return view_gain_bytes(grid, params, 1);
}

int anet_occupancy_view_gain_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const anet_occupancy_params *params, const int16_t *logodds,
                                 int32_t occ, const double *view_R, const double *view_t, int32_t n_views, const double *pts,
                                 int32_t n_pts, int32_t *gain, void *work, int64_t work_bytes, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::ViewScan s;
  if (!occ_grid_of(grid, &s.g)) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_view_gain_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (!occ_params_of(params, s.g, &s.prm)) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_view_gain_dev: bad params (those of anet_occupancy_integrate_dev)");
  if (n_views < 0 || n_pts < 0) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_view_gain_dev: n_views >= 0, n_pts >= 0");
  if (n_views == 0) return ANET_OK;
  if (!logodds || !view_R || !view_t || !gain || !work || (n_pts > 0 && !pts) || (uintptr_t)work % 16)
    return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_view_gain_dev: NULL pointer, or work not aligned to 16 bytes");
  const int64_t reach = view_reach(s.prm, s.g);
  const int64_t slot = anet::view_gain_ws(nullptr, grid->size, reach, 1).slot;
  const int64_t fit = work_bytes / slot;
  if (work_bytes < 0 || fit < 1) return fail(ctx, ANET_ERR_INVALID, "anet_occupancy_view_gain_dev: work_bytes below anet_occupancy_view_gain_workspace_min()");
  // lanes of a launch: views * points < 2^31
  const int64_t lane_cap = (((int64_t)1 << 31) - 1) / std::max<int64_t>(n_pts, 1);
  const int64_t chunk = std::min<int64_t>({fit, (int64_t)n_views, std::max<int64_t>(lane_cap, 1), 65535});
  s.occ = occ; s.reach = (int)reach; s.pts = pts; s.n_pts = n_pts; s.slot = slot;
  hipStream_t st = (hipStream_t)stream;
  const unsigned pieces = (unsigned)std::min<int64_t>((slot / 16 + 255) / 256, 64);
  for (int64_t v0 = 0; v0 < n_views; v0 += chunk) {
    s.n_views = (int)std::min<int64_t>(chunk, n_views - v0);
    s.R = view_R + v0 * 9;
    s.t = view_t + v0 * 3;
    const int64_t lanes = std::max<int64_t>((int64_t)s.n_views * n_pts, s.n_views);
    hipLaunchKernelGGL(anet::k_occ_view_gain, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, s, logodds, (uint8_t *)work,
                       gain + v0);
    ANET_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(anet::k_occ_view_count, dim3(pieces, (unsigned)s.n_views), dim3(256), 0, st, s, (uint8_t *)work, gain + v0);
    ANET_HIP(ctx, hipGetLastError());
  }
  return ANET_OK;
}

}  // extern "C"
