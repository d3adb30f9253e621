// The voxel map and the front-end route search on it (include/allocnet_amd.h).
#include <algorithm>
#include <cmath>

#include "api_internal.h"
#include "path_kernels.h"

extern "C" {

// ---- voxel map (csrc/voxel_kernels.h) -----------------------------------------------------------
static bool vox_grid_of(const anet_voxel_grid *g, anet::VoxGrid *out) {
#pragma clang fp contract(off)
  if (!voxel_grid_ok(g)) return false;
  out->sx = g->size[0]; out->sy = g->size[1]; out->sz = g->size[2];
  out->scale = g->scale;
  const int step[3] = {1, g->size[0], g->size[0] * g->size[1]};
  for (int c = 0; c < 3; ++c) {  // voxel_map.hpp's constructor: oc = o + 0.5 scale, stepScale = (1 / step) scale
    out->o[c] = g->origin[c];
    out->oc[c] = g->origin[c] + 0.5 * g->scale;
    out->ss[c] = (1.0 / (double)step[c]) * g->scale;
  }
  return true;
}
static int64_t vox_count(const anet::VoxGrid &g) { return (int64_t)g.sx * g.sy * g.sz; }
static int64_t comp_chunks(int64_t n) { return (n + anet::kCompChunk - 1) / anet::kCompChunk; }
// workspace: two fronts of a byte per voxel, then the per-chunk counts of the compaction
static int64_t vox_front_bytes(int64_t n) { return round_up(2 * n, 256); }

int anet_voxel_set_occupied_dev(anet_ctx *ctx, const anet_voxel_grid *grid, uint8_t *voxels, const void *records, int64_t n,
                                int64_t stride, int f64, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::VoxGrid g;
  if (!vox_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_set_occupied_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  const int64_t esz = f64 ? 8 : 4;
  if (n < 0 || (f64 != 0 && f64 != 1) || stride < 3 * esz || stride % esz)
    return fail(ctx, ANET_ERR_INVALID, "anet_voxel_set_occupied_dev: n >= 0, f64 in {0, 1}, stride >= 3 elements and a multiple of one");
  if (n == 0) return ANET_OK;
  if (!voxels || !records || (uintptr_t)records % esz) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_set_occupied_dev: NULL or misaligned pointer");
  hipLaunchKernelGGL(anet::k_voxel_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, voxels,
                     (const uint8_t *)records, n, stride, f64);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_voxel_set_occupied_ids_dev(anet_ctx *ctx, const anet_voxel_grid *grid, uint8_t *voxels, const int32_t *ids, int64_t n,
                                    void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::VoxGrid g;
  if (!vox_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_set_occupied_ids_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (n < 0) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_set_occupied_ids_dev: n < 0");
  if (n == 0) return ANET_OK;
  if (!voxels || !ids) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_set_occupied_ids_dev: NULL pointer");
  hipLaunchKernelGGL(anet::k_voxel_scatter_ids, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, voxels, ids, n);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int64_t anet_voxel_workspace(const anet_voxel_grid *grid) {
  anet::VoxGrid g;
  if (!vox_grid_of(grid, &g)) return -1;
  return vox_front_bytes(vox_count(g)) + 4 * comp_chunks(vox_count(g));
}

int anet_voxel_dilate_dev(anet_ctx *ctx, const anet_voxel_grid *grid, uint8_t *voxels, int r, void *work, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::VoxGrid g;
  if (!vox_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_dilate_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (r <= 0) return ANET_OK;  // voxel_map.hpp: no-op, the surface stays what it was
  if (!voxels || !work) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_dilate_dev: NULL pointer");
  const int64_t n = vox_count(g);
  uint8_t *front[2] = {(uint8_t *)work, (uint8_t *)work + n};
  const int64_t tx = (g.sx + anet::kDilTX - 1) / anet::kDilTX, ty = (g.sy + anet::kDilTY - 1) / anet::kDilTY,
                tz = (g.sz + anet::kDilTZ - 1) / anet::kDilTZ;
  hipStream_t st = (hipStream_t)stream;
  // round k writes front[(r - k) & 1], so the last round's front is front[0] whatever r is
  for (int k = 1; k <= r; ++k) {
    hipLaunchKernelGGL(anet::k_voxel_dilate_round, dim3((unsigned)(tx * ty * tz)), dim3(anet::kDilTX, anet::kDilTY), 0, st, g,
                       voxels, front[(r - k + 1) & 1], front[(r - k) & 1], k == 1 ? 1 : 0, tx, ty);
    ANET_HIP(ctx, hipGetLastError());
  }
  return ANET_OK;
}

int anet_voxel_surface_dev(anet_ctx *ctx, const anet_voxel_grid *grid, void *work, int64_t cap, int32_t *ids, int32_t *count,
                           void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::VoxGrid g;
  if (!vox_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_surface_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (cap < 0 || !work || !count || (cap > 0 && !ids)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_surface_dev: cap >= 0, NULL pointer");
  const int64_t n = vox_count(g), nc = comp_chunks(n);
  int32_t *counts = (int32_t *)((uint8_t *)work + vox_front_bytes(n));
  anet::FrontPred p{(const uint8_t *)work, ids};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(anet::k_compact_count<anet::FrontPred>, dim3((unsigned)nc), dim3(anet::kCompThreads), 0, st, p, n, nc, counts);
  ANET_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(anet::k_compact_scan, dim3(1), dim3(anet::kCompThreads), 0, st, counts, nc, count);
  ANET_HIP(ctx, hipGetLastError());
  if (cap > 0) {
    hipLaunchKernelGGL(anet::k_compact_write<anet::FrontPred>, dim3((unsigned)nc), dim3(anet::kCompThreads), 0, st, p, n, nc, counts, cap);
    ANET_HIP(ctx, hipGetLastError());
  }
  return ANET_OK;
}

int anet_voxel_surf_points_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const int32_t *ids, int64_t n, double *out,
                               void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::VoxGrid g;
  if (!vox_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_surf_points_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (n < 0) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_surf_points_dev: n < 0");
  if (n == 0) return ANET_OK;
  if (!ids || !out) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_surf_points_dev: NULL pointer");
  hipLaunchKernelGGL(anet::k_voxel_surf_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, ids, n, out);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_voxel_query_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *voxels, const double *pos, int64_t n,
                         uint8_t *out, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::VoxGrid g;
  if (!vox_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_query_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (n < 0) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_query_dev: n < 0");
  if (n == 0) return ANET_OK;
  if (!voxels || !pos || !out) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_query_dev: NULL pointer");
  hipLaunchKernelGGL(anet::k_voxel_query, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, voxels, pos, n, out);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int64_t anet_voxel_gather_workspace(int64_t n_boxes, int64_t n_points) {
  if (n_boxes < 0 || n_boxes > 65535 || n_points < 0 || n_points >= ((int64_t)1 << 31)) return -1;
  return 4 * (n_boxes * comp_chunks(n_points) + 1);
}

int anet_voxel_gather_boxes_dev(anet_ctx *ctx, int64_t n_boxes, const double *bd, const double *points, int64_t n_points,
                                int64_t max_points, void *work, double *out, int32_t *n_out, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (n_boxes < 0 || n_boxes > 65535 || n_points < 0 || n_points >= ((int64_t)1 << 31) || max_points < 0)
    return fail(ctx, ANET_ERR_INVALID, "anet_voxel_gather_boxes_dev: 0 <= n_boxes <= 65535, 0 <= n_points < 2^31, max_points >= 0");
  if (n_boxes == 0) return ANET_OK;
  if (!bd || !work || !n_out || (n_points > 0 && !points) || (max_points > 0 && !out))
    return fail(ctx, ANET_ERR_INVALID, "anet_voxel_gather_boxes_dev: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  if (n_points == 0) {
    ANET_HIP(ctx, hipMemsetAsync(n_out, 0, sizeof(int32_t) * n_boxes, st));
    return ANET_OK;
  }
  const int64_t nc = comp_chunks(n_points);
  int32_t *counts = (int32_t *)work;
  anet::BoxPred p{bd, points, out};
  const dim3 grid((unsigned)nc, (unsigned)n_boxes);
  hipLaunchKernelGGL(anet::k_compact_count<anet::BoxPred>, grid, dim3(anet::kCompThreads), 0, st, p, n_points, nc, counts);
  ANET_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(anet::k_compact_scan, dim3((unsigned)n_boxes), dim3(anet::kCompThreads), 0, st, counts, nc, n_out);
  ANET_HIP(ctx, hipGetLastError());
  if (max_points > 0) {
    hipLaunchKernelGGL(anet::k_compact_write<anet::BoxPred>, grid, dim3(anet::kCompThreads), 0, st, p, n_points, nc, counts, max_points);
    ANET_HIP(ctx, hipGetLastError());
  }
  return ANET_OK;
}

// ---- front-end route on the voxel map (csrc/path_kernels.h) -------------------------------------------------------------
// workspace: fields [B][n] uint32, walks [B][n + 1] int32, activity words [2][B][n_tiles], PathInfo [B], the "any" word
struct PathLayout {
  int64_t n, n_tiles, fields, walks, active, info, any, total;
  int tiles_x, tiles_y;
};
static bool path_layout(const anet::VoxGrid &g, int64_t B, PathLayout *L) {
  const int64_t n = vox_count(g);
  if (B < 1 || B > 65535 || 17 * n >= (int64_t)0xFFFFFFFF) return false;
  L->n = n;
  L->tiles_x = (g.sx + anet::kPathT - 1) / anet::kPathT;
  L->tiles_y = (g.sy + anet::kPathT - 1) / anet::kPathT;
  L->n_tiles = (int64_t)L->tiles_x * L->tiles_y * ((g.sz + anet::kPathT - 1) / anet::kPathT);
  L->fields = 0;
  L->walks = round_up(4 * B * n, 256);
  L->active = L->walks + round_up(4 * B * (n + 1), 256);
  L->info = L->active + round_up(4 * 2 * B * L->n_tiles, 256);
  L->any = L->info + round_up((int64_t)sizeof(anet::PathInfo) * B, 256);
  L->total = L->any + 256;
  return true;
}
static bool path_box_of(const double *box, anet::PathBox *out) {
  if (!box) return false;
  for (int c = 0; c < 3; ++c) {
    if (std::isnan(box[c]) || std::isnan(box[3 + c])) return false;
    out->lb[c] = box[c];
    out->hb[c] = box[3 + c];
  }
  return true;
}

int64_t anet_voxel_path_workspace(const anet_voxel_grid *grid, int64_t n_problems) {
  anet::VoxGrid g;
  PathLayout L;
  if (!vox_grid_of(grid, &g) || !path_layout(g, n_problems, &L)) return -1;
  return L.total;
}

int anet_voxel_path_field_ptr(const anet_voxel_grid *grid, void *work, int64_t b, uint32_t **field) {
  anet::VoxGrid g;
  PathLayout L;
  if (!vox_grid_of(grid, &g) || !path_layout(g, 1, &L) || !work || !field || b < 0)
    return fail(nullptr, ANET_ERR_INVALID, "anet_voxel_path_field_ptr: bad grid, NULL pointer or b < 0");
  *field = (uint32_t *)work + b * L.n;
  return ANET_OK;
}

int anet_voxel_path_field_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *voxels, const double box[6],
                              const double *starts, int64_t n_problems, void *work, int32_t *rounds, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::VoxGrid g;
  if (!vox_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_path_field_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  PathLayout L;
  if (n_problems < 1 || n_problems > 65535) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_path_field_dev: 1 <= n_problems <= 65535");
  if (!path_layout(g, n_problems, &L)) return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_voxel_path_field_dev: 17 * voxels must stay below 2^32 - 1");
  anet::PathBox bx;
  if (!voxels || !starts || !work || !path_box_of(box, &bx)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_path_field_dev: NULL pointer or NaN box");
  {
    const int rc = ensure_counter(ctx);
    if (rc != ANET_OK) return rc;
  }
  uint8_t *w = (uint8_t *)work;
  anet::PathArgs a{g, bx, voxels, starts, (uint32_t *)(w + L.fields), (uint32_t *)(w + L.active), (uint32_t *)(w + L.any),
                   L.n, L.n_tiles, L.tiles_x, L.tiles_y};
  hipStream_t st = (hipStream_t)stream;
  ANET_HIP(ctx, hipMemsetAsync(a.any, 0xFF, sizeof(uint32_t), st));
  const int64_t items = L.n > L.n_tiles ? L.n : L.n_tiles;
  const unsigned blocks = (unsigned)std::min<int64_t>((items + 255) / 256, 4096);
  hipLaunchKernelGGL(anet::k_path_init, dim3(blocks, (unsigned)n_problems), dim3(256), 0, st, a);
  ANET_HIP(ctx, hipGetLastError());
  // rounds go out in groups; the word copied after group k is read after group k + 1 is queued, so the device is never idle
  // waiting for the host.  A group issued after the field settled finds no active tile: its launches end after one load.
  const int64_t cap = 64 * L.n_tiles + 64;
  int64_t r = 0;
  uint32_t last = 0xFFFFFFFFu;
  bool done = false;
  for (int group = 0; !done; ++group) {
    for (int k = 0; k < anet::kPathRoundGroup; ++k, ++r) {
      hipLaunchKernelGGL(anet::k_path_relax, dim3((unsigned)L.n_tiles, (unsigned)n_problems), dim3(anet::kPathThreads), 0, st,
                         a, (uint32_t)r);
      ANET_HIP(ctx, hipGetLastError());
    }
    const int slot = group & 1;
    ANET_HIP(ctx, hipMemcpyAsync(ctx->h_counter + slot, a.any, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ANET_HIP(ctx, hipEventRecord(ctx->poll_ev[slot], st));
    if (group > 0) {
      ANET_HIP(ctx, hipEventSynchronize(ctx->poll_ev[slot ^ 1]));
      last = (uint32_t)ctx->h_counter[slot ^ 1];
      // the word holds the latest round some tile was stamped for; below the first round of group k + 1: settled
      if (last == 0xFFFFFFFFu || (int64_t)last < r - anet::kPathRoundGroup) done = true;
    }
    if (!done && r >= cap) {
      ANET_HIP(ctx, hipStreamSynchronize(st));
      last = (uint32_t)ctx->h_counter[slot];
      if (last != 0xFFFFFFFFu && (int64_t)last >= r) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_path_field_dev: round cap reached");
      done = true;
    }
  }
  ANET_HIP(ctx, hipStreamSynchronize(st));
  if (rounds) *rounds = last == 0xFFFFFFFFu ? 0 : (int32_t)last + 1;
  return ANET_OK;
}

int anet_voxel_path_extract_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *voxels, const double box[6],
                                const double *starts, const double *goals, int64_t n_problems, void *work, int64_t max_points,
                                double *paths, int32_t *n_points, double *cost, int32_t *status, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::VoxGrid g;
  if (!vox_grid_of(grid, &g)) return fail(ctx, ANET_ERR_INVALID, "anet_voxel_path_extract_dev: bad grid (size >= 1, voxels < 2^31, scale > 0)");
  PathLayout L;
  if (n_problems < 1 || n_problems > 65535 || max_points < 0 || max_points >= ((int64_t)1 << 31))
    return fail(ctx, ANET_ERR_INVALID, "anet_voxel_path_extract_dev: 1 <= n_problems <= 65535, 0 <= max_points < 2^31");
  if (!path_layout(g, n_problems, &L)) return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_voxel_path_extract_dev: 17 * voxels must stay below 2^32 - 1");
  anet::PathBox bx;
  if (!voxels || !starts || !goals || !work || !n_points || !cost || !status || (max_points > 0 && !paths) || !path_box_of(box, &bx))
    return fail(ctx, ANET_ERR_INVALID, "anet_voxel_path_extract_dev: NULL pointer or NaN box");
  uint8_t *w = (uint8_t *)work;
  anet::PathExtractArgs a{g, bx, voxels, starts, goals, (const uint32_t *)(w + L.fields), (int32_t *)(w + L.walks),
                          (anet::PathInfo *)(w + L.info), L.n, max_points, paths, n_points, status, cost};
  hipStream_t st = (hipStream_t)stream;
  const unsigned B = (unsigned)n_problems;
  hipLaunchKernelGGL(anet::k_path_goal, dim3(B), dim3(64), 0, st, a);
  ANET_HIP(ctx, hipGetLastError());
  const unsigned chunks = (unsigned)((L.n + 256 * anet::kPathScanItems - 1) / (256 * anet::kPathScanItems));
  hipLaunchKernelGGL(anet::k_path_nearest<0>, dim3(chunks, B), dim3(256), 0, st, a);
  ANET_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(anet::k_path_nearest<1>, dim3(chunks, B), dim3(256), 0, st, a);
  ANET_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(anet::k_path_walk, dim3(B), dim3(64), 0, st, a);
  ANET_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(anet::k_path_shortcut, dim3(B), dim3(anet::kPathShortcutThreads), 0, st, a);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

}  // extern "C"
