// sfc_gen::convexCover with the voxel map itself instead of its surface points (the map-side counterpart of the points
// overload in sfc_gen.hpp, kept apart so that sfc_gen.hpp builds next to either voxel map header):
//     sfc_gen::convexCover(path, voxelMap, voxelMap.getOrigin(), voxelMap.getCorner(), progress, range, hpolys, eps);
// The per-segment selection runs on the device over the map's surface points (anet_voxel_gather_boxes_dev); only the
// selected points come back to the host for the FIRI batch.  The header also carries sfc_gen::planPath on the map (the
// route search at the top of LearningPlanner::plan), further down.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sfc_gen.hpp"
#include "voxel_map.hpp"

namespace sfc_gen {

// the result is that of the points overload called with map.getSurf(points)
template <typename V3, typename Poly>
inline void convexCover(const std::vector<V3> &path, const voxel_map::VoxelMap &map, const V3 &lowCorner,
                        const V3 &highCorner, const double &progress, const double &range, std::vector<Poly> &hpolys,
                        const double eps = 1.0e-6) {
  hpolys.clear();
  std::vector<double> A, Bv, bd;
  const int S = detail::cover_segments(path, lowCorner, highCorner, progress, range, A, Bv, bd);
  if (S == 0) return;
  anet::Context &ctx = anet::Context::thread_default();
  const double *pts = map.surf_points_dev();
  const int64_t n = map.surf_size();
  void *st = anet_stream(ctx.get());
  double *d_bd = nullptr, *d_work = nullptr, *d_cnt = nullptr, *d_pc = nullptr;
  std::vector<double> cbuf(((size_t)S + 1) / 2), pc;
  std::vector<int32_t> cnt((size_t)S);
  size_t Np = 1;
  int rc = anet_dev_alloc(ctx.get(), bd.size(), &d_bd);
  if (rc == ANET_OK) rc = anet_dev_alloc(ctx.get(), (size_t)(anet_voxel_gather_workspace(S, n) + 7) / 8, &d_work);
  if (rc == ANET_OK) rc = anet_dev_alloc(ctx.get(), cbuf.size(), &d_cnt);
  if (rc == ANET_OK) rc = anet_dev_upload(ctx.get(), d_bd, bd.data(), bd.size());
  // counting pass, then the write pass into [S][Np][3] with Np the largest count, as the points overload pads
  if (rc == ANET_OK) rc = anet_voxel_gather_boxes_dev(ctx.get(), S, d_bd, pts, n, 0, d_work, nullptr, (int32_t *)d_cnt, st);
  if (rc == ANET_OK) rc = anet_dev_download(ctx.get(), cbuf.data(), d_cnt, cbuf.size());
  if (rc == ANET_OK) {
    std::memcpy(cnt.data(), cbuf.data(), sizeof(int32_t) * S);
    for (int k = 0; k < S; ++k) Np = std::max(Np, (size_t)cnt[k]);
    pc.assign((size_t)S * Np * 3, 0.0);
    rc = anet_dev_alloc(ctx.get(), pc.size(), &d_pc);
  }
  if (rc == ANET_OK) rc = anet_voxel_gather_boxes_dev(ctx.get(), S, d_bd, pts, n, (int64_t)Np, d_work, d_pc, (int32_t *)d_cnt, st);
  if (rc == ANET_OK) rc = anet_dev_download(ctx.get(), pc.data(), d_pc, pc.size());
  for (double *p : {d_bd, d_work, d_cnt, d_pc}) anet_dev_free(p);
  ctx.check(rc);
  std::vector<std::vector<double>> sel(S);
  for (int k = 0; k < S; ++k)
    sel[k].assign(pc.begin() + (size_t)k * Np * 3, pc.begin() + ((size_t)k * Np + cnt[k]) * 3);
  detail::cover_finish(S, A, Bv, bd, sel, Np, eps, hpolys);
}

}  // namespace sfc_gen

namespace sfc_gen {

// planPath(s, g, lb, hb, mapPtr, timeout, p) as learning_planner.hpp calls it when the route is empty: a collision-free
// polyline from s to g over the free voxels of [lb, hb] into p, its length returned.  The search runs on the device
// (anet_voxel_path_*: a shortest-path field, a walk back along it, a line-of-sight shortcut; the semantics are in
// allocnet_amd.h).  It is exact and deterministic, so `timeout` bounds nothing.  When g cannot be reached the path ends at
// the reached voxel centre nearest to g (OMPL's planners report such approximate solutions as solved too).  A start that
// is not free returns INFINITY and leaves p as it was.  The map's workspace is allocated per call.
template <typename VS, typename VG, typename VL, typename VH, typename V3>
inline double planPath(const VS &s, const VG &g, const VL &lb, const VH &hb, const voxel_map::VoxelMap *mapPtr,
                       const double &timeout, std::vector<V3> &p) {
  (void)timeout;
  anet::Context &ctx = anet::Context::thread_default();
  const anet_voxel_grid &grid = mapPtr->grid();
  const uint8_t *vox = mapPtr->voxels_dev();
  const double box[6] = {lb(0), lb(1), lb(2), hb(0), hb(1), hb(2)};
  const double sg[6] = {s(0), s(1), s(2), g(0), g(1), g(2)};
  const int64_t ws = anet_voxel_path_workspace(&grid, 1);
  if (ws < 0) throw anet::Error(ANET_ERR_UNSUPPORTED, "sfc_gen::planPath: the map has too many voxels for the search");
  void *st = anet_stream(ctx.get());
  double *d_work = nullptr, *d_sg = nullptr, *d_meta = nullptr, *d_path = nullptr;
  double meta[2] = {0.0, 0.0};  // {n_points, status} as two int32, then the cost
  int32_t np = 0, status = 0;
  int64_t cap = 256;
  int32_t rounds = 0;
  int rc = anet_dev_alloc(ctx.get(), (size_t)(ws + 7) / 8, &d_work);
  if (rc == ANET_OK) rc = anet_dev_alloc(ctx.get(), 6, &d_sg);
  if (rc == ANET_OK) rc = anet_dev_alloc(ctx.get(), 2, &d_meta);
  if (rc == ANET_OK) rc = anet_dev_upload(ctx.get(), d_sg, sg, 6);
  if (rc == ANET_OK) rc = anet_voxel_path_field_dev(ctx.get(), &grid, vox, box, d_sg, 1, d_work, &rounds, st);
  for (int pass = 0; pass < 2 && rc == ANET_OK; ++pass) {  // a second pass only when the path has more than `cap` points
    anet_dev_free(d_path);
    d_path = nullptr;
    rc = anet_dev_alloc(ctx.get(), (size_t)cap * 3, &d_path);
    if (rc == ANET_OK)
      rc = anet_voxel_path_extract_dev(ctx.get(), &grid, vox, box, d_sg, d_sg + 3, 1, d_work, cap, d_path, (int32_t *)d_meta,
                                       d_meta + 1, (int32_t *)d_meta + 1, st);
    if (rc == ANET_OK) rc = anet_dev_download(ctx.get(), meta, d_meta, 2);
    std::memcpy(&np, &meta[0], sizeof(np));
    std::memcpy(&status, (const char *)&meta[0] + sizeof(np), sizeof(status));
    if (np <= cap) break;
    cap = np;
  }
  std::vector<double> pts((size_t)np * 3);
  if (rc == ANET_OK && status >= 0 && np > 0) rc = anet_dev_download(ctx.get(), pts.data(), d_path, pts.size());
  for (double *q : {d_work, d_sg, d_meta, d_path}) anet_dev_free(q);
  ctx.check(rc);
  if (status < 0) throw anet::Error(ANET_ERR_INVALID, "sfc_gen::planPath: the walk found no predecessor");
  if (status == ANET_PATH_INVALID_START) return INFINITY;
  p.clear();
  for (int32_t i = 0; i < np; ++i) p.emplace_back(pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2]);
  return meta[1];
}

}  // namespace sfc_gen
