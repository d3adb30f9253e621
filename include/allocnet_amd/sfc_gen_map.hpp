// sfc_gen::convexCover with the voxel map itself instead of its surface points (the map-side counterpart of the points
// overload in sfc_gen.hpp, kept apart so that sfc_gen.hpp builds next to either voxel map header):
//     sfc_gen::convexCover(path, voxelMap, voxelMap.getOrigin(), voxelMap.getCorner(), progress, range, hpolys, eps);
// The per-segment selection runs on the device over the map's surface points (anet_voxel_gather_boxes_dev); only the
// selected points come back to the host for the FIRI batch.
#pragma once
#include <algorithm>
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
