// The exact first collision of a Trajectory<D> / Piece<D> with the device voxel map (anet_traj_voxel_hit; no counterpart in the
// reference, which never tests a trajectory against its map).  Kept apart from trajectory.hpp, as sfc_gen_map.hpp is from
// sfc_gen.hpp, so that trajectory.hpp does not depend on the map:
//     double t; int piece; voxel_map::Vec3i id;
//     if (getFirstCollision(traj, voxelMap, t, piece, id)) ...   // t: global time, piece: its index, id: the voxel entered
//     if (checkCollisionFree(traj, voxelMap)) ...
// Exact, not sampled: a curve that clips a voxel between two samples is found.  The curve is blocked where voxelMap.query(pos) is
// true: in a voxel != 0 or outside the map.  When it left the map (or the search was undecided: csrc/voxel_hit_kernels.h) there
// is no voxel to name and id is (-1, -1, -1); `code`, where asked for, tells the cases apart (ANET_HIT_*).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "trajectory.hpp"
#include "voxel_map.hpp"

namespace anet {
namespace detail {

inline voxel_map::Vec3i hit_voxel_id(const anet_voxel_grid &g, int32_t code) {
  if (code < 0) return voxel_map::Vec3i(-1, -1, -1);
  const int sx = g.size[0], sy = g.size[1];
  return voxel_map::Vec3i(code % sx, (code / sx) % sy, code / (sx * sy));
}

// n pieces of degree D (coefficients [n][3][D+1], durations [n]) -> true when some piece is not free; t in global time
template <int D>
inline bool first_collision(const std::vector<double> &co, const std::vector<double> &T, const voxel_map::VoxelMap &map, double &t,
                            int &piece, voxel_map::Vec3i &id, int *code) {
  const int n = (int)T.size();
  std::vector<double> th((size_t)n);
  std::vector<int32_t> vx((size_t)n);
  anet::Context &ctx = anet::Context::thread_default();
  const uint8_t *vox = map.voxels_dev();  // (flushes the map's buffered fills and waits for them)
  ctx.check(anet_traj_voxel_hit(ctx.get(), (D + 1) / 2, n, 1, co.data(), T.data(), &map.grid(), vox, th.data(), vx.data()));
  double start = 0.0;
  for (int i = 0; i < n; ++i) {
    if (!(th[(size_t)i] == INFINITY)) {  // a hit, or NaN: nothing is known from this piece's start on
      t = start + th[(size_t)i];
      piece = i;
      id = hit_voxel_id(map.grid(), vx[(size_t)i]);
      if (code) *code = vx[(size_t)i];
      return true;
    }
    start += T[(size_t)i];
  }
  t = INFINITY;
  piece = -1;
  id = voxel_map::Vec3i(-1, -1, -1);
  if (code) *code = ANET_HIT_FREE;
  return false;
}

}  // namespace detail
}  // namespace anet

// true when the trajectory is blocked somewhere: t its first global time there, piece the piece, id the voxel entered
template <int D>
inline bool getFirstCollision(const Trajectory<D> &traj, const voxel_map::VoxelMap &map, double &t, int &piece, voxel_map::Vec3i &id,
                              int *code = nullptr) {
  const int n = traj.getPieceNum();
  if (n < 1) throw anet::Error(ANET_ERR_INVALID, "getFirstCollision: empty trajectory");
  std::vector<double> co((size_t)n * 3 * (D + 1)), T((size_t)n);
  for (int i = 0; i < n; ++i) {
    T[(size_t)i] = traj[i].getDuration();
    const double *c = traj[i].getCoeffMat().data();
    for (int k = 0; k < 3 * (D + 1); ++k) co[(size_t)i * 3 * (D + 1) + k] = c[k];
  }
  return anet::detail::first_collision<D>(co, T, map, t, piece, id, code);
}

// one piece: t in its local time
template <int D>
inline bool getFirstCollision(const Piece<D> &pc, const voxel_map::VoxelMap &map, double &t, voxel_map::Vec3i &id, int *code = nullptr) {
  const double *c = pc.getCoeffMat().data();
  std::vector<double> co(c, c + 3 * (D + 1)), T(1, pc.getDuration());
  int piece = -1;
  return anet::detail::first_collision<D>(co, T, map, t, piece, id, code);
}

template <int D>
inline bool checkCollisionFree(const Trajectory<D> &traj, const voxel_map::VoxelMap &map) {
  double t;
  int piece;
  voxel_map::Vec3i id;
  return !getFirstCollision(traj, map, t, piece, id);
}
template <int D>
inline bool checkCollisionFree(const Piece<D> &pc, const voxel_map::VoxelMap &map) {
  double t;
  voxel_map::Vec3i id;
  return !getFirstCollision(pc, map, t, id);
}
