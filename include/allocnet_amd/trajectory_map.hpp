// The exact first collision of a Trajectory<D> / Piece<D> with the device voxel map (anet_traj_voxel_hit; no counterpart in the
// reference, which never tests a trajectory against its map).  Kept apart from trajectory.hpp, as sfc_gen_map.hpp is from
// sfc_gen.hpp, so that trajectory.hpp does not depend on the map:
//     double t; int piece; voxel_map::Vec3i id;
//     if (getFirstCollision(traj, voxelMap, t, piece, id)) ...   // t: global time, piece: its index, id: the voxel entered
//     if (checkCollisionFree(traj, voxelMap)) ...
// Exact, not sampled: a curve that clips a voxel between two samples is found.  The curve is blocked where voxelMap.query(pos) is
// true: in a voxel != 0 or outside the map.  When it left the map (or the search was undecided: csrc/voxel_hit_kernels.h) there
// is no voxel to name and id is (-1, -1, -1); `code`, where asked for, tells the cases apart (ANET_HIT_*).
//
// The exact clearance to obstacle points (anet_traj_clearance; no counterpart in the reference either):
//     double t; int piece, point;
//     double d = getClearance(traj, points, t, piece, point);   // points: std::vector<anet::Vec3>, or the map: its surface
//     if (checkClearance(traj, voxelMap, 0.3)) ...               // every piece keeps 0.3 m from every surface point
// d is the smallest distance in metres over the whole trajectory, t its global time, piece its piece and point the index of the
// nearest point; +inf (t 0, piece -1, point -1) without a finite point, NaN when a piece has a non-finite coefficient.
//
// The whole body in the corridor (anet_traj_body_margin; upstream GCOPTER's SE(3) constraint, no counterpart in the reference):
//     std::vector<anet::Vec3> verts = ...;                        // body vertices in the body frame, at most ANET_MAX_BODY_VERTS
//     double m = getBodyMargin(traj, flatmap, verts, hPolys, 20);  // max of a_r . (p(t) + R(q(t)) b_k) - h_r, piece i against hPolys[i]
//     if (checkBodyCorridor(traj, flatmap, verts, hPolys, 20)) ...
// q(t) is the attitude flatmap.forward gives at the trajectory's v, a, j with psi = 0.  A SAMPLED check: res + 1 samples per piece.
//
// Stop within known space (anet_traj_stop_margin; no counterpart in the reference): on a map whose blocked set is occupied or
// unknown (OccupancyMap::toVoxelMap), can the vehicle come to rest inside free space from every sample of the trajectory?
//     double t; int piece;
//     double m = getStopMargin(traj, voxelMap, 5.0, 0.1, 0.3, 20, t, piece);  // a_brake 5 m/s^2, t_react 0.1 s, clearance 0.3 m
//     if (checkStoppable(traj, voxelMap, 5.0, 0.1, 0.3, 20)) ...
// m is the least  d(p) - clearance - t_react |v| - v.v / (2 a_brake)  over res + 1 samples of every piece, d the map's distance field
// with walls (VoxelMap::distanceField), t its global time and piece its piece; NaN (t the start of that piece) when a piece has a
// non-finite coefficient or duration.  A SAMPLED check, and the ball form: the direction of v is not used.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "flatness.hpp"
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

namespace anet {
namespace detail {

// n pieces of degree D against one shared cloud -> the smallest clearance; t in global time.  A NaN piece makes the answer NaN.
template <int D>
inline double clearance(const std::vector<double> &co, const std::vector<double> &T, const std::vector<anet::Vec3> &points, double &t,
                        int &piece, int &point) {
  const int n = (int)T.size();
  std::vector<double> pts(points.size() * 3), cl((size_t)n), tt((size_t)n);
  std::vector<int32_t> pi((size_t)n);
  for (size_t j = 0; j < points.size(); ++j)
    for (int c = 0; c < 3; ++c) pts[j * 3 + (size_t)c] = points[j](c);
  anet::Context &ctx = anet::Context::thread_default();
  ctx.check(anet_traj_clearance(ctx.get(), (D + 1) / 2, n, 1, co.data(), T.data(), 1, (int64_t)points.size(), pts.data(), nullptr,
                                cl.data(), pi.data(), tt.data()));
  double best = INFINITY, start = 0.0;
  t = 0.0;
  piece = point = -1;
  for (int i = 0; i < n; ++i) {
    const double c = cl[(size_t)i];
    if (c != c) {  // nothing is known about this piece
      t = 0.0;
      piece = i;
      point = -1;
      return c;
    }
    if (c < best) {
      best = c;
      t = start + tt[(size_t)i];
      piece = i;
      point = pi[(size_t)i];
    }
    start += T[(size_t)i];
  }
  return best;
}

template <int D>
inline void pack_pieces(const Trajectory<D> &traj, const char *who, std::vector<double> &co, std::vector<double> &T) {
  const int n = traj.getPieceNum();
  if (n < 1) throw anet::Error(ANET_ERR_INVALID, who);
  co.resize((size_t)n * 3 * (D + 1));
  T.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    T[(size_t)i] = traj[i].getDuration();
    const double *c = traj[i].getCoeffMat().data();
    for (int k = 0; k < 3 * (D + 1); ++k) co[(size_t)i * 3 * (D + 1) + k] = c[k];
  }
}

inline std::vector<anet::Vec3> surface_of(const voxel_map::VoxelMap &map) {
  std::vector<anet::Vec3> pts;
  map.getSurf(pts);
  return pts;
}

}  // namespace detail
}  // namespace anet

// the smallest distance of the trajectory to the points: t its global time, piece the piece, point the nearest point's index
template <int D>
inline double getClearance(const Trajectory<D> &traj, const std::vector<anet::Vec3> &points, double &t, int &piece, int &point) {
  std::vector<double> co, T;
  anet::detail::pack_pieces<D>(traj, "getClearance: empty trajectory", co, T);
  return anet::detail::clearance<D>(co, T, points, t, piece, point);
}
template <int D>
inline double getClearance(const Trajectory<D> &traj, const voxel_map::VoxelMap &map, double &t, int &piece, int &point) {
  return getClearance(traj, anet::detail::surface_of(map), t, piece, point);
}
// one piece: t in its local time
template <int D>
inline double getClearance(const Piece<D> &pc, const std::vector<anet::Vec3> &points, double &t, int &point) {
  const double *c = pc.getCoeffMat().data();
  std::vector<double> co(c, c + 3 * (D + 1)), T(1, pc.getDuration());
  int piece = -1;
  return anet::detail::clearance<D>(co, T, points, t, piece, point);
}
template <int D>
inline double getClearance(const Piece<D> &pc, const voxel_map::VoxelMap &map, double &t, int &point) {
  return getClearance(pc, anet::detail::surface_of(map), t, point);
}

// true when the clearance is at least min_dist (NaN: false)
template <int D, class PointsOrMap>
inline bool checkClearance(const Trajectory<D> &traj, const PointsOrMap &points, double min_dist) {
  double t;
  int piece, point;
  return getClearance(traj, points, t, piece, point) >= min_dist;
}
template <int D, class PointsOrMap>
inline bool checkClearance(const Piece<D> &pc, const PointsOrMap &points, double min_dist) {
  double t;
  int point;
  return getClearance(pc, points, t, point) >= min_dist;
}

// The sampled body margin: the maximum over the pieces, res + 1 samples of each, the rows of hPolys[i] (one M_i x 4 matrix per piece:
// rows() and operator()(r, c)) and the body vertices; per_piece (may be null) receives the N margins.  -inf: no row at all.
template <int D, class HPoly>
inline double getBodyMargin(const Trajectory<D> &traj, const flatness::FlatnessMap &flatmap, const std::vector<anet::Vec3> &verts,
                            const std::vector<HPoly> &hPolys, int res = 20, double *per_piece = nullptr) {
  std::vector<double> co, T;
  anet::detail::pack_pieces<D>(traj, "getBodyMargin: empty trajectory", co, T);
  if (hPolys.size() != T.size()) throw anet::Error(ANET_ERR_INVALID, "getBodyMargin: one polytope per piece");
  if (verts.empty() || verts.size() > (size_t)ANET_MAX_BODY_VERTS)
    throw anet::Error(ANET_ERR_INVALID, "getBodyMargin: 1 to ANET_MAX_BODY_VERTS body vertices");
  int M = 1;
  for (const auto &h : hPolys) M = std::max(M, (int)h.rows());
  std::vector<double> rows(hPolys.size() * (size_t)M * 4, 0.0);
  for (size_t i = 0; i < hPolys.size(); ++i)
    for (int r = 0; r < (int)hPolys[i].rows(); ++r)
      for (int c = 0; c < 4; ++c) rows[(i * M + r) * 4 + c] = hPolys[i](r, c);
  anet_body_penalty pen = {};
  pen.w_body = 0.0;
  pen.smooth_mu = 1.0;
  pen.res = res;
  pen.poly_rows = M;
  pen.n_verts = (int32_t)verts.size();
  for (size_t k = 0; k < verts.size(); ++k)
    for (int c = 0; c < 3; ++c) pen.verts[k][c] = verts[k](c);
  std::vector<double> m(T.size());
  anet::Context &ctx = anet::Context::thread_default();
  ctx.check(anet_traj_body_margin(ctx.get(), &flatmap.params(), &pen, (D + 1) / 2, (int)T.size(), 1, co.data(), T.data(), rows.data(),
                                  m.data(), nullptr, nullptr, nullptr));
  double best = m[0];
  for (size_t i = 0; i < m.size(); ++i) {
    if (m[i] != m[i]) best = m[i];  // nothing is known about this piece
    else if (best == best && m[i] > best) best = m[i];
    if (per_piece) per_piece[i] = m[i];
  }
  return best;
}
// true when every sampled body vertex stays within tol of its piece's polytope (NaN: false)
template <int D, class HPoly>
inline bool checkBodyCorridor(const Trajectory<D> &traj, const flatness::FlatnessMap &flatmap, const std::vector<anet::Vec3> &verts,
                              const std::vector<HPoly> &hPolys, int res = 20, double tol = 0.0) {
  return getBodyMargin(traj, flatmap, verts, hPolys, res) <= tol;
}

// The sampled stop margin: the minimum over the pieces, res + 1 samples of each, on map.distanceField(true); t its global time
template <int D>
inline double getStopMargin(const Trajectory<D> &traj, const voxel_map::VoxelMap &map, double a_brake, double t_react, double clearance,
                            int res, double &t, int &piece) {
  std::vector<double> co, T;
  anet::detail::pack_pieces<D>(traj, "getStopMargin: empty trajectory", co, T);
  anet_stop_penalty pen = {};
  pen.smooth_mu = 1.0;
  pen.clearance = clearance;
  pen.a_brake = a_brake;
  pen.t_react = t_react;
  pen.res = res;
  std::vector<double> m(T.size()), tt(T.size());
  anet::Context &ctx = anet::Context::thread_default();
  const int32_t *sd2 = map.distanceField(true);  // (flushes the map's buffered fills first)
  ctx.check(anet_traj_stop_margin(ctx.get(), &pen, (D + 1) / 2, (int)T.size(), 1, co.data(), T.data(), &map.grid(), sd2, m.data(),
                                  tt.data(), nullptr, nullptr));
  double best = INFINITY, start = 0.0;
  t = 0.0;
  piece = -1;
  for (size_t i = 0; i < m.size(); ++i) {
    if (m[i] != m[i]) {  // nothing is known about this piece
      t = start;
      piece = (int)i;
      return m[i];
    }
    if (piece < 0 || m[i] < best) {
      best = m[i];
      t = start + tt[i];
      piece = (int)i;
    }
    start += T[i];
  }
  return best;
}
// true when the vehicle can stop `clearance` short of the blocked set from every sample (NaN: false)
template <int D>
inline bool checkStoppable(const Trajectory<D> &traj, const voxel_map::VoxelMap &map, double a_brake, double t_react = 0.0,
                           double clearance = 0.0, int res = 20) {
  double t;
  int piece;
  return getStopMargin(traj, map, a_brake, t_react, clearance, res, t, piece) >= 0.0;
}
