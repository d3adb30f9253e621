// Yaw trajectories (no counterpart in the reference): the heading psi as a one-axis minimum-control polynomial over the pieces and
// durations of a position trajectory, and the sampled check that the direction of travel stays inside the camera's field of view
// while the heading turns no faster than the platform allows.  psi is an unwrapped angle in radians.
//     minco::MincoYaw<2> my;                       // order 2: minimum angular acceleration, cubic pieces
//     my.setConditions(head, tail, N);             // head, tail: psi, dpsi[, ...] at the ends (c = S values each)
//     my.setParameters(yawWaypoints, durations);   // N - 1 headings at the interior nodes, the position trajectory's durations
//     YawTrajectory yaw; my.getTrajectory(yaw);
//     double t; int piece;
//     double m = getYawMargin(traj, yaw, half_fov, v_min, 20, &t, &piece);
//     if (checkYaw(traj, yaw, half_fov, max_rate, v_min, 20)) ...
// m is the least  half_fov - |angle between (v_x, v_y) and (cos psi, sin psi)|  over the res + 1 samples of every piece at which
// |v_xy| >= v_min (+inf when there is none), t its global time; NaN (t the start of that piece) when a piece has a non-finite
// coefficient or duration.  A SAMPLED check (anet_traj_yaw_margin).  C++14, no Eigen or HIP headers needed.
#pragma once
#include <cmath>
#include <vector>

#include "core.hpp"
#include "trajectory.hpp"
#include "trajectory_map.hpp"  // detail::pack_pieces

// The yaw polynomial of a trajectory: per piece 2 SY coefficients, highest power first, and the durations it shares with the
// position trajectory.  Times are located as Trajectory locates them.
class YawTrajectory {
 public:
  YawTrajectory() : order_(0) {}
  YawTrajectory(int order, const std::vector<double> &durations, const std::vector<double> &coeffs)
      : order_(order), T_(durations), c_(coeffs) {
    if (order < 2 || order > 4 || c_.size() != T_.size() * 2 * (size_t)order)
      throw anet::Error(ANET_ERR_INVALID, "YawTrajectory: order 2..4 and 2 * order coefficients per piece");
  }
  int getOrder() const { return order_; }
  int getPieceNum() const { return (int)T_.size(); }
  const std::vector<double> &getDurations() const { return T_; }
  const std::vector<double> &getCoeffs() const { return c_; }  // [piece][2 * order], highest power first
  double getTotalDuration() const {
    double s = 0.0;
    for (size_t i = 0; i < T_.size(); ++i) s += T_[i];
    return s;
  }
  double getYaw(double t) const { return eval(t, false); }
  double getYawRate(double t) const { return eval(t, true); }

 private:
  double eval(double t, bool rate) const {
    if (T_.empty()) throw anet::Error(ANET_ERR_INVALID, "YawTrajectory: empty");
    size_t i = 0;
    for (; i < T_.size(); ++i) {
      if (!(t > T_[i])) break;
      t -= T_[i];
    }
    if (i == T_.size()) {
      --i;
      t += T_[i];
    }
    const int DY = 2 * order_;
    const double *c = c_.data() + i * (size_t)DY;
    double p = c[0], v = 0.0;
    for (int col = 1; col < DY; ++col) {
      v = v * t + p;
      p = p * t + c[col];
    }
    return rate ? v : p;
  }
  int order_;
  std::vector<double> T_, c_;
};

namespace minco {

// The one-axis MINCO behind anet_minco_solve_scalar, shaped like MINCO_SNU of minco.hpp.  One object = one yaw trajectory.
template <int S>
class MincoYaw {
 public:
  static constexpr int D = 2 * S;

  // headState / tailState: c values psi, dpsi[, ddpsi[, dddpsi]] ((i) access); c = bcCols <= S
  template <class V1, class V2>
  inline void setConditions(const V1 &headState, const V2 &tailState, const int &pieceNum, int bcCols = S) {
    N = pieceNum;
    c = bcCols;
    head.assign((size_t)c, 0.0);
    tail.assign((size_t)c, 0.0);
    for (int j = 0; j < c; ++j) {
      head[(size_t)j] = headState(j);
      tail[(size_t)j] = tailState(j);
    }
    T.assign((size_t)N, 0.0);
    wps.assign((size_t)(N > 1 ? N - 1 : 0), 0.0);
    coeffs.assign((size_t)N * D, 0.0);
  }

  // inYaws: the N - 1 headings at the interior nodes, ts: the N durations of the position trajectory
  template <class VP, class VT>
  inline void setParameters(const VP &inYaws, const VT &ts) {
    for (int i = 0; i < N; ++i) T[(size_t)i] = ts(i);
    for (int k = 0; k + 1 < N; ++k) wps[(size_t)k] = inYaws(k);
    anet::Context &ctx = anet::Context::thread_default();
    ctx.check(anet_minco_solve_scalar(ctx.get(), S, c, N, 1, head.data(), tail.data(), wps.data(), T.data(), coeffs.data(), &energy));
  }

  inline void getTrajectory(YawTrajectory &yaw) const { yaw = YawTrajectory(S, T, coeffs); }
  inline void getEnergy(double &e) const { e = energy; }  // int (psi^(S))^2 dt
  inline double getEnergy() const { return energy; }
  inline const std::vector<double> &getCoeffs() const { return coeffs; }

 private:
  int N = 0, c = S;
  std::vector<double> head, tail, wps, T, coeffs;
  double energy = 0.0;
};

}  // namespace minco

namespace anet {
namespace detail {

// per piece margin, local time and peak rate of the sampled yaw check
template <int D>
inline void yaw_margin_rows(const Trajectory<D> &traj, const YawTrajectory &yaw, double half_fov, double v_min, int res,
                            std::vector<double> &T, std::vector<double> &m, std::vector<double> &tt, std::vector<double> &rate) {
  std::vector<double> co;
  pack_pieces<D>(traj, "getYawMargin: empty trajectory", co, T);
  if (yaw.getDurations() != T) throw anet::Error(ANET_ERR_INVALID, "getYawMargin: the yaw trajectory must share the pieces and durations");
  anet_yaw_penalty pen = {};
  pen.half_fov = half_fov;
  pen.res = res;
  m.assign(T.size(), 0.0);
  tt.assign(T.size(), 0.0);
  rate.assign(T.size(), 0.0);
  anet::Context &ctx = anet::Context::thread_default();
  ctx.check(anet_traj_yaw_margin(ctx.get(), &pen, v_min, (D + 1) / 2, yaw.getOrder(), (int)T.size(), 1, co.data(), yaw.getCoeffs().data(),
                                 T.data(), m.data(), tt.data(), rate.data()));
}

}  // namespace detail
}  // namespace anet

// The sampled look margin: the minimum over the pieces, res + 1 samples of each; *t its global time, *piece its piece (either may
// be NULL)
template <int D>
inline double getYawMargin(const Trajectory<D> &traj, const YawTrajectory &yaw, double half_fov, double v_min, int res, double *t,
                           int *piece) {
  std::vector<double> T, m, tt, rate;
  anet::detail::yaw_margin_rows<D>(traj, yaw, half_fov, v_min, res, T, m, tt, rate);
  double best = INFINITY, start = 0.0, bt = 0.0;
  int bp = -1;
  for (size_t i = 0; i < m.size(); ++i) {
    if (m[i] != m[i]) {  // nothing is known about this piece
      best = m[i];
      bt = start;
      bp = (int)i;
      break;
    }
    if (bp < 0 || m[i] < best) {
      best = m[i];
      bt = start + tt[i];
      bp = (int)i;
    }
    start += T[i];
  }
  if (t) *t = bt;
  if (piece) *piece = bp;
  return best;
}

// true when the sampled look margin is >= 0 on every piece and the sampled |dpsi| stays within max_rate (NaN: false)
template <int D>
inline bool checkYaw(const Trajectory<D> &traj, const YawTrajectory &yaw, double half_fov, double max_rate, double v_min = 0.0,
                     int res = 20) {
  std::vector<double> T, m, tt, rate;
  anet::detail::yaw_margin_rows<D>(traj, yaw, half_fov, v_min, res, T, m, tt, rate);
  for (size_t i = 0; i < m.size(); ++i)
    if (!(m[i] >= 0.0) || !(rate[i] <= max_rate)) return false;
  return true;
}
