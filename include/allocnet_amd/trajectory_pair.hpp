// The exact minimum separation between two Trajectory<D> (anet_traj_separation; no counterpart in the reference, which plans one
// vehicle).  Kept apart from trajectory.hpp, as trajectory_map.hpp is:
//     double t; int pieceA, pieceB;
//     double d = getSeparation(trajA, trajB, t0A, t0B, t, pieceA, pieceB);   // t0A, t0B: the global start times
//     if (checkSeparation(trajA, trajB, 0.6, t0A, t0B)) ...                   // at least 0.6 m apart while both exist
//     std::vector<anet::PairSeparation> r = getSeparations(fleet, t0, pairs); // a fleet and a list of index pairs, one call
// d is the smallest distance in metres over the time both trajectories exist (knots: the double sums t0 + T_0 + ... in piece order),
// found between the samples, not on them; t its global time and pieceA, pieceB the two pieces.  +inf (t 0, pieces -1) when they
// share no time, NaN (t 0, pieces -1) on a non-finite or negative duration, a non-finite start time or a non-finite coefficient in
// a piece that is used.  Trajectories of different piece counts are padded with pieces of zero duration, which occupy no time.
// Holding position before the start or after the end is not a mode: prepend or append a constant piece of the wanted duration.
// C++14, no Eigen or HIP includes.
#pragma once
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "trajectory.hpp"

namespace anet {

struct PairSeparation {
  double d, t;
  int pieceA, pieceB;
};

namespace detail {

// the trajectories as one batch [B][N][3][D+1], [B][N], N the largest piece count; false: some trajectory is empty
template <int D>
inline bool pack_fleet(const std::vector<const Trajectory<D> *> &fleet, int &N, std::vector<double> &co, std::vector<double> &T) {
  N = 0;
  for (const Trajectory<D> *tr : fleet) {
    if (tr->getPieceNum() < 1) return false;
    N = tr->getPieceNum() > N ? tr->getPieceNum() : N;
  }
  const size_t per = (size_t)3 * (D + 1);
  co.assign(fleet.size() * (size_t)N * per, 0.0);
  T.assign(fleet.size() * (size_t)N, 0.0);
  for (size_t b = 0; b < fleet.size(); ++b)
    for (int i = 0; i < fleet[b]->getPieceNum(); ++i) {
      T[b * (size_t)N + (size_t)i] = (*fleet[b])[i].getDuration();
      const double *c = (*fleet[b])[i].getCoeffMat().data();
      for (size_t k = 0; k < per; ++k) co[(b * (size_t)N + (size_t)i) * per + k] = c[k];
    }
  return true;
}

template <int D>
inline std::vector<PairSeparation> separations(const std::vector<const Trajectory<D> *> &fleet, const std::vector<double> &t0,
                                               const std::vector<std::pair<int, int>> &pairs, double cutoff) {
  static_assert(D == 3 || D == 5 || D == 7, "orders 2, 3 and 4");
  std::vector<PairSeparation> out(pairs.size());
  if (pairs.empty()) return out;
  if (!t0.empty() && t0.size() != fleet.size()) throw anet::Error(ANET_ERR_INVALID, "getSeparations: one start time per trajectory");
  int N = 0;
  std::vector<double> co, T;
  if (fleet.empty() || !pack_fleet<D>(fleet, N, co, T)) throw anet::Error(ANET_ERR_INVALID, "getSeparation: empty trajectory");
  std::vector<int32_t> pa(pairs.size()), pb(pairs.size()), qa(pairs.size()), qb(pairs.size());
  std::vector<double> sep(pairs.size()), tt(pairs.size());
  for (size_t p = 0; p < pairs.size(); ++p) {
    pa[p] = (int32_t)pairs[p].first;
    pb[p] = (int32_t)pairs[p].second;
  }
  anet::Context &ctx = anet::Context::thread_default();
  ctx.check(anet_traj_separation(ctx.get(), (D + 1) / 2, N, (int64_t)fleet.size(), co.data(), T.data(), t0.empty() ? nullptr : t0.data(),
                                 (int64_t)pairs.size(), pa.data(), pb.data(), cutoff, sep.data(), tt.data(), qa.data(), qb.data()));
  for (size_t p = 0; p < pairs.size(); ++p) out[p] = PairSeparation{sep[p], tt[p], (int)qa[p], (int)qb[p]};
  return out;
}

}  // namespace detail

// a fleet and a list of index pairs in one call; t0 empty: every trajectory starts at 0.  cutoff: a separation at or above it need
// not be refined (it is still an actual distance of the two curves); INFINITY: off
template <int D>
inline std::vector<PairSeparation> getSeparations(const std::vector<Trajectory<D>> &fleet, const std::vector<double> &t0,
                                                  const std::vector<std::pair<int, int>> &pairs, double cutoff = INFINITY) {
  std::vector<const Trajectory<D> *> ptrs;
  for (const Trajectory<D> &tr : fleet) ptrs.push_back(&tr);
  return detail::separations<D>(ptrs, t0, pairs, cutoff);
}

}  // namespace anet

// the smallest distance between trajA started at t0A and trajB started at t0B: t its global time, pieceA / pieceB its pieces
template <int D>
inline double getSeparation(const Trajectory<D> &trajA, const Trajectory<D> &trajB, double t0A, double t0B, double &t, int &pieceA,
                            int &pieceB, double cutoff = INFINITY) {
  const std::vector<const Trajectory<D> *> two{&trajA, &trajB};
  const anet::PairSeparation r =
      anet::detail::separations<D>(two, std::vector<double>{t0A, t0B}, std::vector<std::pair<int, int>>{{0, 1}}, cutoff)[0];
  t = r.t;
  pieceA = r.pieceA;
  pieceB = r.pieceB;
  return r.d;
}

// true when the two keep at least min_dist apart while both exist (NaN: false; no common time: true); separations above min_dist
// are not refined
template <int D>
inline bool checkSeparation(const Trajectory<D> &trajA, const Trajectory<D> &trajB, double min_dist, double t0A = 0.0, double t0B = 0.0) {
  double t;
  int pa, pb;
  const double cutoff = std::nextafter(min_dist, INFINITY);
  return getSeparation(trajA, trajB, t0A, t0B, t, pa, pb, cutoff > 0.0 ? cutoff : 0.0) >= min_dist;
}
