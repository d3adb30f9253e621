// Exact clearance of a trajectory to obstacle points: how close, in metres, the curve comes to the cloud its corridor was inflated
// from (VoxelMap::surf_points_dev, or the per-segment sets of anet_voxel_gather_boxes_dev).
//
// SEMANTICS.  For piece i of duration T_i and the points q_j given for that piece,
//     clearance_i = min over finite points j, min over t in [0, T_i], of || p_i(t) - q_j ||      (Euclidean, metres)
// Per (trajectory, piece): `clearance`; `point`, a minimising point's index within its set (-1: the set has no finite point);
// `t`, the local time of the minimum (0 without a point).  `point` and `t` are diagnostics specified by consistency, as `row`
// and `t` of anet_traj_row_margin are: || p_i(t) - q_point || reproduces `clearance` within the bound; there is no tie-breaking
// rule.  A piece without a finite point has clearance +inf.  A point with a non-finite coordinate is skipped, as setOccupied
// skips such records.  T_i == 0 is the point p_i(0).  A NaN or infinite coefficient or duration, or T_i < 0, gives clearance NaN,
// point -1 and t 0 for that piece only; so does a product c_k T_i^k that is not finite (a power T_i^k that overflows poisons the
// piece also where c_k = 0: the curve is held in normalised time).  Orders s = 2, 3, 4.
//
// PROCEDURE.  One lane per (trajectory, piece), blockIdx.y = piece: the coefficient loads of a wave are contiguous, and all 64
// lanes of a block test the same point set.  The block (one wave) copies the set through LDS in tiles of 64 points; a ballot of
// "index below the count and all three coordinates finite" is the tile's wave-uniform list of points, and every lane reads the
// point under test from the same LDS address (a broadcast).  The lane holds, in registers, the coefficients in normalised time
// u[ax][k] = c_k T^k, their Bernstein control values, and the curve at the kClrK = 9 times tau_k = k / 8.
// CHEAP PART.  Per (lane, point): the 9 squared distances to those positions (7 operations each).  Their minimum ub_j is a
// candidate (an actual distance of the curve), and  lb_j = ub_j - L h / 2  bounds the point's distance from below:  every tau is
// within h / 2 = 1 / 16 of a tau_k, and L = n max_k || b_(k+1) - b_k || >= max ||u'|| from the derivative's control values.  A first
// pass over all points settles `best`, the smallest candidate.  A second pass marks, tile by tile, the points with
//     ub_j < best + L h / 2 + kClrSlack eps scale_j,      scale_j = sum_ax (sum_k |u_ax,k| + |q_j,ax|)
// (compared in squares, the right side rounded up), and the lane then visits ITS marked points of the tile, each lane its own
// next one: a wave refines as often per tile as its busiest lane has survivors, not once per point slot.  The slack covers the
// rounding of the positions (u_k: 8 roundings; Horner: 14; the difference: 1 -- 11.5 eps scale_j on a distance) and of L h / 2
// (7 x 10 / 16 eps sum |u|): a point that is not marked has, in exact arithmetic on the lane's u, no distance below `best`.
// SURVIVORS.  The critical points of g(tau) = || u(tau) - q ||^2 are the roots of h = g' / 2 = (u - q) . u'.  The control values
// of h / n (degree 2n - 1) are formed ONCE per survivor from the Bernstein forms of u - q and u' -- a product of Bernstein
// polynomials is a sum of positive weights times control-value products, so nothing is expanded into monomials and nothing
// cancels that does not cancel in h itself (bern::product_cv).  The roots of h are isolated by the walk of bernstein_walk.h
// (kClrMaxDepth, kClrMaxNodes visits per survivor).  No sign change: dropped (its ends are candidates already).  One change, + to
// -: a maximum, dropped.  One change, - to +: bisected (kClrBisect halvings at most, until the ends are neighbouring doubles) on
// h evaluated from the three component polynomials, Horner per axis for u and u' together -- never from coefficients of g.
// More than one: the midpoint is a candidate and the interval is split; at the depth bound the midpoint stands for the
// cluster.  An interval over which g varies by less than (eps scale_j)^2 yields its midpoint.
// Every candidate's VALUE is the norm of the difference vector at the candidate time, from the components: an actual distance of
// the curve, never below the true minimum by more than its own rounding.
// BUDGETS.  Loops: tiles ceil(count / 64), twice; points per tile 64; marked points per tile 64; interval visits per survivor
// kClrMaxNodes; splits per visit and the climb kClrMaxDepth; bisection kClrBisect -- all structural, no input can spin a wave.
// When the visits run out, or a cluster reaches the depth bound, what has been found so far stands: every candidate is a
// distance of the curve to a point of the set, so the result is a valid upper bound of the clearance whatever was cut short.
// (The kernel has no output for either event; tests/test_traj_clearance_cpu.py counts both on a float64 restatement of this
// procedure with the same constants: none on any fixture case.)
// TOLERANCE.  |clearance - exact| <= 32 eps scale + location term, scale = sum_ax (sum_k |u_ax,k| + |q_ax|); derived in
// tests/traj_clearance_mp.clearance_bound and DESIGN.md 8m.  No atomics: the reduction over the points runs inside one lane in
// point order, so a problem gives the same bits whatever else is in the batch and whatever ld is.  No scratch; LDS 1536 B.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "bernstein_walk.h"

namespace anet {

struct ClearanceArgs {
  const double *coeffs, *T;  // [(i*3+ax)*2S + k][ld], [N][ld]
  const double *points;      // [n_sets][max_points][3]
  const int32_t *counts;     // [n_sets] or nullptr: max_points each
  double *clearance;         // [N][ld]
  int32_t *point;            // [N][ld] or nullptr
  double *t;                 // [N][ld] or nullptr
  int64_t B, ld, max_points;
  int N, per_piece;          // per_piece: piece i uses set i (else set 0)
};

constexpr int kClrK = 9;             // positions per piece at tau_k = k / (kClrK - 1)
constexpr int kClrMaxDepth = 20;     // smallest interval 2^-20
constexpr int kClrMaxNodes = 1024;   // intervals visited per survivor at most
constexpr int kClrBisect = 64;
constexpr double kClrEps = 2.220446049250313e-16;
constexpr double kClrSlack = 16.0;   // in eps * scale_j, see CHEAP PART

template <int S>
__global__ void __launch_bounds__(64) k_traj_clearance(ClearanceArgs a) {
  constexpr int D = 2 * S, n = D - 1;  // D control values per axis, degree n
  constexpr int M = 2 * n;             // control values of h / n, degree 2n - 1
  __shared__ double tile[3][64];
  const int lane = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * 64 + lane;
  const bool act = b0 < a.B;
  const int64_t b = act ? b0 : a.B - 1;  // an idle lane repeats the last problem (it serves the tile loads) and stores nothing
  const int i = blockIdx.y;
  const int64_t ld = a.ld;
  const int64_t o = (int64_t)i * ld + b;
  const double Ti = a.T[o];
  bool bad = !(fabs(Ti) < INFINITY) || Ti < 0.0;
  // u[ax][k]: ascending coefficients of p(T tau)
  double u[3][D], A1;
  bad = !bern::normalised<D>(a.coeffs, i, b, ld, Ti, u, A1) || bad;
  if (bad) {  // the lane goes on with a harmless curve: it still serves the tile loads and the barriers
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
#pragma unroll
      for (int k = 0; k < D; ++k) u[ax][k] = 0.0;
    A1 = 0.0;
  }
  // Bernstein control values bz[ax][ii] = sum_{k<=ii} C(ii,k)/C(n,k) u[ax][k]; the positions at tau_k; L h / 2
  double bz[3][D], pos[3][kClrK];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    bern::to_bernstein<D>(u[ax], bz[ax]);
#pragma unroll
    for (int k = 0; k < kClrK; ++k) pos[ax][k] = bern::horner<D>(u[ax], (double)k / (double)(kClrK - 1));
  }
  const double Lh2 = bern::lipschitz_half_step<n>(bz, kClrK);

  const int set = a.per_piece ? i : 0;
  int64_t cnt = a.max_points;
  if (a.counts) {
    const int64_t c = a.counts[set];
    cnt = c < 0 ? 0 : (c < cnt ? c : cnt);
  }
  const double *P = a.points + (int64_t)set * a.max_points * 3;

  // the tile [base, base + 64) of the set -> LDS; the ballot of the usable points
  auto load_tile = [&](int64_t base) -> unsigned long long {
    __syncthreads();  // the previous tile has been read by every lane
    const int64_t j = base + lane;
    double x = 0.0, y = 0.0, z = 0.0;
    bool ok = false;
    if (j < cnt) {
      x = P[j * 3];
      y = P[j * 3 + 1];
      z = P[j * 3 + 2];
      ok = fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY;
    }
    tile[0][lane] = x;
    tile[1][lane] = y;
    tile[2][lane] = z;
    __syncthreads();
    return __ballot(ok);
  };
  // the smallest squared distance from the 9 positions to (x, y, z), and which position
  auto nearest = [&](double x, double y, double z, int &km) {
    double d2m = INFINITY;
    km = 0;
#pragma unroll
    for (int k = 0; k < kClrK; ++k) {
      const double dx = pos[0][k] - x, dy = pos[1][k] - y, dz = pos[2][k] - z;
      const double d2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
      if (d2 < d2m) { d2m = d2; km = k; }
    }
    return d2m;
  };

  double best2 = INFINITY, bt = 0.0;
  int bp = -1;
  // first pass: the 9 positions against every point, so that `best` is as low as they can make it before any point is tested
  for (int64_t base = 0; base < cnt; base += 64) {
    unsigned long long m = load_tile(base);
    while (m) {
      const int jj = __builtin_ctzll(m);
      m &= m - 1;
      int km;
      const double d2 = nearest(tile[0][jj], tile[1][jj], tile[2][jj], km);
      if (d2 < best2) { best2 = d2; bp = (int)(base + jj); bt = (double)km / (double)(kClrK - 1); }
    }
  }
  // the square of best + L h / 2 + slack, rounded up
  double bestd = sqrt(best2);
  auto threshold2 = [&](double x, double y, double z) {
    const double sc = A1 + (fabs(x) + fabs(y) + fabs(z));
    const double thr = bestd + Lh2 + kClrSlack * kClrEps * sc;
    return thr * thr * (1.0 + 8.0 * kClrEps);
  };
  // second pass, tile by tile: mark, then each lane visits its own marked points
  for (int64_t base = 0; base < cnt; base += 64) {
    unsigned long long m = load_tile(base), live = 0;
    while (m) {
      const int jj = __builtin_ctzll(m);
      m &= m - 1;
      const double x = tile[0][jj], y = tile[1][jj], z = tile[2][jj];
      int km;
      if (nearest(x, y, z, km) < threshold2(x, y, z)) live |= 1ull << jj;
    }
    for (int visit = 0; visit < 64 && live != 0; ++visit) {
      const int jj = __builtin_ctzll(live);
      live &= live - 1;
      const double q[3] = {tile[0][jj], tile[1][jj], tile[2][jj]};
      int km;
      if (!(nearest(q[0], q[1], q[2], km) < threshold2(q[0], q[1], q[2]))) continue;  // `best` has fallen since it was marked
      const double sc = A1 + (fabs(q[0]) + fabs(q[1]) + fabs(q[2]));
      const double flat = (kClrEps * sc) * (kClrEps * sc);
      // a candidate: the distance from the three components at tau
      auto candidate = [&](double tau) {
        double v[3], d2 = 0.0;
        bern::horner3<D>(u, tau, v);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) d2 = __builtin_fma(v[ax] - q[ax], v[ax] - q[ax], d2);
        if (d2 < best2) { best2 = d2; bestd = sqrt(d2); bp = (int)(base + jj); bt = tau; }
      };
      // control values of h / n = (u - q) . u' / n on [0, 1]
      double x[3][D], dv[M];
#pragma unroll
      for (int ax = 0; ax < 3; ++ax)
#pragma unroll
        for (int k = 0; k < D; ++k) x[ax][k] = bz[ax][k] - q[ax];
      bern::product_cv<n>(x, bz, dv);
      bern::Dyadic<kClrMaxDepth, uint32_t> walk;
      for (int guard = 0; guard < kClrMaxNodes; ++guard) {
        double w[M];
        walk.descend<M>(dv, w);
        const bern::Signs sg = bern::signs<M>(w);
        const int var = sg.var, first = sg.first;
        const double mx = sg.mx, width = walk.width(), lo = walk.lo(), mid = lo + 0.5 * width;
        bool split = false;
        if (var == 0) {
          // monotone: its ends are split points or 0, 1
        } else if (2.0 * (double)n * mx * width <= flat) {
          candidate(mid);  // g is constant here to rounding
        } else if (var == 1) {
          if (first < 0) {  // - to +: a minimum
            double l = lo, hgh = lo + width;
            for (int it = 0; it < kClrBisect; ++it) {
              const double mm = 0.5 * (l + hgh);
              if (!(l < mm && mm < hgh)) break;  // neighbouring doubles
              double hm = 0.0;
#pragma unroll
              for (int ax = 0; ax < 3; ++ax) {
                double v = u[ax][n], dd = 0.0;
#pragma unroll
                for (int k = n - 1; k >= 0; --k) {
                  dd = __builtin_fma(dd, mm, v);
                  v = __builtin_fma(v, mm, u[ax][k]);
                }
                hm = __builtin_fma(v - q[ax], dd, hm);
              }
              if (hm < 0.0) l = mm; else hgh = mm;
            }
            candidate(l);
            candidate(hgh);
          }
        } else {
          candidate(mid);  // the split point, or the cluster's location at the depth bound
          split = walk.can_split();
        }
        if (!walk.advance(split)) break;
      }
    }
  }
  if (!act) return;
  a.clearance[o] = bad ? NAN : sqrt(best2);
  if (a.point) a.point[o] = bad ? -1 : bp;
  if (a.t) a.t[o] = bad || bp < 0 ? 0.0 : bt * Ti;
}

}  // namespace anet
