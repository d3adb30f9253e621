// Exact minimum separation between pairs of trajectories of one batch: how close, in metres, two of the B trajectories come to
// each other over the time they share.
//
// SEMANTICS (on the doubles given, exactly).  Knots are float64 by definition: K_0 = t0 (0 without t0), K_(i+1) = K_i + T_i summed in
// piece order in float64.  Piece i lives on global time [K_i, K_(i+1)] and is evaluated at local time t - K_i; a piece with
// K_(i+1) == K_i occupies no time and contributes nothing (T_i = 0: padding).  For the pair (a, b)
//     W = [max(K_0^a, K_0^b), min(K_N^a, K_N^b)],
// the intervals are the maximal sub-intervals of W of positive length between consecutive distinct knots of either trajectory (at
// most 2N - 1), each closed and with its own two pieces at both ends (trajectories need not be continuous), and
//     sep = min over intervals, min over t in the interval, of || p_a,i(t - K_i^a) - p_b,j(t - K_j^b) ||     (Euclidean, metres).
// Per pair: `sep`; `t`, the global time of a minimum; `piece_a`, `piece_b`.  t and the pieces are diagnostics specified by
// consistency, as point and t of anet_traj_clearance are: the distance of the two named pieces at t reproduces sep within the
// bound, t lies in W and in both pieces' spans; there is no tie-breaking rule.  No interval (disjoint or merely touching
// windows): sep = +inf, t = 0, pieces -1.  a == b is a valid pair with separation 0.  sep = NaN, t = 0, pieces -1, for that pair
// only: a duration or t0 of either trajectory that is not finite (or a knot sum that is not), a negative duration; a coefficient
// that is not finite or a product c_k T^k that is not, in a piece that takes part in an interval; a pair index outside [0, B),
// for which nothing is read.  A piece that takes part in no interval is never read.  Orders s = 2, 3, 4.
// CUTOFF (+inf: off).  Every reported sep is an actual distance of the two curves at the reported t, so never below the exact
// minimum by more than the value rounding; it is within the full bound of the exact minimum whenever that minimum is below
// cutoff.  An interval whose certified lower bound is at least cutoff is left at its best sampled distance.
//
// PROCEDURE.  One lane per pair.  pair_a, pair_b and the outputs are plain contiguous planes [P]: a wave reads and writes them
// coalesced.  The coefficient layout stays batch-minor ([row][ld]), so the loads of a wave are gathers by trajectory index: a pair
// list sorted by a turns the a side into broadcasts (64 lanes, one address) and, where b then runs upwards, the b side into
// contiguous runs; an unsorted list costs one memory transaction per lane and row, which is the uncoalesced case of the guides --
// callers that build the list (all a < b: traj_separation) build it sorted.
// The lane first sums both knot sequences (2N + 2 loads) and then walks the intervals with a two-pointer merge over them: the
// current piece indices, their knots and durations are scalars (no register array is indexed at run time); a step advances a,
// advances b or treats the interval [lo, hi = min(next knot of a, next knot of b)], and the pieces' coefficients are loaded when
// an index has advanced since the last interval.  `best` stays in the lane across the intervals: pruning across intervals, no
// atomics, no workspace, and the same bits for a pair whatever else is in the launch and whatever ld is.
// PER INTERVAL.  (1) A piece is held as the Bernstein control values of p(T tau) on [0, 1] (u_k = c_k T^k, then positive weights
// C(i,k)/C(n,k): bern::normalised and bern::to_bernstein), formed when the piece is loaded.  (2) Each is restricted to the common interval
// [alpha, beta] = [(lo - K_i) / T_i, (hi - K_i) / T_i] by two de Casteljau subdivisions (left part at beta, right part at alpha /
// beta): convex combinations of control values, no Taylor shift in monomials.  (3) d = a - b, control value by control value: the
// difference curve in sigma in [0, 1], t = lo + sigma (hi - lo).  (4) CHEAP PART: d at the kSepK = 9 values sigma_k = k / 8 (de
// Casteljau); the smallest squared norm ub is a candidate (an actual distance), and lb = ub - L h / 2, L = n max_k ||d_(k+1) - d_k||
// >= max ||d'||, h / 2 = 1 / 16, bounds the interval from below.  The interval is refined only when
//     ub < min(best, cutoff) + L h / 2 + kSepSlack eps scale,        scale = sum |u^a| + sum |u^b|
// (in squares, the right side rounded up).  (5) SURVIVORS: the rule of clearance_kernels.h with the point at the origin, on the
// walk of bernstein_walk.h (kSepMaxDepth, kSepMaxNodes): control values of h / n = d . d' / n (bern::product_cv); no sign change:
// dropped; one, + to -: a maximum, dropped; one, - to +: bisected (kSepBisect halvings at most, to neighbouring doubles) on h
// evaluated from the three components of d by de Casteljau, both ends candidates; more: the midpoint is a candidate and the
// interval is split.  An interval over which g = ||d||^2 varies by less than (eps scale)^2 yields its midpoint.  Every
// candidate's VALUE is the norm of the difference vector d at the candidate sigma.
// BUDGETS.  Steps of the merge kSepMaxSteps (every step advances an index or the interval: 4N - 1 at most); intervals visited per
// interval of time kSepMaxNodes; splits and the climb kSepMaxDepth; bisection kSepBisect -- structural, no input can spin a
// wave.  When a budget runs out what has been found stands: a valid upper bound.
// TOLERANCE.  |sep - exact| <= 64 eps scale + 4 eps |t| v + location term (v: a bound of the two speeds; |t|: the largest modulus of
// the times involved); derived in tests/traj_separation_mp.separation_bound and DESIGN.md 8n.
// No scratch, no LDS, no barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "bernstein_walk.h"

namespace anet {

struct SeparationArgs {
  const double *coeffs, *T;  // [(i*3+ax)*2S + k][ld], [N][ld]
  const double *t0;          // [B] or nullptr: 0
  const int32_t *pair_a, *pair_b;  // [P]
  double *sep;               // [P]
  double *t;                 // [P] or nullptr
  int32_t *piece_a, *piece_b;  // [P] or nullptr
  int64_t B, ld, P;
  int N;
  double cutoff;
};

constexpr int kSepK = 9;             // values of d per interval at sigma_k = k / (kSepK - 1)
constexpr int kSepMaxSteps = 64;     // steps of the merge: 4 ANET_MAX_PIECES
constexpr int kSepMaxDepth = 20;     // smallest interval 2^-20
constexpr int kSepMaxNodes = 1024;   // intervals visited per interval of time at most
constexpr int kSepBisect = 64;
constexpr double kSepEps = 2.220446049250313e-16;
constexpr double kSepSlack = 64.0;   // in eps * scale, see PER INTERVAL (4)

// piece i of trajectory b -> Bernstein control values of p(T tau) on [0, 1], the coefficient-modulus sum; false: not finite
template <int S>
__device__ __forceinline__ bool sep_load(const SeparationArgs &a, int i, int64_t b, double Ti, double (&z)[3][2 * S], double &A) {
  double u[3][2 * S];
  const bool ok = bern::normalised<2 * S>(a.coeffs, i, b, a.ld, Ti, u, A);
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) bern::to_bernstein<2 * S>(u[ax], z[ax]);
  return ok;
}

// the control values of z on [0, 1] -> those of the same polynomial on [al, be], 0 <= al < be (be may pass 1 by a rounding)
template <int D>
__device__ __forceinline__ void sep_restrict(const double (&z)[D], double al, double be, double (&w)[D]) {
  constexpr int n = D - 1;
#pragma unroll
  for (int k = 0; k < D; ++k) w[k] = z[k];
  const double ob = 1.0 - be;
#pragma unroll
  for (int r = 1; r <= n; ++r)
#pragma unroll
    for (int k = n; k >= r; --k) w[k] = __builtin_fma(be, w[k], ob * w[k - 1]);
  const double ga = al / be, og = 1.0 - ga;
#pragma unroll
  for (int r = 1; r <= n; ++r)
#pragma unroll
    for (int k = 0; k <= n - r; ++k) w[k] = __builtin_fma(ga, w[k + 1], og * w[k]);
}

template <int S>
__global__ void __launch_bounds__(64) k_traj_separation(SeparationArgs a) {
  constexpr int D = 2 * S, n = D - 1;  // D control values per axis, degree n
  constexpr int M = 2 * n;             // control values of h / n, degree 2n - 1
  const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (p >= a.P) return;
  const int64_t ta = a.pair_a[p], tb = a.pair_b[p];
  const int64_t ld = a.ld;
  const int N = a.N;
  bool bad = ta < 0 || ta >= a.B || tb < 0 || tb >= a.B;
  double best2 = INFINITY, bestd = INFINITY, bt = 0.0;
  int bpa = -1, bpb = -1;
  if (!bad) {
    // the knots of both, summed in piece order
    const double K0a = a.t0 ? a.t0[ta] : 0.0, K0b = a.t0 ? a.t0[tb] : 0.0;
    double KNa = K0a, KNb = K0b;
    for (int i = 0; i < N; ++i) {
      const double Ta = a.T[(int64_t)i * ld + ta], Tb = a.T[(int64_t)i * ld + tb];
      bad = bad || !(fabs(Ta) < INFINITY) || Ta < 0.0 || !(fabs(Tb) < INFINITY) || Tb < 0.0;
      KNa += Ta;
      KNb += Tb;
    }
    bad = bad || !(fabs(K0a) < INFINITY) || !(fabs(K0b) < INFINITY) || !(fabs(KNa) < INFINITY) || !(fabs(KNb) < INFINITY);
    int ia = 0, ib = 0, la = -1, lb = -1;
    double Tia = a.T[ta], Tib = a.T[tb];
    double ka0 = K0a, ka1 = K0a + Tia, kb0 = K0b, kb1 = K0b + Tib;
    double lo = fmax(K0a, K0b);
    double za[3][D], zb[3][D], Aa = 0.0, Ab = 0.0;
    for (int step = 0; step < kSepMaxSteps && !bad && ia < N && ib < N; ++step) {
      if (ka1 <= lo) {  // piece ia has ended (or occupies no time)
        ++ia;
        ka0 = ka1;
        if (ia < N) { Tia = a.T[(int64_t)ia * ld + ta]; ka1 = ka0 + Tia; }
        continue;
      }
      if (kb1 <= lo) {
        ++ib;
        kb0 = kb1;
        if (ib < N) { Tib = a.T[(int64_t)ib * ld + tb]; kb1 = kb0 + Tib; }
        continue;
      }
      const double hi = fmin(ka1, kb1);  // > lo
      if (la != ia) { bad = bad || !sep_load<S>(a, ia, ta, Tia, za, Aa); la = ia; }
      if (lb != ib) { bad = bad || !sep_load<S>(a, ib, tb, Tib, zb, Ab); lb = ib; }
      if (bad) break;
      // d = a - b on [lo, hi], control values in sigma
      double d[3][D];
      {
        const double ala = (lo - ka0) / Tia, bea = (hi - ka0) / Tia, alb = (lo - kb0) / Tib, beb = (hi - kb0) / Tib;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          double wa[D], wb[D];
          sep_restrict<D>(za[ax], ala, bea, wa);
          sep_restrict<D>(zb[ax], alb, beb, wb);
#pragma unroll
          for (int k = 0; k < D; ++k) d[ax][k] = wa[k] - wb[k];
        }
      }
      const double wid = hi - lo;
      const double sc = Aa + Ab;
      // || d(sg) ||^2 by de Casteljau on the three components
      auto norm2 = [&](double sg) {
        const double os = 1.0 - sg;
        double d2 = 0.0;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          double w[D];
#pragma unroll
          for (int k = 0; k < D; ++k) w[k] = d[ax][k];
#pragma unroll
          for (int r = 1; r <= n; ++r)
#pragma unroll
            for (int k = 0; k <= n - r; ++k) w[k] = __builtin_fma(sg, w[k + 1], os * w[k]);
          d2 = __builtin_fma(w[0], w[0], d2);
        }
        return d2;
      };
      auto candidate = [&](double sg) {
        const double d2 = norm2(sg);
        if (d2 < best2) {
          best2 = d2;
          bestd = sqrt(d2);
          bt = fmin(__builtin_fma(sg, wid, lo), hi);
          bpa = ia;
          bpb = ib;
        }
        return d2;
      };
      // cheap part
      double ub2 = INFINITY;
      for (int k = 0; k < kSepK; ++k) ub2 = fmin(ub2, candidate((double)k / (double)(kSepK - 1)));
      const double Lh2 = bern::lipschitz_half_step<n>(d, kSepK);
      const double thr = fmin(bestd, a.cutoff) + Lh2 + kSepSlack * kSepEps * sc;
      if (ub2 < thr * thr * (1.0 + 8.0 * kSepEps)) {
        const double flat = (kSepEps * sc) * (kSepEps * sc);
        // control values of h / n = d . d' / n on [0, 1]
        double dv[M];
        bern::product_cv<n>(d, d, dv);
        bern::Dyadic<kSepMaxDepth, uint32_t> walk;
        for (int guard = 0; guard < kSepMaxNodes; ++guard) {
          double w[M];
          walk.descend<M>(dv, w);
          const bern::Signs sn = bern::signs<M>(w);
          const int var = sn.var, first = sn.first;
          const double mx = sn.mx, width = walk.width(), l0 = walk.lo(), mid = l0 + 0.5 * width;
          bool split = false;
          if (var == 0) {
            // monotone: its ends are split points or 0, 1
          } else if (2.0 * (double)n * mx * width <= flat) {
            candidate(mid);  // g is constant here to rounding
          } else if (var == 1) {
            if (first < 0) {  // - to +: a minimum
              double l = l0, hgh = l0 + width;
              for (int it = 0; it < kSepBisect; ++it) {
                const double mm = 0.5 * (l + hgh);
                if (!(l < mm && mm < hgh)) break;  // neighbouring doubles
                const double om = 1.0 - mm;
                double hm = 0.0;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                  double v[D];
#pragma unroll
                  for (int k = 0; k < D; ++k) v[k] = d[ax][k];
#pragma unroll
                  for (int r = 1; r < n; ++r)
#pragma unroll
                    for (int k = 0; k <= n - r; ++k) v[k] = __builtin_fma(mm, v[k + 1], om * v[k]);
                  hm = __builtin_fma(__builtin_fma(mm, v[1], om * v[0]), v[1] - v[0], hm);
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
      lo = hi;
    }
  }
  const bool none = bpa < 0;
  a.sep[p] = bad ? NAN : (none ? INFINITY : sqrt(best2));
  if (a.t) a.t[p] = bad || none ? 0.0 : bt;
  if (a.piece_a) a.piece_a[p] = bad ? -1 : bpa;
  if (a.piece_b) a.piece_b[p] = bad ? -1 : bpb;
}

}  // namespace anet
