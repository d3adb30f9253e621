// Exact margins of a trajectory against linear rows: how far the curve leaves (or how much room it keeps to) the corridor
// polytopes it was planned in, and the per-axis velocity / acceleration boxes QPSolver::solve samples (qp_solver.hpp:244-296).
//
// SEMANTICS.  For derivative order d in {0, 1, 2}, piece i of duration T_i and the M rows (a_r, b_r) given for that piece,
//     margin_i = max over non-padding rows r, max over t in [0, T_i], of  a_r . p_i^(d)(t) - b_r
// Rows are in the planner's form a.x <= b; a row whose four fields are all zero is padding and is skipped.  A positive margin is the
// deepest excursion out of the polytope, a negative one the clearance kept (metres for normalised rows and d = 0).  Per (trajectory,
// piece): `margin`; `row`, a maximising row (-1: the piece has no row); `t`, the local time in [0, T_i] of the maximum (0: no row).
// A piece without rows has margin -inf.  A NaN or infinite coefficient, duration or row field gives margin NaN (row -1, t 0) for
// that piece and only for it.  `row` and `t` are diagnostics, specified by consistency -- a_row . p^(d)(t) - b_row reproduces
// `margin` -- and not by a tie-breaking rule.
//
// PROCEDURE.  One lane per (trajectory, piece), blockIdx.y = piece: every load of a wave is one contiguous row segment.  The lane
// forms the d-th derivative in normalised time once, u[ax][k] = ff(k + d, d) c_(k+d) T^k (so that p^(d)(T tau) = sum_k u_k tau^k:
// no division by T^d anywhere), always as a polynomial of degree n = 2S - 1 whose d highest coefficients are zero: every loop
// below then has compile-time bounds and every array static indices, for all three d in one instantiation.  It converts the three
// components to Bernstein form once (3 x 2S control values, degree-elevated by d, which only tightens the control polygon) and
// keeps them in registers across the row loop.  Per row the 2S control values of g_r = a_r . u - b_r cost 3 FMAs and a
// subtraction each; their maximum `ub` bounds g_r from above on [0, 1]; g_r(0) and g_r(1) are candidates and bound the answer
// from below.
// PRUNING.  A first pass over the rows takes the two ends of every row as candidates (two dot products per row; the rows are read
// again from cache), so `best`, the largest candidate value so far, already holds every end value when the second pass tests a
// row: on synthetic corridors 1.2 rows per piece survive instead of 2.9 with the rows' ends taken in turn.  The second pass only
// marks the rows that survive; the third visits the marked rows, each lane its own next one, and tests them again.  A wave then
// isolates roots as often as its busiest lane has survivors, not once per row slot in which any of its 64 lanes has one (with 1.2
// survivors among 9 rows that is every slot).  A row is finished when
//     ub + kMarginSlack * eps * scale_r <= best,     scale_r = sum_ax |a_ax| sum_k |u_ax,k| + |b_r|.
// The slack covers the rounding of the control values against the polynomial the lane holds: a control value is a sum of at
// most 2S <= 8 terms w_ik u_k with 0 < w_ik <= 1 rounded once, accumulated by FMA (9 roundings on a term's way), and the row's
// three FMAs and subtraction add 4 (one fewer on any one term): 12 roundings of relative size eps / 2 = 6 eps scale_r, rounded up
// to 8.  So a pruned row has max g_r <= best in exact arithmetic on the lane's u: pruning changes the result by nothing beyond
// the error `best` itself carries.
// SURVIVING ROWS.  The control values of g_r' are the differences of those of g_r; the roots of g_r' are isolated by the walk of
// bernstein_walk.h (kMarginMaxDepth, kMarginMaxNodes visits per row).  A visit without a sign change is dropped; one whose first
// sign is negative holds a minimum and is dropped; one with a single + to - change is bisected (kMarginBisect halvings on the
// monomial g_r', which only LOCATES the candidate).  An interval over which g_r varies by less than eps scale_r (width times the
// largest derivative control value) yields its midpoint; so does one at the depth bound (a cluster of critical points: g_r
// varies there by the cube of the width).  Every split point is a candidate.  Loops: rows M, three times; the walk's own;
// bisection kMarginBisect -- all structural.  No scratch, no LDS.
// CANDIDATE VALUES are always taken from the three component polynomials, Horner per axis, then the dot product with a_r, minus
// b_r -- never from the monomial coefficients of g_r (rate_kernels.h explains what that costs on Chebyshev-like pieces).
// TOLERANCE.  |margin - exact| <= 32 eps (sum_ax |a_ax| sum_k |u_ax,k| + |b|), the largest over the piece's rows; derived in
// tests/corridor_margin_mp.margin_bound and DESIGN.md 8k.  No atomics: the reduction over the rows runs inside one lane in row
// order, so a problem gives the same bits whatever else is in the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "bernstein_walk.h"

namespace anet {

struct MarginArgs {
  const double *coeffs, *T, *rows;  // [(i*3+ax)*2S + k][ld], [N][ld], [(i*M + r)*4 + f][ld]
  double *margin;                   // [N][ld]
  int32_t *row;                     // [N][ld] or nullptr
  double *t;                        // [N][ld] or nullptr
  int64_t B, ld;
  int N, M, deriv;
};

constexpr int kMarginMaxDepth = 20;    // smallest interval 2^-20
constexpr int kMarginMaxNodes = 1024;  // intervals visited per row at most
constexpr int kMarginBisect = 48;
constexpr double kMarginEps = 2.220446049250313e-16;
constexpr double kMarginSlack = 8.0;   // in eps * scale_r, see PRUNING

template <int S>
__global__ void __launch_bounds__(64) k_traj_row_margin(MarginArgs a) {
  constexpr int D = 2 * S, n = D - 1;  // D control values, degree n
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int i = blockIdx.y;
  const int64_t ld = a.ld;
  const int64_t o = (int64_t)i * ld + b;
  const double Ti = a.T[o];
  const int dsel = a.deriv;
  bool bad = !(fabs(Ti) < INFINITY);
  // u[ax][k]: ascending coefficients of p^(dsel)(T tau)
  double u[3][D];
  {
    double tk[D];
    tk[0] = 1.0;
#pragma unroll
    for (int k = 1; k < D; ++k) tk[k] = tk[k - 1] * Ti;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      double c[D + 2];  // ascending powers, two zeros on top
#pragma unroll
      for (int p = 0; p < D; ++p) {
        c[p] = a.coeffs[(int64_t)((i * 3 + ax) * D + (n - p)) * ld + b];
        bad = bad || !(fabs(c[p]) < INFINITY);
      }
      c[D] = c[D + 1] = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double f = dsel == 0 ? c[k] : dsel == 1 ? (double)(k + 1) * c[k + 1] : (double)((k + 2) * (k + 1)) * c[k + 2];
        u[ax][k] = f * tk[k];
      }
    }
  }
  if (bad) {
    a.margin[o] = NAN;
    if (a.row) a.row[o] = -1;
    if (a.t) a.t[o] = 0.0;
    return;
  }
  // Bernstein control values of degree n, bz[ax][ii] = sum_{k<=ii} C(ii,k)/C(n,k) u[ax][k]; A[ax] = sum_k |u[ax][k]|; the ends
  double bz[3][D], A[3], p1[3];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    double s1 = u[ax][n], sa = fabs(u[ax][n]);
#pragma unroll
    for (int k = n - 1; k >= 0; --k) {
      s1 = s1 + u[ax][k];  // Horner at tau = 1
      sa += fabs(u[ax][k]);
    }
    p1[ax] = s1;
    A[ax] = sa;
    bern::to_bernstein<D>(u[ax], bz[ax]);
  }
  double best = -INFINITY, bt = 0.0;
  int brow = -1;
  // first pass: the two ends of every row, so that `best` is as high as the ends can make it before any row is tested for pruning
  for (int r = 0; r < a.M; ++r) {
    const int64_t ro = (int64_t)((i * a.M + r) * 4) * ld + b;
    const double ra = a.rows[ro], rb = a.rows[ro + ld], rc = a.rows[ro + 2 * ld], rd = a.rows[ro + 3 * ld];
    if (ra == 0.0 && rb == 0.0 && rc == 0.0 && rd == 0.0) continue;  // padding
    if (!(fabs(ra) < INFINITY && fabs(rb) < INFINITY && fabs(rc) < INFINITY && fabs(rd) < INFINITY)) {
      bad = true;
      break;
    }
    const double g0 = __builtin_fma(rc, u[2][0], __builtin_fma(rb, u[1][0], ra * u[0][0])) - rd;
    const double g1 = __builtin_fma(rc, p1[2], __builtin_fma(rb, p1[1], ra * p1[0])) - rd;
    if (g0 > best) { best = g0; brow = r; bt = 0.0; }
    if (g1 > best) { best = g1; brow = r; bt = 1.0; }
  }
  // second pass: the control values of every row against `best`; the rows that may still raise it are marked in a mask
  // (M <= ANET_MAX_POLY_ROWS = 50 bits)
  uint64_t live = 0;
  for (int r = 0; r < (bad ? 0 : a.M); ++r) {
    const int64_t ro = (int64_t)((i * a.M + r) * 4) * ld + b;
    const double ra = a.rows[ro], rb = a.rows[ro + ld], rc = a.rows[ro + 2 * ld], rd = a.rows[ro + 3 * ld];
    if (ra == 0.0 && rb == 0.0 && rc == 0.0 && rd == 0.0) continue;  // padding
    double ub = -INFINITY;
#pragma unroll
    for (int ii = 0; ii < D; ++ii) ub = fmax(ub, __builtin_fma(rc, bz[2][ii], __builtin_fma(rb, bz[1][ii], ra * bz[0][ii])) - rd);
    const double scale = __builtin_fma(fabs(rc), A[2], __builtin_fma(fabs(rb), A[1], __builtin_fma(fabs(ra), A[0], fabs(rd))));
    if (ub + kMarginSlack * kMarginEps * scale > best) live |= (uint64_t)1 << r;
  }
  // third pass: the marked rows, each lane its own next one, so that a wave isolates roots as often as its busiest lane has marked
  // rows and not once per row slot; a row is tested again, `best` may have risen since it was marked
  for (int q = 0; q < a.M && live != 0; ++q) {
    const int r = __builtin_ctzll(live);
    live &= live - 1;
    const int64_t ro = (int64_t)((i * a.M + r) * 4) * ld + b;
    const double ra = a.rows[ro], rb = a.rows[ro + ld], rc = a.rows[ro + 2 * ld], rd = a.rows[ro + 3 * ld];
    // a_r . (x, y, z) - b_r
    auto dotrow = [&](double x, double y, double z) { return __builtin_fma(rc, z, __builtin_fma(rb, y, ra * x)) - rd; };
    // a candidate: the value from the three components
    auto candidate = [&](double tau) {
      double v[3];
      bern::horner3<D>(u, tau, v);
      const double g = dotrow(v[0], v[1], v[2]);
      if (g > best) { best = g; brow = r; bt = tau; }
    };
    double cv[D], ub;
#pragma unroll
    for (int ii = 0; ii < D; ++ii) {
      cv[ii] = dotrow(bz[0][ii], bz[1][ii], bz[2][ii]);
      ub = ii == 0 ? cv[0] : fmax(ub, cv[ii]);
    }
    const double scale = __builtin_fma(fabs(rc), A[2], __builtin_fma(fabs(rb), A[1], __builtin_fma(fabs(ra), A[0], fabs(rd))));
    if (!(ub + kMarginSlack * kMarginEps * scale > best)) continue;  // pruned
    // control values of g_r' / n and the monomial g_r' (which only locates)
    double dv[n], gd[n];
#pragma unroll
    for (int k = 0; k < n; ++k) {
      dv[k] = cv[k + 1] - cv[k];
      gd[k] = (double)(k + 1) * __builtin_fma(rc, u[2][k + 1], __builtin_fma(rb, u[1][k + 1], ra * u[0][k + 1]));
    }
    bern::Dyadic<kMarginMaxDepth, uint32_t> walk;
    for (int guard = 0; guard < kMarginMaxNodes; ++guard) {
      double w[n];
      walk.descend<n>(dv, w);
      const bern::Signs sg = bern::signs<n>(w);
      const int var = sg.var, first = sg.first;
      const double mx = sg.mx, width = walk.width(), lo = walk.lo(), mid = lo + 0.5 * width;
      bool split = false;
      if (var == 0) {
        // monotone: its ends are split points or 0, 1
      } else if ((double)n * mx * width <= kMarginEps * scale) {
        candidate(mid);  // g_r is constant here to rounding
      } else if (var == 1) {
        if (first > 0) {  // + to -: a maximum
          double l = lo, h = lo + width;
          for (int it = 0; it < kMarginBisect; ++it) {
            const double m = 0.5 * (l + h);
            if (bern::horner<n>(gd, m) > 0.0) l = m; else h = m;
          }
          candidate(0.5 * (l + h));
        }
      } else {
        candidate(mid);  // the split point, or the cluster's location at the depth bound
        split = walk.can_split();
      }
      if (!walk.advance(split)) break;
    }
  }
  a.margin[o] = bad ? NAN : best;
  if (a.row) a.row[o] = bad ? -1 : brow;
  if (a.t) a.t[o] = bad ? 0.0 : bt * Ti;
}

}  // namespace anet
