// Stop within known space: the penalty of the MINCO objective that couples speed with the distance to the blocked set, and the
// sampled check that goes with it.  Semantics: include/allocnet_amd.h (anet_minco_stop_partial_grads_dev, anet_traj_stop_margin_dev).
//
// THE TERM.  With `blocked` = occupied or unknown, d the trilinear distance field (dist_query.h) and v, a the velocity and acceleration
// of the piece, a vehicle that reacts for t_react and then brakes at a_brake comes to rest within t_react |v| + v.v / (2 a_brake) of
// where it is; the term holds that ball, grown by `clearance`, inside free space:
//     s_eps = sqrt(v.v + eps^2)       g = t_react s_eps + (v.v) hb + clearance - d,  hb = 0.5 / a_brake (formed once, on the host)
//     Phi = w smoothedL1_mu(g)        kappa = t_react / s_eps + 1 / a_brake
//     F = -w phi' grad d              G = w phi' kappa v             (dg/dp = -grad d, dg/dv = kappa v)
// and t_react == 0 drops s_eps from g and kappa altogether (eps may then be 0 and v = 0 is no singular point).
//   * s_eps >= |v|, so g is never below the true excess: a piece whose samples are all inactive has a sampled margin >= 0 there.
//   * v.v >= 0, so the term dominates the obstacle term of the same clearance, w and mu: a caller uses one or the other.
//   * a_brake = +inf and t_react = 0 give hb = kappa = 0, G = 0: the obstacle term.
//
// PENALTY (k_minco_stop).  The shape of k_minco_obstacle: one workgroup per trajectory, durations and coefficients staged in LDS,
// lanes over the flattened samples (i, j) in rounds of kStopBlock; Phi, F[3], G[3], H = sigma (F . v + G . a) and tau of a sample
// are left in LDS, then output row r = (i, ax, k) | (i, Phi) | (i, H) is contracted by lane r mod kStopBlock in ascending j into an
// accumulator kept across the rounds (two rows per lane at most: N (3 D + 2) <= 416).  A coefficient row has two sources; for the
// power k of tau that the coefficient multiplies, a sample contributes
//     k == 0:  F_ax            k >= 1:  fma(F_ax, tau, k G_ax) * tau * ... * tau   (k - 1 multiplications, left to right)
// i.e. F tau^k + k G tau^(k-1) with the common power factored out, and the accumulator takes that one number by one addition.
// p, v and a come from one Horner recurrence in FMAs, highest power first; a is twice the second-order Horner value.
// No atomics, no workspace; the bits of trajectory b do not depend on the launch or on ld.  `accumulate`: one unfused addition of
// the complete share (add_unfused).  All outputs of b are NaN when a duration of b is not finite or <= 0, when d is NaN or -inf at
// a sample (a non-finite position; the all-blocked map), or when v.v or a.a is not finite at one.
//
// MARGIN (k_traj_stop_margin).  A SAMPLED check, as k_traj_body_margin: the field is no polynomial in t, so nothing bounds the value
// between the samples.  One lane per (trajectory, piece), blockIdx.y = piece.  At sigma = j / res, tau = sigma T_i, j = 0..res (the
// sample times of the penalty and the piece's end; p and v by the penalty's recurrence, so the same bits):
//     m = ((d - clearance) - t_react |v|) - (v.v) hb,   |v| = sqrt(v.v) exactly, no eps, nothing contracted
// and the first minimum over j is kept with its tau, |v| and d.  A non-finite coefficient or duration of the piece, a duration <= 0
// or a NaN m gives NaN in all four outputs of that piece only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "dist_query.h"     // DistGrid, dist_sample
#include "penalty_terms.h"  // smoothed_l1, add_unfused

namespace anet {

constexpr int kStopBlock = 256;
constexpr int kStopMaxPieces = 16;  // ANET_MAX_PIECES (checked where the launch is)

struct StopTerm {
  double clearance, t_react, eps2, hb, inv_ab;  // eps2 = speed_eps^2, hb = 0.5 / a_brake, inv_ab = 1 / a_brake (0 for +inf)
};

struct StopArgs {
  const double *coeffs, *T;    // [(i*3+ax)*2S + col][ld], [N][ld]
  const int32_t *sd2;
  double *gdC, *gdT, *pcost;   // pcost may be nullptr
  int64_t B, ld;
  int N, res, accumulate;
  double w, mu;
  StopTerm k;
  DistGrid g;
};

// sigma and tau of a sample: one rounding each, never contracted (the rule of the obstacle term)
__device__ __forceinline__ void stop_sample_time(const int j, const int res, const double Ti, double &sigma, double &tau) {
#pragma clang fp contract(off)
  sigma = (double)j / (double)res;
  tau = sigma * Ti;
}

// p, v and a of one axis at tau; c holds the D coefficients of the axis, highest power first, `st` apart
template <int D>
__device__ __forceinline__ void stop_horner(const double *c, const int64_t st, const double tau, double &p, double &v, double &a) {
  double h = 0.0;
  p = c[0];
  v = 0.0;
#pragma unroll
  for (int col = 1; col < D; ++col) {
    h = __builtin_fma(h, tau, v);
    v = __builtin_fma(v, tau, p);
    p = __builtin_fma(p, tau, c[(int64_t)col * st]);
  }
  a = 2.0 * h;
}

template <int S>
struct StopShared {
  static constexpr int D = 2 * S;
  static constexpr int kRows = 3 * D + 2;  // output rows per piece: 3 D coefficients, Phi, H
  double eT[kStopMaxPieces];
  double eC[kStopMaxPieces * 3 * D];
  double smp[9][kStopBlock];               // Phi, F[3], G[3], H, tau of this round's samples
  double sums[kStopMaxPieces * 2];         // per piece: sum Phi, sum H
  int32_t bad;
};

template <int S>
__global__ void __launch_bounds__(kStopBlock) k_minco_stop(const StopArgs a) {
  using Sh = StopShared<S>;
  constexpr int D = Sh::D, kRows = Sh::kRows;
  __shared__ Sh sh;
  const int tid = threadIdx.x, N = a.N, res = a.res;
  const int64_t b = blockIdx.x, ld = a.ld;
  const double inv_mu = 1.0 / a.mu;
  const StopTerm k = a.k;

  if (tid < N) sh.eT[tid] = a.T[(int64_t)tid * ld + b];
  for (int e = tid; e < N * 3 * D; e += kStopBlock) sh.eC[e] = a.coeffs[(int64_t)e * ld + b];
  if (tid == 0) sh.bad = 0;
  __syncthreads();
  bool t_bad = false;
  for (int i = 0; i < N; ++i) {
    const double Ti = sh.eT[i];
    t_bad = t_bad || !(fabs(Ti) < INFINITY) || !(Ti > 0.0);
  }

  const int total_rows = N * kRows;
  const int row0 = tid, row1 = tid + kStopBlock;
  const int pi0 = row0 / kRows, q0 = row0 % kRows, pi1 = row1 / kRows, q1 = row1 % kRows;
  double acc0 = 0.0, acc1 = 0.0;

  const int64_t M = (int64_t)N * res;
  for (int64_t base = 0; base < M && !t_bad; base += kStopBlock) {
    const int64_t gs = base + tid;
    const bool has = gs < M;
    const int i = has ? (int)(gs / res) : 0, j = has ? (int)(gs % res) : 0;
    double sigma, tau;
    stop_sample_time(j, res, sh.eT[i], sigma, tau);
    double pb[3], vb[3], ab[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) stop_horner<D>(sh.eC + (i * 3 + ax) * D, 1, tau, pb[ax], vb[ax], ab[ax]);
    double Phi = 0.0, F[3] = {0.0, 0.0, 0.0}, G[3] = {0.0, 0.0, 0.0};
    if (has) {
      double d, gd[3];
      dist_sample(a.g, a.sd2, pb[0], pb[1], pb[2], d, gd[0], gd[1], gd[2]);
      const double vv = __builtin_fma(vb[2], vb[2], __builtin_fma(vb[1], vb[1], vb[0] * vb[0]));
      // NaN (a non-finite position) or -inf (the all-blocked map); a velocity or an acceleration that is not finite (H = sigma
      // (F.v + G.a) would otherwise poison gdT alone)
      const double aa = __builtin_fma(ab[2], ab[2], __builtin_fma(ab[1], ab[1], ab[0] * ab[0]));
      if (!(d > -INFINITY) || !(vv < INFINITY) || !(aa < INFINITY)) sh.bad = 1;
      double g = __builtin_fma(vv, k.hb, k.clearance - d), kappa = k.inv_ab;
      if (k.t_react > 0.0) {
        const double s_eps = sqrt(vv + k.eps2);
        g = __builtin_fma(k.t_react, s_eps, g);
        kappa += k.t_react / s_eps;
      }
      double f, df;
      smoothed_l1(a.mu, inv_mu, g, f, df);
      const double wf = a.w * df, wk = wf * kappa;
      Phi = a.w * f;
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        F[ax] = -wf * gd[ax];
        G[ax] = wk * vb[ax];
      }
    }
    const double Fv = __builtin_fma(F[2], vb[2], __builtin_fma(F[1], vb[1], F[0] * vb[0]));
    const double FvGa = __builtin_fma(G[2], ab[2], __builtin_fma(G[1], ab[1], __builtin_fma(G[0], ab[0], Fv)));
    __syncthreads();  // (smp[] of the previous round has been read)
    sh.smp[0][tid] = Phi;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      sh.smp[1 + ax][tid] = F[ax];
      sh.smp[4 + ax][tid] = G[ax];
    }
    sh.smp[7][tid] = sigma * FvGa;
    sh.smp[8][tid] = tau;
    __syncthreads();
    auto contract = [&](const int row, const int pi, const int q, double &acc) {
      if (row >= total_rows) return;
      const int64_t lo = max((int64_t)pi * res, base), hi = min((int64_t)(pi + 1) * res, min(base + kStopBlock, M));
      if (q < 3 * D) {
        const int ax = q / D, pw = D - 1 - q % D;
        const double kpw = (double)pw;
        for (int64_t gg = lo; gg < hi; ++gg) {
          const int l = (int)(gg - base);
          const double tl = sh.smp[8][l];
          double term = sh.smp[1 + ax][l];
          if (pw >= 1) term = __builtin_fma(term, tl, kpw * sh.smp[4 + ax][l]);
          for (int e = 1; e < pw; ++e) term *= tl;
          acc += term;
        }
      } else {
        const int src = q == 3 * D ? 0 : 7;
        for (int64_t gg = lo; gg < hi; ++gg) acc += sh.smp[src][(int)(gg - base)];
      }
    };
    contract(row0, pi0, q0, acc0);
    contract(row1, pi1, q1, acc1);
  }

  __syncthreads();
  const bool nan_out = t_bad || sh.bad != 0;
  const double qnan = __builtin_nan("");
  auto put = [&](double *p, const double v) { *p = a.accumulate ? add_unfused(*p, v) : v; };
  auto finish = [&](const int row, const int pi, const int q, const double acc) {
    if (row >= total_rows) return;
    if (q < 3 * D) {
      const double step = sh.eT[pi] / (double)res;
      put(a.gdC + (int64_t)(pi * 3 * D + q) * ld + b, nan_out ? qnan : step * acc);
    } else {
      sh.sums[pi * 2 + (q - 3 * D)] = acc;
    }
  };
  finish(row0, pi0, q0, acc0);
  finish(row1, pi1, q1, acc1);
  __syncthreads();
  if (tid < N) {
    const double Ti = sh.eT[tid], step = Ti / (double)res, sPhi = sh.sums[tid * 2];
    const double gT = sPhi / (double)res + step * sh.sums[tid * 2 + 1];
    put(a.gdT + (int64_t)tid * ld + b, nan_out ? qnan : gT);
    if (a.pcost) put(a.pcost + (int64_t)tid * ld + b, nan_out ? qnan : step * sPhi);
  }
}

// ---- the sampled margin --------------------------------------------------------------------------------------------------------
constexpr int kStopMarginBlock = 64;

struct StopMarginArgs {
  const double *coeffs, *T;
  const int32_t *sd2;
  double *margin, *t, *speed, *dist;  // [N][ld]; t, speed, dist may be nullptr
  int64_t B, ld;
  int N, res;
  StopTerm k;
  DistGrid g;
};

__device__ __forceinline__ double stop_margin_value(const StopTerm &k, const double d, const double speed, const double vv) {
#pragma clang fp contract(off)
  return ((d - k.clearance) - k.t_react * speed) - vv * k.hb;
}

template <int S>
__global__ void __launch_bounds__(kStopMarginBlock) k_traj_stop_margin(const StopMarginArgs a) {
  constexpr int D = 2 * S;
  const int64_t b = (int64_t)blockIdx.x * kStopMarginBlock + threadIdx.x;
  if (b >= a.B) return;
  const int i = blockIdx.y;
  const int64_t ld = a.ld, o = (int64_t)i * ld + b;
  const double Ti = a.T[o];
  double c[3][D];
  bool bad = !(fabs(Ti) < INFINITY) || !(Ti > 0.0);
#pragma unroll
  for (int ax = 0; ax < 3; ++ax)
#pragma unroll
    for (int col = 0; col < D; ++col) {
      c[ax][col] = a.coeffs[(int64_t)((i * 3 + ax) * D + col) * ld + b];
      bad = bad || !(fabs(c[ax][col]) < INFINITY);
    }
  double best = 0.0, bt = 0.0, bs = 0.0, bd = 0.0;
  for (int j = 0; j <= (bad ? -1 : a.res); ++j) {
    double sigma, tau;
    stop_sample_time(j, a.res, Ti, sigma, tau);
    double p[3], v[3], acc[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) stop_horner<D>(c[ax], 1, tau, p[ax], v[ax], acc[ax]);
    double d, gx, gy, gz;
    dist_sample(a.g, a.sd2, p[0], p[1], p[2], d, gx, gy, gz);
    const double vv = __builtin_fma(v[2], v[2], __builtin_fma(v[1], v[1], v[0] * v[0]));
    const double speed = sqrt(vv);
    const double m = stop_margin_value(a.k, d, speed, vv);
    bad = bad || m != m;
    if (j == 0 || m < best) {
      best = m;
      bt = tau;
      bs = speed;
      bd = d;
    }
  }
  const double qnan = __builtin_nan("");
  a.margin[o] = bad ? qnan : best;
  if (a.t) a.t[o] = bad ? qnan : bt;
  if (a.speed) a.speed[o] = bad ? qnan : bs;
  if (a.dist) a.dist[o] = bad ? qnan : bd;
}

}  // namespace anet
