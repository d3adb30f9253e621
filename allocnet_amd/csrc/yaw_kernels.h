// Yaw trajectories: a one-axis MINCO over the pieces and durations of a position trajectory, the penalty that couples the two
// (field of view, yaw rate, yaw effort), its sampled check, and flat states that use the yaw.  Semantics: include/allocnet_amd.h
// (anet_minco_solve_scalar_dev, anet_minco_propagate_grad_scalar_dev, anet_minco_yaw_partial_grads_dev, anet_traj_yaw_margin_dev,
// anet_traj_states_yaw_dev).
//
// ONE-AXIS MINCO (k_minco_solve_scalar, k_minco_propagate_scalar).  The solve and the adjoint of minco_kernels.h for one axis:
// Factor, solve_axis and the sweeps of minco_core.h as they stand, and propagate_axis with its axis count set to 1.  One lane per
// trajectory, one generic instantiation per order at kYawMaxPieces pieces, the factor of a lane in LDS (kScalarBlock).  Layout:
// coeffs [N * 2S][ld], wps [N - 1][ld].
//
// THE TERM.  psi is an unwrapped angle in radians, a polynomial of order SY per piece; h = (v_x, v_y) the horizontal velocity and
// (a_x, a_y) the horizontal acceleration of the position piece, u = (cos psi, sin psi), ca = cos(half_fov):
//     s_eps  = sqrt(h.h + eps^2)
//     g_look = ca s_eps - h.u              Phi_look = w_look smoothedL1_mu_look(g_look)
//     g_rate = dpsi^2 - max_rate^2         Phi_rate = w_rate smoothedL1_mu_rate(g_rate)
//     G = w_look phi'_look (ca h / s_eps - u)     (x and y; the z rows receive nothing)
//     A = w_look phi'_look (h_x sin psi - h_y cos psi)          R = w_rate phi'_rate 2 dpsi
//   * s_eps >= |h| and ca >= 0 (half_fov <= pi / 2), so g_look is never below ca |h| - h.u: an inactive sample has its horizontal
//     velocity inside the field of view.
//   * the look term scales with speed: at rest any heading is free, up to ca eps.
//
// PENALTY (k_minco_yaw).  The shape of k_minco_stop: one workgroup per trajectory, durations and both coefficient sets staged in
// LDS (the z rows of the position are only tested for finiteness), lanes over the flattened samples (i, j) in rounds of kYawBlock;
// Phi, G[2], A, R, H = sigma (G . a + A dpsi + R ddpsi) and tau of a sample are left in LDS, then output row
// r = (i, x | y, k) | (i, yaw, k) | (i, Phi) | (i, H) is contracted by lane r mod kYawBlock in ascending j into an accumulator kept
// across the rounds (two rows per lane at most: N (2 D + DY + 2) <= 416).  A sample contributes to the coefficient of tau^k
//     position row:  k G_ax tau^(k-1)                   (k = 0: nothing)
//     yaw row:       A tau^k + k R tau^(k-1)            as fma(A, tau, k R) * tau * ... * tau (k - 1 multiplications), k = 0: A
// The effort term w_energy int (psi^(SY))^2 is the closed form per piece (yaw_energy), added where the rows are finished.
// No atomics, no workspace; the bits of trajectory b do not depend on the launch or on ld.  `accumulate` governs gdC, gdT and
// pcost (one unfused addition of the complete share, add_unfused); gdCy is always written.  All outputs of b are NaN when a
// duration of b is not finite or <= 0, a position or yaw coefficient of b is not finite, or a sample value is not finite.
//
// MARGIN (k_traj_yaw_margin).  A SAMPLED check: nothing bounds the angle between the samples.  One lane per (trajectory, piece),
// blockIdx.y = piece.  At sigma = j / res, tau = sigma T_i, j = 0..res: among the samples with |h| >= v_min the first minimum of
// half_fov - |atan2(h x u, h . u)| with its tau (+inf and 0 when there is none; a sample at rest, |h| = 0, has no direction and
// counts at v_min = 0 with the angle 0), and the largest |dpsi| over all res + 1 samples.
//
// FLAT STATES (k_traj_flat_states_yaw).  k_traj_flat_states with psi, dpsi of the yaw piece at the same local time and
// flat_forward<true>.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "flatness_kernels.h"  // flat_forward, piece_derivs, flat_tilt, kFlatStateFields
#include "minco_kernels.h"     // propagate_axis, PropArgs, kSolveBlock (minco_core.h: Factor, solve_axis)
#include "penalty_terms.h"     // smoothed_l1, add_unfused
#include "stop_kernels.h"      // stop_sample_time, stop_horner: the sample times and the recurrence of the penalties

namespace anet {

constexpr int kYawBlock = 256;
constexpr int kYawMaxPieces = 16;  // ANET_MAX_PIECES (checked where the launch is)

// ---- one-axis MINCO ------------------------------------------------------------------------------------------------------------
// The block-tridiagonal factor of a lane (Factor<S, 16>: 50 / 84 / 118 doubles at S = 2 / 3 / 4) lives in LDS, and so does the
// adjoint's dJ/dT row: with both in registers the generic 16-piece instantiations need more than 256 VGPRs at the higher orders
// (as the three-axis ones do, which spill to AGPRs).  At S = 4 a lane's share is 944 + 128 B, so a workgroup is 32 lanes there --
// 34 KiB, four workgroups per CU -- where 64 lanes would pass 64 KiB; the trajectories in flight per CU are the same either way,
// since LDS bounds them.
template <int S>
constexpr int kScalarBlock = S == 4 ? 32 : 64;

template <int S>
__global__ void __launch_bounds__(kScalarBlock<S>) k_minco_solve_scalar(SolveArgs a) {
  constexpr int m = S - 1, D = 2 * S, NB = kYawMaxPieces;
  const int64_t b = (int64_t)blockIdx.x * kScalarBlock<S> + threadIdx.x;
  if (b >= a.B) return;
  const int N = a.N, np = a.c - 1;
  const int64_t ld = a.ld;
  __shared__ Factor<S, NB> Fs[kScalarBlock<S>];
  Factor<S, NB> &F = Fs[threadIdx.x];
  double tt[NB];  // all loads first, none behind a branch on the piece count (as the generic k_minco_solve)
#pragma unroll
  for (int i = 0; i < NB; ++i) tt[i] = a.T[(int64_t)(i < N ? i : 0) * ld + b];
#pragma unroll
  for (int i = 0; i < NB; ++i)
    if (i < N) F.r[i] = fast_rcp(tt[i]);
  F.factorize(N, np);
  double P[NB + 1], hv[m], tv[m], X[NB + 1][m];
  const double *hp = a.head + b, *tp = a.tail + b;
#pragma unroll
  for (int k = 0; k <= NB; ++k) {
    const double *src = (k == 0) ? hp : (k < N) ? a.wps + (int64_t)(k - 1) * ld + b : tp;
    const double v = *src;
    P[k] = (k <= N) ? v : 0.0;
  }
#pragma unroll
  for (int j = 0; j < m; ++j) {
    const int64_t row = (j < np) ? 1 + j : 0;
    const double h = hp[row * ld], t = tp[row * ld];
    hv[j] = (j < np) ? h : 0.0;
    tv[j] = (j < np) ? t : 0.0;
  }
  double *cp = a.coeffs ? a.coeffs + b : nullptr;
  const double e = solve_axis<S, NB>(F, N, np, P, hv, tv, X, [&](int piece, int col, double v) {
    if (cp) cp[(int64_t)(piece * D + col) * ld] = v;
  });
  if (a.energy) a.energy[b] = e;
}

// a.gdT may be nullptr (= zeros): the durations are shared with the position trajectory, whose adjoint takes the direct share.
// propagate_axis in its PIPE form (the loads of a piece issued one piece ahead, as k_minco_propagate_axis has it): the form
// without it holds six values more than 256 VGPRs at S = 4.
template <int S>
__global__ void __launch_bounds__(kScalarBlock<S>) k_minco_propagate_scalar(PropArgs a) {
  constexpr int NB = kYawMaxPieces;
  const int64_t b = (int64_t)blockIdx.x * kScalarBlock<S> + threadIdx.x;
  if (b >= a.B) return;
  const int N = a.N, np = a.c - 1;
  const int64_t ld = a.ld;
  __shared__ Factor<S, NB> Fs[kScalarBlock<S>];
  Factor<S, NB> &F = Fs[threadIdx.x];
  __shared__ double gTs[kScalarBlock<S>][NB];
  double(&gT)[NB] = gTs[threadIdx.x];
  double Tlast = 0.0;
#pragma unroll
  for (int i = 0; i < NB; ++i)
    if (i < N) {
      const double t = a.T[i * ld + b];
      F.r[i] = fast_rcp(t);
      gT[i] = a.gdT ? a.gdT[i * ld + b] : 0.0;
      if (i == N - 1) Tlast = t;
    }
  F.factorize(N, np);
  propagate_axis<S, NB, false, true, 1>(F, N, np, a, b, 0, Tlast, gT, true);
#pragma unroll
  for (int i = 0; i < NB; ++i)
    if (i < N) a.gradT[i * ld + b] = gT[i];
}

// ---- the penalty ---------------------------------------------------------------------------------------------------------------
struct YawTerm {
  double w_look, mu_look, ca, eps2;  // ca = cos(half_fov), eps2 = speed_eps^2 (formed once, on the host)
  double w_rate, mu_rate, mr2;       // mr2 = max_rate^2 (+inf allowed)
  double w_energy;
};

struct YawArgs {
  const double *coeffs, *ycoeffs, *T;  // [(i*3+ax)*2S + col][ld], [i*2SY + col][ld], [N][ld]
  double *gdC, *gdCy, *gdT, *pcost;    // pcost may be nullptr
  int64_t B, ld;
  int N, res, accumulate;
  YawTerm k;
};

// The effort of one yaw piece, int_0^T (psi^(SY))^2 dt, from its DY coefficients c (highest power first):
//   g_j = c_j j! / (j - SY)!  (j >= SY),  E = sum_jk g_j g_k T^(j+k-2SY+1) / (j+k-2SY+1),  dE/dc_j = 2 (j!/(j-SY)!) sum_k ...,
//   dE/dT = (psi^(SY)(T))^2.  dc gets DY entries in the order of c (zeros for the powers below SY).
template <int SY>
__device__ __forceinline__ void yaw_energy(const double *c, const double T, double &E, double &dT, double *dc) {
  constexpr int DY = 2 * SY;
  double tp[DY];
  tp[0] = 1.0;
#pragma unroll
  for (int e = 1; e < DY; ++e) tp[e] = tp[e - 1] * T;
  double g[SY], f[SY];
#pragma unroll
  for (int q = 0; q < SY; ++q) {
    double fj = 1.0;
#pragma unroll
    for (int e = 0; e < SY; ++e) fj *= (double)(SY + q - e);
    f[q] = fj;
    g[q] = fj * c[DY - 1 - (SY + q)];
  }
  E = 0.0;
  double top = 0.0;
#pragma unroll
  for (int q = 0; q < SY; ++q) {
    double row = 0.0;
#pragma unroll
    for (int r = 0; r < SY; ++r) row = __builtin_fma(tp[q + r + 1] / (double)(q + r + 1), g[r], row);
    E = __builtin_fma(g[q], row, E);
    dc[DY - 1 - (SY + q)] = 2.0 * f[q] * row;
    dc[DY - 1 - q] = 0.0;
    top = __builtin_fma(g[q], tp[q], top);
  }
  dT = top * top;
}

template <int S, int SY>
struct YawShared {
  static constexpr int D = 2 * S, DY = 2 * SY;
  static constexpr int kRows = 2 * D + DY + 2;  // output rows per piece: x and y coefficients, yaw coefficients, Phi, H
  double eT[kYawMaxPieces];
  double eC[kYawMaxPieces * 2 * D];             // x and y only
  double eY[kYawMaxPieces * DY];
  double smp[7][kYawBlock];                     // Phi, G[2], A, R, H, tau of this round's samples
  double sums[kYawMaxPieces * 2];               // per piece: sum Phi, sum H
  double eE[kYawMaxPieces * DY];                // per piece: dE/dc of the effort
  double en[kYawMaxPieces * 2];                 // per piece: E, dE/dT
  int32_t bad;
};

template <int S, int SY>
__global__ void __launch_bounds__(kYawBlock) k_minco_yaw(const YawArgs a) {
  using Sh = YawShared<S, SY>;
  constexpr int D = Sh::D, DY = Sh::DY, kRows = Sh::kRows;
  __shared__ Sh sh;
  const int tid = threadIdx.x, N = a.N, res = a.res;
  const int64_t b = blockIdx.x, ld = a.ld;
  const YawTerm k = a.k;
  const double inv_mu_look = 1.0 / k.mu_look, inv_mu_rate = 1.0 / k.mu_rate;

  if (tid == 0) sh.bad = 0;
  __syncthreads();
  if (tid < N) sh.eT[tid] = a.T[(int64_t)tid * ld + b];
  bool c_bad = false;
  for (int e = tid; e < N * 3 * D; e += kYawBlock) {
    const double v = a.coeffs[(int64_t)e * ld + b];
    const int pi = e / (3 * D), q = e % (3 * D);
    if (q < 2 * D) sh.eC[pi * 2 * D + q] = v;
    c_bad = c_bad || !(fabs(v) < INFINITY);
  }
  for (int e = tid; e < N * DY; e += kYawBlock) {
    const double v = a.ycoeffs[(int64_t)e * ld + b];
    sh.eY[e] = v;
    c_bad = c_bad || !(fabs(v) < INFINITY);
  }
  if (c_bad) sh.bad = 1;
  __syncthreads();
  bool t_bad = sh.bad != 0;
  for (int i = 0; i < N; ++i) {
    const double Ti = sh.eT[i];
    t_bad = t_bad || !(fabs(Ti) < INFINITY) || !(Ti > 0.0);
  }

  const int total_rows = N * kRows;
  const int row0 = tid, row1 = tid + kYawBlock;
  const int pi0 = row0 / kRows, q0 = row0 % kRows, pi1 = row1 / kRows, q1 = row1 % kRows;
  double acc0 = 0.0, acc1 = 0.0;

  const int64_t M = (int64_t)N * res;
  for (int64_t base = 0; base < M && !t_bad; base += kYawBlock) {
    const int64_t gs = base + tid;
    const bool has = gs < M;
    const int i = has ? (int)(gs / res) : 0, j = has ? (int)(gs % res) : 0;
    double sigma, tau;
    stop_sample_time(j, res, sh.eT[i], sigma, tau);
    double pb[2], hb[2], ab[2], psi, dpsi, ddpsi;
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) stop_horner<D>(sh.eC + (i * 2 + ax) * D, 1, tau, pb[ax], hb[ax], ab[ax]);
    stop_horner<DY>(sh.eY + i * DY, 1, tau, psi, dpsi, ddpsi);
    double Phi = 0.0, G[2] = {0.0, 0.0}, A = 0.0, R = 0.0;
    if (has) {
      const double hh = __builtin_fma(hb[1], hb[1], hb[0] * hb[0]), aa = __builtin_fma(ab[1], ab[1], ab[0] * ab[0]);
      const double rr = dpsi * dpsi;
      // a sample value that is not finite (H would otherwise poison gdT alone)
      if (!(hh < INFINITY) || !(aa < INFINITY) || !(rr < INFINITY) || !(fabs(ddpsi) < INFINITY) || !(fabs(psi) < INFINITY)) sh.bad = 1;
      if (k.w_look > 0.0) {
        double sn, cs;
        sincos(psi, &sn, &cs);
        const double s_eps = sqrt(hh + k.eps2), hu = __builtin_fma(hb[1], sn, hb[0] * cs);
        const double g = __builtin_fma(k.ca, s_eps, -hu);
        double f, df;
        smoothed_l1(k.mu_look, inv_mu_look, g, f, df);
        const double wf = k.w_look * df, cr = k.ca / s_eps;
        Phi = k.w_look * f;
        G[0] = wf * __builtin_fma(cr, hb[0], -cs);
        G[1] = wf * __builtin_fma(cr, hb[1], -sn);
        A = wf * __builtin_fma(hb[0], sn, -(hb[1] * cs));
      }
      if (k.w_rate > 0.0) {
        double f, df;
        smoothed_l1(k.mu_rate, inv_mu_rate, rr - k.mr2, f, df);
        Phi = __builtin_fma(k.w_rate, f, Phi);
        R = k.w_rate * df * (2.0 * dpsi);
      }
    }
    const double H = __builtin_fma(R, ddpsi, __builtin_fma(A, dpsi, __builtin_fma(G[1], ab[1], G[0] * ab[0])));
    __syncthreads();  // (smp[] of the previous round has been read)
    sh.smp[0][tid] = Phi;
    sh.smp[1][tid] = G[0];
    sh.smp[2][tid] = G[1];
    sh.smp[3][tid] = A;
    sh.smp[4][tid] = R;
    sh.smp[5][tid] = sigma * H;
    sh.smp[6][tid] = tau;
    __syncthreads();
    auto contract = [&](const int row, const int pi, const int q, double &acc) {
      if (row >= total_rows) return;
      const int64_t lo = max((int64_t)pi * res, base), hi = min((int64_t)(pi + 1) * res, min(base + kYawBlock, M));
      if (q < 2 * D) {  // position row: k G tau^(k-1)
        const int ax = q / D, pw = D - 1 - q % D;
        if (pw == 0) return;
        const double kpw = (double)pw;
        for (int64_t gg = lo; gg < hi; ++gg) {
          const int l = (int)(gg - base);
          const double tl = sh.smp[6][l];
          double term = kpw * sh.smp[1 + ax][l];
          for (int e = 1; e < pw; ++e) term *= tl;
          acc += term;
        }
      } else if (q < 2 * D + DY) {  // yaw row: A tau^k + k R tau^(k-1)
        const int pw = DY - 1 - (q - 2 * D);
        const double kpw = (double)pw;
        for (int64_t gg = lo; gg < hi; ++gg) {
          const int l = (int)(gg - base);
          const double tl = sh.smp[6][l];
          double term = sh.smp[3][l];
          if (pw >= 1) term = __builtin_fma(term, tl, kpw * sh.smp[4][l]);
          for (int e = 1; e < pw; ++e) term *= tl;
          acc += term;
        }
      } else {
        const int src = q == 2 * D + DY ? 0 : 5;
        for (int64_t gg = lo; gg < hi; ++gg) acc += sh.smp[src][(int)(gg - base)];
      }
    };
    contract(row0, pi0, q0, acc0);
    contract(row1, pi1, q1, acc1);
  }

  __syncthreads();
  const bool nan_out = t_bad || sh.bad != 0;
  const double qnan = __builtin_nan("");
  const bool with_energy = k.w_energy > 0.0;
  if (tid < N) {  // the effort of piece tid
    double E = 0.0, dT = 0.0, dc[DY];
#pragma unroll
    for (int col = 0; col < DY; ++col) dc[col] = 0.0;
    if (with_energy && !nan_out) yaw_energy<SY>(sh.eY + tid * DY, sh.eT[tid], E, dT, dc);
#pragma unroll
    for (int col = 0; col < DY; ++col) sh.eE[tid * DY + col] = dc[col];
    sh.en[tid * 2] = E;
    sh.en[tid * 2 + 1] = dT;
  }
  auto sums = [&](const int row, const int pi, const int q, const double acc) {
    if (row < total_rows && q >= 2 * D + DY) sh.sums[pi * 2 + (q - 2 * D - DY)] = acc;
  };
  sums(row0, pi0, q0, acc0);
  sums(row1, pi1, q1, acc1);
  __syncthreads();
  auto put = [&](double *p, const double v) { *p = a.accumulate ? add_unfused(*p, v) : v; };
  auto finish = [&](const int row, const int pi, const int q, const double acc) {
    if (row >= total_rows || q >= 2 * D + DY) return;
    const double step = sh.eT[pi] / (double)res;
    if (q < 2 * D) {
      put(a.gdC + (int64_t)(pi * 3 * D + q) * ld + b, nan_out ? qnan : step * acc);
    } else {
      const int col = q - 2 * D;
      const double v = with_energy ? __builtin_fma(k.w_energy, sh.eE[pi * DY + col], step * acc) : step * acc;
      a.gdCy[(int64_t)(pi * DY + col) * ld + b] = nan_out ? qnan : v;
    }
  };
  finish(row0, pi0, q0, acc0);
  finish(row1, pi1, q1, acc1);
  // the z rows receive nothing: zeros when written, untouched bits when accumulated (x + 0), NaN with the rest of b
  for (int e = tid; e < N * D; e += kYawBlock) put(a.gdC + (int64_t)((e / D) * 3 * D + 2 * D + e % D) * ld + b, nan_out ? qnan : 0.0);
  if (tid < N) {
    const double Ti = sh.eT[tid], step = Ti / (double)res, sPhi = sh.sums[tid * 2];
    double gT = sPhi / (double)res + step * sh.sums[tid * 2 + 1], pc = step * sPhi;
    if (with_energy) {
      gT = __builtin_fma(k.w_energy, sh.en[tid * 2 + 1], gT);
      pc = __builtin_fma(k.w_energy, sh.en[tid * 2], pc);
    }
    put(a.gdT + (int64_t)tid * ld + b, nan_out ? qnan : gT);
    if (a.pcost) put(a.pcost + (int64_t)tid * ld + b, nan_out ? qnan : pc);
  }
}

// ---- the sampled margin --------------------------------------------------------------------------------------------------------
constexpr int kYawMarginBlock = 64;

struct YawMarginArgs {
  const double *coeffs, *ycoeffs, *T;
  double *margin, *t, *rate;  // [N][ld]; t and rate may be nullptr
  int64_t B, ld;
  int N, res;
  double half_fov, v_min;
};

// |h|, h x u and h . u with nothing contracted
__device__ __forceinline__ void yaw_look_parts(const double hx, const double hy, const double sn, const double cs, double &hn,
                                               double &cross, double &dot) {
#pragma clang fp contract(off)
  hn = sqrt(hx * hx + hy * hy);
  cross = hx * sn - hy * cs;
  dot = hx * cs + hy * sn;
}

template <int S, int SY>
__global__ void __launch_bounds__(kYawMarginBlock) k_traj_yaw_margin(const YawMarginArgs a) {
  constexpr int D = 2 * S, DY = 2 * SY;
  const int64_t b = (int64_t)blockIdx.x * kYawMarginBlock + threadIdx.x;
  if (b >= a.B) return;
  const int i = blockIdx.y;
  const int64_t ld = a.ld, o = (int64_t)i * ld + b;
  const double Ti = a.T[o];
  double c[2][D], cy[DY];
  bool bad = !(fabs(Ti) < INFINITY) || !(Ti > 0.0);
#pragma unroll
  for (int ax = 0; ax < 3; ++ax)
#pragma unroll
    for (int col = 0; col < D; ++col) {
      const double v = a.coeffs[(int64_t)((i * 3 + ax) * D + col) * ld + b];
      if (ax < 2) c[ax][col] = v;
      bad = bad || !(fabs(v) < INFINITY);
    }
#pragma unroll
  for (int col = 0; col < DY; ++col) {
    cy[col] = a.ycoeffs[(int64_t)(i * DY + col) * ld + b];
    bad = bad || !(fabs(cy[col]) < INFINITY);
  }
  double best = INFINITY, bt = 0.0, rate = 0.0;
  for (int j = 0; j <= (bad ? -1 : a.res); ++j) {
    double sigma, tau;
    stop_sample_time(j, a.res, Ti, sigma, tau);
    double p[2], h[2], ac[2], psi, dpsi, ddpsi;
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) stop_horner<D>(c[ax], 1, tau, p[ax], h[ax], ac[ax]);
    stop_horner<DY>(cy, 1, tau, psi, dpsi, ddpsi);
    double sn, cs, hn, cross, dot;
    sincos(psi, &sn, &cs);
    yaw_look_parts(h[0], h[1], sn, cs, hn, cross, dot);
    const double m = a.half_fov - (hn > 0.0 ? fabs(atan2(cross, dot)) : 0.0);  // at rest there is no direction: the angle is 0
    bad = bad || m != m || dpsi != dpsi;
    if (hn >= a.v_min && m < best) {
      best = m;
      bt = tau;
    }
    rate = fmax(rate, fabs(dpsi));
  }
  const double qnan = __builtin_nan("");
  a.margin[o] = bad ? qnan : best;
  if (a.t) a.t[o] = bad ? qnan : bt;
  if (a.rate) a.rate[o] = bad ? qnan : rate;
}

// ---- flat states with the yaw --------------------------------------------------------------------------------------------------
struct FlatStatesYawArgs {
  const double *coeffs, *ycoeffs, *T, *tq;
  double *out;
  int64_t B, ld;
  int N, nq;
  FlatParams fp;
};

// k_traj_flat_states (the piece location, the 11 fields) with psi, dpsi of the yaw piece at the same local time
template <int S, int SY>
__global__ void __launch_bounds__(256) k_traj_flat_states_yaw(FlatStatesYawArgs a) {
  constexpr int D = 2 * S, DY = 2 * SY;
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const int64_t ld = a.ld;
  const int N = a.N;
  for (int q = 0; q < a.nq; ++q) {
    double t = a.tq[(int64_t)q * ld + b];
    int idx = 0;
    double dur = 0.0;
    for (; idx < N; ++idx) {
      dur = a.T[(int64_t)idx * ld + b];
      if (!(t > dur)) break;
      t -= dur;
    }
    if (idx == N) {
      --idx;
      t += a.T[(int64_t)idx * ld + b];
    }
    double d[3][3];
    piece_derivs<S, 3>(a.coeffs + (int64_t)(idx * 3 * D) * ld + b, ld, t, d);
    double psi, dpsi, ddpsi;
    stop_horner<DY>(a.ycoeffs + (int64_t)(idx * DY) * ld + b, ld, t, psi, dpsi, ddpsi);
    FlatMid m;
    flat_forward<true>(a.fp, d[0], d[1], d[2], psi, dpsi, m);
    double *o = a.out + (int64_t)(q * kFlatStateFields) * ld + b;
    o[0] = m.thr;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[(int64_t)(1 + k) * ld] = m.q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[(int64_t)(5 + k) * ld] = m.o[k];
    o[(int64_t)8 * ld] = sqrt(dot3(d[0], d[0]));
    o[(int64_t)9 * ld] = flat_tilt(m.q);
    o[(int64_t)10 * ld] = sqrt(dot3(m.o, m.o));
  }
}

}  // namespace anet
