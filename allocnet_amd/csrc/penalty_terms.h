// The corridor / velocity / acceleration penalty J_pen on scalars: the smoothed L1, the per-piece scales, the normalised
// coefficients and the terms of one sample, written once for the kernel forms that evaluate it --
//   piece_penalty_part (minco_kernels.h: lane per (trajectory, piece), its SPLIT / sample-split shapes, and the vector phase 2
//     of the one-launch evaluation, minco_fused_kernel.h),
//   mx_column_set + mx_pair_epilogue (piece_grad_mx.h: k_piece_grad_mx and the MX phase 2 of the one-launch evaluation),
//   persist_eval, phase E4 (lbfgs_minco_persistent.h: the one-launch L-BFGS run).
// A form owns its data movement and its shape: where the basis rows come from (scalar loads, LDS, Horner rows, matrix
// operands), how the weights s1 / s2 reach the gradient, which wave-uniform test stands in front of a block, and how it
// obtains the reciprocals 1 / T, 1 / mu, 1 / res.  Every function here is arithmetic on values the caller holds; none
// changes a rounding or an order of summation of the form that calls it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace anet {

struct Penalty {
  double rho, wc, wv, wa, mu, vmax, amax;
  int res, M;
};
// From the penalty of the C ABI (P: anet_penalty; a template so that this header stands without the C header).  M: the corridor
// rows per piece the launch walks -- the caller's poly_rows, or 0 where it has no rows.
template <class P>
inline Penalty to_kernel_penalty(const P &pen, int M) {
  return {pen.rho, pen.w_corridor, pen.w_vel, pen.w_acc, pen.smooth_mu, pen.max_vel, pen.max_acc, pen.res, M};
}

// firi::smoothedL1 (gcopter/firi.hpp:60-84), 0 below 0.
__device__ __forceinline__ void smoothed_l1(double mu, double inv_mu, double x, double &f, double &df) {
  const double xd = x * inv_mu, sq = xd * xd, mm = __builtin_fma(-0.5, x, mu);
  double fm = mm * sq * xd, dm = sq * __builtin_fma(-0.5, xd, 3.0 * mm * inv_mu);
  const bool hi = x > mu, neg = x < 0.0;
  f = neg ? 0.0 : (hi ? x - 0.5 * mu : fm);
  df = neg ? 0.0 : (hi ? 1.0 : dm);
}

// The same function in units of mu and without selects: smoothed L1 of x = mu u is mu F(u), its slope F'(u), with
// F(u) = uc^3 (1 - uc/2) + max(u - 1, 0), F'(u) = uc^2 (3 - 2 uc), uc = clamp(u, 0, 1).
__device__ __forceinline__ void smoothed_l1_unit(double u, double &F, double &dF) {
  const double w = fmax(u, 0.0), uc = fmin(w, 1.0), sq = uc * uc;
  F = __builtin_fma(sq * uc, __builtin_fma(-0.5, uc, 1.0), w - uc);
  dF = sq * __builtin_fma(-2.0, uc, 3.0);
}

// The constants of one piece: weights times mu (the sample costs are sums of F), the limits in units of mu
// (u = |a1| kv - cv, |a2| ka - ca from the normalised-time sums a1 = T v, a2 = T^2 a), the weights K1, K2 of a limit's
// slope in the gradient w.r.t. c~, and the quadrature step T / res.  The reciprocals are inputs: the forms obtain them
// differently (rT an IEEE division, fast_rcp or the chain's own 1 / T; inv_mu, inv_res on the device or on the host).
// The corridor weight K0 is the caller's: step wcm where the normals are held divided by mu, step wc where they are not.
struct PieceScales {
  double wcm, wvm, wam, kv, ka, cv, ca, K1, K2, step;
};
__device__ __forceinline__ PieceScales piece_scales(const Penalty &pp, const double Ti, const double rT, const double inv_mu,
                                                    const double inv_res) {
  const double rT2 = rT * rT, step = Ti * inv_res;
  return {pp.wc * pp.mu, pp.wv * pp.mu, pp.wa * pp.mu, rT * inv_mu, rT2 * inv_mu, pp.vmax * inv_mu, pp.amax * inv_mu,
          step * rT * pp.wv, step * rT2 * pp.wa, step};
}

// Normalised time: c~_k = c_k T^k (column col holds the power k = D - 1 - col), so that the states at sample j depend on
// tau_j = j / res only, and back: d/dc_k = T^k d/dc~_k, added to gC or in place.  (C: anything c[ax][col] reads, e.g. padded rows.)
template <int S, class C>
__device__ __forceinline__ void normalised_coeffs(const C &c, const double Ti, double (&ct)[3][2 * S]) {
  double tk = 1.0;
#pragma unroll
  for (int col = 2 * S - 1; col >= 0; --col) {
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) ct[ax][col] = c[ax][col] * tk;
    tk *= Ti;
  }
}
template <int S>
__device__ __forceinline__ void add_coeff_grad(const double (&gN)[3][2 * S], const double Ti, double (&gC)[3][2 * S]) {
  double tk = 1.0;
#pragma unroll
  for (int col = 2 * S - 1; col >= 0; --col) {
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) gC[ax][col] = __builtin_fma(gN[ax][col], tk, gC[ax][col]);
    tk *= Ti;
  }
}
template <int S>
__device__ __forceinline__ void scale_coeff_grad(double (&gC)[3][2 * S], const double Ti) {
  double tk = 1.0;
#pragma unroll
  for (int col = 2 * S - 1; col >= 0; --col) {
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) gC[ax][col] *= tk;
    tk *= Ti;
  }
}

// The velocity / acceleration limits of ONE AXIS of one sample from a1 = sum c~ tab', a2 = sum c~ tab'': adds the cost (in
// units of step) to `cost` and the share of Rs = (Rs1 + 2 Rs2) / T to Rs1 / Rs2, returns the weights s1, s2 the rows tab',
// tab'' enter the gradient w.r.t. c~ with.  Only one of +v, -v (+a, -a) can be violated: the slope has the sign of a1 (a2).
// The wave-uniform test in front stays with the caller, and so does the loop over the axes: the lane forms spend s1, s2 on
// the gradient axis by axis, and a function of the three axes at once keeps six weights alive across that --
// k_piece_grad<4, false, 1> went from 28 to 132 bytes of scratch, k_piece_grad<3, true, 4> from two waves per SIMD to one.
// limit_terms_masked: mask(f, df) is applied to each row's F and F' before they are used -- E4 of the one-launch L-BFGS run
// zeroes them in the lanes whose sample does not exist; limit_terms is the same with nothing applied.
template <class Mask>
__device__ __forceinline__ void limit_terms_masked(const PieceScales &k, const double a1, const double a2, double &cost,
                                                   double &Rs1, double &Rs2, double &s1, double &s2, Mask &&mask) {
  double f, df;
  smoothed_l1_unit(__builtin_fma(fabs(a1), k.kv, -k.cv), f, df);
  mask(f, df);
  cost = __builtin_fma(k.wvm, f, cost);
  s1 = k.K1 * copysign(df, a1);
  Rs1 = __builtin_fma(s1, a1, Rs1);
  smoothed_l1_unit(__builtin_fma(fabs(a2), k.ka, -k.ca), f, df);
  mask(f, df);
  cost = __builtin_fma(k.wam, f, cost);
  s2 = k.K2 * copysign(df, a2);
  Rs2 = __builtin_fma(s2, a2, Rs2);
}
__device__ __forceinline__ void limit_terms(const PieceScales &k, const double a1, const double a2, double &cost, double &Rs1,
                                            double &Rs2, double &s1, double &s2) {
  limit_terms_masked(k, a1, a2, cost, Rs1, Rs2, s1, s2, [](double &, double &) {});
}

// One corridor row at one sample, u = (a.p - b) / mu with h = (a, b / mu): adds F(u) to Fs and F'(u) a to G.  F goes into
// Fs in two updates (the linear part, then the cubic one by an FMA).  E4 of the one-launch L-BFGS run adds
// smoothed_l1_unit's F in ONE addition instead -- another rounding -- and keeps that written out: its bits feed an
// optimiser run whose iterates the tests pin, so the two are not to be converged in passing.
__device__ __forceinline__ void corridor_row_terms(const double u, const double (&h)[4], double &Fs, double &G0, double &G1,
                                                   double &G2) {
  const double w = fmax(u, 0.0), uc = fmin(w, 1.0), sq = uc * uc;
  Fs += w - uc;
  Fs = __builtin_fma(sq * uc, __builtin_fma(-0.5, uc, 1.0), Fs);
  const double df = sq * __builtin_fma(-2.0, uc, 3.0);
  G0 = __builtin_fma(df, h[0], G0);
  G1 = __builtin_fma(df, h[1], G1);
  G2 = __builtin_fma(df, h[2], G2);
}

// d/dT at fixed c.  The quadrature weight T / res gives csum / res; the sample times t_j = tau_j T move with T, and since
// tau tab[j][d+1][col] = (k - d) tab[j][d][col] their part is (1/T) (acc - (Rs1 + 2 Rs2)) with
// acc = sum_col c~[col] k gN[col] over the first NCOL columns (the last one has k = 0) and gN the gradient w.r.t. c~.
template <int S, int NCOL>
__device__ __forceinline__ double sample_time_moment(const double (&ct)[3][2 * S], const double (&gN)[3][2 * S]) {
  double acc = 0.0;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax)
#pragma unroll
    for (int col = 0; col < NCOL; ++col) acc = __builtin_fma(ct[ax][col] * (double)(2 * S - 1 - col), gN[ax][col], acc);
  return acc;
}
__device__ __forceinline__ double duration_grad(const double csum, const double inv_res, const double rT, const double acc,
                                                const double Rs1, const double Rs2) {
  return csum * inv_res + rT * (acc - __builtin_fma(2.0, Rs2, Rs1));
}

// old + v in two roundings, never one fused operation: with `accumulate` the result of k_flat_piece_grad and k_minco_avoid is bit for
// bit the sum of the two separate results
__device__ __forceinline__ double add_unfused(double old, double v) {
#pragma clang fp contract(off)
  return old + v;
}

}  // namespace anet
