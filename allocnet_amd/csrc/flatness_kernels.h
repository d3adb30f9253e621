// Differential flatness of a quadrotor with linear + parasitic drag: from (v, a, j, psi, dpsi) to thrust, attitude quaternion
// and body rate, the adjoint of that map, and the kernels built on the two (pointwise, along trajectories, as a penalty of the
// MINCO objective).  One statement of the map (flat_forward) and one of its adjoint (flat_adjoint) serve every kernel form here,
// as lbfgs_step.h does for the optimiser step.
//
// The map, in vector form (e3 = (0, 0, 1); m mass, g gravity, dh / dv horizontal / vertical drag, cp parasitic drag, eps the
// smoothing of the speed):
//   w   = (1 + cp sqrt(|v|^2 + eps)) v
//   zu  = a + (dh/m) w + g e3,            z = zu / |zu|
//   u   = j + (dh/m) dw/dt,               dz = (I - z z^T) u / |zu|
//   thr = z . (m a + dv w + m g e3)
//   q   = tilt(z) * yaw(psi),             tilt(z) = (sqrt(2 (1 + z3)) / 2, -z2 / sqrt(2 (1 + z3)), z1 / sqrt(2 (1 + z3)), 0)
//   omg = body rate of (z, dz, psi, dpsi)
// The adjoint is derived from this forward by hand, step by step in reverse (each block below names the forward step it
// reverses); the tests pin it by automatic differentiation of an independent restatement and by finite differences.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "minco_core.h"     // with_order
#include "penalty_terms.h"  // smoothed_l1, normalised_coeffs

namespace anet {

struct FlatParams {
  double mass, grav, dh, dv, cp, eps;
};

// what the adjoint needs of a forward evaluation (the kernels are stateless: the backward kernel recomputes this)
struct FlatMid {
  double s, wt, dwt, iL, zu_dot, den, iod, ot;
  double w[3], z[3], u[3], dz[3], f[3];
  double ch, sh, cps, sps;  // cos / sin of psi / 2 and of psi
  double thr, q[4], o[3];
};

__device__ __forceinline__ double dot3(const double (&x)[3], const double (&y)[3]) {
  return __builtin_fma(x[2], y[2], __builtin_fma(x[1], y[1], x[0] * y[0]));
}

// YAW = false: psi = dpsi = 0 and no trigonometry (the only caller of the reference's forward passes 0.0, 0.0)
template <bool YAW>
__device__ __forceinline__ void flat_forward(const FlatParams &p, const double (&v)[3], const double (&a)[3], const double (&j)[3],
                                             const double psi, const double dpsi, FlatMid &m) {
  const double dhm = p.dh / p.mass;
  m.s = sqrt(dot3(v, v) + p.eps);
  m.wt = __builtin_fma(p.cp, m.s, 1.0);
  double zu[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    m.w[k] = m.wt * v[k];
    zu[k] = __builtin_fma(dhm, m.w[k], a[k]);
  }
  zu[2] += p.grav;
  m.iL = 1.0 / sqrt(dot3(zu, zu));
#pragma unroll
  for (int k = 0; k < 3; ++k) m.z[k] = zu[k] * m.iL;
  // dw/dt = wt a + (cp v.a / s) v
  m.dwt = p.cp * dot3(v, a) / m.s;
#pragma unroll
  for (int k = 0; k < 3; ++k) m.u[k] = __builtin_fma(dhm, __builtin_fma(m.wt, a[k], m.dwt * v[k]), j[k]);
  m.zu_dot = dot3(m.z, m.u);
#pragma unroll
  for (int k = 0; k < 3; ++k) m.dz[k] = __builtin_fma(-m.z[k], m.zu_dot, m.u[k]) * m.iL;
#pragma unroll
  for (int k = 0; k < 3; ++k) m.f[k] = __builtin_fma(p.mass, a[k], p.dv * m.w[k]);
  m.f[2] = __builtin_fma(p.mass, p.grav, m.f[2]);
  m.thr = dot3(m.z, m.f);
  // tilt quaternion, then the yaw about the body z axis
  m.den = sqrt(2.0 * (1.0 + m.z[2]));
  const double t0 = 0.5 * m.den, t1 = -m.z[1] / m.den, t2 = m.z[0] / m.den;
  if constexpr (YAW) {
    sincos(0.5 * psi, &m.sh, &m.ch);
    sincos(psi, &m.sps, &m.cps);
  } else {
    m.ch = 1.0; m.sh = 0.0; m.cps = 1.0; m.sps = 0.0;
  }
  m.q[0] = t0 * m.ch;
  m.q[1] = __builtin_fma(t1, m.ch, t2 * m.sh);
  m.q[2] = __builtin_fma(t2, m.ch, -(t1 * m.sh));
  m.q[3] = t0 * m.sh;
  // body rate
  m.iod = 1.0 / (1.0 + m.z[2]);
  m.ot = m.dz[2] * m.iod;
  const double A = m.z[0] * m.sps - m.z[1] * m.cps, Bv = m.z[0] * m.cps + m.z[1] * m.sps;
  m.o[0] = m.dz[0] * m.sps - m.dz[1] * m.cps - A * m.ot;
  m.o[1] = m.dz[0] * m.cps + m.dz[1] * m.sps - Bv * m.ot;
  m.o[2] = (m.z[1] * m.dz[0] - m.z[0] * m.dz[1]) * m.iod + (YAW ? dpsi : 0.0);
}

// Adjoint of flat_forward at the point `m` was computed at: upstream gradients of thr, q, omg -> gradients of v, a, j, psi, dpsi.
template <bool YAW>
__device__ __forceinline__ void flat_adjoint(const FlatParams &p, const double (&v)[3], const double (&a)[3], const FlatMid &m,
                                             const double thr_b, const double (&qb)[4], const double (&ob)[3], double (&vb)[3],
                                             double (&ab)[3], double (&jb)[3], double &psib, double &dpsib) {
  const double dhm = p.dh / p.mass;
  double zb[3], dzb[3];
  // omg(z, dz, psi, dpsi)
  dpsib = ob[2];
  psib = ob[0] * m.o[1] - ob[1] * m.o[0];  // d o0 / d psi = o1, d o1 / d psi = -o0
  const double A = m.z[0] * m.sps - m.z[1] * m.cps, Bv = m.z[0] * m.cps + m.z[1] * m.sps;
  const double r0 = ob[0] * m.sps + ob[1] * m.cps, r1 = ob[1] * m.sps - ob[0] * m.cps;
  const double cr = m.z[1] * m.dz[0] - m.z[0] * m.dz[1];
  const double otb = -(ob[0] * A + ob[1] * Bv);
  const double o2i = ob[2] * m.iod;
  dzb[0] = __builtin_fma(o2i, m.z[1], r0);
  dzb[1] = __builtin_fma(-o2i, m.z[0], r1);
  dzb[2] = otb * m.iod;
  zb[0] = -(r0 * m.ot) - o2i * m.dz[1];
  zb[1] = -(r1 * m.ot) + o2i * m.dz[0];
  zb[2] = -(o2i * cr + otb * m.dz[2] * m.iod) * m.iod;  // through 1 / (1 + z3)
  // q(z, psi)
  const double t1 = -m.z[1] / m.den, t2 = m.z[0] / m.den;  // (tilt's w component is den / 2)
  const double t0b = qb[0] * m.ch + qb[3] * m.sh, t1b = qb[1] * m.ch - qb[2] * m.sh, t2b = qb[1] * m.sh + qb[2] * m.ch;
  if constexpr (YAW) psib += 0.5 * (qb[1] * m.q[2] - qb[0] * m.q[3] - qb[2] * m.q[1] + qb[3] * m.q[0]);
  const double iden = 1.0 / m.den;
  const double denb = 0.5 * t0b - (t1b * t1 + t2b * t2) * iden;
  zb[0] = __builtin_fma(t2b, iden, zb[0]);
  zb[1] = __builtin_fma(-t1b, iden, zb[1]);
  zb[2] = __builtin_fma(denb, iden, zb[2]);  // d den / d z3 = 1 / den
  // thr = z . f
  double fb[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    zb[k] = __builtin_fma(thr_b, m.f[k], zb[k]);
    fb[k] = thr_b * m.z[k];
  }
  // dz = (u - z (z.u)) / |zu|
  double rb[3], r[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    rb[k] = dzb[k] * m.iL;
    r[k] = __builtin_fma(-m.z[k], m.zu_dot, m.u[k]);
  }
  const double iLb = dot3(dzb, r), rbz = dot3(rb, m.z);
  double ub[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ub[k] = __builtin_fma(-m.z[k], rbz, rb[k]);
    zb[k] -= __builtin_fma(rb[k], m.zu_dot, m.u[k] * rbz);
  }
  // z = zu / |zu|, 1 / |zu|
  const double zbz = dot3(zb, m.z);
  double zub[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) zub[k] = m.iL * (__builtin_fma(-m.z[k], zbz, zb[k]) - iLb * m.iL * m.z[k]);
  // f = m a + dv w + m g e3;  u = j + (dh/m) dw;  zu = a + (dh/m) w + g e3
  double wb[3], dwb[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    jb[k] = ub[k];
    dwb[k] = dhm * ub[k];
    wb[k] = __builtin_fma(p.dv, fb[k], dhm * zub[k]);
    ab[k] = __builtin_fma(p.mass, fb[k], zub[k]);
  }
  // dw = wt a + dwt v,  dwt = cp (v.a) / s
  double wtb = dot3(dwb, a);
  const double dwtb = dot3(dwb, v);
  const double vab = dwtb * p.cp / m.s;
  double sb = -dwtb * m.dwt / m.s;
  // w = wt v,  wt = 1 + cp s,  s = sqrt(|v|^2 + eps)
  wtb += dot3(wb, v);
  sb = __builtin_fma(p.cp, wtb, sb);
  const double sbs = sb / m.s;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ab[k] = __builtin_fma(m.wt, dwb[k], __builtin_fma(vab, v[k], ab[k]));
    vb[k] = __builtin_fma(m.dwt, dwb[k], __builtin_fma(vab, a[k], __builtin_fma(m.wt, wb[k], sbs * v[k])));
  }
}

// Tilt angle from the quaternion: sin^2(tilt / 2) = q1^2 + q2^2, cos^2(tilt / 2) = q0^2 + q3^2.  process() publishes
// acos(1 - 2 (q1^2 + q2^2)); that form loses a small tilt (1 - 2 x rounds x away: 2 % at 1e-7 rad) and is NaN where x rounds
// above 1 next to inversion.  The half-angle tangent keeps the relative accuracy of q at every tilt in [0, pi].
__device__ __forceinline__ double flat_tilt_of(const double s2, const double c2) { return 2.0 * atan2(sqrt(s2), sqrt(c2)); }
__device__ __forceinline__ double flat_tilt(const double (&q)[4]) {
  return flat_tilt_of(q[1] * q[1] + q[2] * q[2], q[0] * q[0] + q[3] * q[3]);
}

// ------------------------------------------------------------------------------------------
// pointwise: one lane per element
// ------------------------------------------------------------------------------------------
struct FlatFwdArgs {
  const double *vel, *acc, *jer, *psi, *dpsi;
  double *thr, *quat, *omg;
  int64_t n, ld;
  FlatParams fp;
};

__device__ __forceinline__ void load3(const double *p, int64_t ld, int64_t e, double (&x)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) x[k] = p[(int64_t)k * ld + e];
}

template <bool YAW>
__global__ void __launch_bounds__(256) k_flat_forward(FlatFwdArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n) return;
  double v[3], ac[3], j[3];
  load3(a.vel, a.ld, e, v);
  load3(a.acc, a.ld, e, ac);
  load3(a.jer, a.ld, e, j);
  const double psi = (YAW && a.psi) ? a.psi[e] : 0.0, dpsi = (YAW && a.dpsi) ? a.dpsi[e] : 0.0;
  FlatMid m;
  flat_forward<YAW>(a.fp, v, ac, j, psi, dpsi, m);
  a.thr[e] = m.thr;
#pragma unroll
  for (int k = 0; k < 4; ++k) a.quat[(int64_t)k * a.ld + e] = m.q[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) a.omg[(int64_t)k * a.ld + e] = m.o[k];
}

struct FlatBwdArgs {
  const double *vel, *acc, *jer, *psi, *dpsi;
  const double *pos_grad, *vel_grad, *thr_grad, *quat_grad, *omg_grad;
  double *pos_total, *vel_total, *acc_total, *jer_total, *psi_total, *dpsi_total;
  int64_t n, ld;
  FlatParams fp;
};

// FlatnessMap::backward: vel_grad and pos_grad pass through additively (the flat outputs do not depend on the position)
template <bool YAW>
__global__ void __launch_bounds__(256) k_flat_backward(FlatBwdArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n) return;
  const int64_t ld = a.ld;
  double v[3], ac[3], j[3];
  load3(a.vel, ld, e, v);
  load3(a.acc, ld, e, ac);
  load3(a.jer, ld, e, j);
  const double psi = (YAW && a.psi) ? a.psi[e] : 0.0, dpsi = (YAW && a.dpsi) ? a.dpsi[e] : 0.0;
  FlatMid m;
  flat_forward<YAW>(a.fp, v, ac, j, psi, dpsi, m);
  double qb[4], ob[3], vb[3], ab[3], jb[3], psib, dpsib;
#pragma unroll
  for (int k = 0; k < 4; ++k) qb[k] = a.quat_grad[(int64_t)k * ld + e];
  load3(a.omg_grad, ld, e, ob);
  flat_adjoint<true>(a.fp, v, ac, m, a.thr_grad[e], qb, ob, vb, ab, jb, psib, dpsib);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.vel_total[(int64_t)k * ld + e] = vb[k] + (a.vel_grad ? a.vel_grad[(int64_t)k * ld + e] : 0.0);
    a.acc_total[(int64_t)k * ld + e] = ab[k];
    a.jer_total[(int64_t)k * ld + e] = jb[k];
    if (a.pos_total) a.pos_total[(int64_t)k * ld + e] = a.pos_grad ? a.pos_grad[(int64_t)k * ld + e] : 0.0;
  }
  if (a.psi_total) a.psi_total[e] = psib;
  if (a.dpsi_total) a.dpsi_total[e] = dpsib;
}

// ------------------------------------------------------------------------------------------
// along trajectories
// ------------------------------------------------------------------------------------------
// velocity, acceleration, jerk (and, ND = 4, snap) of one piece at local time t: ascending powers, tn *= t, as k_traj_eval
template <int S, int ND>
__device__ __forceinline__ void piece_derivs(const double *cm, const int64_t ld, const double t, double (&d)[ND][3]) {
  constexpr int D = 2 * S, DEG = D - 1;
#pragma unroll
  for (int q = 0; q < ND; ++q) {
    const int dd = q + 1;
    double acc[3] = {0.0, 0.0, 0.0};
    double tn = 1.0;
#pragma unroll
    for (int i = DEG - dd; i >= 0; --i) {
      const int k = DEG - i;
      double f = 1.0;
      for (int e = 0; e < dd; ++e) f *= (double)(k - e);
      const double w = f * tn;
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) acc[ax] += w * cm[(int64_t)(ax * D + i) * ld];
      tn *= t;
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) d[q][ax] = acc[ax];
  }
}

constexpr int kFlatStateFields = 11;  // thr, q0..q3, omg0..2, speed, tilt, body-rate magnitude

struct FlatStatesArgs {
  const double *coeffs, *T, *tq;
  double *out;
  int64_t B, ld;
  int N, nq;
  FlatParams fp;
};

// One lane per trajectory, nq queries: locatePieceIdx as k_traj_eval, then v, a, j at the query and the forward map with
// psi = dpsi = 0; the four numbers process() publishes next to them.
template <int S>
__global__ void __launch_bounds__(256) k_traj_flat_states(FlatStatesArgs a) {
  constexpr int D = 2 * S;
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
    FlatMid m;
    flat_forward<false>(a.fp, d[0], d[1], d[2], 0.0, 0.0, m);
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

struct FlatExtremaArgs {
  const double *coeffs, *T;
  double *out;  // [4][ld]: min thrust, max thrust, max tilt, max body rate
  int64_t B, ld;
  int N, res;
  FlatParams fp;
};

// A SAMPLED check: each piece at t = j T_i / res, j = 0..res, both ends included.  Thrust, tilt and body rate are not polynomials
// in t (they go through 1 / |zu| and a square root), so the root isolation of rate_kernels.h, which bounds |v| and |a| exactly,
// does not apply; between the samples the extrema may be exceeded.
// One lane per (trajectory, piece): 64 trajectories x kFlatExtremaRows piece rows per workgroup (a row takes the pieces
// threadIdx.y, threadIdx.y + rows, ...), then the reduction over the rows through LDS.
constexpr int kFlatExtremaRows = 4;
template <int S>
__global__ void __launch_bounds__(64 * kFlatExtremaRows) k_traj_flat_extrema(FlatExtremaArgs a) {
  constexpr int D = 2 * S, R = kFlatExtremaRows;
  __shared__ double red[R][5][64];
  const int lane = threadIdx.x, row = threadIdx.y;
  const int64_t b = (int64_t)blockIdx.x * 64 + lane;
  const bool live = b < a.B;
  const int64_t bb = live ? b : a.B - 1;  // (every lane reaches the barrier; lanes past the batch write nothing)
  const int64_t ld = a.ld;
  double lo = INFINITY, hi = -INFINITY, tilt_s2 = 0.0, tilt_c2 = INFINITY, bdr2 = 0.0;
  const double inv_res = 1.0 / (double)a.res;
  for (int i = row; i < a.N; i += R) {
    const double Ti = a.T[(int64_t)i * ld + bb];
    const double *cm = a.coeffs + (int64_t)(i * 3 * D) * ld + bb;
    for (int j = 0; j <= a.res; ++j) {
      const double t = (double)j * Ti * inv_res;
      double d[3][3];
      piece_derivs<S, 3>(cm, ld, t, d);
      FlatMid m;
      flat_forward<false>(a.fp, d[0], d[1], d[2], 0.0, 0.0, m);
      lo = fmin(lo, m.thr);
      hi = fmax(hi, m.thr);
      // the tilt grows with sin^2(tilt / 2) and falls with cos^2(tilt / 2): the largest of the one and the smallest of the other
      // (the same sample up to rounding) give the largest tilt, converted once per trajectory
      tilt_s2 = fmax(tilt_s2, m.q[1] * m.q[1] + m.q[2] * m.q[2]);
      tilt_c2 = fmin(tilt_c2, m.q[0] * m.q[0] + m.q[3] * m.q[3]);
      bdr2 = fmax(bdr2, dot3(m.o, m.o));
    }
  }
  red[row][0][lane] = lo;
  red[row][1][lane] = hi;
  red[row][2][lane] = tilt_s2;
  red[row][3][lane] = bdr2;
  red[row][4][lane] = tilt_c2;
  __syncthreads();
  if (row == 0 && live) {
#pragma unroll
    for (int r = 1; r < R; ++r) {
      lo = fmin(lo, red[r][0][lane]);
      hi = fmax(hi, red[r][1][lane]);
      tilt_s2 = fmax(tilt_s2, red[r][2][lane]);
      bdr2 = fmax(bdr2, red[r][3][lane]);
      tilt_c2 = fmin(tilt_c2, red[r][4][lane]);
    }
    a.out[b] = lo;
    a.out[ld + b] = hi;
    a.out[2 * ld + b] = flat_tilt_of(tilt_s2, tilt_c2);
    a.out[3 * ld + b] = sqrt(bdr2);
  }
}

// ------------------------------------------------------------------------------------------
// penalty of the MINCO objective on thrust, tilt and body rate
// ------------------------------------------------------------------------------------------
struct FlatPenalty {
  double w_thr, w_tilt, w_bdr, mu, thr_min, thr_max, cos_tilt_max, bdr_max2;
  int res;
};

struct FlatPieceGradArgs {
  const double *coeffs, *T;
  double *gdC, *gdT, *pcost;
  int64_t B, ld;
  int N, accumulate;
  FlatParams fp;
  FlatPenalty pp;
};

// One lane per (trajectory, piece), blockIdx.y = piece, as k_piece_grad.
//   J_flat = sum_i (T_i/res) sum_{j<res} [ w_thr (phi(thr - thr_max) + phi(thr_min - thr)) + w_tilt phi(cos(tilt_max) - cos(tilt))
//                                        + w_bdr phi(|omg|^2 - bdr_max^2) ]   at t_j = j T_i / res, psi = dpsi = 0,
// phi = smoothed_l1 (penalty_terms.h), cos(tilt) = 1 - 2 (q1^2 + q2^2).  Writes (accumulate: adds) the partial gradients w.r.t. the
// piece's coefficients and duration, and the piece's share of J_flat.
// Normalised time as in k_piece_grad: with c~_k = c_k T^k, d^d p / dt^d (t_j) = T^-d sum_col c~[col] tab[j][d][col].  The rows
// d = 1, 2, 3 are read from k_piece_grad's basis table (wave-uniform index: scalar loads); the snap row d = 4, which only the
// dJ/dT term needs and the table does not hold, is built in registers from tau_j.
//   dJ/dc~ = (T/res) sum_j (vb T^-1 tab1 + ab T^-2 tab2 + jb T^-3 tab3),   dJ/dc_k = T^k dJ/dc~_k
//   dJ/dT  = (1/res) sum_j Phi_j + (T/res) sum_j tau_j (vb.a + ab.j + jb.snap)(t_j)        (coefficients fixed)
// with (vb, ab, jb) the adjoint of the sample's penalty Phi_j.
template <int S>
__global__ void __launch_bounds__(256) k_flat_piece_grad(FlatPieceGradArgs a, const double *__restrict__ tab) {
  constexpr int D = 2 * S;
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const int64_t ld = a.ld;
  const int i = blockIdx.y;
  const FlatPenalty pp = a.pp;
  const double Ti = a.T[(int64_t)i * ld + b];
  double ct[3][D];  // c~
  {
    const double *cm = a.coeffs + (int64_t)(i * 3 * D) * ld + b;
    double c[3][D];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
#pragma unroll
      for (int col = 0; col < D; ++col) c[ax][col] = cm[(int64_t)(ax * D + col) * ld];
    normalised_coeffs<S>(c, Ti, ct);
  }
  double gN[3][D];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax)
#pragma unroll
    for (int col = 0; col < D; ++col) gN[ax][col] = 0.0;
  const double inv_mu = 1.0 / pp.mu, inv_res = 1.0 / (double)pp.res;
  const double rT = 1.0 / Ti, rT2 = rT * rT, rT3 = rT2 * rT, rT4 = rT2 * rT2;
  double csum = 0.0, gts = 0.0;
  for (int j = 0; j < pp.res; ++j) {
    const double *tb = tab + (size_t)j * 4 * D;
    const double tau = (double)j * inv_res;
    double t4[D];  // k (k-1) (k-2) (k-3) tau^(k-4), column col holds power k = D - 1 - col
    {
      double tn = 1.0;
#pragma unroll
      for (int col = D - 1; col >= 0; --col) {
        const int k = D - 1 - col;
        if (k < 4) {
          t4[col] = 0.0;
        } else {
          t4[col] = (double)(k * (k - 1) * (k - 2) * (k - 3)) * tn;
          tn *= tau;
        }
      }
    }
    double v[3], ac[3], jr[3], sn[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      double x1 = 0.0, x2 = 0.0, x3 = 0.0, x4 = 0.0;
#pragma unroll
      for (int col = 0; col < D; ++col) {
        x1 = __builtin_fma(ct[ax][col], tb[D + col], x1);
        x2 = __builtin_fma(ct[ax][col], tb[2 * D + col], x2);
        x3 = __builtin_fma(ct[ax][col], tb[3 * D + col], x3);
        x4 = __builtin_fma(ct[ax][col], t4[col], x4);
      }
      v[ax] = x1 * rT; ac[ax] = x2 * rT2; jr[ax] = x3 * rT3; sn[ax] = x4 * rT4;
    }
    FlatMid m;
    flat_forward<false>(a.fp, v, ac, jr, 0.0, 0.0, m);
    double f, df, phi, thr_b, qb[4] = {0.0, 0.0, 0.0, 0.0}, ob[3];
    smoothed_l1(pp.mu, inv_mu, m.thr - pp.thr_max, f, df);
    phi = pp.w_thr * f;
    thr_b = pp.w_thr * df;
    smoothed_l1(pp.mu, inv_mu, pp.thr_min - m.thr, f, df);
    phi = __builtin_fma(pp.w_thr, f, phi);
    thr_b = __builtin_fma(-pp.w_thr, df, thr_b);
    const double q12 = m.q[1] * m.q[1] + m.q[2] * m.q[2];
    smoothed_l1(pp.mu, inv_mu, pp.cos_tilt_max - (1.0 - 2.0 * q12), f, df);
    phi = __builtin_fma(pp.w_tilt, f, phi);
    qb[1] = 4.0 * pp.w_tilt * df * m.q[1];
    qb[2] = 4.0 * pp.w_tilt * df * m.q[2];
    smoothed_l1(pp.mu, inv_mu, dot3(m.o, m.o) - pp.bdr_max2, f, df);
    phi = __builtin_fma(pp.w_bdr, f, phi);
#pragma unroll
    for (int k = 0; k < 3; ++k) ob[k] = 2.0 * pp.w_bdr * df * m.o[k];
    csum += phi;
    if (__any(phi > 0.0)) {  // wave-uniform: inside every limit the adjoint is not computed (its inputs are all zero)
      double vb[3], ab[3], jb[3], psib, dpsib;
      flat_adjoint<false>(a.fp, v, ac, m, thr_b, qb, ob, vb, ab, jb, psib, dpsib);
      gts = __builtin_fma(tau, dot3(vb, ac) + dot3(ab, jr) + dot3(jb, sn), gts);
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        const double s1 = vb[ax] * rT, s2 = ab[ax] * rT2, s3 = jb[ax] * rT3;
#pragma unroll
        for (int col = 0; col < D; ++col)
          gN[ax][col] = __builtin_fma(s3, tb[3 * D + col], __builtin_fma(s2, tb[2 * D + col], __builtin_fma(s1, tb[D + col], gN[ax][col])));
      }
    }
  }
  const double step = Ti * inv_res;
  {
    double tk = step;  // (T/res) T^k
#pragma unroll
    for (int col = D - 1; col >= 0; --col) {
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        double *g = a.gdC + (int64_t)((i * 3 + ax) * D + col) * ld + b;
        const double val = gN[ax][col] * tk;
        *g = a.accumulate ? add_unfused(*g, val) : val;
      }
      tk *= Ti;
    }
  }
  const double gT = __builtin_fma(step, gts, csum * inv_res), pc = step * csum;
  double *g = a.gdT + (int64_t)i * ld + b;
  *g = a.accumulate ? add_unfused(*g, gT) : gT;
  if (a.pcost) {
    double *c = a.pcost + (int64_t)i * ld + b;
    *c = a.accumulate ? add_unfused(*c, pc) : pc;
  }
}

}  // namespace anet
