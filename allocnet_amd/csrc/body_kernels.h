// Whole-body corridor terms: the vertices b_k of a body-fixed polytope, rotated by the attitude the trajectory itself implies
// (flat_forward<false>, psi = dpsi = 0), against the rows of the piece's corridor polytope -- as a penalty of the MINCO objective
// with its partial gradients (k_body_piece_grad) and as a sampled margin (k_traj_body_margin).  Semantics: include/allocnet_amd.h.
//
// R(q) is the homogeneous quadratic form of the quaternion q = (w, v):  R b = (w^2 - v.v) b + 2 (v.b) v + 2 w (v x b).  For
// g = a . R(q) b:   dg/dw = 2 w (a.b) + 2 a.(v x b),   dg/dv = -2 (a.b) v + 2 (v.b) a + 2 (a.v) b + 2 w (b x a).
// q(v, a) stays on the unit sphere and flat_adjoint applies the exact Jacobian of q, so the radial part of the quaternion's
// gradient is annihilated: any extension of R off the sphere gives the same composed gradient.
// With weights c = w phi'(g) summed over rows and vertices, only
//     pb = sum c a_r  (3 values)   and   Ab = sum c a_r b_k^T  (9 values)
// are accumulated across the loops; with tr = trace(Ab) and x = sum c (b x a) (the antisymmetric part of Ab)
//     qb_w = 2 w tr + 2 v.x,      qb_v = -2 tr v + 2 (Ab + Ab^T) v + 2 w x.
// q does not depend on the jerk (only the body rate does), so the adjoint returns jb = 0 and the jerk enters dJ/dT alone.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "flatness_kernels.h"  // flat_forward, flat_adjoint, piece_derivs, dot3
#include "penalty_terms.h"     // smoothed_l1, normalised_coeffs, add_unfused

namespace anet {

constexpr int kMaxBodyVerts = 16;  // ANET_MAX_BODY_VERTS

// the body: K vertices in the body frame, shared by the batch (kernel argument: every read of it is a scalar load)
struct BodyVerts {
  double b[kMaxBodyVerts][3];
  double rmax;  // max_k |b_k|
  int K;
};

// rotation matrix of the quaternion, homogeneous form (row-major)
__device__ __forceinline__ void body_rot(const double (&q)[4], double (&R)[3][3]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
  R[0][0] = ww + xx - yy - zz; R[0][1] = 2.0 * (x * y - w * z);  R[0][2] = 2.0 * (x * z + w * y);
  R[1][0] = 2.0 * (x * y + w * z);  R[1][1] = ww - xx + yy - zz; R[1][2] = 2.0 * (y * z - w * x);
  R[2][0] = 2.0 * (x * z - w * y);  R[2][1] = 2.0 * (y * z + w * x);  R[2][2] = ww - xx - yy + zz;
}

struct BodyPieceGradArgs {
  const double *coeffs, *T, *hpolys;
  double *gdC, *gdT, *pcost;
  int64_t B, ld;
  int N, accumulate, res, M;
  double w, mu;
  FlatParams fp;
  BodyVerts body;
};

// One lane per (trajectory, piece), blockIdx.y = piece, in normalised time as k_flat_piece_grad:
//   J_body = sum_i (T_i/res) sum_{j<res} sum_r sum_k  w phi( a_r . (p(t_j) + R(q(t_j)) b_k) - h_r ),   t_j = j T_i / res.
// The state rows d = 0..3 are read from k_piece_grad's basis table (wave-uniform index: scalar loads).  Per sample: p, v, a, j
// and the forward map; per row (read per lane, coalesced) ra = R^T a_r once, then g = (a_r.p - h_r) + ra.b_k per vertex; the
// row's weights are summed into (cs, m = sum c b_k) and leave the row loop as pb += cs a_r, Ab += a_r m^T.  A row with
// a_r.p - h_r + |a_r| max|b_k| <= 0 has phi = 0 at every vertex and skips them (padding rows, all zero, are such rows).
//   dJ/dc~ = (T/res) sum_j (pb tab0 + vb T^-1 tab1 + ab T^-2 tab2),   dJ/dc_k = T^k dJ/dc~_k
//   dJ/dT  = (1/res) sum_j Phi_j + (T/res) sum_j tau_j (pb.v + vb.a + ab.j)(t_j)        (coefficients fixed)
// A sample at which no lane of the wave has an active term skips the adjoint and the gradient update (wave-uniform branch):
// far from the rows cost and gradients are exactly 0.  No atomics, no workspace, no array indexed at run time.
template <int S>
__global__ void __launch_bounds__(256) k_body_piece_grad(BodyPieceGradArgs a, const double *__restrict__ tab) {
  constexpr int D = 2 * S;
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const int64_t ld = a.ld;
  const int i = blockIdx.y;
  const int M = a.M, K = a.body.K;
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
  const double mu = a.mu, inv_mu = 1.0 / mu, inv_res = 1.0 / (double)a.res, wgt = a.w, rmax = a.body.rmax;
  const double rT = 1.0 / Ti, rT2 = rT * rT, rT3 = rT2 * rT;
  const double *hp = a.hpolys + (int64_t)(i * M * 4) * ld + b;
  double csum = 0.0, gts = 0.0;
  for (int j = 0; j < a.res; ++j) {
    const double *tb = tab + (size_t)j * 4 * D;
    const double tau = (double)j * inv_res;
    double p[3], v[3], ac[3], jr[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0;
#pragma unroll
      for (int col = 0; col < D; ++col) {
        x0 = __builtin_fma(ct[ax][col], tb[col], x0);
        x1 = __builtin_fma(ct[ax][col], tb[D + col], x1);
        x2 = __builtin_fma(ct[ax][col], tb[2 * D + col], x2);
        x3 = __builtin_fma(ct[ax][col], tb[3 * D + col], x3);
      }
      p[ax] = x0; v[ax] = x1 * rT; ac[ax] = x2 * rT2; jr[ax] = x3 * rT3;
    }
    FlatMid m;
    flat_forward<false>(a.fp, v, ac, jr, 0.0, 0.0, m);
    double R[3][3];
    body_rot(m.q, R);
    double phi = 0.0, pb[3] = {0.0, 0.0, 0.0}, Ab[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int r = 0; r < M; ++r) {
      const double *row = hp + (int64_t)(r * 4) * ld;
      const double ar[3] = {row[0], row[ld], row[2 * ld]};
      const double g0 = dot3(ar, p) - row[3 * ld];
      if (__builtin_fma(sqrt(dot3(ar, ar)), rmax, g0) <= 0.0) continue;  // (a NaN goes on and reaches every output of the piece)
      double ra[3];  // R^T a_r
#pragma unroll
      for (int c = 0; c < 3; ++c) ra[c] = __builtin_fma(ar[2], R[2][c], __builtin_fma(ar[1], R[1][c], ar[0] * R[0][c]));
      double cs = 0.0, mv[3] = {0.0, 0.0, 0.0};
      for (int k = 0; k < K; ++k) {
        const double b0 = a.body.b[k][0], b1 = a.body.b[k][1], b2 = a.body.b[k][2];
        const double g = __builtin_fma(ra[2], b2, __builtin_fma(ra[1], b1, __builtin_fma(ra[0], b0, g0)));
        double f, df;
        smoothed_l1(mu, inv_mu, g, f, df);
        phi += f;
        cs += df;
        mv[0] = __builtin_fma(df, b0, mv[0]);
        mv[1] = __builtin_fma(df, b1, mv[1]);
        mv[2] = __builtin_fma(df, b2, mv[2]);
      }
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        pb[x] = __builtin_fma(cs, ar[x], pb[x]);
#pragma unroll
        for (int c = 0; c < 3; ++c) Ab[x][c] = __builtin_fma(ar[x], mv[c], Ab[x][c]);
      }
    }
    csum += phi;
    if (__any(!(phi <= 0.0))) {  // wave-uniform: with no active term in the wave the adjoint's inputs are all zero (NaN counts as active)
      // (the weight w_body enters here once: phi, pb, Ab are sums of phi and phi')
      const double qv[3] = {m.q[1], m.q[2], m.q[3]};
      const double tr = Ab[0][0] + Ab[1][1] + Ab[2][2];
      const double xa[3] = {Ab[2][1] - Ab[1][2], Ab[0][2] - Ab[2][0], Ab[1][0] - Ab[0][1]};  // sum c (b x a)
      double qb[4];
      qb[0] = 2.0 * wgt * __builtin_fma(m.q[0], tr, dot3(qv, xa));
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        double sv = 0.0;  // ((Ab + Ab^T) v)_x
#pragma unroll
        for (int c = 0; c < 3; ++c) sv = __builtin_fma(Ab[x][c] + Ab[c][x], qv[c], sv);
        qb[1 + x] = 2.0 * wgt * (__builtin_fma(m.q[0], xa[x], sv) - tr * qv[x]);
      }
      const double ob[3] = {0.0, 0.0, 0.0};
      double vb[3], ab[3], jb[3], psib, dpsib;
      flat_adjoint<false>(a.fp, v, ac, m, 0.0, qb, ob, vb, ab, jb, psib, dpsib);
      double pw[3];
#pragma unroll
      for (int x = 0; x < 3; ++x) pw[x] = wgt * pb[x];
      gts = __builtin_fma(tau, dot3(pw, v) + dot3(vb, ac) + dot3(ab, jr), gts);
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        const double s1 = vb[ax] * rT, s2 = ab[ax] * rT2;
#pragma unroll
        for (int col = 0; col < D; ++col)
          gN[ax][col] = __builtin_fma(s2, tb[2 * D + col], __builtin_fma(s1, tb[D + col], __builtin_fma(pw[ax], tb[col], gN[ax][col])));
      }
    }
  }
  csum *= wgt;
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

struct BodyMarginArgs {
  const double *coeffs, *T, *hpolys;
  double *margin, *t;    // [N][ld]; t may be nullptr
  int32_t *row, *vert;   // [N][ld] or nullptr
  int64_t B, ld;
  int N, res, M;
  FlatParams fp;
  BodyVerts body;
};

// A SAMPLED check, as k_traj_flat_extrema: the attitude is no polynomial in t, so nothing bounds the margin between the samples.
// One lane per (trajectory, piece), blockIdx.y = piece; the output is per piece, so nothing is reduced across lanes.  Per sample
// t = j T_i / res, j = 0..res (both ends): p, v, a, j in ascending powers of t as k_traj_eval, the forward map, then
// a_r . p - h_r + (R^T a_r) . b_k over the non-padding rows and the vertices; the first maximum in (sample, row, vertex) order is kept
// with its t, row and vertex.  No row: -inf (row, vert -1, t 0).  A non-finite coefficient, duration or row field: NaN (the same).
template <int S>
__global__ void __launch_bounds__(64) k_traj_body_margin(BodyMarginArgs a) {
  constexpr int D = 2 * S, DEG = D - 1;
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int i = blockIdx.y;
  const int64_t ld = a.ld;
  const int64_t o = (int64_t)i * ld + b;
  const int M = a.M, K = a.body.K;
  const double Ti = a.T[o];
  const double *cm = a.coeffs + (int64_t)(i * 3 * D) * ld + b;
  const double *hp = a.hpolys + (int64_t)(i * M * 4) * ld + b;
  bool bad = !(fabs(Ti) < INFINITY);
#pragma unroll
  for (int f = 0; f < 3 * D; ++f) bad = bad || !(fabs(cm[(int64_t)f * ld]) < INFINITY);
  for (int r = 0; r < M * 4; ++r) bad = bad || !(fabs(hp[(int64_t)r * ld]) < INFINITY);
  double best = -INFINITY, bt = 0.0;
  int brow = -1, bvert = -1;
  const double inv_res = 1.0 / (double)a.res;
  for (int j = 0; j <= (bad ? -1 : a.res); ++j) {
    const double t = (double)j * Ti * inv_res;
    double p[3] = {0.0, 0.0, 0.0};
    {
      double tn = 1.0;
#pragma unroll
      for (int col = DEG; col >= 0; --col) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) p[ax] += tn * cm[(int64_t)(ax * D + col) * ld];
        tn *= t;
      }
    }
    double d[3][3];
    piece_derivs<S, 3>(cm, ld, t, d);
    FlatMid m;
    flat_forward<false>(a.fp, d[0], d[1], d[2], 0.0, 0.0, m);
    double R[3][3];
    body_rot(m.q, R);
    for (int r = 0; r < M; ++r) {
      const double *row = hp + (int64_t)(r * 4) * ld;
      const double ar[3] = {row[0], row[ld], row[2 * ld]}, h = row[3 * ld];
      if (ar[0] == 0.0 && ar[1] == 0.0 && ar[2] == 0.0 && h == 0.0) continue;  // padding
      const double g0 = dot3(ar, p) - h;
      double ra[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) ra[c] = __builtin_fma(ar[2], R[2][c], __builtin_fma(ar[1], R[1][c], ar[0] * R[0][c]));
      for (int k = 0; k < K; ++k) {
        const double g = __builtin_fma(ra[2], a.body.b[k][2], __builtin_fma(ra[1], a.body.b[k][1], __builtin_fma(ra[0], a.body.b[k][0], g0)));
        if (g > best) { best = g; brow = r; bvert = k; bt = t; }
      }
    }
  }
  a.margin[o] = bad ? NAN : best;
  if (a.t) a.t[o] = bt;
  if (a.row) a.row[o] = brow;
  if (a.vert) a.vert[o] = bvert;
}

}  // namespace anet
