// Waypoints as vertex weights of corridor overlaps: the unconstrained variable of the corridor-constrained MINCO L-BFGS
// (anet_lbfgs_minco_sfc*, api_sfc.hip; include/allocnet_amd.h).
//
// For waypoint w = 0 .. N-2 of a problem, v_0 .. v_{k-1} are the vertices of overlap(polytope w, polytope w + 1), padded with
// zero rows to a common K; the waypoint has K variables xi_{w,0..K-1}, variable j belongs to vertex j, padded slots hold 0.
//   forward    S = sum_j xi_j^2,   P_w = (sum_j xi_j^2 v_j) / S        a convex combination of the vertices for every xi != 0
//   gradient   dJ/dxi_j = 2 xi_j ((v_j - P_w) . dJ/dP_w) / S          (exactly 0 in a padded slot, which so stays 0)
//   norm       P_w depends on xi / |xi| only, so the gradient is orthogonal to xi and |xi| can only grow along a run:
//              w_norm max(S - 1, 0)^3 per waypoint joins the cost, 6 w_norm max(S - 1, 0)^2 xi_j the gradient
//   inverse    backward_p: minimise |P_w(xi) - p|^2 over xi from the vertex mean xi_j = 1 / sqrt(k) (j < k); the minimiser is
//              not unique for k > 4 -- P_w(xi) and the distance |P_w(xi) - p| are the results, and a p outside the overlap keeps
//              a positive distance
// This is upstream GCOPTER's forwardP / backwardGradP / backwardP (gcopter.hpp), with the weight of v_0 carried as an ordinary
// entry instead of as the last one (upstream stores v_0 and the edges v_j - v_0; the point is the same).
//
// Layout: batch-minor with the common row stride ld, as the L-BFGS workspace:  xi[(w K + j)][ld],  verts[((w K + j) 3 + a)][ld],
// count[w][ld] (int32),  waypoints [(3 w + a)][ld] as the cost + gradient kernels read them.
// Launch shape of the transform kernels: one lane per (problem, waypoint), blockIdx.y = w, 256 lanes per workgroup: every
// load and store of a wave is one contiguous row segment (512 bytes), there is no LDS and nothing is shared between lanes.
// They stream 8 (4 K + 5) bytes (forward) and 8 (4 K + 7) + 8 K bytes (backward) per lane plus the three norm rows.
// The sum over the waypoints of a problem's norm terms is taken by ONE lane per problem in a fixed order (the lane of w = 0 in
// k_sfc_backward_grad), not by atomics: results do not depend on the order in which workgroups run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "minco_core.h"            // forward_T, backward_T
#include "workspace_constants.h"   // IS_*

namespace anet {

constexpr int kSfcBlock = 256;

// ---- corridor -> stacked overlaps -> batch-minor vertices ---------------------------------------------------------------------
// hpolys [N M 4][ld] (a.x <= b, zero rows padding) -> stacked [(w B + b)][2 M][4] in the raw form h.[x;1] <= 0 (column 3 negated):
// rows 0..M-1 polytope w, rows M..2M-1 polytope w + 1.  grid (ceil(B / 256), (N - 1) * 2 M).
__global__ void __launch_bounds__(kSfcBlock) k_sfc_pack_overlaps(const double *hpolys, int64_t B, int64_t ld, int M, double *stacked) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b >= B) return;
  const int w = blockIdx.y / (2 * M), r = blockIdx.y % (2 * M);
  const int poly = r < M ? w : w + 1, row = r < M ? r : r - M;
  const double *src = hpolys + ((int64_t)(poly * M + row) * 4) * ld + b;
  double *dst = stacked + (((int64_t)w * B + b) * 2 * M + r) * 4;
  dst[0] = src[0];
  dst[1] = src[ld];
  dst[2] = src[2 * ld];
  dst[3] = -src[3 * ld];
}

// what the enumeration left ([(w B + b)][K][3], count, status per stacked polytope) -> verts / count / status batch-minor.  An
// overlap of more than K vertices keeps its first K (still a convex subset of the overlap): count is clamped and status says
// truncated.  Slots behind count are written as zeros.  grid (ceil(B / 256), N - 1).
__global__ void __launch_bounds__(kSfcBlock) k_sfc_pack_vertices(const double *v_in, const int32_t *count_in, const int32_t *status_in,
                                                                 int64_t B, int64_t ld, int K, double *verts, int32_t *count,
                                                                 int32_t *status) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b >= B) return;
  const int w = blockIdx.y;
  const int64_t p = (int64_t)w * B + b;
  const int k_true = count_in[p], k = k_true < K ? k_true : K;
  const double *src = v_in + p * K * 3;
  double *dst = verts + (int64_t)w * K * 3 * ld + b;
  for (int j = 0; j < K; ++j)
    for (int a = 0; a < 3; ++a) dst[(int64_t)(j * 3 + a) * ld] = j < k ? src[j * 3 + a] : 0.0;
  count[(int64_t)w * ld + b] = k;
  if (status) status[(int64_t)w * ld + b] = status_in[p];
}

// ---- the transform ---------------------------------------------------------------------------------------------------------------
// norm: three rows per waypoint, [3 (N - 1)][ld]: rows w: 1 / S; rows (N - 1) + w: w_norm max(S - 1, 0)^3; rows 2 (N - 1) + w:
// 6 w_norm max(S - 1, 0)^2.  S = 0 (no start point given for a waypoint without an overlap) gives P = 0 and 1 / S = 0.
__global__ void __launch_bounds__(kSfcBlock) k_sfc_forward_p(const double *xi, const double *verts, int64_t B, int64_t ld, int K,
                                                             double w_norm, double *wps, double *norm) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b >= B) return;
  const int w = blockIdx.y, nwp = gridDim.y;
  const double *x = xi + (int64_t)w * K * ld + b, *v = verts + (int64_t)w * K * 3 * ld + b;
  double S = 0.0, px = 0.0, py = 0.0, pz = 0.0;
  for (int j = 0; j < K; ++j) {
    const double q = x[(int64_t)j * ld], q2 = q * q;
    S += q2;
    px += q2 * v[(int64_t)(3 * j) * ld];
    py += q2 * v[(int64_t)(3 * j + 1) * ld];
    pz += q2 * v[(int64_t)(3 * j + 2) * ld];
  }
  const double inv = S > 0.0 ? 1.0 / S : 0.0;
  wps[(int64_t)(3 * w) * ld + b] = px * inv;
  wps[(int64_t)(3 * w + 1) * ld + b] = py * inv;
  wps[(int64_t)(3 * w + 2) * ld + b] = pz * inv;
  const double over = S > 1.0 ? S - 1.0 : 0.0;
  norm[(int64_t)w * ld + b] = inv;
  norm[(int64_t)(nwp + w) * ld + b] = w_norm * over * over * over;
  norm[(int64_t)(2 * nwp + w) * ld + b] = 6.0 * w_norm * over * over;
}

// grad_xi_j = 2 xi_j ((v_j - P) . grad_p) / S + 6 w_norm max(S - 1, 0)^2 xi_j; cost (or nullptr): cost[b] += sum_w of the norm
// cost rows, added by the lane of w = 0 in ascending w.
__global__ void __launch_bounds__(kSfcBlock) k_sfc_backward_grad(const double *xi, const double *verts, const double *wps,
                                                                 const double *norm, const double *grad_p, int64_t B, int64_t ld,
                                                                 int K, double *grad_xi, double *cost) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b >= B) return;
  const int w = blockIdx.y, nwp = gridDim.y;
  const double *x = xi + (int64_t)w * K * ld + b, *v = verts + (int64_t)w * K * 3 * ld + b;
  double *g = grad_xi + (int64_t)w * K * ld + b;
  const double Px = wps[(int64_t)(3 * w) * ld + b], Py = wps[(int64_t)(3 * w + 1) * ld + b], Pz = wps[(int64_t)(3 * w + 2) * ld + b];
  const double gx = grad_p[(int64_t)(3 * w) * ld + b], gy = grad_p[(int64_t)(3 * w + 1) * ld + b],
               gz = grad_p[(int64_t)(3 * w + 2) * ld + b];
  const double inv2 = 2.0 * norm[(int64_t)w * ld + b], cn = norm[(int64_t)(2 * nwp + w) * ld + b];
  for (int j = 0; j < K; ++j) {
    const double q = x[(int64_t)j * ld];
    const double dot = (v[(int64_t)(3 * j) * ld] - Px) * gx + (v[(int64_t)(3 * j + 1) * ld] - Py) * gy +
                       (v[(int64_t)(3 * j + 2) * ld] - Pz) * gz;
    g[(int64_t)j * ld] = q * (dot * inv2) + cn * q;
  }
  if (cost && w == 0) {
    double f = cost[b];
    for (int i = 0; i < nwp; ++i) f += norm[(int64_t)(nwp + i) * ld + b];
    cost[b] = f;
  }
}

// ---- backward_p: the batch of (N - 1) * ld problems of K variables each ---------------------------------------------------------
// Problem q = w ld + b, row stride ldq = (N - 1) ld: x[j][ldq], f[ldq], g[j][ldq] are an L-BFGS state of n = K (workspace.h).
// f = |P(x) - p|^2, g_j = 4 x_j ((v_j - P) . (P - p)) / S.  Lanes b >= B are marked finished at the start and skipped here.
__global__ void __launch_bounds__(kSfcBlock) k_sfc_tiny_nls(const double *x, const double *verts, const double *p, int64_t B,
                                                            int64_t ld, int K, double *f, double *g) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b >= B) return;
  const int w = blockIdx.y;
  const int64_t ldq = (int64_t)gridDim.y * ld, q = (int64_t)w * ld + b;
  const double *v = verts + (int64_t)w * K * 3 * ld + b;
  double S = 0.0, px = 0.0, py = 0.0, pz = 0.0;
  for (int j = 0; j < K; ++j) {
    const double t = x[(int64_t)j * ldq + q], t2 = t * t;
    S += t2;
    px += t2 * v[(int64_t)(3 * j) * ld];
    py += t2 * v[(int64_t)(3 * j + 1) * ld];
    pz += t2 * v[(int64_t)(3 * j + 2) * ld];
  }
  const double inv = S > 0.0 ? 1.0 / S : 0.0;
  px *= inv; py *= inv; pz *= inv;
  const double rx = px - p[(int64_t)(3 * w) * ld + b], ry = py - p[(int64_t)(3 * w + 1) * ld + b], rz = pz - p[(int64_t)(3 * w + 2) * ld + b];
  f[q] = rx * rx + ry * ry + rz * rz;
  const double inv4 = 4.0 * inv;
  for (int j = 0; j < K; ++j) {
    const double t = x[(int64_t)j * ldq + q];
    const double dot = (v[(int64_t)(3 * j) * ld] - px) * rx + (v[(int64_t)(3 * j + 1) * ld] - py) * ry +
                       (v[(int64_t)(3 * j + 2) * ld] - pz) * rz;
    g[(int64_t)j * ldq + q] = t * (dot * inv4);
  }
}

// start of backward_p: x_j = 1 / sqrt(k) for j < k, else 0; a waypoint without a vertex (and every lane b >= B of the padded row)
// is marked finished.  `is`: the IS_* rows of the L-BFGS state, zeroed by the caller.  grid (ceil(ld / 256), N - 1).
__global__ void __launch_bounds__(kSfcBlock) k_sfc_tiny_start(const int32_t *count, int64_t B, int64_t ld, int K, double *x, int *is) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b >= ld) return;
  const int w = blockIdx.y;
  const int64_t ldq = (int64_t)gridDim.y * ld, q = (int64_t)w * ld + b;
  const int k = b < B ? count[q] : 0;
  const double x0 = k > 0 ? 1.0 / sqrt((double)k) : 0.0;
  for (int j = 0; j < K; ++j) x[(int64_t)j * ldq + q] = j < k ? x0 : 0.0;
  if (k < 1) {
    is[(int64_t)IS_DONE * ldq + q] = 1;
    is[(int64_t)IS_RET * ldq + q] = 0;
  }
}

// no start waypoints: xi at the vertex mean in the layout of the transform, residual 0.  grid (ceil(B / 256), N - 1).
__global__ void __launch_bounds__(kSfcBlock) k_sfc_mean_start(const int32_t *count, int64_t B, int64_t ld, int K, double *xi,
                                                              double *residual) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b >= B) return;
  const int w = blockIdx.y, k = count[(int64_t)w * ld + b];
  const double x0 = k > 0 ? 1.0 / sqrt((double)k) : 0.0;
  for (int j = 0; j < K; ++j) xi[(int64_t)(w * K + j) * ld + b] = j < k ? x0 : 0.0;
  residual[(int64_t)w * ld + b] = 0.0;
}

// end of backward_p: xi = x / |x| in the layout of the transform, residual[w][ld] = |P(xi) - p| (+inf for a waypoint without a
// vertex, whose xi is 0).
__global__ void __launch_bounds__(kSfcBlock) k_sfc_tiny_finish(const double *x, const double *verts, const double *p,
                                                               const int32_t *count, int64_t B, int64_t ld, int K, double *xi,
                                                               double *residual) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b >= B) return;
  const int w = blockIdx.y;
  const int64_t ldq = (int64_t)gridDim.y * ld, q = (int64_t)w * ld + b;
  const double *v = verts + (int64_t)w * K * 3 * ld + b;
  double *out = xi + (int64_t)w * K * ld + b;
  double S = 0.0;
  for (int j = 0; j < K; ++j) {
    const double t = x[(int64_t)j * ldq + q];
    S += t * t;
  }
  if (count[q] < 1 || !(S > 0.0)) {
    for (int j = 0; j < K; ++j) out[(int64_t)j * ld] = 0.0;
    residual[q] = __builtin_inf();
    return;
  }
  const double scale = 1.0 / sqrt(S);
  double S1 = 0.0, px = 0.0, py = 0.0, pz = 0.0;
  for (int j = 0; j < K; ++j) {
    const double t = x[(int64_t)j * ldq + q] * scale, t2 = t * t;
    out[(int64_t)j * ld] = t;
    S1 += t2;
    px += t2 * v[(int64_t)(3 * j) * ld];
    py += t2 * v[(int64_t)(3 * j + 1) * ld];
    pz += t2 * v[(int64_t)(3 * j + 2) * ld];
  }
  const double inv = 1.0 / S1;
  const double rx = px * inv - p[(int64_t)(3 * w) * ld + b], ry = py * inv - p[(int64_t)(3 * w + 1) * ld + b],
               rz = pz * inv - p[(int64_t)(3 * w + 2) * ld + b];
  residual[q] = sqrt(rx * rx + ry * ry + rz * rz);
}

// ---- the two ends of an optimisation over x = (xi rows, tau rows) ------------------------------------------------------------------
// A problem with a waypoint of fewer than two vertices, or whose enumeration found no interior (status 1), does not run: it is
// marked finished with `code` before the first evaluation and its xi and T are never written.  status may be nullptr.
__global__ void __launch_bounds__(kSfcBlock) k_sfc_mark_no_overlap(const int32_t *count, const int32_t *status, int64_t B, int64_t ld,
                                                                   int nwp, int code, int *is) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b >= B) return;
  bool bad = false;
  for (int w = 0; w < nwp; ++w) bad = bad || count[(int64_t)w * ld + b] < 2 || (status && status[(int64_t)w * ld + b] == 1);
  if (bad) {
    is[(int64_t)IS_DONE * ld + b] = 1;
    is[(int64_t)IS_RET * ld + b] = code;
  }
}

// mode 0: (xi, T) -> x before the first evaluation; mode 1: x -> (xi, T) for the problems that ran.  Row blockIdx.y of x: [0, nxi)
// xi, [nxi, nxi + nt) tau.  grid (ceil(B / 256), nxi + nt).
__global__ void __launch_bounds__(kSfcBlock) k_sfc_map(double *x, double *xi, double *T, const int *is, int64_t B, int64_t ld, int nxi,
                                                       int code, int mode) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b >= B) return;
  const int v = blockIdx.y;
  const int64_t i = (int64_t)v * ld + b;
  if (mode == 0) {
    x[i] = v < nxi ? xi[i] : backward_T(T[(int64_t)(v - nxi) * ld + b]);
    return;
  }
  if (is[(int64_t)IS_DONE * ld + b] && is[(int64_t)IS_RET * ld + b] == code) return;
  if (v < nxi) xi[i] = x[i];
  else T[(int64_t)(v - nxi) * ld + b] = forward_T(x[i]);
}

// a problem that did not run has no cost
__global__ void __launch_bounds__(kSfcBlock) k_sfc_no_cost(const int *is, int64_t B, int64_t ld, int code, double *cost) {
  const int64_t b = (int64_t)blockIdx.x * kSfcBlock + threadIdx.x;
  if (b < B && is[(int64_t)IS_DONE * ld + b] && is[(int64_t)IS_RET * ld + b] == code) cost[b] = __builtin_nan("");
}

}  // namespace anet
