// The shortest smoothed polyline through a corridor with one point in every overlap: upstream GCOPTER's getShortestPath in the
// variables of sfc_param_kernels.h (anet_sfc_shortest_path*, api_sfc.hip; include/allocnet_amd.h).
//
// A problem has N polytopes; P_0 = start and P_N = goal are fixed, P_w(xi) for w = 1 .. N-1 is the transform of
// sfc_param_kernels.h on the vertices of overlap(polytope w-1, polytope w): K variables xi per waypoint, padded slots hold 0.
//   cost       L(xi) = sum_{i=0}^{N-1} sqrt(|P_{i+1} - P_i|^2 + eps^2)  +  w_norm sum_w max(S_w - 1, 0)^3        (eps in metres)
//   in P       dL/dP_w = (P_w - P_{w-1}) / l_{w-1} - (P_{w+1} - P_w) / l_w,   l_i the smoothed length of leg i
//   in xi      dL/dxi_j = 2 xi_j ((v_j - P_w) . dL/dP_w) / S_w + 6 w_norm max(S_w - 1, 0)^2 xi_j      (exactly 0 in a padded slot)
// Both terms and the chain to xi are those of sfc_param_kernels.h, restated here because one evaluation is ONE launch.
//
// Launch shape of k_sfc_path_eval: one lane per PROBLEM, 256 lanes per workgroup, the waypoints in sequence.  The lane keeps
// P_{w-1}, P_w, P_{w+1} and S_w, S_{w+1} in registers: the forward pass over the rows of waypoint w + 1 gives the second leg of
// waypoint w, then the gradient pass reads the rows of waypoint w again.  The cost is so summed by the lane itself, legs in
// ascending order and then the norm terms in ascending order: no atomics, nothing shared between lanes, and a batch with one
// problem changed returns the same bits for the others.  Layout batch-minor with the row stride ld of the L-BFGS state
// (xi[(w K + j)][ld], verts[((w K + j) 3 + a)][ld], start / goal [3][ld]): every load and store of a wave is one contiguous
// 512-byte row segment.  Per problem the kernel requests 8 ((N-1) (8 K read + K written) + 7) bytes; 8 ((N-1) 5 K + 7) of them
// are compulsory (every xi and vertex row once, every gradient row once, start, goal, cost) -- the second read of a waypoint's
// rows comes 4 K rows after the first.  A lane per (problem, waypoint) would recompute both neighbours (16 K rows read per
// waypoint) and leave the cost to one lane that needs every leg.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "workspace_constants.h"   // IS_*

namespace anet {

constexpr int kSfcPathBlock = 256;

struct SfcPathPoint { double x, y, z, S; };

// S = sum_j xi_j^2, P = (sum_j xi_j^2 v_j) / S of waypoint row block (x, v); S = 0 gives P = 0
__device__ inline SfcPathPoint sfc_path_forward(const double *x, const double *v, int64_t ld, int K) {
  double S = 0.0, px = 0.0, py = 0.0, pz = 0.0;
  for (int j = 0; j < K; ++j) {
    const double q = x[(int64_t)j * ld], q2 = q * q;
    S += q2;
    px += q2 * v[(int64_t)(3 * j) * ld];
    py += q2 * v[(int64_t)(3 * j + 1) * ld];
    pz += q2 * v[(int64_t)(3 * j + 2) * ld];
  }
  const double inv = S > 0.0 ? 1.0 / S : 0.0;
  return SfcPathPoint{px * inv, py * inv, pz * inv, S};
}

// xi [(nwp K)][ld], verts [(nwp K 3)][ld], start / goal [3][ld] -> f [ld], g [(nwp K)][ld]; nwp = N - 1 >= 1 waypoints.
// grid ceil(B / 256).
__global__ void __launch_bounds__(kSfcPathBlock) k_sfc_path_eval(const double *xi, const double *verts, const double *start,
                                                                 const double *goal, int64_t B, int64_t ld, int nwp, int K,
                                                                 double eps2, double w_norm, double *f, double *g) {
  const int64_t b = (int64_t)blockIdx.x * kSfcPathBlock + threadIdx.x;
  if (b >= B) return;
  const int64_t wx = (int64_t)K * ld, wv = 3 * wx;   // rows of one waypoint
  const double *x = xi + b, *v = verts + b;
  double *gw = g + b;
  double ax = start[b], ay = start[ld + b], az = start[2 * ld + b];        // P_{w-1}
  SfcPathPoint c = sfc_path_forward(x, v, ld, K);                           // P_w
  double dx = c.x - ax, dy = c.y - ay, dz = c.z - az;
  double la = sqrt(dx * dx + dy * dy + dz * dz + eps2);                     // leg into P_w
  double legs = la, norms = 0.0;
  for (int w = 0; w < nwp; ++w) {
    SfcPathPoint n;                                                         // P_{w+1}
    if (w + 1 < nwp) n = sfc_path_forward(x + wx, v + wv, ld, K);
    else n = SfcPathPoint{goal[b], goal[ld + b], goal[2 * ld + b], 0.0};
    const double ex = n.x - c.x, ey = n.y - c.y, ez = n.z - c.z;
    const double lb = sqrt(ex * ex + ey * ey + ez * ez + eps2);             // leg out of P_w
    legs += lb;
    const double gx = dx / la - ex / lb, gy = dy / la - ey / lb, gz = dz / la - ez / lb;
    const double inv2 = c.S > 0.0 ? 2.0 / c.S : 0.0, over = c.S > 1.0 ? c.S - 1.0 : 0.0;
    const double cn = 6.0 * w_norm * over * over;
    norms += w_norm * over * over * over;
    for (int j = 0; j < K; ++j) {
      const double q = x[(int64_t)j * ld];
      const double dot = (v[(int64_t)(3 * j) * ld] - c.x) * gx + (v[(int64_t)(3 * j + 1) * ld] - c.y) * gy +
                         (v[(int64_t)(3 * j + 2) * ld] - c.z) * gz;
      gw[(int64_t)j * ld] = q * (dot * inv2) + cn * q;
    }
    c = n; dx = ex; dy = ey; dz = ez; la = lb;
    x += wx; v += wv; gw += wx;
  }
  f[b] = legs + norms;
}

// start from the vertex mean: xi_j = 1 / sqrt(k) for j < k, else 0 -- for the problems that run (`is`: the IS_* rows after
// k_sfc_mark_no_overlap; a problem marked with `code` keeps its xi).  grid (ceil(B / 256), N - 1).
__global__ void __launch_bounds__(kSfcPathBlock) k_sfc_path_mean_start(const int32_t *count, const int *is, int64_t B, int64_t ld,
                                                                       int K, int code, double *xi) {
  const int64_t b = (int64_t)blockIdx.x * kSfcPathBlock + threadIdx.x;
  if (b >= B) return;
  if (is[(int64_t)IS_DONE * ld + b] && is[(int64_t)IS_RET * ld + b] == code) return;
  const int w = blockIdx.y, k = count[(int64_t)w * ld + b];
  const double x0 = k > 0 ? 1.0 / sqrt((double)k) : 0.0;
  for (int j = 0; j < K; ++j) xi[(int64_t)(w * K + j) * ld + b] = j < k ? x0 : 0.0;
}

// x <-> xi around the run (row blockIdx.y); mode 1 leaves the xi of a problem that did not run.  grid (ceil(B / 256), (N-1) K).
__global__ void __launch_bounds__(kSfcPathBlock) k_sfc_path_map(double *x, double *xi, const int *is, int64_t B, int64_t ld, int code,
                                                                int mode) {
  const int64_t b = (int64_t)blockIdx.x * kSfcPathBlock + threadIdx.x;
  if (b >= B) return;
  const int64_t i = (int64_t)blockIdx.y * ld + b;
  if (mode == 0) { x[i] = xi[i]; return; }
  if (is[(int64_t)IS_DONE * ld + b] && is[(int64_t)IS_RET * ld + b] == code) return;
  xi[i] = x[i];
}

// the unsmoothed length sum_i |P_{i+1} - P_i| of start, wps [3 (N-1)][ld], goal, legs in ascending order; NaN for a problem that
// did not run.  grid ceil(B / 256).
__global__ void __launch_bounds__(kSfcPathBlock) k_sfc_path_length(const double *start, const double *goal, const double *wps,
                                                                   const int *is, int64_t B, int64_t ld, int nwp, int code,
                                                                   double *length) {
  const int64_t b = (int64_t)blockIdx.x * kSfcPathBlock + threadIdx.x;
  if (b >= B) return;
  if (is[(int64_t)IS_DONE * ld + b] && is[(int64_t)IS_RET * ld + b] == code) { length[b] = __builtin_nan(""); return; }
  double ax = start[b], ay = start[ld + b], az = start[2 * ld + b], len = 0.0;
  for (int w = 0; w <= nwp; ++w) {
    const double *p = w < nwp ? wps + (int64_t)(3 * w) * ld : goal;
    const double cx = p[b], cy = p[ld + b], cz = p[2 * ld + b];
    const double dx = cx - ax, dy = cy - ay, dz = cz - az;
    len += sqrt(dx * dx + dy * dy + dz * dz);
    ax = cx; ay = cy; az = cz;
  }
  length[b] = len;
}

}  // namespace anet
