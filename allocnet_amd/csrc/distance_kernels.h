// The exact Euclidean distance field of the voxel map, its trilinear query, and the obstacle penalty of the MINCO objective.
//
// FIELD (anet_voxel_distance_dev).  sd2[v] is the SIGNED SQUARED distance in voxel units, an exact integer: for a free v
// + min over blocked u of |v - u|^2, for a blocked v - min over free u of |v - u|^2, +-kDistNone for a minimum over nothing.  With
// `walls` the voxels outside the map count as blocked.  |v - u|^2 separates by axis, so three passes of the one-dimensional min-plus
// transform  out[i] = min_j (g[j] + (i - j)^2)  along x, y, z give it exactly.  Both polarities share ONE int32 array through all
// three passes: after every pass value > 0 <=> free and value < 0 <=> blocked, a pass reads g+ = max(s, 0) and g- = max(-s, 0) of a
// line and a free voxel needs only the envelope of g+ (its g- is 0 and stays 0), a blocked one only that of g-.  So a lane forms ONE
// envelope, of g(j) = max(sigma s[j], 0) with sigma its own sign, and writes sigma * result.  Walls are two virtual sources of g+
// with value 0 at -1 and `size`, in every pass.
// THE PASS is a pruned brute-force min-plus over the line in LDS: lane at i starts from best = g[i] (and the walls) and looks at
// i - d, i + d for d = 1, 2, ... while d^2 < best -- every candidate is >= d^2, so the loop may stop there and the result is exact.
// On a map with obstacles the loop ends after about the distance to the nearest one, which is what makes it cheaper here than the
// parabola envelope of Felzenszwalb-Huttenlocher (a serial stack per line: one lane per line, strided LDS or global traffic) or
// Meijster's two scans; its worst case, a line with one far source, is size reads per voxel, bounded by the 4096 limit.  A lane whose
// polarity has no source anywhere in its workgroup's run of lines (x pass) or tile (y, z) skips the loop: two flags per run or tile,
// set while it is staged, not per line -- a line without a source next to one that has one still walks its full reach.  Arithmetic is uint32:
// finite values are <= 3 * 4096^2 < 2^26, kDistNone + d^2 < 2^32 never wraps and never beats best.
//   k_vox_dist_x     the lines along x are contiguous: a workgroup stages a contiguous run of whole lines straight from the bytes,
//                    four bytes per load where the run is word-aligned, and writes int32.
//   k_vox_dist_axis  y and z: a workgroup stages a tile of `tx` adjacent x times the whole line ([line][tx] in LDS, every global
//                    access a run of tx int32 along x), then overwrites it in place -- no scratch beyond sd2.  64 KiB of LDS:
//                    two workgroups of 512 lanes per CU.
// No atomics, deterministic, no scratch.
//
// QUERY (dist_sample: k_vox_dist_query and the penalty).  Centre value D(v) = scale sgn(sd2) sqrt(|sd2|); per axis
// u = (p - oc) / scale (not contracted), i0 = clamp(floor(u), 0, max(size - 2, 0)), f = clamp(u - i0, 0, 1), i1 = min(i0 + 1,
// size - 1); dist = the trilinear interpolant, grad = its gradient inside the cell / scale (an IEEE division), 0 on an axis where f
// was clamped or size == 1: beyond the outermost centres the field continues as a constant.  The sums of the interpolant may be
// contracted into FMAs (only u and f are protected).  The eight loads are issued before the first sqrt.
//
// PENALTY (k_minco_obstacle).  k_minco_avoid without its neighbour loop: one workgroup per trajectory, durations and coefficients
// staged in LDS, lanes over the flattened samples (i, j) in rounds of kObsBlock, Phi, F[3], H = sigma (F . v), tau of a sample left
// in LDS, then output row r = (i, ax, k) | (i, Phi) | (i, H) contracted by lane r mod kObsBlock in ascending j into an accumulator
// kept across the rounds (two rows per lane at most: N (3 D + 2) <= 416).  No atomics, no workspace; the bits of trajectory b do not
// depend on the launch or on ld.  `accumulate`: one unfused addition of the complete share (add_unfused).
// SIBLING: k_minco_stop (stop_kernels.h) is this kernel with the velocity and acceleration rows of the chain rule added and equals it
// to the bit at a_brake = inf, t_react = 0 (tests/test_stop_penalty_gpu.py): a change to the staging, the rounds, the contraction order
// or the NaN rule here is made there too.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "dist_query.h"     // kDistNone, DistGrid, dist_axis, dist_sample
#include "penalty_terms.h"  // smoothed_l1, add_unfused

namespace anet {

constexpr int kDistMaxAxis = 4096;
constexpr int kDistXBlock = 256;
constexpr int kDistXCap = 4096;           // int32 of LDS of k_vox_dist_x: one line of the longest axis
constexpr int kDistXRun = 1024;           // lines are grouped into runs of about this many voxels
constexpr int kDistAxisBlock = 512;
constexpr int kDistAxisCap = 16384;       // int32 of LDS of k_vox_dist_axis, two flag words included: 64 KiB, two workgroups per CU
constexpr int kDistAxisMaxTx = 128;

// out(i) = min(g(i), walls, min_j g(j) + (i - j)^2) over the line s[0 .. L) with element stride `st` in LDS; g(j) = max(sg s[j], 0)
__device__ __forceinline__ uint32_t dist_line_min(const int32_t *s, const int st, const int L, const int i, const int sg,
                                                  const bool walls) {
  auto g = [&](const int j) { return (uint32_t)max(sg * s[j * st], 0); };
  uint32_t best = g(i);
  if (walls) {
    const uint32_t w = (uint32_t)min(i + 1, L - i);
    best = min(best, w * w);
  }
  const int reach = max(i, L - 1 - i);
  for (int d = 1; d <= reach; ++d) {
    const uint32_t dd = (uint32_t)d * (uint32_t)d;
    if (dd >= best) break;
    if (i - d >= 0) best = min(best, g(i - d) + dd);
    if (i + d < L) best = min(best, g(i + d) + dd);
  }
  return min(best, (uint32_t)kDistNone);
}

// x pass, from the bytes: workgroup `blockIdx.x` takes `rows` consecutive lines (a contiguous run of rows * sx voxels)
__global__ void __launch_bounds__(kDistXBlock) k_vox_dist_x(const uint8_t *__restrict__ vox, int32_t *__restrict__ sd2, const int sx,
                                                            const int64_t n_lines, const int rows, const int walls) {
  __shared__ int32_t line[kDistXCap];
  __shared__ int32_t has[2];  // the run holds a source of g+ (a blocked voxel) / of g- (a free one): a skip only, never a value
  const int tid = threadIdx.x;
  const int64_t l0 = (int64_t)blockIdx.x * rows;
  const int nl = (int)min((int64_t)rows, n_lines - l0);
  const int cnt = nl * sx;  // <= kDistXCap (the launch)
  const int64_t base = l0 * sx;
  if (tid < 2) has[tid] = 0;
  __syncthreads();
  // the bytes, a word at a time where the word lies inside the array and the pointer is word-aligned
  const int lead = (int)((4 - ((uintptr_t)(vox + base) & 3)) & 3);  // bytes in front of the first aligned word
  bool any_b = false, any_f = false;
  auto put = [&](const int e, const uint32_t byte) {
    const bool b = byte != 0;
    line[e] = b ? -kDistNone : kDistNone;
    any_b |= b;
    any_f |= !b;
  };
  for (int e = tid; e < min(lead, cnt); e += kDistXBlock) put(e, vox[base + e]);
  const int words = cnt > lead ? (cnt - lead) / 4 : 0;
  for (int wi = tid; wi < words; wi += kDistXBlock) {
    const uint32_t w = *(const uint32_t *)(vox + base + lead + 4 * (int64_t)wi);
#pragma unroll
    for (int k = 0; k < 4; ++k) put(lead + 4 * wi + k, (w >> (8 * k)) & 0xffu);
  }
  for (int e = lead + 4 * words + tid; e < cnt; e += kDistXBlock) put(e, vox[base + e]);
  if (any_b) has[0] = 1;
  if (any_f) has[1] = 1;
  __syncthreads();
  const bool src_b = has[0] != 0 || walls, src_f = has[1] != 0;
  for (int e = tid; e < cnt; e += kDistXBlock) {
    const int r = e / sx, i = e - r * sx;
    const int32_t own = line[e];
    const int sg = own > 0 ? 1 : -1;
    uint32_t out = (uint32_t)kDistNone;
    if (sg > 0 ? src_b : src_f) out = dist_line_min(line + r * sx, 1, sx, i, sg, sg > 0 && walls);
    sd2[base + e] = sg * (int32_t)out;
  }
}

// y or z pass, in place: the tile x in [x0, x0 + tx) of line (blockIdx.y), L elements `stride` apart; tx = 1 << tx_log2
__global__ void __launch_bounds__(kDistAxisBlock) k_vox_dist_axis(int32_t *__restrict__ sd2, const int sx, const int L,
                                                                  const int64_t stride, const int64_t outer_stride, const int tx_log2,
                                                                  const int walls) {
  __shared__ int32_t tile[kDistAxisCap];
  int32_t *has = tile + kDistAxisCap - 2;  // the tile holds a source of g+ / of g-; the launch leaves these two words free
  const int tid = threadIdx.x, tx = 1 << tx_log2;
  const int x0 = blockIdx.x * tx, w = min(tx, sx - x0);
  int32_t *p = sd2 + (int64_t)blockIdx.y * outer_stride + x0;
  const int cnt = L * tx;  // <= kDistAxisCap - 2 (the launch)
  if (tid < 2) has[tid] = 0;
  __syncthreads();
  bool any_b = false, any_f = false;
  for (int e = tid; e < cnt; e += kDistAxisBlock) {
    const int l = e >> tx_log2, xl = e & (tx - 1);
    if (xl < w) {
      const int32_t v = p[(int64_t)l * stride + xl];
      tile[e] = v;
      any_b |= v != kDistNone;   // a source of g+: a blocked voxel, or a free one with a finite value
      any_f |= v != -kDistNone;  // a source of g-
    }
  }
  if (any_b) has[0] = 1;
  if (any_f) has[1] = 1;
  __syncthreads();
  const bool src_b = has[0] != 0 || walls, src_f = has[1] != 0;
  for (int e = tid; e < cnt; e += kDistAxisBlock) {
    const int l = e >> tx_log2, xl = e & (tx - 1);
    if (xl >= w) continue;
    const int32_t own = tile[e];
    const int sg = own > 0 ? 1 : -1;
    // without a source of its polarity anywhere in the tile the value stands (it is kDistNone: a source would have shown)
    const uint32_t out = (sg > 0 ? src_b : src_f) ? dist_line_min(tile + xl, tx, L, l, sg, sg > 0 && walls) : (uint32_t)abs(own);
    p[(int64_t)l * stride + xl] = sg * (int32_t)out;
  }
}

// ---- the query -----------------------------------------------------------------------------------------------------------------
// (DistGrid, dist_axis, dist_sample: dist_query.h)
__global__ void __launch_bounds__(256) k_vox_dist_query(const DistGrid g, const int32_t *__restrict__ sd2,
                                                        const double *__restrict__ pos, const int64_t n, double *__restrict__ dist,
                                                        double *__restrict__ grad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double d, gx, gy, gz;
  dist_sample(g, sd2, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], d, gx, gy, gz);
  dist[i] = d;
  if (grad) {
    grad[3 * i] = gx;
    grad[3 * i + 1] = gy;
    grad[3 * i + 2] = gz;
  }
}

// ---- the penalty ---------------------------------------------------------------------------------------------------------------
constexpr int kObsBlock = 256;
constexpr int kObsMaxPieces = 16;  // ANET_MAX_PIECES (checked where the launch is)

struct ObstacleArgs {
  const double *coeffs, *T;    // [(i*3+ax)*2S + col][ld], [N][ld]
  const int32_t *sd2;
  double *gdC, *gdT, *pcost;   // pcost may be nullptr
  int64_t B, ld;
  int N, res, accumulate;
  double w, mu, clearance;
  DistGrid g;
};

// sigma and tau of a sample: one rounding each, never contracted
__device__ __forceinline__ void obstacle_sample_time(const int j, const int res, const double Ti, double &sigma, double &tau) {
#pragma clang fp contract(off)
  sigma = (double)j / (double)res;
  tau = sigma * Ti;
}

template <int S>
struct ObstacleShared {
  static constexpr int D = 2 * S;
  static constexpr int kRows = 3 * D + 2;  // output rows per piece: 3 D coefficients, Phi, H
  double eT[kObsMaxPieces];
  double eC[kObsMaxPieces * 3 * D];
  double smp[6][kObsBlock];                // Phi, F[3], H, tau of this round's samples
  double sums[kObsMaxPieces * 2];          // per piece: sum Phi, sum H
  int32_t bad;
};

template <int S>
__global__ void __launch_bounds__(kObsBlock) k_minco_obstacle(const ObstacleArgs a) {
  using Sh = ObstacleShared<S>;
  constexpr int D = Sh::D, kRows = Sh::kRows;
  __shared__ Sh sh;
  const int tid = threadIdx.x, N = a.N, res = a.res;
  const int64_t b = blockIdx.x, ld = a.ld;
  const double inv_mu = 1.0 / a.mu;

  if (tid < N) sh.eT[tid] = a.T[(int64_t)tid * ld + b];
  for (int e = tid; e < N * 3 * D; e += kObsBlock) sh.eC[e] = a.coeffs[(int64_t)e * ld + b];
  if (tid == 0) sh.bad = 0;
  __syncthreads();
  bool t_bad = false;
  for (int i = 0; i < N; ++i) {
    const double Ti = sh.eT[i];
    t_bad = t_bad || !(fabs(Ti) < INFINITY) || !(Ti > 0.0);
  }

  const int total_rows = N * kRows;
  const int row0 = tid, row1 = tid + kObsBlock;
  const int pi0 = row0 / kRows, q0 = row0 % kRows, pi1 = row1 / kRows, q1 = row1 % kRows;
  double acc0 = 0.0, acc1 = 0.0;

  const int64_t M = (int64_t)N * res;
  for (int64_t base = 0; base < M && !t_bad; base += kObsBlock) {
    const int64_t gs = base + tid;
    const bool has = gs < M;
    const int i = has ? (int)(gs / res) : 0, j = has ? (int)(gs % res) : 0;
    double sigma, tau;
    obstacle_sample_time(j, res, sh.eT[i], sigma, tau);
    double pb[3], vb[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const double *c = sh.eC + (i * 3 + ax) * D;
      double p = c[0], v = 0.0;
#pragma unroll
      for (int col = 1; col < D; ++col) {
        v = __builtin_fma(v, tau, p);
        p = __builtin_fma(p, tau, c[col]);
      }
      pb[ax] = p;
      vb[ax] = v;
    }
    double Phi = 0.0, F0 = 0.0, F1 = 0.0, F2 = 0.0;
    if (has) {
      double d, gx, gy, gz;
      dist_sample(a.g, a.sd2, pb[0], pb[1], pb[2], d, gx, gy, gz);
      if (!(d > -INFINITY)) sh.bad = 1;  // NaN (a non-finite position) or -inf (the all-blocked map)
      double f, df;
      smoothed_l1(a.mu, inv_mu, a.clearance - d, f, df);
      const double k = -a.w * df;
      Phi = a.w * f;
      F0 = k * gx;
      F1 = k * gy;
      F2 = k * gz;
    }
    __syncthreads();  // (smp[] of the previous round has been read)
    sh.smp[0][tid] = Phi;
    sh.smp[1][tid] = F0;
    sh.smp[2][tid] = F1;
    sh.smp[3][tid] = F2;
    sh.smp[4][tid] = sigma * __builtin_fma(F2, vb[2], __builtin_fma(F1, vb[1], F0 * vb[0]));
    sh.smp[5][tid] = tau;
    __syncthreads();
    auto contract = [&](const int row, const int pi, const int q, double &acc) {
      if (row >= total_rows) return;
      const int64_t lo = max((int64_t)pi * res, base), hi = min((int64_t)(pi + 1) * res, min(base + kObsBlock, M));
      const int src = q < 3 * D ? 1 + q / D : (q == 3 * D ? 0 : 4);
      const int pw = q < 3 * D ? D - 1 - q % D : 0;
      for (int64_t gg = lo; gg < hi; ++gg) {
        const int l = (int)(gg - base);
        double term = sh.smp[src][l];
        const double tl = sh.smp[5][l];
        for (int e = 0; e < pw; ++e) term *= tl;
        acc += term;
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

}  // namespace anet
