// Front-end route on the device voxel map: sfc_gen::planPath's contract (a collision-free polyline from s to g, its length
// as the cost) by a resolution-complete shortest-path field, a walk back along it and a line-of-sight shortcut.
//   free voxel   vox == 0 and its centre posI2D(id) = id * scale + oc inside the box [lb, hb]
//   graph        26 neighbours, integer weights 10 / 14 / 17 (face / edge / corner); a move by d is an edge only when the
//                whole 2x2(x2) block it spans, cur + e with e_i in {0, d_i}, is free (no corner cutting)
//   k_path_init          field = UINT32_MAX, the start voxel 0, the start tile active for round 0; activity words "never"
//   k_path_relax         one round: each active tile loads its distances and free bytes with a one-voxel halo into LDS,
//                        relaxes in place until a sweep changes nothing (or the sweep cap), writes back the voxels it
//                        changed and stamps the neighbour tiles its changed boundary voxels touch (itself if capped) active
//                        for the next round.  No flags are read within a launch: a tile that read a stale halo value is
//                        re-run in the next launch, where it sees the new one.  Values only decrease and every value read,
//                        stale or not, is the length of a real path, so the fixed point is the exact field whatever the
//                        schedule (and equal to a CPU Dijkstra's: integer sums).
//   k_path_goal          per problem: start / goal tests and the status
//   k_path_nearest_*     APPROXIMATE only: two passes over the reached voxels, the least squared distance of a centre to g,
//                        then the lowest id at it (atomic min on the double's bits and on ids: order-independent)
//   k_path_walk          one wave per problem: from the target to the start, at each step the first neighbour in the order
//                        dz, dy, dx in {-1, 0, 1} with d[n] + w == d[cur] and an edge to cur (one lane per neighbour)
//   k_path_shortcut      one workgroup per problem: greedy, from W_i to the LARGEST visible W_k (lanes test the candidates
//                        with a 3-D DDA, a block max picks one); the path and its length
// Rounding: centres, the DDA and the cost are written in functions that carry fp contract(off) (see voxel_kernels.h), so a
// numpy restatement agrees bit for bit.  Plain loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_kernels.h"

namespace anet {

constexpr uint32_t kPathInf = 0xFFFFFFFFu;
// 16^3 tiles, one z column of 16 voxels per thread: cubic tiles need the fewest rounds for a front to cross the map (the
// rounds grow with the tile count along the longest axis) and carry the least halo (18^3 / 16^3 = 1.42); 23.3 KB of
// distances + 5.8 KB of free bytes leave room for five workgroups per CU.
constexpr int kPathT = 16, kPathH = kPathT + 2;
constexpr int kPathThreads = kPathT * kPathT;
constexpr int kPathSweepCap = 64;
constexpr int kPathRoundGroup = 8;     // rounds issued between two reads of the "active next round" word
constexpr double kPathTieEps = 1e-9;  // DDA crossings closer than this (segment parameter in [0, 1]) count as one
enum { kPathExact = 0, kPathApproximate = 1, kPathInvalidStart = 2 };

struct PathBox {
  double lb[3], hb[3];
};

struct PathInfo {        // per problem, in the workspace
  uint64_t best_d2;      // APPROXIMATE: bits of the least squared distance (non-negative doubles order as their bits)
  int32_t target, status, start, walk_len, err, pad;
};

__device__ inline double path_centre(const VoxGrid &g, int c, int64_t i) {
#pragma clang fp contract(off)
  return (double)i * g.scale + g.oc[c];
}

__device__ inline bool path_free(const VoxGrid &g, const PathBox &b, const uint8_t *__restrict__ vox, int64_t x, int64_t y,
                                 int64_t z) {
  if (x < 0 || y < 0 || z < 0 || x >= g.sx || y >= g.sy || z >= g.sz) return false;
  if (vox[x + (int64_t)g.sx * (y + (int64_t)g.sy * z)] != 0) return false;
  const double cx = path_centre(g, 0, x), cy = path_centre(g, 1, y), cz = path_centre(g, 2, z);
  return cx >= b.lb[0] && cx <= b.hb[0] && cy >= b.lb[1] && cy <= b.hb[1] && cz >= b.lb[2] && cz <= b.hb[2];
}

// the voxel of a position when it is free, else -1
__device__ inline int64_t path_free_voxel(const VoxGrid &g, const PathBox &b, const uint8_t *__restrict__ vox, const double *p) {
  int64_t i;
  if (!vox_index(g, p[0], p[1], p[2], i)) return -1;
  const int64_t sxy = (int64_t)g.sx * g.sy, z = i / sxy, y = (i - z * sxy) / g.sx, x = i - z * sxy - y * g.sx;
  return path_free(g, b, vox, x, y, z) ? i : -1;
}

// neighbourhood bit of offset (dx, dy, dz): (dx + 1) + 3 (dy + 1) + 9 (dz + 1), the centre is bit 13
__device__ constexpr int path_nb(int dx, int dy, int dz) { return (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1); }
// the block a move by (dx, dy, dz) spans, as neighbourhood bits
__device__ constexpr uint32_t path_block(int dx, int dy, int dz) {
  uint32_t m = 0;
  for (int e = 0; e < 8; ++e) m |= 1u << path_nb((e & 1) ? dx : 0, (e & 2) ? dy : 0, (e & 4) ? dz : 0);
  return m;
}
__device__ constexpr uint32_t path_weight(int dx, int dy, int dz) {
  return (dx != 0) + (dy != 0) + (dz != 0) == 1 ? 10u : (dx != 0) + (dy != 0) + (dz != 0) == 2 ? 14u : 17u;
}

struct PathArgs {
  VoxGrid g;
  PathBox box;
  const uint8_t *vox;
  const double *starts;  // [B][3]
  uint32_t *field;       // [B][n]
  uint32_t *active;      // [2][B][n_tiles]: tile t of problem b runs round r when active[r & 1][b][t] == r
  uint32_t *any;         // the latest round some tile was stamped for
  int64_t n, n_tiles;
  int tiles_x, tiles_y;
};

__global__ void __launch_bounds__(256) k_path_init(PathArgs a) {
  const int b = blockIdx.y, B = gridDim.y;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t s = path_free_voxel(a.g, a.box, a.vox, a.starts + 3 * b);
  int64_t st = -1;
  if (s >= 0) {
    const int64_t sxy = (int64_t)a.g.sx * a.g.sy, z = s / sxy, y = (s - z * sxy) / a.g.sx, x = s - z * sxy - y * a.g.sx;
    st = x / kPathT + (int64_t)a.tiles_x * (y / kPathT + (int64_t)a.tiles_y * (z / kPathT));
  }
  uint32_t *f = a.field + (int64_t)b * a.n;
  for (int64_t i = i0; i < a.n; i += stride) f[i] = i == s ? 0u : kPathInf;
  for (int64_t t = i0; t < a.n_tiles; t += stride) {
    a.active[(int64_t)b * a.n_tiles + t] = t == st ? 0u : kPathInf;
    a.active[((int64_t)B + b) * a.n_tiles + t] = kPathInf;
    if (t == st) *a.any = 0u;
  }
}

__global__ void __launch_bounds__(kPathThreads) k_path_relax(PathArgs a, uint32_t r) {
  const int b = blockIdx.y, B = gridDim.y;
  const int64_t t = blockIdx.x;
  if (a.active[((int64_t)(r & 1) * B + b) * a.n_tiles + t] != r) return;
  __shared__ uint32_t sd[kPathH][kPathH][kPathH];
  __shared__ uint8_t sf[kPathH][kPathH][kPathH];
  __shared__ uint32_t s_dirs;
  const int tx = (int)(t % a.tiles_x), ty = (int)((t / a.tiles_x) % a.tiles_y), tz = (int)(t / ((int64_t)a.tiles_x * a.tiles_y));
  const int64_t x0 = (int64_t)tx * kPathT, y0 = (int64_t)ty * kPathT, z0 = (int64_t)tz * kPathT;
  const int64_t sx = a.g.sx, sxy = (int64_t)a.g.sx * a.g.sy;
  uint32_t *f = a.field + (int64_t)b * a.n;
  const int tid = threadIdx.x;
  if (tid == 0) s_dirs = 0;
  for (int c = tid; c < kPathH * kPathH * kPathH; c += kPathThreads) {
    const int hx = c % kPathH, hy = (c / kPathH) % kPathH, hz = c / (kPathH * kPathH);
    const int64_t x = x0 + hx - 1, y = y0 + hy - 1, z = z0 + hz - 1;
    const bool fr = path_free(a.g, a.box, a.vox, x, y, z);
    sd[hz][hy][hx] = fr ? f[x + sx * y + sxy * z] : kPathInf;
    sf[hz][hy][hx] = fr ? 1 : 0;
  }
  __syncthreads();
  const int lx = tid % kPathT, ly = tid / kPathT;
  // edge masks: bit k of em[lz] (k = neighbourhood bit) set when the move to that neighbour is an edge
  uint32_t em[kPathT];
#pragma unroll
  for (int lz = 0; lz < kPathT; ++lz) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 27; ++k) m |= (uint32_t)sf[lz + k / 9][ly + (k / 3) % 3][lx + k % 3] << k;
    uint32_t e = 0;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      if (k == 13) continue;
      const uint32_t bl = path_block(k % 3 - 1, (k / 3) % 3 - 1, k / 9 - 1);
      e |= (uint32_t)((m & bl) == bl) << k;
    }
    em[lz] = (m >> 13 & 1u) ? e : 0u;
  }
  uint32_t chg = 0;  // bit lz: this voxel changed in some sweep
  bool capped = false;
  for (int sweep = 0;; ++sweep) {
    bool any = false;
    // Gauss-Seidel along the column, upward on even sweeps and downward on odd ones; neighbours' columns race benignly
    // (a 32-bit LDS word is read whole, and either value is an upper bound)
#pragma unroll
    for (int j = 0; j < kPathT; ++j) {
      const int lz = (sweep & 1) ? kPathT - 1 - j : j;
      const uint32_t m = em[lz];
      const uint32_t cur = sd[lz + 1][ly + 1][lx + 1];
      uint32_t best = cur;
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        if (k == 13) continue;
        const uint32_t v = sd[lz + k / 9][ly + (k / 3) % 3][lx + k % 3];
        const uint32_t c = v + path_weight(k % 3 - 1, (k / 3) % 3 - 1, k / 9 - 1);
        best = ((m >> k) & 1u) && c > v && c < best ? c : best;  // c <= v only when v is UINT32_MAX (unreached)
      }
      if (best < cur) {
        sd[lz + 1][ly + 1][lx + 1] = best;
        chg |= 1u << lz;
        any = true;
      }
    }
    const bool again = __syncthreads_or(any);
    if (!again) break;
    if (sweep + 1 == kPathSweepCap) {
      capped = true;
      break;
    }
  }
  // write back the changed voxels; collect the neighbour tiles that a changed boundary voxel touches
  const int64_t x = x0 + lx, y = y0 + ly;
  if (chg) {
    for (int lz = 0; lz < kPathT; ++lz)
      if (chg >> lz & 1u) f[x + sx * y + sxy * (z0 + lz)] = sd[lz + 1][ly + 1][lx + 1];
    const uint32_t xs = (lx == 0 ? 1u : 0u) | 2u | (lx == kPathT - 1 ? 4u : 0u);
    const uint32_t ys = (ly == 0 ? 1u : 0u) | 2u | (ly == kPathT - 1 ? 4u : 0u);
    const uint32_t zs = (chg & 1u ? 1u : 0u) | 2u | (chg >> (kPathT - 1) & 1u ? 4u : 0u);
    uint32_t dirs = 0;
    for (int k = 0; k < 27; ++k)
      if ((xs >> (k % 3) & 1u) && (ys >> ((k / 3) % 3) & 1u) && (zs >> (k / 9) & 1u)) dirs |= 1u << k;
    dirs &= ~(1u << 13);
    if (dirs) atomicOr(&s_dirs, dirs);
  }
  __syncthreads();
  const uint32_t dirs = s_dirs | (capped ? 1u << 13 : 0u);
  if (tid < 27 && (dirs >> tid & 1u)) {
    const int nx = tx + tid % 3 - 1, ny = ty + (tid / 3) % 3 - 1, nz = tz + tid / 9 - 1;
    const int tiles_z = (int)(a.n_tiles / ((int64_t)a.tiles_x * a.tiles_y));
    if (nx >= 0 && ny >= 0 && nz >= 0 && nx < a.tiles_x && ny < a.tiles_y && nz < tiles_z) {
      a.active[((int64_t)((r + 1) & 1) * B + b) * a.n_tiles + nx + (int64_t)a.tiles_x * (ny + (int64_t)a.tiles_y * nz)] = r + 1;
      *a.any = r + 1;
    }
  }
}

// ---- extraction ----------------------------------------------------------------------------------------------------------
struct PathExtractArgs {
  VoxGrid g;
  PathBox box;
  const uint8_t *vox;
  const double *starts, *goals;  // [B][3]
  const uint32_t *field;         // [B][n]
  int32_t *walk;                 // [B][n + 1]: target first, start last
  PathInfo *info;                // [B]
  int64_t n, cap;
  double *paths;                 // [B][cap][3]
  int32_t *n_points, *status;
  double *cost;
};

__global__ void __launch_bounds__(64) k_path_goal(PathExtractArgs a) {
  const int b = blockIdx.x;
  if (threadIdx.x != 0) return;
  PathInfo &in = a.info[b];
  const uint32_t *f = a.field + (int64_t)b * a.n;
  const int64_t s = path_free_voxel(a.g, a.box, a.vox, a.starts + 3 * b);
  const int64_t gv = path_free_voxel(a.g, a.box, a.vox, a.goals + 3 * b);
  in.best_d2 = 0x7FF0000000000000ull;  // +inf
  in.target = 0x7FFFFFFF;
  in.start = (int32_t)s;
  in.walk_len = 0;
  in.err = 0;
  if (s < 0 || f[s] != 0u) {
    in.status = kPathInvalidStart;
  } else if (gv >= 0 && f[gv] != kPathInf) {
    in.status = kPathExact;
    in.target = (int32_t)gv;
  } else {
    in.status = kPathApproximate;
  }
}

__device__ inline uint64_t path_d2_bits(const VoxGrid &g, int64_t i, const double *q) {
#pragma clang fp contract(off)
  const int64_t sxy = (int64_t)g.sx * g.sy, z = i / sxy, y = (i - z * sxy) / g.sx, x = i - z * sxy - y * g.sx;
  const double dx = path_centre(g, 0, x) - q[0], dy = path_centre(g, 1, y) - q[1], dz = path_centre(g, 2, z) - q[2];
  const double d2 = dx * dx + dy * dy + dz * dz;
  return d2 == d2 ? (uint64_t)__double_as_longlong(d2) : 0x7FF0000000000000ull;  // NaN (a non-finite goal) counts as +inf
}

__device__ inline uint64_t wave_min_u64(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t w = (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

constexpr int kPathScanItems = 16;
// pass 0: least squared distance over the reached voxels; pass 1: lowest reached id at that distance
template <int kPass>
__global__ void __launch_bounds__(256) k_path_nearest(PathExtractArgs a) {
  const int b = blockIdx.y;
  PathInfo &in = a.info[b];
  if (in.status != kPathApproximate) return;
  const uint32_t *f = a.field + (int64_t)b * a.n;
  const double *q = a.goals + 3 * b;
  const uint64_t want = kPass ? in.best_d2 : 0;
  const int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * kPathScanItems;
  uint64_t best = ~0ull;
  for (int j = 0; j < kPathScanItems; ++j) {
    const int64_t i = base + j;
    if (i >= a.n || f[i] == kPathInf) continue;
    const uint64_t d = path_d2_bits(a.g, i, q);
    if (kPass == 0) best = d < best ? d : best;
    else if (d == want && (uint64_t)i < best) best = (uint64_t)i;
  }
  best = wave_min_u64(best);
  if ((threadIdx.x & 63) == 0 && best != ~0ull) {
    if (kPass == 0) atomicMin((unsigned long long *)&in.best_d2, (unsigned long long)best);
    else atomicMin(&in.target, (int32_t)best);
  }
}

__global__ void __launch_bounds__(64) k_path_walk(PathExtractArgs a) {
  const int b = blockIdx.x, l = threadIdx.x;
  PathInfo &in = a.info[b];
  if (in.status == kPathInvalidStart) return;
  const uint32_t *f = a.field + (int64_t)b * a.n;
  int32_t *w = a.walk + (int64_t)b * (a.n + 1);
  const int64_t sx = a.g.sx, sxy = (int64_t)a.g.sx * a.g.sy;
  const int dx = l % 3 - 1, dy = (l / 3) % 3 - 1, dz = l / 9 - 1;
  const uint32_t bl = l < 27 ? path_block(dx, dy, dz) : 0u, wt = l < 27 && l != 13 ? path_weight(dx, dy, dz) : 0u;
  int64_t cur = in.target;
  int64_t len = 0;
  if (l == 0) w[0] = (int32_t)cur;
  while (cur != in.start) {
    const int64_t z = cur / sxy, y = (cur - z * sxy) / sx, x = cur - z * sxy - y * sx;
    bool fr = false;
    uint32_t d = kPathInf;
    if (l < 27) {
      fr = path_free(a.g, a.box, a.vox, x + dx, y + dy, z + dz);
      if (fr) d = f[(x + dx) + sx * (y + dy) + sxy * (z + dz)];
    }
    const uint32_t fm = (uint32_t)__ballot(fr);
    const uint32_t dcur = (uint32_t)__shfl((int)d, 13, 64);
    const bool ok = l < 27 && l != 13 && (fm & bl) == bl && d != kPathInf && d + wt == dcur;
    const uint64_t vm = __ballot(ok);
    if (vm == 0 || len >= a.n) {  // no predecessor: the field is not the converged one for this start and box
      if (l == 0) in.err = 1;
      return;
    }
    const int k = __ffsll((unsigned long long)vm) - 1;
    cur += (int64_t)(k % 3 - 1) + sx * ((k / 3) % 3 - 1) + sxy * (k / 9 - 1);
    ++len;
    if (l == 0) w[len] = (int32_t)cur;
  }
  if (l == 0) in.walk_len = (int32_t)(len + 1);
}

// waypoint k of W: W_0 = s, W_k = centre of walk[m - k], W_M = g when EXACT; m = 0 gives [s, end]
struct PathWaypoints {
  const VoxGrid *g;
  const double *s, *q;
  const int32_t *walk;
  int m, M;
  bool exact;
  __device__ void get(int k, double *p) const {
    if (k == 0) {
      p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
      return;
    }
    if (k == M && exact) {
      p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
      return;
    }
    const int64_t i = walk[m == 0 ? 0 : m - k], sxy = (int64_t)g->sx * g->sy;
    const int64_t z = i / sxy, y = (i - z * sxy) / g->sx, x = i - z * sxy - y * g->sx;
    p[0] = path_centre(*g, 0, x); p[1] = path_centre(*g, 1, y); p[2] = path_centre(*g, 2, z);
  }
};

// 3-D DDA (Amanatides-Woo) from P to Q, both in free voxels: every voxel it visits is free.  Only axes with moves left
// take part; where the next crossings of several of them lie within kPathTieEps of each other (in the segment's parameter),
// the whole block spanned at that step is checked and all of them step.  Exact equality is not enough: the crossing
// parameters are rounded, so a segment through a voxel edge or corner can come out a hair to one side of it and skip the
// voxel that the point on the edge itself belongs to.
__device__ inline bool path_visible(const VoxGrid &g, const PathBox &bx, const uint8_t *__restrict__ vox, const double *P,
                                    const double *Q) {
#pragma clang fp contract(off)
  int64_t cur[3], end[3];
  int step[3];
  double tmax[3], tdel[3];
  const int size[3] = {g.sx, g.sy, g.sz};
  for (int c = 0; c < 3; ++c) {
    cur[c] = (int)((P[c] - g.o[c]) / g.scale);
    end[c] = (int)((Q[c] - g.o[c]) / g.scale);
    cur[c] = cur[c] < 0 ? 0 : cur[c] >= size[c] ? size[c] - 1 : cur[c];  // (in range already: both points are free)
    end[c] = end[c] < 0 ? 0 : end[c] >= size[c] ? size[c] - 1 : end[c];
    const double dir = Q[c] - P[c];
    step[c] = dir > 0.0 ? 1 : dir < 0.0 ? -1 : 0;
    if (step[c] == 0) {
      tmax[c] = __builtin_inf();
      tdel[c] = __builtin_inf();
    } else {
      const double bnd = (double)(cur[c] + (step[c] > 0 ? 1 : 0)) * g.scale + g.o[c];
      tmax[c] = (bnd - P[c]) / dir;
      tdel[c] = g.scale / fabs(dir);
    }
  }
  if (!path_free(g, bx, vox, cur[0], cur[1], cur[2])) return false;
  while (cur[0] != end[0] || cur[1] != end[1] || cur[2] != end[2]) {
    double tm = __builtin_inf();
    for (int c = 0; c < 3; ++c)
      if (cur[c] != end[c] && tmax[c] < tm) tm = tmax[c];
    int mask = 0;
    for (int c = 0; c < 3; ++c)
      if (cur[c] != end[c] && tmax[c] <= tm + kPathTieEps) mask |= 1 << c;
    if (mask == 0) mask = (cur[0] != end[0]) ? 1 : (cur[1] != end[1]) ? 2 : 4;  // (unreachable: a remaining axis moves)
    for (int e = 1; e < 8; ++e) {
      if (e & ~mask) continue;
      if (!path_free(g, bx, vox, cur[0] + ((e & 1) ? step[0] : 0), cur[1] + ((e & 2) ? step[1] : 0),
                     cur[2] + ((e & 4) ? step[2] : 0)))
        return false;
    }
    for (int c = 0; c < 3; ++c)
      if (mask >> c & 1) {
        cur[c] += step[c];
        tmax[c] = tmax[c] + tdel[c];
      }
  }
  return true;
}

__device__ inline double path_seg_len(const double *p, const double *q) {
#pragma clang fp contract(off)
  const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}

constexpr int kPathShortcutThreads = 256;
__global__ void __launch_bounds__(kPathShortcutThreads) k_path_shortcut(PathExtractArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, tid = threadIdx.x;
  const PathInfo &in = a.info[b];
  __shared__ int s_best;
  if (in.status == kPathInvalidStart || in.err) {
    if (tid == 0) {
      a.n_points[b] = 0;
      a.cost[b] = __builtin_inf();
      a.status[b] = in.err ? -1 : in.status;
    }
    return;
  }
  PathWaypoints W{&a.g, a.starts + 3 * b, a.goals + 3 * b, a.walk + (int64_t)b * (a.n + 1), in.walk_len - 1, 0,
                  in.status == kPathExact};
  W.M = W.m == 0 ? 1 : W.m;
  double *out = a.paths + (int64_t)b * a.cap * 3;
  double prev[3], wi[3], wk[3];
  W.get(0, prev);
  if (tid == 0 && a.cap > 0) {
    out[0] = prev[0]; out[1] = prev[1]; out[2] = prev[2];
  }
  int i = 0, cnt = 1;
  double cost = 0.0;
  while (i < W.M) {
    W.get(i, wi);
    int best = -1;
    for (int hi = W.M; hi > i; hi -= kPathShortcutThreads) {
      const int k = hi - tid;
      bool vis = false;
      if (k > i) {
        W.get(k, wk);
        vis = path_visible(a.g, a.box, a.vox, wi, wk);
      }
      if (tid == 0) s_best = -1;
      __syncthreads();
      if (vis) atomicMax(&s_best, k);
      __syncthreads();
      best = s_best;
      __syncthreads();
      if (best > i) break;
    }
    if (best <= i) best = i + 1;  // (unreachable: W_i -> W_i+1 spans one free block)
    i = best;
    W.get(i, wk);
    if (tid == 0 && cnt < a.cap) {
      out[cnt * 3] = wk[0]; out[cnt * 3 + 1] = wk[1]; out[cnt * 3 + 2] = wk[2];
    }
    cost = cost + path_seg_len(prev, wk);
    prev[0] = wk[0]; prev[1] = wk[1]; prev[2] = wk[2];
    ++cnt;
  }
  if (tid == 0) {
    a.n_points[b] = cnt;
    a.cost[b] = cost;
    a.status[b] = in.status;
  }
}

}  // namespace anet
