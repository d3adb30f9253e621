// Log-odds occupancy grid from sensor scans, next to the byte grid of voxel_kernels.h (no counterpart in the reference, whose
// mapCallBack stamps a finished world cloud).  int16 log-odds per voxel in the voxel order of the byte grid, kOccUnknown for a
// voxel no ray has crossed.  Everything that decides a voxel is integer or an individually rounded double, so the grid is the same
// bits as the restatement's (tests/occupancy_np.py) and a function of the SET of rays of a scan.
//   occ_walk            THE statement of which cells a segment o -> q visits (below); the scan and the ray query share it
//   k_occ_carve         one lane per record: range test, truncation, walk; mark 1 in every visited cell but a hit's end cell
//   k_occ_hit           one lane per record: the end cell only (no walk); mark 2 there unless the ray was truncated
//   k_occ_mark_atomic   both in one launch: atomicOr of the flag bits 1 / 2 into the mark's 32-bit word (the measured alternative)
//   k_occ_update        one lane per cell of the sub-box the scan can reach: one clamped update per marked voxel, mark cleared
//   k_occ_reset         grid = unknown, marks = 0
//   k_occ_to_voxels     the hand-over: log-odds -> the bytes voxel_kernels.h / path_kernels.h / distance_kernels.h take
//   k_depth_to_points   one lane per kept pixel of a depth image: world points [n][3], NaN rows for rejected pixels
//   k_voxel_raycast     one lane per segment: the first visited in-bounds cell with a byte != 0, and the parameter it was entered at
//
// The walk of a segment o -> q over the grid (origin, scale):
//   cell(p)_c = floor((p_c - origin_c) / scale).  NOT the truncation of setOccupied / query (vox_index): the two agree inside the
//   map, but a point up to one voxel below the origin is in cell -1 here, outside, where truncation puts it into cell 0.
//   per axis: dir = q_c - o_c, step = sign(dir), bnd = (double)(cur_c + (step > 0)) * scale + origin_c, tmax = (bnd - o_c) / dir,
//   tdel = scale / |dir|; both infinite for dir == 0 (path_visible's set-up).
//   while cur != end: tm = the least tmax over the axes with cur_c != end_c; every such axis with tmax <= tm + 1e-9 steps, all
//   together, tmax += tdel; the new cell is visited.  On a tie only the diagonal cell is visited, not the other cells of the block:
//   for carving the conservative side (nothing is declared free that the ray merely touches).
//   visited: the start cell and each cell after a step; the last is the end cell.  Cells outside the map are walked through.
// Every floating-point operation is rounded on its own (contraction off in each function that computes one).
// Bounds: a cell index must stay below 2^30 in magnitude and the two cells at most kOccMaxSpan + 1 apart per axis, or the segment
// is refused (occ_walk_setup); every step moves at least one axis one cell towards the end cell, so a walk takes at most
// 3 * (kOccMaxSpan + 1) steps whatever the input.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace anet {

// the grid as these kernels need it (voxel_kernels.h, with the map's kernels, belongs to api_voxel.hip alone)
struct OccGrid {
  int sx, sy, sz;
  double o[3], scale;
};

constexpr int16_t kOccUnknown = INT16_MIN;
constexpr int kOccMaxSpan = 65536;     // cells per axis a segment may span (max_range / scale <= kOccMaxSpan)
constexpr double kOccTieEps = 1e-9;    // crossings this close in the segment's parameter step together
constexpr double kOccCellLimit = 1073741824.0;  // 2^30

struct OccParams {
  int hit, miss, lo, hi;
  double min_range, max_range;
};

struct OccWalk {
  int cur[3], end[3], step[3];
  double tmax[3], tdel[3];
};

// floor((p - origin_c) / scale) as an int, false when it reaches 2^30 in magnitude (or is not finite)
__host__ __device__ inline bool occ_cell(const OccGrid &g, double p, int c, int &cell) {
#pragma clang fp contract(off)
  const double f = floor((p - g.o[c]) / g.scale);
  if (!(fabs(f) < kOccCellLimit)) return false;
  cell = (int)f;
  return true;
}

// false: a cell index out of range or a span above max_span on an axis -- the segment is not walked.  The scan allows
// kOccMaxSpan + 1 (max_range / scale <= kOccMaxSpan, and the floor of either end may add a cell), the ray query kOccMaxSpan.
__device__ inline bool occ_walk_setup(const OccGrid &g, const double *o, const double *q, OccWalk &w, int max_span = kOccMaxSpan + 1) {
#pragma clang fp contract(off)
  for (int c = 0; c < 3; ++c) {
    if (!occ_cell(g, o[c], c, w.cur[c]) || !occ_cell(g, q[c], c, w.end[c])) return false;
    const int span = w.end[c] > w.cur[c] ? w.end[c] - w.cur[c] : w.cur[c] - w.end[c];
    if (span > max_span) return false;
    const double dir = q[c] - o[c];
    w.step[c] = dir > 0.0 ? 1 : dir < 0.0 ? -1 : 0;
    if (w.step[c] == 0) {
      w.tmax[c] = __builtin_inf();
      w.tdel[c] = __builtin_inf();
    } else {
      const double bnd = (double)(w.cur[c] + (w.step[c] > 0 ? 1 : 0)) * g.scale + g.o[c];
      w.tmax[c] = (bnd - o[c]) / dir;
      w.tdel[c] = g.scale / fabs(dir);
    }
  }
  return true;
}

// start and end cell beyond the same face of the map: no visited cell is inside it
__device__ inline bool occ_walk_misses_map(const OccGrid &g, const OccWalk &w) {
  const int size[3] = {g.sx, g.sy, g.sz};
  for (int c = 0; c < 3; ++c)
    if ((w.cur[c] < 0 && w.end[c] < 0) || (w.cur[c] >= size[c] && w.end[c] >= size[c])) return true;
  return false;
}

__device__ inline bool occ_inside(const OccGrid &g, const int *cell, int64_t &idx) {
  if (cell[0] < 0 || cell[1] < 0 || cell[2] < 0 || cell[0] >= g.sx || cell[1] >= g.sy || cell[2] >= g.sz) return false;
  idx = (int64_t)cell[0] + (int64_t)g.sx * ((int64_t)cell[1] + (int64_t)g.sy * cell[2]);
  return true;
}

// visit(cell, t, is_end) for the start cell (t = 0) and each cell after a step (t = that step's tm); visit returns false to stop.
// An axis with cur_c != end_c has step_c != 0 and end_c on that side (floor, the subtraction and the division are monotone), so
// every round takes the walk at least one cell closer to the end cell.
template <class Visit>
__device__ inline void occ_walk(OccWalk &w, Visit &&visit) {
#pragma clang fp contract(off)
  bool at_end = w.cur[0] == w.end[0] && w.cur[1] == w.end[1] && w.cur[2] == w.end[2];
  if (!visit(w.cur, 0.0, at_end)) return;
  while (!at_end) {
    double tm = __builtin_inf();
    for (int c = 0; c < 3; ++c)
      if (w.cur[c] != w.end[c] && w.tmax[c] < tm) tm = w.tmax[c];
    int mask = 0;
    for (int c = 0; c < 3; ++c)
      if (w.cur[c] != w.end[c] && w.tmax[c] <= tm + kOccTieEps) mask |= 1 << c;
    if (mask == 0) mask = (w.cur[0] != w.end[0]) ? 1 : (w.cur[1] != w.end[1]) ? 2 : 4;  // (unreachable: a remaining axis moves)
    for (int c = 0; c < 3; ++c)
      if (mask >> c & 1) {
        w.cur[c] += w.step[c];
        w.tmax[c] = w.tmax[c] + w.tdel[c];
      }
    at_end = w.cur[0] == w.end[0] && w.cur[1] == w.end[1] && w.cur[2] == w.end[2];
    if (!visit(w.cur, tm, at_end)) return;
  }
}

__device__ inline bool occ_record(const uint8_t *rec, int64_t r, int64_t stride, int f64, double *p) {
  const uint8_t *b = rec + r * stride;
  if (f64) {
    const double *d = (const double *)b;
    p[0] = d[0]; p[1] = d[1]; p[2] = d[2];
  } else {
    const float *f = (const float *)b;
    p[0] = (double)f[0]; p[1] = (double)f[1]; p[2] = (double)f[2];
  }
  return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

// The ray of a record from the sensor origin o: false when the record is skipped (non-finite, or shorter than min_range); q is
// the far end of the walk, truncated set when it was pulled in to max_range.
__device__ inline bool occ_ray(const OccParams &prm, const double *o, const double *p, double *q, bool &truncated) {
#pragma clang fp contract(off)
  const double dx = p[0] - o[0], dy = p[1] - o[1], dz = p[2] - o[2];
  const double len = sqrt(dx * dx + dy * dy + dz * dz);
  if (len < prm.min_range) return false;
  truncated = len > prm.max_range;
  if (truncated) {
    const double r = prm.max_range / len;
    q[0] = o[0] + dx * r; q[1] = o[1] + dy * r; q[2] = o[2] + dz * r;
  } else {
    q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
  }
  return true;
}

struct OccScan {
  OccGrid g;
  OccParams prm;
  double o[3];
  const uint8_t *rec;
  int64_t n, stride;
  int f64;
};

// Plain byte stores: every store of this launch writes 1, so the races are between equal values (as in k_voxel_scatter); the hit
// launch that follows on the same stream writes 2 over them, which is what makes a hit win.
__global__ void __launch_bounds__(256) k_occ_carve(OccScan s, uint8_t *__restrict__ marks) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= s.n) return;
  double p[3], q[3];
  bool truncated;
  if (!occ_record(s.rec, r, s.stride, s.f64, p) || !occ_ray(s.prm, s.o, p, q, truncated)) return;
  OccWalk w;
  if (!occ_walk_setup(s.g, s.o, q, w) || occ_walk_misses_map(s.g, w)) return;
  const OccGrid &g = s.g;
  occ_walk(w, [&](const int *cell, double, bool is_end) {
    int64_t i;
    if ((!is_end || truncated) && occ_inside(g, cell, i)) marks[i] = 1;
    return true;
  });
}

__global__ void __launch_bounds__(256) k_occ_hit(OccScan s, uint8_t *__restrict__ marks) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= s.n) return;
  double p[3], q[3];
  bool truncated;
  if (!occ_record(s.rec, r, s.stride, s.f64, p) || !occ_ray(s.prm, s.o, p, q, truncated) || truncated) return;
  OccWalk w;
  if (!occ_walk_setup(s.g, s.o, q, w)) return;  // (the same refusal as the carve launch: such a ray marks nothing)
  int64_t i;
  if (occ_inside(s.g, w.end, i)) marks[i] = 2;
}

// The alternative: one launch, the flag bits 1 (miss) / 2 (hit) OR-ed into the 32-bit word that holds the voxel's mark byte.
__global__ void __launch_bounds__(256) k_occ_mark_atomic(OccScan s, uint32_t *__restrict__ words) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= s.n) return;
  double p[3], q[3];
  bool truncated;
  if (!occ_record(s.rec, r, s.stride, s.f64, p) || !occ_ray(s.prm, s.o, p, q, truncated)) return;
  OccWalk w;
  if (!occ_walk_setup(s.g, s.o, q, w) || occ_walk_misses_map(s.g, w)) return;
  const OccGrid &g = s.g;
  occ_walk(w, [&](const int *cell, double, bool is_end) {
    int64_t i;
    if (occ_inside(g, cell, i)) atomicOr(&words[i >> 2], (uint32_t)((is_end && !truncated) ? 2 : 1) << (8 * (int)(i & 3)));
    return true;
  });
}

// The sub-box [lo, lo + ext) of cells a scan can reach, cut to the map by the host.  A mark with bit 2 is a hit, any other
// non-zero mark a miss; one update per marked voxel, in int32, and the mark goes back to 0.
struct OccBox {
  int lo[3], ext[3];
};
__global__ void __launch_bounds__(256) k_occ_update(OccGrid g, OccParams prm, OccBox bx, int16_t *__restrict__ logodds,
                                                   uint8_t *__restrict__ marks) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = (int64_t)bx.ext[0] * bx.ext[1] * bx.ext[2];
  if (t >= n) return;
  const int x = bx.lo[0] + (int)(t % bx.ext[0]), y = bx.lo[1] + (int)((t / bx.ext[0]) % bx.ext[1]),
            z = bx.lo[2] + (int)(t / ((int64_t)bx.ext[0] * bx.ext[1]));
  const int64_t i = (int64_t)x + (int64_t)g.sx * ((int64_t)y + (int64_t)g.sy * z);
  const uint8_t m = marks[i];
  if (m == 0) return;
  marks[i] = 0;
  const int32_t L = logodds[i] == kOccUnknown ? 0 : (int32_t)logodds[i];
  int32_t v;
  if (m & 2) {
    v = L + prm.hit;
    v = v < prm.hi ? v : prm.hi;
  } else {
    v = L + prm.miss;
    v = v > prm.lo ? v : prm.lo;
  }
  logodds[i] = (int16_t)v;
}

__global__ void __launch_bounds__(256) k_occ_reset(int64_t n, int16_t *__restrict__ logodds, uint8_t *__restrict__ marks,
                                                  int64_t n_marks) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) logodds[t] = kOccUnknown;
  if (t < n_marks) marks[t] = 0;
}

__global__ void __launch_bounds__(256) k_occ_to_voxels(int64_t n, const int16_t *__restrict__ logodds, int occ, int unknown_blocked,
                                                      uint8_t *__restrict__ vox) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int16_t L = logodds[t];
  vox[t] = L == kOccUnknown ? (uint8_t)(unknown_blocked != 0) : (uint8_t)((int)L >= occ);
}

// Pixels (u, v) with u, v in {0, step, 2 step, ...}, row-major.  z = depth * depth_scale; x = (u - cx) / fx * z;
// y = (v - cy) / fy * z; world_r = (R[r][0] x + R[r][1] y) + R[r][2] z + t[r].
struct DepthCam {
  double fx, fy, cx, cy, R[9], t[3], depth_scale, min_depth, max_depth;
  int width, height, step, nu, nv, u16;
};
__global__ void __launch_bounds__(256) k_depth_to_points(DepthCam cam, const void *__restrict__ depth, double *__restrict__ out) {
#pragma clang fp contract(off)
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (int64_t)cam.nu * cam.nv) return;
  const int u = (int)(k % cam.nu) * cam.step, v = (int)(k / cam.nu) * cam.step;
  const int64_t pix = (int64_t)v * cam.width + u;
  const double d = cam.u16 ? (double)((const uint16_t *)depth)[pix] : (double)((const float *)depth)[pix];
  const double z = d * cam.depth_scale;
  double *o = out + k * 3;
  if (!isfinite(z) || z <= cam.min_depth || z > cam.max_depth) {
    o[0] = o[1] = o[2] = __builtin_nan("");
    return;
  }
  const double x = ((double)u - cam.cx) / cam.fx * z, y = ((double)v - cam.cy) / cam.fy * z;
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = (cam.R[r * 3] * x + cam.R[r * 3 + 1] * y) + cam.R[r * 3 + 2] * z + cam.t[r];
}

// First hit of segment i on the byte grid.  Cells outside the map are passed through: they are NOT blocked here, unlike in
// k_voxel_query, so a sensor outside the map sees into it.  hit: the linear index, ANET_HIT_FREE (-1) or ANET_HIT_INVALID (-3).
__global__ void __launch_bounds__(256) k_voxel_raycast(OccGrid g, const uint8_t *__restrict__ vox, const double *__restrict__ origins,
                                                      const double *__restrict__ ends, int64_t n, int32_t *__restrict__ hit,
                                                      double *__restrict__ t_out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const double o[3] = {origins[r * 3], origins[r * 3 + 1], origins[r * 3 + 2]};
  const double q[3] = {ends[r * 3], ends[r * 3 + 1], ends[r * 3 + 2]};
  int32_t h = -3;
  double t = __builtin_nan("");
  OccWalk w;
  const bool finite = isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
  if (finite && occ_walk_setup(g, o, q, w, kOccMaxSpan)) {
    h = -1;
    t = 1.0;
    if (!occ_walk_misses_map(g, w))
      occ_walk(w, [&](const int *cell, double tm, bool) {
        int64_t i;
        if (occ_inside(g, cell, i) && vox[i] != 0) {
          h = (int32_t)i;
          t = tm;
          return false;
        }
        return true;
      });
  }
  hit[r] = h;
  if (t_out) t_out[r] = t;
}

}  // namespace anet
