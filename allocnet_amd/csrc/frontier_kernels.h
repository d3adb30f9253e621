// Exploration goals on the occupancy grid of occupancy_kernels.h: the frontier between known-free and unknown space, connected
// components of a byte grid, and the number of unknown voxels a scan from a pose would reveal.  Everything is
// integer or an individually rounded double, as in occupancy_kernels.h, so every result is the restatement's (tests/frontier_np.py)
// bit for bit and a function of the inputs alone, whatever order lanes, waves and atomics run in.
//   k_occ_frontier      one lane per voxel: known, below occ, in the box, and a face neighbour INSIDE the map unknown
//   k_vox_label_tile    one workgroup per 8 x 8 x 4 tile: label equivalence resolved in LDS, labels = the tile-local minimum index
//   k_vox_label_merge   one lane per voxel: the links that cross a tile face, edge or corner, by root chasing and atomicMin on roots
//   k_vox_label_flatten one lane per voxel: label = its root
//   k_vox_root_count / k_vox_root_scan / k_vox_root_rank   the roots (labels[v] == v) compacted in ascending order
//   k_vox_stats         one lane per voxel: count, integer coordinate sums and cell box of its component, wave-aggregated
//   k_occ_view_gain     one lane per (view, template point): occ_ray + occ_walk, a mark byte per unknown cell seen
//   k_occ_view_count    sums and clears the marks of every view's slot
//
// Labels.  labels[v] is a parent pointer throughout: -1 off the mask, otherwise an index <= v of the same component.  A link is
// only ever made from a root to a smaller index (atomicMin), so the root of a tree is its least member, and once every pair of
// neighbouring voxels has been united the root of v's tree is the least index of v's component.  unite(a, b): chase both to their
// roots; equal: done; else atomicMin(&L[larger], smaller); if the word still held the larger root the link is made, otherwise
// somebody else re-parented it meanwhile and the union goes on from what the word held (that value and `smaller` are both in the
// component, and the word now holds the lesser of them, so no link is lost).  A stale read can only return an older parent, which
// is still an ancestor-or-self of a tree of the same component.  One pass of all unions settles the labels; a second pass that
// links nothing is the proof, and what the host loop waits for.
// Tiles keep the traffic local: inside a tile the unions run on LDS, and only pairs that straddle tiles touch global memory.
#pragma once
#include "occupancy_kernels.h"
#include "workspace_constants.h"

namespace anet {

// ---- frontier ------------------------------------------------------------------------------------------------------------------
constexpr int kFrontierBlocks = 2048;  // workgroups of k_occ_frontier at the most: each strides over the voxels and adds to the count once
__global__ void __launch_bounds__(256) k_occ_frontier(OccGrid g, OccBox bx, const int16_t *__restrict__ L, int occ,
                                                     uint8_t *__restrict__ mask, unsigned long long *__restrict__ count) {
  // (fewer than 2^31 voxels: 32-bit index arithmetic.)  The grid is capped (kFrontierBlocks) and strides over the voxels, so
  // that the count costs a bounded number of adds on its one word (DESIGN.md section 8u has the measurement).
  const uint32_t n = (uint32_t)g.sx * (uint32_t)g.sy * (uint32_t)g.sz, stride = gridDim.x * blockDim.x;
  const uint32_t sxy = (uint32_t)g.sx * (uint32_t)g.sy;
  int ones = 0;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += stride) {
    const uint32_t row = v / (uint32_t)g.sx;
    const int x = (int)(v - row * (uint32_t)g.sx), z = (int)(row / (uint32_t)g.sy), y = (int)(row - (uint32_t)z * (uint32_t)g.sy);
    const bool in_box = x >= bx.lo[0] && x < bx.lo[0] + bx.ext[0] && y >= bx.lo[1] && y < bx.lo[1] + bx.ext[1] && z >= bx.lo[2] &&
                        z < bx.lo[2] + bx.ext[2];
    bool f = false;
    if (in_box) {
      const int16_t l = L[v];
      if (l != kOccUnknown && (int)l < occ)
        f = (x > 0 && L[v - 1] == kOccUnknown) || (x + 1 < g.sx && L[v + 1] == kOccUnknown) ||
            (y > 0 && L[v - g.sx] == kOccUnknown) || (y + 1 < g.sy && L[v + g.sx] == kOccUnknown) ||
            (z > 0 && L[v - sxy] == kOccUnknown) || (z + 1 < g.sz && L[v + sxy] == kOccUnknown);
    }
    mask[v] = f ? 1 : 0;
    ones += f ? 1 : 0;
  }
  if (count) {
    __shared__ int block_sum;
    if (threadIdx.x == 0) block_sum = 0;
    __syncthreads();
    for (int d = 32; d > 0; d >>= 1) ones += __shfl_xor(ones, d);
    if ((threadIdx.x & 63) == 0 && ones) atomicAdd(&block_sum, ones);
    __syncthreads();
    if (threadIdx.x == 0 && block_sum) atomicAdd(count, (unsigned long long)block_sum);
  }
}

// ---- connected components ------------------------------------------------------------------------------------------------------
constexpr int kLabelTX = 8, kLabelTY = 8, kLabelTZ = 4;  // 256 voxels, one lane each; x fastest, so local and global order agree
constexpr int kLabelRoundGroup = 2;                      // rounds issued between two reads of the "last round that linked" word

struct LabelGrid {
  int sx, sy, sz, ntx, nty, ntz;
};

// the "forward" half of the neighbourhood, (dz, dy, dx) > 0 in that order: each unordered pair of neighbours is united once.
// The three face offsets come first: connectivity 6 takes those, 26 all thirteen.
__device__ __constant__ const int8_t kLabelFwd[13][3] = {{1, 0, 0},  {0, 1, 0},  {0, 0, 1},   {-1, 1, 0}, {1, 1, 0},  {-1, 0, 1}, {1, 0, 1},
                                                         {0, -1, 1}, {0, 1, 1},  {-1, -1, 1}, {1, -1, 1}, {-1, 1, 1}, {1, 1, 1}};

template <class Load, class Min>
__device__ inline bool label_unite(int a, int b, Load &&load, Min &&atomic_min) {
  bool linked = false;
  for (;;) {
    for (int p; (p = load(a)) != a;) a = p;
    for (int p; (p = load(b)) != b;) b = p;
    if (a == b) return linked;
    if (a < b) {
      const int t = a; a = b; b = t;
    }
    const int old = atomic_min(a, b);  // a: the larger root
    if (old == a) return true;
    linked = true;  // (the word changed hands: somebody's link went in, the labels are not settled)
    a = old;
  }
}

__global__ void __launch_bounds__(256) k_vox_label_tile(LabelGrid g, const uint8_t *__restrict__ mask, int n_fwd,
                                                       int32_t *__restrict__ labels) {
  __shared__ int lbl[256];
  volatile int *vl = lbl;
  const int tid = threadIdx.x;
  const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
  const int64_t n_tiles = (int64_t)g.ntx * g.nty * g.ntz;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // (uniform over the workgroup: the barriers are met by all)
    const int tx = (int)(tile % g.ntx), ty = (int)((tile / g.ntx) % g.nty), tz = (int)(tile / ((int64_t)g.ntx * g.nty));
    const int x = tx * kLabelTX + lx, y = ty * kLabelTY + ly, z = tz * kLabelTZ + lz;
    const bool inside = x < g.sx && y < g.sy && z < g.sz;
    const int64_t v = (int64_t)x + (int64_t)g.sx * ((int64_t)y + (int64_t)g.sy * z);
    const bool m = inside && mask[v] != 0;
    lbl[tid] = m ? tid : -1;
    __syncthreads();
    if (m)
      for (int k = 0; k < n_fwd; ++k) {
        const int nx = lx + kLabelFwd[k][0], ny = ly + kLabelFwd[k][1], nz = lz + kLabelFwd[k][2];
        if (nx < 0 || nx >= kLabelTX || ny < 0 || ny >= kLabelTY || nz >= kLabelTZ) continue;
        const int nt = nx + kLabelTX * (ny + kLabelTY * nz);
        if (vl[nt] < 0) continue;
        label_unite(tid, nt, [&](int i) { return vl[i]; }, [&](int i, int val) { return atomicMin(&lbl[i], val); });
      }
    __syncthreads();
    if (m) {
      int r = tid;
      for (int p; (p = vl[r]) != r;) r = p;
      const int rx = tx * kLabelTX + (r & 7), ry = ty * kLabelTY + ((r >> 3) & 7), rz = tz * kLabelTZ + (r >> 6);
      labels[v] = (int32_t)((int64_t)rx + (int64_t)g.sx * ((int64_t)ry + (int64_t)g.sy * rz));
    } else if (inside) {
      labels[v] = -1;
    }
    __syncthreads();  // (the next tile overwrites lbl)
  }
}

__device__ inline int label_load(const int32_t *labels, int i) {
  return __hip_atomic_load(&labels[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) k_vox_label_merge(LabelGrid g, int n_fwd, int32_t *labels, int32_t *changed, int32_t round) {
  const uint32_t n = (uint32_t)g.sx * (uint32_t)g.sy * (uint32_t)g.sz;
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n || label_load(labels, (int)v) < 0) return;
  const uint32_t row = v / (uint32_t)g.sx;
  const int x = (int)(v - row * (uint32_t)g.sx), z = (int)(row / (uint32_t)g.sy), y = (int)(row - (uint32_t)z * (uint32_t)g.sy);
  bool linked = false;
  for (int k = 0; k < n_fwd; ++k) {
    const int nx = x + kLabelFwd[k][0], ny = y + kLabelFwd[k][1], nz = z + kLabelFwd[k][2];
    if (nx < 0 || nx >= g.sx || ny < 0 || ny >= g.sy || nz >= g.sz) continue;
    if (nx / kLabelTX == x / kLabelTX && ny / kLabelTY == y / kLabelTY && nz / kLabelTZ == z / kLabelTZ) continue;  // the tile pass united them
    const int64_t nb = (int64_t)nx + (int64_t)g.sx * ((int64_t)ny + (int64_t)g.sy * nz);
    if (label_load(labels, (int)nb) < 0) continue;
    linked |= label_unite((int)v, (int)nb, [&](int i) { return label_load(labels, i); },
                          [&](int i, int val) { return atomicMin(&labels[i], val); });
  }
  if (linked) *changed = round;  // (every store of a launch writes the same value)
}

__global__ void __launch_bounds__(256) k_vox_label_flatten(int64_t n, int32_t *labels) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  int r = label_load(labels, (int)v);
  if (r < 0 || r == (int)v) return;
  for (int p; (p = label_load(labels, r)) != r;) r = p;
  __hip_atomic_store(&labels[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- component statistics ------------------------------------------------------------------------------------------------------
// roots per block of kCompScanBlock voxels
__global__ void __launch_bounds__(kCompScanBlock) k_vox_root_count(int64_t n, const int32_t *__restrict__ labels, int32_t *__restrict__ blocks) {
  const int64_t v = (int64_t)blockIdx.x * kCompScanBlock + threadIdx.x;
  const bool root = v < n && labels[v] == (int32_t)v;
  __shared__ int sum;
  if (threadIdx.x == 0) sum = 0;
  __syncthreads();
  const int c = __popcll(__ballot(root));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&sum, c);
  __syncthreads();
  if (threadIdx.x == 0) blocks[blockIdx.x] = sum;
}

// exclusive scan of the block counts in place by ONE workgroup, 256 at a time with the carry in a register; the total is the
// number of components
__global__ void __launch_bounds__(256) k_vox_root_scan(int64_t n_blocks, int32_t *__restrict__ blocks, int32_t *__restrict__ n_components) {
  __shared__ int buf[256];
  int carry = 0;
  for (int64_t base = 0; base < n_blocks; base += 256) {
    const int64_t i = base + threadIdx.x;
    const int mine = i < n_blocks ? blocks[i] : 0;
    buf[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int add = (int)threadIdx.x >= d ? buf[threadIdx.x - d] : 0;
      __syncthreads();
      buf[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < n_blocks) blocks[i] = carry + buf[threadIdx.x] - mine;
    carry += buf[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_components = carry;
}

struct CompStats {
  int32_t max_components;
  int32_t *root, *count, *bbox;
  unsigned long long *sum;
};

// the rank of every root at its own index, and the rows of the first max_components components at their identities
__global__ void __launch_bounds__(kCompScanBlock) k_vox_root_rank(int64_t n, const int32_t *__restrict__ labels, const int32_t *__restrict__ blocks,
                                                                 int32_t *__restrict__ rank, CompStats s) {
  const int64_t v = (int64_t)blockIdx.x * kCompScanBlock + threadIdx.x;
  const bool root = v < n && labels[v] == (int32_t)v;
  __shared__ int wave_sum[kCompScanBlock / 64];
  const unsigned long long b = __ballot(root);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_sum[wave] = __popcll(b);
  __syncthreads();
  if (!root) return;
  int r = blocks[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) r += wave_sum[w];
  rank[v] = r;
  if (r >= s.max_components) return;
  s.root[r] = (int32_t)v;
  s.count[r] = 0;
  unsigned long long *sum = s.sum + (int64_t)r * 3;
  int32_t *bb = s.bbox + (int64_t)r * 6;
  sum[0] = sum[1] = sum[2] = 0;
  bb[0] = bb[1] = bb[2] = INT32_MAX;
  bb[3] = bb[4] = bb[5] = -1;
}

// Each wave reduces in registers once per distinct component among its voxels (usually one or two: x runs fastest) and one lane
// adds the wave's share.  Integer adds, minima and maxima: exact and order-free.
__global__ void __launch_bounds__(256) k_vox_stats(LabelGrid g, const int32_t *__restrict__ labels, const int32_t *__restrict__ rank,
                                                  CompStats s) {
  const uint32_t n = (uint32_t)g.sx * (uint32_t)g.sy * (uint32_t)g.sz;
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  int r = -1;
  if (v < n) {
    const int32_t l = labels[v];
    if (l >= 0 && (uint32_t)l < n) {
      r = rank[l];
      if (r >= s.max_components) r = -1;
    }
  }
  unsigned long long todo = __ballot(r >= 0);
  if (todo == 0) return;
  const uint32_t row = v / (uint32_t)g.sx;
  const int x = (int)(v - row * (uint32_t)g.sx), z = (int)(row / (uint32_t)g.sy), y = (int)(row - (uint32_t)z * (uint32_t)g.sy);
  const int lane = threadIdx.x & 63;
  while (todo) {  // (wave-uniform)
    const int leader = __ffsll((long long)todo) - 1;
    const int r0 = __shfl(r, leader);
    const bool mine = r == r0;
    int cnt = mine ? 1 : 0;
    int lo[3] = {mine ? x : INT32_MAX, mine ? y : INT32_MAX, mine ? z : INT32_MAX};
    int hi[3] = {mine ? x : -1, mine ? y : -1, mine ? z : -1};
    long long sum[3] = {mine ? x : 0, mine ? y : 0, mine ? z : 0};
    for (int d = 32; d > 0; d >>= 1) {
      cnt += __shfl_xor(cnt, d);
      for (int c = 0; c < 3; ++c) {
        const int a = __shfl_xor(lo[c], d), b = __shfl_xor(hi[c], d);
        lo[c] = a < lo[c] ? a : lo[c];
        hi[c] = b > hi[c] ? b : hi[c];
        sum[c] += __shfl_xor(sum[c], d);
      }
    }
    if (lane == leader) {
      unsigned long long *out = s.sum + (int64_t)r0 * 3;
      int32_t *bb = s.bbox + (int64_t)r0 * 6;
      atomicAdd(&s.count[r0], cnt);
      for (int c = 0; c < 3; ++c) {
        atomicAdd(&out[c], (unsigned long long)sum[c]);
        // (the box only grows and a stale read shows a smaller one: the test skips no update that is needed, and most that are not)
        if (lo[c] < bb[c]) atomicMin(&bb[c], lo[c]);
        if (hi[c] > bb[3 + c]) atomicMax(&bb[3 + c], hi[c]);
      }
    }
    todo &= ~__ballot(mine);
  }
}

// ---- view gain -----------------------------------------------------------------------------------------------------------------
struct ViewScan {
  OccGrid g;
  OccParams prm;
  int occ, reach;          // reach = ceil(max_range / scale) + 1 cells, the scan's (anet_occupancy_integrate_dev)
  const double *R, *t;     // [V][9], [V][3] of this chunk
  const double *pts;       // [n_pts][3], sensor frame
  int n_views, n_pts;
  int64_t slot;            // mark bytes per view
};

// The pose of view v and the sub-box of cells its rays can reach, cut to the map: false when an entry of R or t is not finite
// (gain -1).  empty: no cell of the box is in the map, or the view's own cell index is out of range (no ray is walked: gain 0).
__device__ inline bool view_pose(const ViewScan &s, int v, double *R, double *t, OccBox &bx, bool &empty) {
  bool finite = true;
  for (int i = 0; i < 9; ++i) {
    R[i] = s.R[(int64_t)v * 9 + i];
    finite = finite && isfinite(R[i]);
  }
  for (int i = 0; i < 3; ++i) {
    t[i] = s.t[(int64_t)v * 3 + i];
    finite = finite && isfinite(t[i]);
  }
  empty = true;
  if (!finite) return false;
  const int size[3] = {s.g.sx, s.g.sy, s.g.sz};
  bool any = true;
  for (int c = 0; c < 3; ++c) {
    int cell;
    if (!occ_cell(s.g, t[c], c, cell)) return true;
    const int64_t lo = (int64_t)cell - s.reach > 0 ? (int64_t)cell - s.reach : 0;
    const int64_t hi = (int64_t)cell + s.reach < size[c] - 1 ? (int64_t)cell + s.reach : size[c] - 1;
    if (hi < lo) any = false;
    bx.lo[c] = (int)lo;
    bx.ext[c] = any ? (int)(hi - lo + 1) : 0;
  }
  empty = !any;
  return true;
}

// Lanes: view-major, template point fastest.  Marks are plain byte stores of 1 (races between equal values, as in k_occ_carve).
__global__ void __launch_bounds__(256) k_occ_view_gain(ViewScan s, const int16_t *__restrict__ L, uint8_t *__restrict__ marks,
                                                      int32_t *__restrict__ gain) {
#pragma clang fp contract(off)
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double R[9], t[3];
  OccBox bx;
  bool empty;
  if (k < s.n_views) gain[k] = view_pose(s, (int)k, R, t, bx, empty) ? 0 : -1;  // (the count launch adds to it)
  if (k >= (int64_t)s.n_views * s.n_pts) return;
  const int v = (int)(k / s.n_pts), r = (int)(k % s.n_pts);
  if (!view_pose(s, v, R, t, bx, empty) || empty) return;
  const double x = s.pts[(int64_t)r * 3], y = s.pts[(int64_t)r * 3 + 1], z = s.pts[(int64_t)r * 3 + 2];
  double p[3], q[3];
  for (int c = 0; c < 3; ++c) p[c] = (R[c * 3] * x + R[c * 3 + 1] * y) + R[c * 3 + 2] * z + t[c];
  bool truncated;
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) || !occ_ray(s.prm, t, p, q, truncated)) return;
  OccWalk w;
  if (!occ_walk_setup(s.g, t, q, w) || occ_walk_misses_map(s.g, w)) return;
  uint8_t *slot = marks + (int64_t)v * s.slot;
  const OccGrid &g = s.g;
  const int occ = s.occ;
  occ_walk(w, [&](const int *cell, double, bool) {
    int64_t i;
    if (!occ_inside(g, cell, i)) return true;
    const int16_t l = L[i];
    if (l == kOccUnknown) {
      const int bxc = cell[0] - bx.lo[0], byc = cell[1] - bx.lo[1], bzc = cell[2] - bx.lo[2];
      // (every visited cell is within `reach` of the view's: the test keeps a store inside the slot whatever the arithmetic did)
      if (bxc >= 0 && bxc < bx.ext[0] && byc >= 0 && byc < bx.ext[1] && bzc >= 0 && bzc < bx.ext[2])
        slot[(int64_t)bxc + (int64_t)bx.ext[0] * ((int64_t)byc + (int64_t)bx.ext[1] * bzc)] = 1;
      return true;
    }
    return (int)l < occ;
  });
}

// grid (pieces, views of the chunk): 16 mark bytes per lane and step, summed (a mark is 0 or 1) and cleared; one add per wave
__global__ void __launch_bounds__(256) k_occ_view_count(ViewScan s, uint8_t *__restrict__ marks, int32_t *__restrict__ gain) {
  const int v = blockIdx.y;
  double R[9], t[3];
  OccBox bx;
  bool empty;
  if (!view_pose(s, v, R, t, bx, empty) || empty) return;
  const int64_t cells = (int64_t)bx.ext[0] * bx.ext[1] * bx.ext[2], pieces = (cells + 15) / 16;  // (cells <= slot, a multiple of 16)
  uint4 *slot = (uint4 *)(marks + (int64_t)v * s.slot);
  int sum = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pieces; i += (int64_t)gridDim.x * blockDim.x) {
    const uint4 m = slot[i];
    if ((m.x | m.y | m.z | m.w) != 0) {
      sum += __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
      slot[i] = make_uint4(0, 0, 0, 0);
    }
  }
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&gain[v], sum);
}

}  // namespace anet
