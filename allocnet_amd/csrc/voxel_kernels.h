// Device voxel map: the semantics of voxel_map::VoxelMap (gcopter/voxel_map.hpp, voxel_dilater.hpp) on a byte grid.
//   voxel i = x + sx * (y + sy * z), values 0 Unoccupied, 1 Occupied, 2 Dilated.
//   k_voxel_scatter      one lane per cloud record: finite test, (pos - o) / scale truncated toward zero, bounds, store 1
//   k_voxel_scatter_ids  one lane per integer index triple: bounds, store 1
//   k_voxel_dilate_round one synchronous frontier round over a 3-D tile with a one-voxel halo in LDS
//   k_compact_*          count / scan / write stream compaction, ascending and deterministic (no order-dependent atomics)
//   k_voxel_surf_points  ids -> (n, 3) float64 with the reference's two roundings (product, then sum)
//   k_voxel_query        n positions -> n bytes, true outside the map
// Where a result must match the reference bit for bit, floating-point contraction is off: hipcc fuses a * b + c into
// v_fma_f64 by default, which rounds once where the reference rounds twice.  The pragma covers only the expressions
// written in the function that carries it, so the arithmetic is spelled out there (__dmul_rn / __dadd_rn are plain
// operators in other functions and would still be fused after inlining).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace anet {

struct VoxGrid {
  int sx, sy, sz;
  double o[3], scale;
  double oc[3], ss[3];  // o + 0.5 * scale; (1.0 / step) * scale -- computed on the host, as the reference does
};

// floor-free truncation of (pos - o) / scale with the bounds test folded in: trunc(q) in [0, size) <=> -1 < q < size,
// which also drops non-finite and out-of-int-range values without converting them.
__device__ inline bool vox_index(const VoxGrid &g, double px, double py, double pz, int64_t &idx) {
#pragma clang fp contract(off)
  const double qx = (px - g.o[0]) / g.scale, qy = (py - g.o[1]) / g.scale, qz = (pz - g.o[2]) / g.scale;
  if (!(qx > -1.0 && qx < (double)g.sx && qy > -1.0 && qy < (double)g.sy && qz > -1.0 && qz < (double)g.sz)) return false;
  idx = (int64_t)(int)qx + (int64_t)g.sx * ((int64_t)(int)qy + (int64_t)g.sy * (int64_t)(int)qz);
  return true;
}

// records: n of them, `stride` bytes apart, three float32 (f64 == 0) or float64 (f64 == 1) coordinates first.  mapCallBack
// (learning_planning.cpp) skips a record with a non-finite coordinate; every store writes the same byte, so races are benign.
__global__ void __launch_bounds__(256) k_voxel_scatter(VoxGrid g, uint8_t *__restrict__ vox, const uint8_t *__restrict__ rec,
                                                      int64_t n, int64_t stride, int f64) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint8_t *p = rec + r * stride;
  double x, y, z;
  if (f64) {
    const double *d = (const double *)p;
    x = d[0]; y = d[1]; z = d[2];
  } else {
    const float *f = (const float *)p;
    x = (double)f[0]; y = (double)f[1]; z = (double)f[2];
  }
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return;
  int64_t i;
  if (vox_index(g, x, y, z, i)) vox[i] = 1;
}

// setOccupied(Eigen::Vector3i id) for n index triples: in-bounds ones are set to 1, the rest dropped
__global__ void __launch_bounds__(256) k_voxel_scatter_ids(VoxGrid g, uint8_t *__restrict__ vox, const int32_t *__restrict__ xyz,
                                                          int64_t n) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int x = xyz[r * 3], y = xyz[r * 3 + 1], z = xyz[r * 3 + 2];
  if (x >= 0 && y >= 0 && z >= 0 && x < g.sx && y < g.sy && z < g.sz)
    vox[(int64_t)x + (int64_t)g.sx * ((int64_t)y + (int64_t)g.sy * z)] = 1;
}

// One dilation round.  Sources: voxels == 1 (first round) or the previous front (later rounds).  Every in-bounds voxel
// that is 0 and has a source among its 26 in-bounds neighbours becomes 2 and joins the next front; `next` is written for
// every voxel.  Reads of `vox` by other tiles cannot race with these writes: a write turns 0 into 2, which changes
// neither "== 1" nor the owner-only "== 0" test.
constexpr int kDilTX = 64, kDilTY = 4, kDilTZ = 4;
constexpr int kDilHX = kDilTX + 2, kDilHY = kDilTY + 2, kDilHZ = kDilTZ + 2;
__global__ void __launch_bounds__(kDilTX * kDilTY) k_voxel_dilate_round(VoxGrid g, uint8_t *__restrict__ vox,
                                                                       const uint8_t *__restrict__ prev,
                                                                       uint8_t *__restrict__ next, int first,
                                                                       int64_t tiles_x, int64_t tiles_y) {
  __shared__ uint8_t src[kDilHZ][kDilHY][kDilHX];
  const int64_t t = blockIdx.x;
  const int64_t x0 = (t % tiles_x) * kDilTX, y0 = ((t / tiles_x) % tiles_y) * kDilTY, z0 = t / (tiles_x * tiles_y) * kDilTZ;
  const int64_t sx = g.sx, sxy = (int64_t)g.sx * g.sy;
  const int tid = threadIdx.x + kDilTX * threadIdx.y;
  for (int c = tid; c < kDilHX * kDilHY * kDilHZ; c += kDilTX * kDilTY) {
    const int hx = c % kDilHX, hy = (c / kDilHX) % kDilHY, hz = c / (kDilHX * kDilHY);
    const int64_t x = x0 + hx - 1, y = y0 + hy - 1, z = z0 + hz - 1;
    uint8_t s = 0;
    if (x >= 0 && y >= 0 && z >= 0 && x < g.sx && y < g.sy && z < g.sz) {
      const int64_t i = x + sx * y + sxy * z;
      s = first ? (uint8_t)(vox[i] == 1) : (uint8_t)(prev[i] != 0);
    }
    src[hz][hy][hx] = s;
  }
  __syncthreads();
  const int lx = threadIdx.x, ly = threadIdx.y;
  const int64_t x = x0 + lx, y = y0 + ly;
  if (x >= g.sx || y >= g.sy) return;
  for (int lz = 0; lz < kDilTZ; ++lz) {
    const int64_t z = z0 + lz;
    if (z >= g.sz) break;
    const int64_t i = x + sx * y + sxy * z;
    uint8_t hit = 0;
    if (vox[i] == 0) {
#pragma unroll
      for (int dz = 0; dz < 3; ++dz)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) hit |= src[lz + dz][ly + dy][lx + dx];  // (the centre is never a source here)
      if (hit) vox[i] = 2;
    }
    next[i] = hit;
  }
}

// ---- stream compaction: for each of K lists, the items i in [0, n) that pass a test, in ascending order --------------
// count: per (chunk, list) the number of passing items; scan: exclusive offsets per list and the true total; write: each
// chunk recounts and stores its items at their offsets, as long as the offset is below the caller's capacity.
constexpr int kCompThreads = 256, kCompItems = 16, kCompChunk = kCompThreads * kCompItems;

__device__ inline int block_exclusive_scan(int v, int *sh, int &total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < kCompThreads; d <<= 1) {
    const int a = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const int incl = sh[t];
  total = sh[kCompThreads - 1];
  __syncthreads();
  return incl - v;
}

struct FrontPred {  // item i passes when front[i] != 0; emitted as its index
  const uint8_t *front;
  int32_t *ids;
  __device__ bool test(int, int64_t i) const { return front[i] != 0; }
  __device__ void emit(int, int64_t i, int64_t slot, int64_t) const { ids[slot] = (int32_t)i; }
};

// point i passes box k when every row r of bd[k] (6 x 4, h . [p; 1]) gives ((h0 p0 + h1 p1) + h2 p2) + h3 < 0: the loop of
// sfc_gen::convexCover and, for rows with a single +-1 entry, the same single rounding as the matrix product of firi.py.
struct BoxPred {
  const double *bd;   // [K][6][4]
  const double *pts;  // [n][3]
  double *out;        // [K][cap][3]
  __device__ bool test(int k, int64_t i) const {
#pragma clang fp contract(off)
    const double *h = bd + (int64_t)k * 24;
    const double p0 = pts[i * 3], p1 = pts[i * 3 + 1], p2 = pts[i * 3 + 2];
    bool inside = true;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double v = h[r * 4] * p0 + h[r * 4 + 1] * p1 + h[r * 4 + 2] * p2 + h[r * 4 + 3];
      inside = inside && v < 0.0;
    }
    return inside;
  }
  __device__ void emit(int k, int64_t i, int64_t slot, int64_t cap) const {
    double *o = out + ((int64_t)k * cap + slot) * 3;
    o[0] = pts[i * 3]; o[1] = pts[i * 3 + 1]; o[2] = pts[i * 3 + 2];
  }
};

template <class P>
__global__ void __launch_bounds__(kCompThreads) k_compact_count(P p, int64_t n, int64_t n_chunks, int32_t *__restrict__ counts) {
  __shared__ int sh[kCompThreads];
  const int k = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * kCompChunk + (int64_t)threadIdx.x * kCompItems;
  int c = 0;
  for (int j = 0; j < kCompItems; ++j)
    if (base + j < n) c += p.test(k, base + j) ? 1 : 0;
  int total;
  block_exclusive_scan(c, sh, total);
  if (threadIdx.x == 0) counts[(int64_t)k * n_chunks + blockIdx.x] = total;
}

// one block per list: counts[k][*] -> exclusive offsets in place, totals[k] = the true count
__global__ void __launch_bounds__(kCompThreads) k_compact_scan(int32_t *__restrict__ counts, int64_t n_chunks,
                                                             int32_t *__restrict__ totals) {
  __shared__ int sh[kCompThreads];
  int32_t *c = counts + (int64_t)blockIdx.x * n_chunks;
  int carry = 0;
  for (int64_t b = 0; b < n_chunks; b += kCompThreads) {
    const int64_t j = b + threadIdx.x;
    const int v = j < n_chunks ? c[j] : 0;
    int tot;
    const int ex = block_exclusive_scan(v, sh, tot);
    if (j < n_chunks) c[j] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

template <class P>
__global__ void __launch_bounds__(kCompThreads) k_compact_write(P p, int64_t n, int64_t n_chunks,
                                                              const int32_t *__restrict__ offsets, int64_t cap) {
  __shared__ int sh[kCompThreads];
  const int k = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * kCompChunk + (int64_t)threadIdx.x * kCompItems;
  uint32_t mask = 0;
  for (int j = 0; j < kCompItems; ++j)
    if (base + j < n && p.test(k, base + j)) mask |= 1u << j;
  int total;
  int64_t slot = offsets[(int64_t)k * n_chunks + blockIdx.x] + block_exclusive_scan(__popc(mask), sh, total);
  for (int j = 0; j < kCompItems; ++j)
    if (mask >> j & 1u) {
      if (slot < cap) p.emit(k, base + j, slot, cap);
      ++slot;
    }
}

// surface point of voxel id: the reference keeps ids in offset form (x, y sx, z sx sy) and returns id * stepScale + oc,
// a product and a sum, each rounded
__global__ void __launch_bounds__(256) k_voxel_surf_points(VoxGrid g, const int32_t *__restrict__ ids, int64_t n,
                                                          double *__restrict__ out) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t id = ids[t], sxy = (int64_t)g.sx * g.sy;
  const int64_t z = id / sxy, y = (id - z * sxy) / g.sx, x = id - z * sxy - y * g.sx;
  const double off[3] = {(double)x, (double)(y * g.sx), (double)(z * sxy)};
#pragma unroll
  for (int c = 0; c < 3; ++c) out[t * 3 + c] = off[c] * g.ss[c] + g.oc[c];
}

// VoxelMap::query(pos): voxels[id] != 0 inside the map, true outside
__global__ void __launch_bounds__(256) k_voxel_query(VoxGrid g, const uint8_t *__restrict__ vox, const double *__restrict__ pos,
                                                    int64_t n, uint8_t *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  int64_t i;
  out[t] = vox_index(g, pos[t * 3], pos[t * 3 + 1], pos[t * 3 + 2], i) ? (uint8_t)(vox[i] != 0) : (uint8_t)1;
}

}  // namespace anet
