// geo_utils::enumerateVs (gcopter/geo_utils.hpp:155-202, with filterVs :128-150), batched: the vertices of a corridor polytope
// given by its half-spaces.  No hull code: a polytope has at most 128 rows (two stacked FIRI outputs), and in 3-D its vertices are
// the feasible intersections of row triples -- C(rows, 3) independent 3x3 solves and a feasibility sweep each.
//
// One statement of the semantics, used by every layer above (include/allocnet_amd.h, the Python and C++ facades):
//   rows        h0 x + h1 y + h2 z + h3 <= 0 (GCOPTER's raw form), all-zero normals are padding and may stand anywhere; the others
//               are scaled to unit normals (n, d) in their order, and (i, j, k) below counts THOSE rows
//   candidate   a triple i < j < k with |det(n_i, n_j, n_k)| >= kPolyMinDet (1e-8: the solve's position error is about
//               eps_mach * |x| / |det|, and must stay under epsilon at the tens of metres of a map); its point solves the three
//               plane equations by Cramer's rule
//   feasible    n_r . x + d_r <= epsilon for every row r
//   merge       candidates are visited in ascending lexicographic order of (i, j, k); one is DROPPED when a vertex kept before it
//               lies within res = max(epsilon, mag * DBL_EPSILON) of it in the max-norm, mag = the largest absolute coordinate
//               among the kept vertices and the candidate itself; else it is kept, at the end of the list.  So the output order is
//               that of the first triple that produced each vertex, whatever the launch shape.
//               (Deviation from filterVs, which rounds to a grid of that resolution and compares cells: two points 1e-12 apart stay
//               distinct there when they straddle a cell edge.  A distance does not have that seam.)
//   active      per kept vertex the rows with |n_r . x + d_r| <= epsilon, as bits of two uint64 indexed by the ORIGINAL row number
//   status      0 ok; 1 no vertices, count = 0: depth[b] (anet_polytope_depth, normalised) is <= 0, NaN, -inf (padding only) or +inf
//               (unbounded) and the polytope is skipped -- the reference's `return false` -- or no triple gave a feasible point (a
//               slab, a wedge: unbounded sets of finite depth that contain a line).  An unbounded polytope WITH vertices (a
//               half-infinite prism) is not detected: its vertices are returned, as the reference's hull of the dual would return
//               something; corridors carry their bounding box.  2: more vertices than max_vertices (count is the true number, the
//               first max_vertices are written) or more than kPolyMaxKept = 256 distinct ones: the kept list is full, count stays 256 (a
//               lower bound) and further candidates are dropped.  A polytope of 128 rows has at most 2 * rows - 4 = 252 true
//               vertices; near-coincident planes can add a few spurious ones, so this is improbable, not impossible
//
// Shape.  The normalised rows sit in LDS once per polytope.  A wave takes 64 consecutive triples (lane = triple, unranked in
// closed form), sweeps the rows at a wave-uniform LDS index, leaves as soon as no lane is feasible any more, and compacts the
// feasible points in ballot order into a 64-slot stage.  The merge wave then inserts them one by one against the kept list in LDS
// (lanes = kept vertices): LDS is rows + 256 kept + 64 staged per wave whatever the degeneracy -- 40 planes through an apex are
// 9880 feasible candidates of ONE vertex.  WPP waves work on a polytope: 1 (four polytopes per workgroup, no workgroup barrier) or
// 4 (the workgroup's waves take consecutive chunks of a round, wave 0 merges their stages in chunk order).  Every triple is
// computed by the same instructions in both, so the results are the same bits.
//
// FP64, contraction off: a residual is the sum a numpy restatement forms, so decisions at epsilon do not depend on the compiler.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace anet {

constexpr int kPolyMaxRows = 128;
constexpr int kPolyMaxKept = 256;
constexpr int kPolyWaves = 4;  // waves per workgroup
constexpr double kPolyMinDet = 1e-8;

struct PolyVertsArgs {
  const double *hpoly;  // [B][H][4]
  const double *depth;  // [B]: anet_polytope_depth_dev(normalise = 1)
  double *verts;        // [B][max_vertices][3]
  int32_t *count;       // [B]
  uint64_t *active;     // [B][max_vertices][2] or nullptr
  int32_t *status;      // [B] or nullptr
  int64_t B;
  int H, max_vertices;
  double eps;
};

// doubles of LDS per polytope: rows [H][4], kept [kPolyMaxKept][3], stage [wpp][64][3], then ints: orig [H], n, staged [wpp]
__host__ __device__ inline int poly_lds_doubles(int H, int wpp) {
  return 4 * H + 3 * kPolyMaxKept + 3 * 64 * wpp + (H + 1 + wpp + 1) / 2;
}

// the waves of one polytope meet: a workgroup barrier when they are the workgroup, else (one wave) LDS is in order within the wave
// and only the compiler must be kept from moving accesses across
template <int WPP>
__device__ __forceinline__ void poly_sync() {
  if constexpr (WPP == kPolyWaves) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

__device__ __forceinline__ int poly_c3(int m) { return m * (m - 1) * (m - 2) / 6; }

// triple number t (lexicographic, 0 <= t < C(n, 3)) -> i < j < k
__device__ __forceinline__ void poly_unrank(int t, int n, int &i, int &j, int &k) {
  const int total = poly_c3(n);
  int lo = 0, hi = n - 3;  // the largest i with  #triples whose first index is below i  <= t
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (total - poly_c3(n - mid) <= t) lo = mid; else hi = mid - 1;
  }
  i = lo;
  const int r = t - (total - poly_c3(n - i)), m = n - 1 - i;  // pair number r among the m rows behind i
  lo = 0; hi = m - 2;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mid * (2 * m - mid - 1) / 2 <= r) lo = mid; else hi = mid - 1;
  }
  j = i + 1 + lo;
  k = j + 1 + (r - lo * (2 * m - lo - 1) / 2);
}

template <int WPP>
__global__ void __launch_bounds__(64 * kPolyWaves) k_polytope_vertices(PolyVertsArgs g) {
  static_assert(WPP == 1 || WPP == kPolyWaves, "one wave or the whole workgroup per polytope");
  constexpr int PPB = kPolyWaves / WPP;  // polytopes per workgroup
  extern __shared__ double sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = wave / WPP, sub = wave % WPP;
  const int64_t b = (int64_t)blockIdx.x * PPB + slot;
  const int H = g.H;
  // (everything below is uniform over the waves of a polytope, so their barriers match; with WPP == 1 there is no barrier)
  if (b >= g.B) return;
  const double depth = g.depth[b];
  if (!(depth > 0.0 && depth < INFINITY)) {
    if (sub == 0 && lane == 0) {
      g.count[b] = 0;
      if (g.status) g.status[b] = 1;
    }
    return;
  }
  double *rows = sm + (size_t)slot * poly_lds_doubles(H, WPP);
  double *kept = rows + 4 * H;
  double *stage = kept + 3 * kPolyMaxKept;
  int *orig = (int *)(stage + 3 * 64 * WPP);
  int *meta = orig + H;  // [0]: rows, [1 + w]: staged by wave w
  const uint64_t lt = (1ull << lane) - 1ull;

  if (sub == 0) {  // the non-padding rows, unit normals, in their order
    int n = 0;
    for (int base = 0; base < H; base += 64) {
      const int r = base + lane;
      double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0;
      if (r < H) {
        const double *h = g.hpoly + (b * H + r) * 4;
        h0 = h[0]; h1 = h[1]; h2 = h[2]; h3 = h[3];
      }
      const bool row = r < H && !(h0 == 0.0 && h1 == 0.0 && h2 == 0.0);
      const uint64_t m = __ballot(row);
      if (row) {
        const int pos = n + __popcll(m & lt);
        const double nrm = sqrt(h0 * h0 + h1 * h1 + h2 * h2);
        rows[pos * 4] = h0 / nrm; rows[pos * 4 + 1] = h1 / nrm; rows[pos * 4 + 2] = h2 / nrm; rows[pos * 4 + 3] = h3 / nrm;
        orig[pos] = r;
      }
      n += __popcll(m);
    }
    if (lane == 0) meta[0] = n;
  }
  poly_sync<WPP>();
  const int n = meta[0];
  const int ntri = n >= 3 ? poly_c3(n) : 0;
  const int rounds = (ntri + 64 * WPP - 1) / (64 * WPP);
  const double eps = g.eps;
  int nkept = 0;     // merge wave only; never above kPolyMaxKept
  bool over = false;  // merge wave only: a distinct candidate found the kept list full
  double mag = 0.0;  // merge wave only

  for (int round = 0; round < rounds; ++round) {
    const int t = (round * WPP + sub) * 64 + lane;
    bool feas = t < ntri;
    double x = 0.0, y = 0.0, z = 0.0;
    if (feas) {
      int i, j, k;
      poly_unrank(t, n, i, j, k);
      const double a0 = rows[i * 4], a1 = rows[i * 4 + 1], a2 = rows[i * 4 + 2], ad = rows[i * 4 + 3];
      const double b0 = rows[j * 4], b1 = rows[j * 4 + 1], b2 = rows[j * 4 + 2], bd = rows[j * 4 + 3];
      const double c0 = rows[k * 4], c1 = rows[k * 4 + 1], c2 = rows[k * 4 + 2], cd = rows[k * 4 + 3];
      // u = b x c, v = c x a, w = a x b;  det = a . u;  x = -(ad u + bd v + cd w) / det
      const double u0 = b1 * c2 - b2 * c1, u1 = b2 * c0 - b0 * c2, u2 = b0 * c1 - b1 * c0;
      const double v0 = c1 * a2 - c2 * a1, v1 = c2 * a0 - c0 * a2, v2 = c0 * a1 - c1 * a0;
      const double w0 = a1 * b2 - a2 * b1, w1 = a2 * b0 - a0 * b2, w2 = a0 * b1 - a1 * b0;
      const double det = a0 * u0 + a1 * u1 + a2 * u2;
      feas = fabs(det) >= kPolyMinDet;
      if (feas) {
        x = -(ad * u0 + bd * v0 + cd * w0) / det;
        y = -(ad * u1 + bd * v1 + cd * w1) / det;
        z = -(ad * u2 + bd * v2 + cd * w2) / det;
      }
    }
    // feasibility sweep, rows at a wave-uniform index; the wave leaves once none of its lanes is feasible
    for (int r0 = 0; r0 < n; r0 += 4) {
      if (__ballot(feas) == 0ull) break;
      const int r1 = min(r0 + 4, n);
      for (int r = r0; r < r1; ++r) {
        const double res = rows[r * 4] * x + rows[r * 4 + 1] * y + rows[r * 4 + 2] * z + rows[r * 4 + 3];
        feas = feas && res <= eps;  // (a NaN point is not feasible)
      }
    }
    const uint64_t fm = __ballot(feas);
    if (feas) {
      double *s = stage + (sub * 64 + __popcll(fm & lt)) * 3;
      s[0] = x; s[1] = y; s[2] = z;
    }
    if (lane == 0) meta[1 + sub] = __popcll(fm);
    poly_sync<WPP>();
    if (sub == 0) {
      for (int w = 0; w < WPP; ++w) {
        const int staged = meta[1 + w];
        for (int c = 0; c < staged; ++c) {
          const double *s = stage + (w * 64 + c) * 3;
          const double cx = s[0], cy = s[1], cz = s[2];
          const double m = fmax(mag, fmax(fabs(cx), fmax(fabs(cy), fabs(cz))));
          const double res = fmax(eps, m * DBL_EPSILON);
          bool dup = false;
          const int have = nkept;
          for (int q = lane; q < have; q += 64)
            dup = dup || (fabs(kept[q * 3] - cx) <= res && fabs(kept[q * 3 + 1] - cy) <= res && fabs(kept[q * 3 + 2] - cz) <= res);
          if (__ballot(dup) == 0ull) {
            if (nkept >= kPolyMaxKept) { over = true; continue; }
            if (lane == 0) { kept[nkept * 3] = cx; kept[nkept * 3 + 1] = cy; kept[nkept * 3 + 2] = cz; }
            ++nkept;
            mag = m;
            poly_sync<1>();  // the next candidate's lanes read what lane 0 wrote (same wave)
          }
        }
      }
    }
    poly_sync<WPP>();  // the stages are free again
  }

  if (sub != 0) return;
  const int nout = min(nkept, g.max_vertices);
  if (lane == 0) {
    g.count[b] = nkept;
    if (g.status) g.status[b] = nkept == 0 ? 1 : (nkept > g.max_vertices || over) ? 2 : 0;
  }
  for (int q = lane; q < nout; q += 64) {
    const double vx = kept[q * 3], vy = kept[q * 3 + 1], vz = kept[q * 3 + 2];
    double *o = g.verts + (b * g.max_vertices + q) * 3;
    o[0] = vx; o[1] = vy; o[2] = vz;
    if (g.active) {
      uint64_t lo = 0ull, hi = 0ull;
      for (int r = 0; r < n; ++r) {
        const double res = rows[r * 4] * vx + rows[r * 4 + 1] * vy + rows[r * 4 + 2] * vz + rows[r * 4 + 3];
        if (fabs(res) <= eps) {
          const int o_r = orig[r];
          if (o_r < 64) lo |= 1ull << o_r; else hi |= 1ull << (o_r - 64);
        }
      }
      g.active[(b * g.max_vertices + q) * 2] = lo;
      g.active[(b * g.max_vertices + q) * 2 + 1] = hi;
    }
  }
}

}  // namespace anet
