// Exact first collision of a trajectory with the device voxel map: per (trajectory, piece) the first local time at which the
// curve is in a blocked voxel or leaves the map, and which voxel.  Not sampled: no curve clips a voxel between two samples.
//
// SEMANTICS.  Grid g (anet_voxel_grid), voxels the device byte grid.  For a position p:
//     q_ax = (p_ax - origin_ax) / scale;   inside(p) <=> -1 < q_ax < size_ax on all three axes;   cell(p) = trunc(q) per axis;
//     blocked(p) <=> !inside(p) || voxels[cell(p)] != 0
// which is anet_voxel_query (vox_index in voxel_kernels.h) verbatim, truncation toward zero included: cell 0 of an axis spans
// -1 < q < 1, the cell changes at q = 1, 2, ..., size - 1, the map is left at q <= -1 or q >= size.  For piece i (coefficients
// highest power first, duration T_i, order S in {2, 3, 4})
//     t_hit = inf { t in [0, T_i] : blocked(p_i(t)) },        +inf when the set is empty
// so that the minimum over the pieces (plus the earlier durations) is the trajectory's answer.  Per (trajectory, piece), [N][ld]:
//   t_hit  double;
//   voxel  int32 (may be NULL): the linear index x + sx (y + sy z) of the blocked voxel entered; kHitFree = -1; kHitOutside = -2:
//          the curve left the map; kHitInvalid = -3.
// A curve that starts blocked has t_hit = 0 (p(0) is formed as query forms it: the same subtraction and division).  A piece with
// T_i == 0 is the point p_i(0).  A NaN or infinite coefficient or duration, T_i < 0, or a piece whose coefficients in voxel units
// sum to more than kHitMaxScale (their differences would overflow) gives t_hit = NaN and voxel = -3 for that piece and only for it.
// One more answer carries -3: a FINITE t_hit with voxel = -3 means the node budget ran out; the curve is free before t_hit and
// nothing is known from t_hit on (the conservative answer: callers treat it as a hit).
//
// PROCEDURE.  One lane per (trajectory, piece), blockIdx.y = piece: every coefficient load of a wave is one contiguous row
// segment.  The lane forms q_ax in normalised time once, qu[ax][k] = c_k T^k / scale (k = 0: (c_0 - origin) / scale), converts
// the three components to Bernstein form (3 x 2S control values) and keeps both in registers.  It then visits dyadic
// sub-intervals [idx, idx + 1] / 2^lev of [0, 1] left first and without a stack (the walk of bernstein_walk.h, with a 64-bit
// index for the depth 32.  The (lev, idx) state is written out here: through bern::Dyadic the kernel measured 0.8 % slower at
// 131 072 trajectories; the midpoint halving is not used here either).  A visit blossoms the control values straight to [a, b] -- de Casteljau at b, then at a / b on the left
// part -- so it costs O(S^2) whatever its depth, and reduces each axis to its smallest and largest control value (the curve's
// box on [a, b]), its two end values and whether its control values rise or fall strictly (the component is monotone).  Then:
//   * the box covers at most kHitBoxCells cells: they are looked up.  None blocked and none outside: the interval is FREE.
//   * otherwise, the cell of the start point q(a) is blocked: HIT at a (everything before a was free).
//   * otherwise, the box is two cells that differ on one axis, and that axis is monotone: if its end value is still in the start
//     cell the interval is FREE; if not, the crossing of the plane between the two cells is located by bisection (kHitBisect
//     halvings at most) on Horner values of the component polynomial qu[ax] -- never on re-expanded coefficients, see
//     rate_kernels.h -- with cell(q) != start cell as the test, which is query's own: HIT at the first time found beyond the plane.
//   * otherwise the interval is split; at the depth bound 2^-kHitDepth it is decided by the cell of its midpoint (blocked: HIT
//     at a).
// The box is NOT widened by the rounding slack.  Inside the band of width tol_pos (below) either answer is allowed, and a
// widened box would make every trajectory that lies exactly in a cell plane (constant height z = k scale + origin: the common
// planar case) see the blocked cells below it at every depth.  For the same reason a de Casteljau step is written
// w_k + t (w_k+1 - w_k): a constant component keeps its exact value at every depth and is looked up in the cell query gives it.
// LOOPS.  Visits: kHitMaxNodes; the climb to the next interval: kHitDepth; bisection: kHitBisect; the cell scan: kHitBoxCells.
// All structural: no input can spin a wave.  No LDS, no scratch (every array has compile-time indices; the crossing axis selects
// its coefficients by conditional moves), no atomics, and nothing a lane does depends on another lane: a piece gives the same bits
// whatever else is in the batch.  If the budget of visits runs out the answer is the conservative one described above.
// COST.  Voxel reads are byte gathers through a const __restrict__ pointer; a planner map (200 x 200 x 40 = 1.6 MB) stays in L2.
// A free piece is halved until each part's box is at most kHitBoxCells cells; the inner visits make no lookup.  Counted with the
// float64 restatement tests/traj_voxel_hit_mp.hit_float64 on 300 free jerk and 300 free snap pieces of 1 to 4 m in 0.25 m voxels:
// 13 visits and 36 byte lookups in the median, 21 visits and 56 lookups at the 90th percentile, 29 and 80 at most.
//
// ACCURACY.  t* the exact infimum, ax the axis whose plane is crossed there, u_ax,k the coefficients of q_ax in normalised time:
//     |t_hit - t*| <= T_i 2^-kHitDepth + kHitC eps (sum_k |u_ax,k| + |q_plane|) / |dq_ax/dtau (tau*)| T_i
// kHitC = 32 from the operation count: the coefficients qu_k = c_k T^k / scale carry at most 8 roundings (6 products for T^k, the
// product with c_k, the division) = 4 eps |u_k|; Horner of degree <= 7 without fused operations 14 roundings = 7 eps sum |u_k|;
// the bisection resolves tau to 2^-53, at most 7 eps sum |u_k| / |q'| because |q'| <= 7 sum |u_k|; t = tau T one more rounding,
// at most 3.5 eps sum |u_k| / |q'|: 21.5 eps to first order, rounded up to the power of two 32 (tests/traj_voxel_hit_mp.hit_bound,
// DESIGN.md 8l).  The bound grows without limit at a tangency; what holds for every input is the band
//     tol_pos = max(2^-kHitDepth L_i, kHitC eps scale_i)
// (L_i: the arc-length bound from the derivative control values, scale_i: sum_k |u_ax,k| + |q_plane| at its largest over the axes
// and planes the piece's box reaches; in voxel units): a blocked voxel the exact curve penetrates deeper than tol_pos is never
// missed, one it stays farther than tol_pos from is never reported, and a reported voxel is non-zero in the map with p(t_hit)
// within tol_pos of its closed box (for -2: of leaving).  The control values of a visit carry the Bernstein conversion (9
// roundings) and two de Casteljau passes of at most 7 steps of 3 roundings each: 51 roundings of eps / 2 on values bounded by
// sum_k |u_k| = 25.5 eps, plus the 4 eps of the coefficients: below kHitC eps scale_i.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "bernstein_walk.h"

namespace anet {

struct HitArgs {
  const double *coeffs, *T;  // [(i*3+ax)*2S + k][ld], [N][ld]
  const uint8_t *vox;        // sx * sy * sz bytes, x fastest
  double *t_hit;             // [N][ld]
  int32_t *voxel;            // [N][ld] or nullptr
  int64_t B, ld;
  int N;
  int size[3];
  double o[3], scale;
};

constexpr int kHitDepth = 32;        // smallest interval 2^-32
constexpr int kHitMaxNodes = 2048;   // intervals visited per piece at most
constexpr int kHitBisect = 56;       // halvings of a crossing at most (it stops when the midpoint meets an end)
constexpr int kHitBoxCells = 8;      // a box of more cells is split, not looked up
constexpr double kHitC = 32.0;       // in eps * scale: see ACCURACY
constexpr double kHitMaxScale = 1e300;
constexpr int32_t kHitFree = -1, kHitOutside = -2, kHitInvalid = -3;

// the cell of q on an axis of `size` cells, query's rule; -1 and `size` stand for the two outsides
__device__ inline int hit_cell(double q, int size) { return q <= -1.0 ? -1 : (q >= (double)size ? size : (int)q); }

template <int S>
__global__ void __launch_bounds__(64) k_traj_voxel_hit(HitArgs a) {
  constexpr int D = 2 * S, n = D - 1;  // D control values, degree n
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int i = blockIdx.y;
  const int64_t ld = a.ld;
  const int64_t o = (int64_t)i * ld + b;
  const uint8_t *__restrict__ vox = a.vox;
  const int sx = a.size[0], sy = a.size[1], sz = a.size[2];
  const double Ti = a.T[o];
  bool bad = !(Ti >= 0.0 && Ti < INFINITY);
  // qu[ax][k]: ascending coefficients of q_ax(T tau); bz: its Bernstein control values on [0, 1]
  double qu[3][D], bz[3][D];
  {
    double tk[D];
    tk[0] = 1.0;
#pragma unroll
    for (int k = 1; k < D; ++k) tk[k] = tk[k - 1] * Ti;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      double sa = 0.0;
#pragma unroll
      for (int p = 0; p < D; ++p) {
        const double c = a.coeffs[(int64_t)((i * 3 + ax) * D + (n - p)) * ld + b];
        bad = bad || !(fabs(c) < INFINITY);
        qu[ax][p] = (p == 0 ? c - a.o[ax] : c * tk[p]) / a.scale;
        sa += fabs(qu[ax][p]);
      }
      bad = bad || !(sa < kHitMaxScale);
      bern::to_bernstein<D>(qu[ax], bz[ax]);
    }
  }
  if (bad) {
    a.t_hit[o] = NAN;
    if (a.voxel) a.voxel[o] = kHitInvalid;
    return;
  }
  // -1: free; -2: outside; else the linear index of a blocked voxel.  The only voxel read, and only of indices inside the grid.
  auto probe = [&](int x, int y, int z) -> int32_t {
    if (x < 0 || y < 0 || z < 0 || x >= sx || y >= sy || z >= sz) return kHitOutside;
    const int64_t id = (int64_t)x + (int64_t)sx * ((int64_t)y + (int64_t)sy * (int64_t)z);
    return vox[id] != 0 ? (int32_t)id : kHitFree;
  };
  auto horner = [&](const double(&g)[D], double tau) { return bern::horner<D>(g, tau); };
  double tau_hit = INFINITY;
  int32_t vhit = kHitFree;
  bool done = false;
  int lev = 0;
  uint64_t idx = 0;
  for (int guard = 0; guard < kHitMaxNodes; ++guard) {
    const double width = ldexp(1.0, -lev), aa = (double)idx * width, bb = (double)(idx + 1) * width;
    const double rr = aa / bb;
    // the control values on [aa, bb], one axis at a time, reduced to the box, the ends and the direction
    double mn[3], mx[3], w0[3], wn[3];
    int mono[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      double w[D];
#pragma unroll
      for (int k = 0; k < D; ++k) w[k] = bz[ax][k];
      if (bb < 1.0) {  // the left part of the split at bb: [0, bb]
        double le[D];
        le[0] = w[0];
#pragma unroll
        for (int q = 1; q < D; ++q) {
#pragma unroll
          for (int k = 0; k < D - q; ++k) w[k] = __builtin_fma(bb, w[k + 1] - w[k], w[k]);
          le[q] = w[0];
        }
#pragma unroll
        for (int k = 0; k < D; ++k) w[k] = le[k];
      }
      if (aa > 0.0) {  // the right part of the split of [0, bb] at aa / bb: [aa, bb]
        double ri[D];
        ri[n] = w[n];
#pragma unroll
        for (int q = 1; q < D; ++q) {
#pragma unroll
          for (int k = 0; k < D - q; ++k) w[k] = __builtin_fma(rr, w[k + 1] - w[k], w[k]);
          ri[n - q] = w[n - q];
        }
#pragma unroll
        for (int k = 0; k < D; ++k) w[k] = ri[k];
      }
      double lo = w[0], hi = w[0];
      bool up = true, down = true;
#pragma unroll
      for (int k = 1; k < D; ++k) {
        lo = fmin(lo, w[k]);
        hi = fmax(hi, w[k]);
        up = up && w[k] > w[k - 1];
        down = down && w[k] < w[k - 1];
      }
      mn[ax] = lo; mx[ax] = hi; w0[ax] = w[0]; wn[ax] = w[n];
      mono[ax] = up ? 1 : (down ? -1 : 0);
    }
    const int lx = hit_cell(mn[0], sx), hx = hit_cell(mx[0], sx), ly = hit_cell(mn[1], sy), hy = hit_cell(mx[1], sy),
              lz = hit_cell(mn[2], sz), hz = hit_cell(mx[2], sz);
    const int nx = hx - lx + 1, ny = hy - ly + 1, nz = hz - lz + 1;
    const int64_t count = (int64_t)nx * ny * nz;
    bool split = false, decided = false;  // decided: free, or a hit was found
    if (count <= kHitBoxCells) {
      bool any = false;
      int x = lx, y = ly, z = lz;
      for (int c = 0; c < kHitBoxCells && c < (int)count; ++c) {
        any = any || probe(x, y, z) != kHitFree;
        if (++x > hx) {
          x = lx;
          if (++y > hy) { y = ly; ++z; }
        }
      }
      if (!any) {
        decided = true;  // free
      } else {
        const int cx = hit_cell(w0[0], sx), cy = hit_cell(w0[1], sy), cz = hit_cell(w0[2], sz);
        const int32_t at = probe(cx, cy, cz);
        if (at != kHitFree) {  // the start point is blocked and everything before it was free
          tau_hit = aa; vhit = at; done = true; decided = true;
        } else if (count == 2) {
          const int ax = nx == 2 ? 0 : (ny == 2 ? 1 : 2);
          const int dir = ax == 0 ? mono[0] : (ax == 1 ? mono[1] : mono[2]);
          if (dir != 0) {
            const int size = ax == 0 ? sx : (ax == 1 ? sy : sz);
            const int cs = ax == 0 ? cx : (ax == 1 ? cy : cz);
            const double end = ax == 0 ? wn[0] : (ax == 1 ? wn[1] : wn[2]);
            decided = true;
            if (hit_cell(end, size) != cs) {  // it crosses into the other cell, which is the blocked one
              double g[D];
#pragma unroll
              for (int k = 0; k < D; ++k) g[k] = ax == 0 ? qu[0][k] : (ax == 1 ? qu[1][k] : qu[2][k]);
              double l = aa, h = bb;
              for (int it = 0; it < kHitBisect; ++it) {
                const double m = 0.5 * (l + h);
                if (!(m > l && m < h)) break;
                if (hit_cell(horner(g, m), size) != cs) h = m; else l = m;
              }
              const int co = cs == (ax == 0 ? lx : (ax == 1 ? ly : lz)) ? cs + 1 : cs - 1;
              tau_hit = h;
              vhit = probe(ax == 0 ? co : cx, ax == 1 ? co : cy, ax == 2 ? co : cz);
              done = true;
            }
          }
        }
      }
    }
    if (!decided) {
      if (lev < kHitDepth) {
        split = true;
      } else {  // the depth bound: the cell of the midpoint decides
        const double m = 0.5 * (aa + bb);
        const int32_t at = probe(hit_cell(horner(qu[0], m), sx), hit_cell(horner(qu[1], m), sy), hit_cell(horner(qu[2], m), sz));
        if (at != kHitFree) { tau_hit = aa; vhit = at; done = true; }
      }
    }
    if (done) break;
    if (split) {
      ++lev;
      idx <<= 1;
    } else {
      for (int q = 0; q < kHitDepth && lev > 0 && (idx & 1u); ++q) { idx >>= 1; --lev; }
      if (lev == 0) { done = true; break; }  // the whole piece is free
      idx += 1;
    }
  }
  if (!done) {  // the budget ran out: free before the first undecided interval, unknown from there on
    tau_hit = (double)idx * ldexp(1.0, -lev);
    vhit = kHitInvalid;
  }
  a.t_hit[o] = vhit == kHitFree ? INFINITY : tau_hit * Ti;
  if (a.voxel) a.voxel[o] = vhit;
}

}  // namespace anet
