// The trilinear query of the exact distance field (distance_kernels.h builds the field and states the query's rule; include/allocnet_amd.h
// is the contract): the device functions that more than one translation unit needs -- api_distance.hip for k_vox_dist_query and
// k_minco_obstacle, api_stop.hip for k_minco_stop and k_traj_stop_margin.  No kernel is defined here.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace anet {

constexpr int32_t kDistNone = INT32_MAX;  // ANET_DIST_NONE

struct DistGrid {
  int size[3];
  double oc[3], scale;  // oc = origin + 0.5 * scale, formed on the host as voxel_map.hpp forms it
};

// cell and fraction of one axis; `moves`: the interpolant depends on the coordinate there (f not clamped, more than one voxel)
__device__ __forceinline__ void dist_axis(const double p, const double oc, const double scale, const int size, int &i0, int &i1,
                                          double &f, bool &moves) {
#pragma clang fp contract(off)
  const double u = (p - oc) / scale;
  const double hi = (double)max(size - 2, 0);
  const double fl = fmin(fmax(floor(u), 0.0), hi);  // clamped in double: no conversion of a huge value
  i0 = (int)fl;
  i1 = min(i0 + 1, size - 1);
  const double fr = u - fl;
  f = fmin(fmax(fr, 0.0), 1.0);
  moves = size > 1 && fr >= 0.0 && fr <= 1.0;
}

// dist and grad of the field at p.  A non-finite coordinate gives NaN in all four; a sentinel corner (a uniform map) +-inf and 0.
__device__ __forceinline__ void dist_sample(const DistGrid &g, const int32_t *__restrict__ sd2, const double px, const double py,
                                            const double pz, double &dist, double &gx, double &gy, double &gz) {
  if (!(fabs(px) < INFINITY && fabs(py) < INFINITY && fabs(pz) < INFINITY)) {
    dist = gx = gy = gz = __builtin_nan("");
    return;
  }
  int x0, x1, y0, y1, z0, z1;
  double fx, fy, fz;
  bool mx, my, mz;
  dist_axis(px, g.oc[0], g.scale, g.size[0], x0, x1, fx, mx);
  dist_axis(py, g.oc[1], g.scale, g.size[1], y0, y1, fy, my);
  dist_axis(pz, g.oc[2], g.scale, g.size[2], z0, z1, fz, mz);
  const int64_t sx = g.size[0], sxy = sx * g.size[1];
  const int64_t r00 = y0 * sx + z0 * sxy, r10 = y1 * sx + z0 * sxy, r01 = y0 * sx + z1 * sxy, r11 = y1 * sx + z1 * sxy;
  const int32_t s000 = sd2[r00 + x0], s100 = sd2[r00 + x1], s010 = sd2[r10 + x0], s110 = sd2[r10 + x1];
  const int32_t s001 = sd2[r01 + x0], s101 = sd2[r01 + x1], s011 = sd2[r11 + x0], s111 = sd2[r11 + x1];
  auto none = [](const int32_t s) { return s == kDistNone || s == -kDistNone; };
  if (none(s000) || none(s100) || none(s010) || none(s110) || none(s001) || none(s101) || none(s011) || none(s111)) {
    dist = s000 > 0 ? INFINITY : -INFINITY;
    gx = gy = gz = 0.0;
    return;
  }
  auto D = [&](const int32_t s) {
    const double r = sqrt((double)abs(s));
    return g.scale * (s < 0 ? -r : r);
  };
  const double d000 = D(s000), d100 = D(s100), d010 = D(s010), d110 = D(s110);
  const double d001 = D(s001), d101 = D(s101), d011 = D(s011), d111 = D(s111);
  const double ex = 1.0 - fx, ey = 1.0 - fy, ez = 1.0 - fz;
  // along x, then y, then z
  const double c00 = d000 * ex + d100 * fx, c10 = d010 * ex + d110 * fx, c01 = d001 * ex + d101 * fx, c11 = d011 * ex + d111 * fx;
  const double c0 = c00 * ey + c10 * fy, c1 = c01 * ey + c11 * fy;
  dist = c0 * ez + c1 * fz;
  const double e00 = d100 - d000, e10 = d110 - d010, e01 = d101 - d001, e11 = d111 - d011;
  gx = mx ? ((e00 * ey + e10 * fy) * ez + (e01 * ey + e11 * fy) * fz) / g.scale : 0.0;
  gy = my ? ((c10 - c00) * ez + (c11 - c01) * fz) / g.scale : 0.0;
  gz = mz ? (c1 - c0) / g.scale : 0.0;
}

}  // namespace anet
