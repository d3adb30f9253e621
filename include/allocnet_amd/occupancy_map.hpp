// voxel_map::OccupancyMap: a log-odds occupancy grid on the MI355X, filled from sensor scans by ray carving (anet_occupancy_*),
// next to voxel_map::VoxelMap, which it hands its state to.  The reference has no counterpart: its mapCallBack stamps the
// simulator's finished world cloud.  A scan also says what is free (the voxels between the sensor and a return), what is unknown
// (the voxels no ray crossed) and what has changed (a voxel seen through often enough becomes free again); the rules are in
// allocnet_amd.h.  Constructed like VoxelMap, plus the parameters; toVoxelMap writes the bytes dilate, getSurf, planPath and the
// trajectory checks take.  voxel_map::raycast is the first hit of a segment on a VoxelMap's bytes (a line-of-sight test, or the
// sensor of a simulation).  frontier / frontierClusters / viewGain say where to look next on a map with unknown space, and
// voxel_map::components labels the mutually reachable free voxels of a VoxelMap (anet_occupancy_frontier_dev,
// anet_voxel_label_components_dev, anet_voxel_component_stats_dev, anet_occupancy_view_gain_dev).
// Vectors are duck-typed as in core.hpp: anything with (i) access goes in.  C++14, no Eigen or HIP headers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "core.hpp"
#include "voxel_map.hpp"

namespace voxel_map {

// anet_occupancy_params from probabilities: units * log(p / (1 - p)), rounded to the nearest integer
inline anet_occupancy_params occupancyParams(double p_hit = 0.7, double p_miss = 0.4, double p_min = 0.12, double p_max = 0.97,
                                             double min_range = 0.0, double max_range = 10.0, double units = 1000.0) {
  anet_occupancy_params p;
  p.hit = (int32_t)std::lround(units * std::log(p_hit / (1.0 - p_hit)));
  p.miss = (int32_t)std::lround(units * std::log(p_miss / (1.0 - p_miss)));
  p.lo = (int32_t)std::lround(units * std::log(p_min / (1.0 - p_min)));
  p.hi = (int32_t)std::lround(units * std::log(p_max / (1.0 - p_max)));
  p.min_range = min_range;
  p.max_range = max_range;
  return p;
}

// a frontier cluster: its least voxel index, voxel count, world centroid origin + (sum / count + 0.5) scale, inclusive cell box
struct FrontierCluster {
  int32_t root, count;
  double centroid[3];
  int32_t lo[3], hi[3];
};

namespace detail {
// device bytes for the length of a call
struct DevBytes {
  anet::Context &ctx;
  double *p = nullptr;
  size_t doubles;
  DevBytes(anet::Context &c, size_t bytes) : ctx(c), doubles((bytes + 7) / 8 + 1) { ctx.check(anet_dev_alloc(ctx.get(), doubles, &p)); }
  DevBytes(const DevBytes &) = delete;
  DevBytes &operator=(const DevBytes &) = delete;
  ~DevBytes() { anet_dev_free(p); }
  template <class T>
  void put(const T *host, size_t n) {
    std::vector<double> buf((n * sizeof(T) + 7) / 8);
    std::memcpy(buf.data(), host, n * sizeof(T));
    ctx.check(anet_dev_upload(ctx.get(), p, buf.data(), buf.size()));
  }
  template <class T>
  std::vector<T> get(size_t n) const {
    std::vector<double> buf((n * sizeof(T) + 7) / 8);
    ctx.check(anet_dev_download(ctx.get(), buf.data(), p, buf.size()));
    std::vector<T> out(n);
    std::memcpy(out.data(), buf.data(), n * sizeof(T));
    return out;
  }
};

// labels of the bytes != 0 of `mask` (host, one per voxel): -1 off the set, else the least voxel index of the component; the
// device labels and the workspace stay in labels_out / work_out when given
inline std::vector<int32_t> label(anet::Context &ctx, const anet_voxel_grid &g, const std::vector<uint8_t> &mask, int connectivity,
                                  DevBytes *labels_out = nullptr, DevBytes *work_out = nullptr) {
  const size_t n = mask.size();
  const int64_t ws = anet_voxel_components_workspace(&g);
  if (ws < 0) throw anet::Error(ANET_ERR_INVALID, "voxel_map::components: bad grid");
  DevBytes dm(ctx, n), own_l(ctx, labels_out ? 8 : n * 4), own_w(ctx, work_out ? 8 : (size_t)ws);
  DevBytes &dl = labels_out ? *labels_out : own_l, &dw = work_out ? *work_out : own_w;
  dm.put(mask.data(), n);
  ctx.check(anet_voxel_label_components_dev(ctx.get(), &g, (const uint8_t *)dm.p, connectivity, (int32_t *)dl.p, dw.p, nullptr,
                                            anet_stream(ctx.get())));
  return dl.get<int32_t>(n);
}
}  // namespace detail

class OccupancyMap {
 public:
  OccupancyMap() = default;
  template <class V3i, class V3d>
  OccupancyMap(const V3i &size, const V3d &origin, const double &voxScale, const anet_occupancy_params &params = occupancyParams())
      : prm_(params) {
    for (int c = 0; c < 3; ++c) {
      g_.size[c] = (int32_t)size(c);
      g_.origin[c] = origin(c);
    }
    g_.scale = voxScale;
    const int64_t ws = anet_occupancy_workspace(&g_);
    if (ws < 0) throw anet::Error(ANET_ERR_INVALID, "voxel_map::OccupancyMap: sizes >= 1, fewer than 2^31 voxels, scale > 0");
    voxNum_ = (int64_t)g_.size[0] * g_.size[1] * g_.size[2];
    anet::Context &ctx = anet::Context::thread_default();
    logodds_ = alloc_bytes(ctx, (size_t)voxNum_ * 2);
    work_ = alloc_bytes(ctx, (size_t)ws);
    reset();
  }
  OccupancyMap(const OccupancyMap &) = delete;
  OccupancyMap &operator=(const OccupancyMap &) = delete;
  OccupancyMap(OccupancyMap &&o) noexcept { swap(o); }
  OccupancyMap &operator=(OccupancyMap &&o) noexcept {
    swap(o);
    return *this;
  }
  ~OccupancyMap() {
    anet_dev_free((double *)logodds_);
    anet_dev_free((double *)work_);
  }

  Vec3i getSize() const { return Vec3i(g_.size[0], g_.size[1], g_.size[2]); }
  double getScale() const { return g_.scale; }
  anet::Vec3 getOrigin() const { return anet::Vec3(g_.origin[0], g_.origin[1], g_.origin[2]); }
  const anet_occupancy_params &params() const { return prm_; }
  const anet_voxel_grid &grid() const { return g_; }
  const int16_t *logodds_dev() const { return (const int16_t *)logodds_; }

  // every voxel unknown again
  void reset() {
    anet::Context &ctx = anet::Context::thread_default();
    ctx.check(anet_occupancy_reset_dev(ctx.get(), &g_, (int16_t *)logodds_, work_, anet_stream(ctx.get())));
    ctx.check(anet_synchronize(ctx.get()));
  }

  // one scan: world-frame points (anything with (i) access) seen from `origin`
  template <class V3d, class O3d>
  void insertPointCloud(const std::vector<V3d> &points, const O3d &origin) {
    std::vector<double> flat;
    flat.reserve(points.size() * 3);
    for (const V3d &p : points) {
      flat.push_back(p(0)); flat.push_back(p(1)); flat.push_back(p(2));
    }
    const double o[3] = {origin(0), origin(1), origin(2)};
    anet::Context &ctx = anet::Context::thread_default();
    ctx.check(anet_occupancy_integrate(ctx.get(), &g_, &prm_, (int16_t *)logodds_, o, flat.data(), (int64_t)points.size(), 24, 1, work_));
  }
  // one scan from a PointCloud2's float32 records in the world frame: n of them, point_step bytes apart, x y z first
  template <class O3d>
  void insertPointCloud(const float *data, size_t n, size_t point_step, const O3d &origin) {
    const double o[3] = {origin(0), origin(1), origin(2)};
    anet::Context &ctx = anet::Context::thread_default();
    ctx.check(anet_occupancy_integrate(ctx.get(), &g_, &prm_, (int16_t *)logodds_, o, data, (int64_t)n, (int64_t)point_step, 0, work_));
  }
  // one scan from a depth image on the HOST (row-major [height][width], float metres or uint16_t times depth_scale), intrinsics
  // fx, fy, cx, cy, the camera-to-world pose R (anything with (r, c) access) and t; the sensor origin is t
  template <class Pixel, class M3, class V3d>
  void insertDepth(const Pixel *depth, int width, int height, double fx, double fy, double cx, double cy, const M3 &R, const V3d &t,
                   int step = 1, double depth_scale = 1.0, double min_depth = 0.0,
                   double max_depth = std::numeric_limits<double>::infinity()) {
    static_assert((std::is_same<Pixel, float>::value || std::is_same<Pixel, uint16_t>::value), "depth pixels are float or uint16_t");
    if (width < 1 || height < 1 || step < 1) throw anet::Error(ANET_ERR_INVALID, "voxel_map::OccupancyMap::insertDepth: width, height, step >= 1");
    const double K[4] = {fx, fy, cx, cy}, tt[3] = {t(0), t(1), t(2)};
    double RR[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) RR[r * 3 + c] = R(r, c);
    anet::Context &ctx = anet::Context::thread_default();
    const size_t bytes = (size_t)width * height * sizeof(Pixel);
    const size_t n = (size_t)((width + step - 1) / step) * (size_t)((height + step - 1) / step);
    std::vector<double> buf((bytes + 7) / 8);
    std::memcpy(buf.data(), depth, bytes);
    uint8_t *d = alloc_bytes(ctx, buf.size() * 8 + n * 24);
    double *pts = (double *)(d + buf.size() * 8);
    void *st = anet_stream(ctx.get());
    int rc = anet_dev_upload(ctx.get(), (double *)d, buf.data(), buf.size());
    if (rc == ANET_OK)
      rc = anet_depth_to_points_dev(ctx.get(), d, std::is_same<Pixel, uint16_t>::value ? 1 : 0, width, height, step, depth_scale, K, RR,
                                    tt, min_depth, max_depth, pts, st);
    if (rc == ANET_OK) rc = anet_occupancy_integrate_dev(ctx.get(), &g_, &prm_, (int16_t *)logodds_, tt, pts, (int64_t)n, 24, 1, work_, st);
    if (rc == ANET_OK) rc = anet_synchronize(ctx.get());
    anet_dev_free((double *)d);
    ctx.check(rc);
  }

  // the hand-over: vm's bytes become 1 where the log-odds are known and >= occ, and where they are unknown when unknownBlocked;
  // 0 elsewhere.  vm must have this map's size, origin and scale; its surface is what its next dilate makes it.
  void toVoxelMap(VoxelMap &vm, int occ = 0, bool unknownBlocked = true) const {
    const anet_voxel_grid &o = vm.grid();
    if (std::memcmp(o.size, g_.size, sizeof(g_.size)) != 0 || std::memcmp(o.origin, g_.origin, sizeof(g_.origin)) != 0 || o.scale != g_.scale)
      throw anet::Error(ANET_ERR_INVALID, "voxel_map::OccupancyMap::toVoxelMap: the VoxelMap must have this map's size, origin and scale");
    vm.flush();
    anet::Context &ctx = anet::Context::thread_default();
    ctx.check(anet_occupancy_to_voxels_dev(ctx.get(), &g_, (const int16_t *)logodds_, occ, unknownBlocked ? 1 : 0, vm.vox_,
                                           anet_stream(ctx.get())));
    ctx.check(anet_synchronize(ctx.get()));
    vm.stale_ = true;
    vm.dist_valid_[0] = vm.dist_valid_[1] = false;
  }

  // overwrite the grid with a host copy (a saved map): one value per voxel
  void setLogOdds(const std::vector<int16_t> &L) {
    if ((int64_t)L.size() != voxNum_) throw anet::Error(ANET_ERR_INVALID, "voxel_map::OccupancyMap::setLogOdds: one value per voxel");
    std::vector<double> buf((size_t)((voxNum_ * 2 + 7) / 8));
    std::memcpy(buf.data(), L.data(), (size_t)voxNum_ * 2);
    anet::Context &ctx = anet::Context::thread_default();
    ctx.check(anet_dev_upload(ctx.get(), (double *)logodds_, buf.data(), buf.size()));
  }

  // the frontier: one byte per voxel, 1 where the voxel is known, below occ and has an unknown face neighbour inside the map
  std::vector<uint8_t> frontier(int occ = 0, int64_t *count = nullptr) const {
    anet::Context &ctx = anet::Context::thread_default();
    detail::DevBytes dm(ctx, (size_t)voxNum_), dc(ctx, 8);
    ctx.check(anet_occupancy_frontier_dev(ctx.get(), &g_, (const int16_t *)logodds_, occ, nullptr, nullptr, (uint8_t *)dm.p, (int64_t *)dc.p,
                                          anet_stream(ctx.get())));
    if (count) *count = dc.get<int64_t>(1)[0];
    return dm.get<uint8_t>((size_t)voxNum_);
  }

  // the frontier grouped into connected clusters (6 or 26 neighbours) of at least min_size voxels, in ascending root order
  std::vector<FrontierCluster> frontierClusters(int occ = 0, int min_size = 8, int connectivity = 26, int max_components = 65536) const {
    anet::Context &ctx = anet::Context::thread_default();
    const size_t n = (size_t)voxNum_, m = (size_t)max_components;
    const int64_t ws = anet_voxel_components_workspace(&g_);
    detail::DevBytes dl(ctx, n * 4), dw(ctx, (size_t)ws), dn(ctx, 8), dr(ctx, m * 4), dc(ctx, m * 4), ds(ctx, m * 24), db(ctx, m * 24);
    detail::label(ctx, g_, frontier(occ), connectivity, &dl, &dw);
    ctx.check(anet_voxel_component_stats_dev(ctx.get(), &g_, (const int32_t *)dl.p, max_components, (int32_t *)dn.p, (int32_t *)dr.p,
                                             (int32_t *)dc.p, (int64_t *)ds.p, (int32_t *)db.p, dw.p, anet_stream(ctx.get())));
    const size_t k = std::min<size_t>((size_t)dn.get<int32_t>(1)[0], m);
    const std::vector<int32_t> root = dr.get<int32_t>(k), cnt = dc.get<int32_t>(k), box = db.get<int32_t>(k * 6);
    const std::vector<int64_t> sum = ds.get<int64_t>(k * 3);
    std::vector<FrontierCluster> out;
    for (size_t i = 0; i < k; ++i) {
      if (cnt[i] < min_size) continue;
      FrontierCluster c;
      c.root = root[i];
      c.count = cnt[i];
      for (int a = 0; a < 3; ++a) {
        c.centroid[a] = g_.origin[a] + ((double)sum[i * 3 + a] / (double)cnt[i] + 0.5) * g_.scale;
        c.lo[a] = box[i * 6 + a];
        c.hi[a] = box[i * 6 + 3 + a];
      }
      out.push_back(c);
    }
    return out;
  }

  // per pose (R [V][9] row-major camera-to-world, t [V][3]) the number of distinct unknown voxels a scan with the sensor-frame
  // template pts [n][3] would cross, by this map's parameters; -1 for a pose with a non-finite entry
  std::vector<int32_t> viewGain(const std::vector<double> &R, const std::vector<double> &t, const std::vector<double> &pts, int occ = 0) const {
    const size_t V = t.size() / 3, n = pts.size() / 3;
    if (R.size() != V * 9 || t.size() != V * 3 || pts.size() != n * 3)
      throw anet::Error(ANET_ERR_INVALID, "voxel_map::OccupancyMap::viewGain: R [V][9], t [V][3], pts [n][3]");
    if (V == 0) return std::vector<int32_t>();
    anet::Context &ctx = anet::Context::thread_default();
    // at most eight views per chunk: a slot of marks is megabytes on a large map at a long range
    const int64_t ws = anet_occupancy_view_gain_workspace(&g_, &prm_, (int32_t)std::min<size_t>(V, 8));
    if (ws < 0) throw anet::Error(ANET_ERR_INVALID, "voxel_map::OccupancyMap::viewGain: bad parameters");
    detail::DevBytes dR(ctx, V * 72), dt(ctx, V * 24), dp(ctx, n * 24), dg(ctx, V * 4), dw(ctx, (size_t)ws);
    dR.put(R.data(), R.size());
    dt.put(t.data(), t.size());
    if (n) dp.put(pts.data(), pts.size());
    const std::vector<double> zero(dw.doubles, 0.0);  // the marks start at zero (and are zero again afterwards)
    ctx.check(anet_dev_upload(ctx.get(), dw.p, zero.data(), zero.size()));
    ctx.check(anet_occupancy_view_gain_dev(ctx.get(), &g_, &prm_, (const int16_t *)logodds_, occ, dR.p, dt.p, (int32_t)V, dp.p, (int32_t)n,
                                           (int32_t *)dg.p, dw.p, ws, anet_stream(ctx.get())));
    return dg.get<int32_t>(V);
  }

  // host copy of the grid: ANET_OCC_UNKNOWN where nothing was observed
  std::vector<int16_t> getLogOdds() const {
    std::vector<double> buf((size_t)((voxNum_ * 2 + 7) / 8));
    anet::Context &ctx = anet::Context::thread_default();
    ctx.check(anet_dev_download(ctx.get(), buf.data(), (const double *)logodds_, buf.size()));
    std::vector<int16_t> out((size_t)voxNum_);
    std::memcpy(out.data(), buf.data(), (size_t)voxNum_ * 2);
    return out;
  }

 private:
  anet_voxel_grid g_{};
  anet_occupancy_params prm_{};
  int64_t voxNum_ = 0;
  uint8_t *logodds_ = nullptr, *work_ = nullptr;

  static uint8_t *alloc_bytes(anet::Context &ctx, size_t bytes) {
    double *p = nullptr;
    ctx.check(anet_dev_alloc(ctx.get(), (bytes + 7) / 8, &p));
    return (uint8_t *)p;
  }
  void swap(OccupancyMap &o) noexcept {
    std::swap(g_, o.g_); std::swap(prm_, o.prm_); std::swap(voxNum_, o.voxNum_);
    std::swap(logodds_, o.logodds_); std::swap(work_, o.work_);
  }
};

// First hit of the segment o -> q on the map's bytes (anet_voxel_raycast_dev): the linear index of the first visited voxel != 0
// and, in t, the parameter in [0, 1] at which it was entered; ANET_HIT_FREE and t = 1 when there is none, ANET_HIT_INVALID and
// NaN for a segment that cannot be walked.  The outside of the map is passed through, not blocked (unlike VoxelMap::query).
template <class A, class B>
inline int32_t raycast(const VoxelMap &map, const A &o, const B &q, double &t) {
  anet::Context &ctx = anet::Context::thread_default();
  double *buf = nullptr;  // o [3], q [3], t [1], the voxel index [1]
  ctx.check(anet_dev_alloc(ctx.get(), 8, &buf));
  double h[8] = {(double)o(0), (double)o(1), (double)o(2), (double)q(0), (double)q(1), (double)q(2), 0.0, 0.0};
  int rc = anet_dev_upload(ctx.get(), buf, h, 6);
  if (rc == ANET_OK)
    rc = anet_voxel_raycast_dev(ctx.get(), &map.grid(), map.voxels_dev(), buf, buf + 3, 1, (int32_t *)(buf + 7), buf + 6, anet_stream(ctx.get()));
  if (rc == ANET_OK) rc = anet_dev_download(ctx.get(), h, buf, 8);
  anet_dev_free(buf);
  ctx.check(rc);
  t = h[6];
  int32_t v;
  std::memcpy(&v, &h[7], sizeof(v));
  return v;
}

// Connected components of the FREE voxels of a map (6 or 26 neighbours): one label per voxel, -1 for a blocked voxel, else the
// least voxel index of the component -- two free voxels are mutually reachable exactly when their labels are equal.
inline std::vector<int32_t> components(const VoxelMap &map, int connectivity = 26) {
  std::vector<uint8_t> free_bytes = map.getVoxels();
  for (uint8_t &b : free_bytes) b = b == 0 ? 1 : 0;
  return detail::label(anet::Context::thread_default(), map.grid(), free_bytes, connectivity);
}

}  // namespace voxel_map
