// Source-compatible stand-in for the reference's voxel_map::VoxelMap (src/planner/include/gcopter/voxel_map.hpp,
// voxel_dilater.hpp) with the map on the MI355X: the fill, the dilation, the surface and convexCover's per-segment point
// selection run as device kernels behind the C ABI (anet_voxel_*).  Same constructor, public members and constants;
// byte-identical voxels and bit-identical surface coordinates.  One difference the caller can see: getSurf lists the
// surface in ascending voxel index order (x fastest), the reference in breadth-first discovery order -- the same set.
//   - setOccupied(pos) and setOccupied(id) one at a time (mapCallBack's loop) are buffered on the host and scattered in
//     one launch each before the next call that reads the map; setOccupied(data, n, point_step) takes a PointCloud2's
//     float32 records in bulk.
//   - query(pos) one point at a time (OMPL's validity checker) answers from a host mirror of the voxel bytes, refreshed
//     lazily after a dilate or a flush; query(pos, n, out) batches on the device.
// Vectors are duck-typed as in core.hpp: anything with (i) access goes in, Eigen::Vector3d / Vector3i come out.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "core.hpp"

namespace voxel_map {

constexpr uint8_t Unoccupied = 0;
constexpr uint8_t Occupied = 1;
constexpr uint8_t Dilated = 2;

// integer 3-vector (what the reference returns as Eigen::Vector3i)
struct Vec3i {
  int v[3] = {0, 0, 0};
  Vec3i() = default;
  Vec3i(int x, int y, int z) : v{x, y, z} {}
  int &operator()(int i) { return v[i]; }
  int operator()(int i) const { return v[i]; }
  template <class V, class = typename std::enable_if<std::is_constructible<V, int, int, int>::value &&
                                                     !std::is_same<V, Vec3i>::value>::type>
  operator V() const {
    return V(v[0], v[1], v[2]);
  }
};

class OccupancyMap;  // occupancy_map.hpp: writes the voxel bytes from its log-odds (toVoxelMap)

class VoxelMap {
  friend class OccupancyMap;

 public:
  VoxelMap() = default;
  template <class V3i, class V3d>
  VoxelMap(const V3i &size, const V3d &origin, const double &voxScale) : scale_(voxScale) {
    for (int c = 0; c < 3; ++c) {
      g_.size[c] = (int32_t)size(c);
      g_.origin[c] = origin(c);
    }
    g_.scale = voxScale;
    const int64_t ws = anet_voxel_workspace(&g_);
    if (ws < 0) throw anet::Error(ANET_ERR_INVALID, "voxel_map::VoxelMap: sizes >= 1, fewer than 2^31 voxels, scale > 0");
    voxNum_ = (int64_t)g_.size[0] * g_.size[1] * g_.size[2];
    anet::Context &ctx = anet::Context::thread_default();
    vox_ = alloc_bytes(ctx, voxNum_);
    work_ = alloc_bytes(ctx, ws);
    count_ = alloc_bytes(ctx, 8);
    std::vector<double> zero((size_t)((voxNum_ + 7) / 8), 0.0);
    ctx.check(anet_dev_upload(ctx.get(), (double *)vox_, zero.data(), zero.size()));
    mirror_.assign((size_t)voxNum_, Unoccupied);
  }
  VoxelMap(const VoxelMap &) = delete;
  VoxelMap &operator=(const VoxelMap &) = delete;
  VoxelMap(VoxelMap &&o) noexcept { swap(o); }
  VoxelMap &operator=(VoxelMap &&o) noexcept {
    swap(o);
    return *this;
  }
  ~VoxelMap() {
    for (uint8_t *p : {vox_, work_, count_, ids_, pts_, dist_[0], dist_[1]}) anet_dev_free((double *)p);
  }

  Vec3i getSize() const { return Vec3i(g_.size[0], g_.size[1], g_.size[2]); }
  double getScale() const { return scale_; }
  anet::Vec3 getOrigin() const { return anet::Vec3(g_.origin[0], g_.origin[1], g_.origin[2]); }
  anet::Vec3 getCorner() const {
    return anet::Vec3((double)g_.size[0] * scale_ + g_.origin[0], (double)g_.size[1] * scale_ + g_.origin[1],
                      (double)g_.size[2] * scale_ + g_.origin[2]);
  }
  const std::vector<uint8_t> &getVoxels() const {
    refresh();
    return mirror_;
  }

  // setOccupied(Eigen::Vector3d pos) / setOccupied(Eigen::Vector3i id)
  template <class V>
  void setOccupied(const V &p) {
    set_one(p, std::is_integral<typename std::decay<decltype(p(0))>::type>());
  }
  // PointCloud2 records: n of them, point_step bytes apart, x y z float32 first; non-finite records are skipped
  void setOccupied(const float *data, size_t n, size_t point_step) {
    flush();
    if (n == 0) return;
    anet::Context &ctx = anet::Context::thread_default();
    const size_t bytes = (n - 1) * point_step + 3 * sizeof(float);
    std::vector<double> buf((bytes + 7) / 8);
    std::memcpy(buf.data(), data, bytes);
    uint8_t *d = alloc_bytes(ctx, buf.size() * 8);
    int rc = anet_dev_upload(ctx.get(), (double *)d, buf.data(), buf.size());
    if (rc == ANET_OK)
      rc = anet_voxel_set_occupied_dev(ctx.get(), &g_, vox_, d, (int64_t)n, (int64_t)point_step, 0, anet_stream(ctx.get()));
    if (rc == ANET_OK) rc = anet_synchronize(ctx.get());
    anet_dev_free((double *)d);
    ctx.check(rc);
    stale_ = true;
    dist_valid_[0] = dist_valid_[1] = false;
  }

  void dilate(const int &r) {
    if (r <= 0) return;
    flush();
    anet::Context &ctx = anet::Context::thread_default();
    void *st = anet_stream(ctx.get());
    ctx.check(anet_voxel_dilate_dev(ctx.get(), &g_, vox_, r, work_, st));
    ctx.check(anet_voxel_surface_dev(ctx.get(), &g_, work_, ids_cap_, (int32_t *)ids_, (int32_t *)count_, st));
    double c8 = 0.0;
    ctx.check(anet_dev_download(ctx.get(), &c8, (const double *)count_, 1));
    int32_t n;
    std::memcpy(&n, &c8, sizeof(n));
    if (n > ids_cap_) {  // the last front stays in the workspace: compact again into a buffer that fits
      anet_dev_free((double *)ids_);
      ids_ = nullptr;
      ids_cap_ = 0;
      ids_ = alloc_bytes(ctx, (size_t)n * 4);
      ids_cap_ = n;
      ctx.check(anet_voxel_surface_dev(ctx.get(), &g_, work_, ids_cap_, (int32_t *)ids_, (int32_t *)count_, st));
    }
    nsurf_ = n;
    pts_dev_valid_ = pts_host_valid_ = false;
    stale_ = true;
    dist_valid_[0] = dist_valid_[1] = false;
  }

  template <class V3i, class V3d>
  void getSurfInBox(const V3i &center, const int &halfWidth, std::vector<V3d> &points) const {
    const std::vector<double> &p = surf_points();
    std::vector<int32_t> ids = surf_ids();
    const int64_t sx = g_.size[0], sxy = (int64_t)g_.size[0] * g_.size[1];
    for (size_t i = 0; i < ids.size(); ++i) {
      const int64_t id = ids[i], z = id / sxy, y = (id - z * sxy) / sx, x = id - z * sxy - y * sx;
      if (std::llabs(x - center(0)) <= halfWidth && std::llabs(y - center(1)) <= halfWidth && std::llabs(z - center(2)) <= halfWidth)
        points.emplace_back(p[i * 3], p[i * 3 + 1], p[i * 3 + 2]);
    }
  }
  template <class V3d>
  void getSurf(std::vector<V3d> &points) const {
    const std::vector<double> &p = surf_points();
    points.reserve(points.size() + (size_t)nsurf_);
    for (int64_t i = 0; i < nsurf_; ++i) points.emplace_back(p[i * 3], p[i * 3 + 1], p[i * 3 + 2]);
  }

  // query(Eigen::Vector3d pos) / query(Eigen::Vector3i id): true outside the map or in a voxel != 0
  template <class V>
  bool query(const V &p) const {
    return query_one(p, std::is_integral<typename std::decay<decltype(p(0))>::type>());
  }
  // batched: pos [n][3] HOST doubles -> out[n] 0/1 on the device
  void query(const double *pos, size_t n, uint8_t *out) const {
    flush();
    if (n == 0) return;
    anet::Context &ctx = anet::Context::thread_default();
    uint8_t *dp = alloc_bytes(ctx, n * 24), *dq = alloc_bytes(ctx, n);
    std::vector<double> res((n + 7) / 8);
    int rc = anet_dev_upload(ctx.get(), (double *)dp, pos, n * 3);
    if (rc == ANET_OK) rc = anet_voxel_query_dev(ctx.get(), &g_, vox_, (const double *)dp, (int64_t)n, dq, anet_stream(ctx.get()));
    if (rc == ANET_OK) rc = anet_dev_download(ctx.get(), res.data(), (const double *)dq, res.size());
    anet_dev_free((double *)dp);
    anet_dev_free((double *)dq);
    ctx.check(rc);
    std::memcpy(out, res.data(), n);
  }

  template <class V3i>
  anet::Vec3 posI2D(const V3i &id) const {
    const double s = scale_, h = 0.5 * s;
    return anet::Vec3((double)id(0) * s + (g_.origin[0] + h), (double)id(1) * s + (g_.origin[1] + h),
                      (double)id(2) * s + (g_.origin[2] + h));
  }
  template <class V3d>
  Vec3i posD2I(const V3d &pos) const {
    return Vec3i((int)((pos(0) - g_.origin[0]) / scale_), (int)((pos(1) - g_.origin[1]) / scale_),
                 (int)((pos(2) - g_.origin[2]) / scale_));
  }

  // The exact distance field (anet_voxel_distance_dev): DEVICE int32 [voxels], the signed squared distance in voxel units, + to the
  // nearest blocked voxel for a free one, - to the nearest free voxel for a blocked one; walls: the outside counts as blocked.
  // Computed on first use after a change of the map, one per value of `walls`.
  const int32_t *distanceField(bool walls = true) const {
    flush();
    const int k = walls ? 1 : 0;
    if (dist_valid_[k]) return (const int32_t *)dist_[k];
    anet::Context &ctx = anet::Context::thread_default();
    if (!dist_[k]) dist_[k] = alloc_bytes(ctx, (size_t)voxNum_ * 4);
    ctx.check(anet_voxel_distance_dev(ctx.get(), &g_, vox_, k, (int32_t *)dist_[k], anet_stream(ctx.get())));
    dist_valid_[k] = true;
    return (const int32_t *)dist_[k];
  }
  // The distance in metres from p to the nearest obstacle, negative inside one: the trilinear interpolant of the field's centre
  // values (anet_voxel_distance_query_dev; constant beyond the outermost voxel centres); grad: its gradient.
  template <class V>
  double getDistance(const V &p, bool walls = true) const {
    double d = 0.0, g[3];
    distance_one(p, walls, d, g);
    return d;
  }
  // (grad: anything with assignable (i) access; a bool lvalue is `walls` of the overload above, never a gradient)
  template <class V, class G, class = typename std::enable_if<!std::is_same<typename std::remove_cv<G>::type, bool>::value>::type>
  double getDistance(const V &p, G &grad, bool walls = true) const {
    double d = 0.0, g[3];
    distance_one(p, walls, d, g);
    for (int c = 0; c < 3; ++c) grad(c) = g[c];
    return d;
  }

  // device side, for convexCover and other kernels: the voxel bytes, the surface's ascending ids and points [n][3]
  const anet_voxel_grid &grid() const { return g_; }
  const uint8_t *voxels_dev() const {
    flush();
    return vox_;
  }
  const int32_t *surf_ids_dev() const { return (const int32_t *)ids_; }
  const double *surf_points_dev() const {  // computed on the device, not downloaded
    ensure_points_dev();
    return (const double *)pts_;
  }
  int64_t surf_size() const { return nsurf_; }
  // flush the buffered single-point fills (one scatter launch for the positions, one for the index triples)
  void flush() const {
    if (pend_.empty() && pend_ids_.empty()) return;
    anet::Context &ctx = anet::Context::thread_default();
    const size_t n = pend_.size() / 3, m = pend_ids_.size() / 3;
    uint8_t *d = alloc_bytes(ctx, n * 24 + m * 12);
    int rc = ANET_OK;
    if (n > 0) {
      rc = anet_dev_upload(ctx.get(), (double *)d, pend_.data(), n * 3);
      if (rc == ANET_OK) rc = anet_voxel_set_occupied_dev(ctx.get(), &g_, vox_, d, (int64_t)n, 24, 1, anet_stream(ctx.get()));
    }
    if (m > 0 && rc == ANET_OK) {
      std::vector<double> buf((m * 12 + 7) / 8);
      std::memcpy(buf.data(), pend_ids_.data(), m * 12);
      rc = anet_dev_upload(ctx.get(), (double *)(d + n * 24), buf.data(), buf.size());
      if (rc == ANET_OK)
        rc = anet_voxel_set_occupied_ids_dev(ctx.get(), &g_, vox_, (const int32_t *)(d + n * 24), (int64_t)m, anet_stream(ctx.get()));
    }
    if (rc == ANET_OK) rc = anet_synchronize(ctx.get());
    anet_dev_free((double *)d);
    ctx.check(rc);
    pend_.clear();
    pend_ids_.clear();
    stale_ = true;
    dist_valid_[0] = dist_valid_[1] = false;
  }

 private:
  anet_voxel_grid g_{};
  double scale_ = 0.0;
  int64_t voxNum_ = 0;
  uint8_t *vox_ = nullptr, *work_ = nullptr, *count_ = nullptr, *ids_ = nullptr;
  mutable uint8_t *pts_ = nullptr, *dist_[2] = {nullptr, nullptr};
  mutable bool dist_valid_[2] = {false, false};
  int64_t ids_cap_ = 0, nsurf_ = 0;
  mutable int64_t pts_cap_ = 0;
  mutable bool pts_dev_valid_ = false, pts_host_valid_ = false, stale_ = false;
  mutable std::vector<double> pend_, pts_host_;
  mutable std::vector<int32_t> pend_ids_;
  mutable std::vector<uint8_t> mirror_;

  static uint8_t *alloc_bytes(anet::Context &ctx, size_t bytes) {
    double *p = nullptr;
    ctx.check(anet_dev_alloc(ctx.get(), (bytes + 7) / 8, &p));
    return (uint8_t *)p;
  }
  void swap(VoxelMap &o) noexcept {
    std::swap(g_, o.g_); std::swap(scale_, o.scale_); std::swap(voxNum_, o.voxNum_);
    std::swap(vox_, o.vox_); std::swap(work_, o.work_); std::swap(count_, o.count_); std::swap(ids_, o.ids_);
    std::swap(pts_, o.pts_); std::swap(ids_cap_, o.ids_cap_); std::swap(nsurf_, o.nsurf_); std::swap(pts_cap_, o.pts_cap_);
    std::swap(pts_dev_valid_, o.pts_dev_valid_); std::swap(pts_host_valid_, o.pts_host_valid_); std::swap(stale_, o.stale_);
    pend_.swap(o.pend_); pend_ids_.swap(o.pend_ids_); pts_host_.swap(o.pts_host_);
    mirror_.swap(o.mirror_);
    for (int k = 0; k < 2; ++k) {
      std::swap(dist_[k], o.dist_[k]);
      std::swap(dist_valid_[k], o.dist_valid_[k]);
    }
  }
  template <class V>
  void set_one(const V &pos, std::false_type) {
    if (!(std::isfinite((double)pos(0)) && std::isfinite((double)pos(1)) && std::isfinite((double)pos(2)))) return;
    pend_.push_back(pos(0)); pend_.push_back(pos(1)); pend_.push_back(pos(2));
  }
  template <class V>
  void set_one(const V &id, std::true_type) {  // the index itself; the kernel drops it when it is out of bounds
    pend_ids_.push_back((int32_t)id(0)); pend_ids_.push_back((int32_t)id(1)); pend_ids_.push_back((int32_t)id(2));
  }
  template <class V>
  void distance_one(const V &p, bool walls, double &d, double (&g)[3]) const {
    const int32_t *sd2 = distanceField(walls);
    anet::Context &ctx = anet::Context::thread_default();
    double *buf = nullptr;  // pos [3], dist [1], grad [3]
    ctx.check(anet_dev_alloc(ctx.get(), 7, &buf));
    double h[7] = {(double)p(0), (double)p(1), (double)p(2), 0.0, 0.0, 0.0, 0.0};
    int rc = anet_dev_upload(ctx.get(), buf, h, 3);
    if (rc == ANET_OK) rc = anet_voxel_distance_query_dev(ctx.get(), &g_, sd2, buf, 1, buf + 3, buf + 4, anet_stream(ctx.get()));
    if (rc == ANET_OK) rc = anet_dev_download(ctx.get(), h, buf, 7);
    anet_dev_free(buf);
    ctx.check(rc);
    d = h[3];
    for (int c = 0; c < 3; ++c) g[c] = h[4 + c];
  }
  void refresh() const {
    flush();
    if (!stale_) return;
    anet::Context &ctx = anet::Context::thread_default();
    std::vector<double> buf((size_t)((voxNum_ + 7) / 8));
    ctx.check(anet_dev_download(ctx.get(), buf.data(), (const double *)vox_, buf.size()));
    std::memcpy(mirror_.data(), buf.data(), (size_t)voxNum_);
    stale_ = false;
  }
  template <class V>
  bool query_one(const V &pos, std::false_type) const {
    refresh();
    int64_t i = 0, mul = 1;
    for (int c = 0; c < 3; ++c) {
      const double q = (pos(c) - g_.origin[c]) / scale_;  // trunc(q) in [0, size) <=> -1 < q < size
      if (!(q > -1.0 && q < (double)g_.size[c])) return true;
      i += (int64_t)(int)q * mul;
      mul *= g_.size[c];
    }
    return mirror_[(size_t)i] != 0;
  }
  template <class V>
  bool query_one(const V &id, std::true_type) const {
    refresh();
    for (int c = 0; c < 3; ++c)
      if (id(c) < 0 || id(c) >= g_.size[c]) return true;
    return mirror_[(size_t)(id(0) + (int64_t)g_.size[0] * (id(1) + (int64_t)g_.size[1] * id(2)))] != 0;
  }
  std::vector<int32_t> surf_ids() const {
    std::vector<double> buf((size_t)((nsurf_ + 1) / 2));
    std::vector<int32_t> ids((size_t)nsurf_);
    if (nsurf_ == 0) return ids;
    anet::Context &ctx = anet::Context::thread_default();
    ctx.check(anet_dev_download(ctx.get(), buf.data(), (const double *)ids_, buf.size()));
    std::memcpy(ids.data(), buf.data(), (size_t)nsurf_ * 4);
    return ids;
  }
  void ensure_points_dev() const {  // the surface points [n][3] on the device, once per dilate
    if (pts_dev_valid_) return;
    anet::Context &ctx = anet::Context::thread_default();
    if (nsurf_ > pts_cap_) {
      anet_dev_free((double *)pts_);
      pts_ = nullptr;
      pts_cap_ = 0;
      pts_ = alloc_bytes(ctx, (size_t)nsurf_ * 24);
      pts_cap_ = nsurf_;
    }
    if (nsurf_ > 0)
      ctx.check(anet_voxel_surf_points_dev(ctx.get(), &g_, (const int32_t *)ids_, nsurf_, (double *)pts_, anet_stream(ctx.get())));
    pts_dev_valid_ = true;
  }
  const std::vector<double> &surf_points() const {  // their host copy, downloaded on first use after a dilate
    if (pts_host_valid_) return pts_host_;
    ensure_points_dev();
    pts_host_.assign((size_t)nsurf_ * 3, 0.0);
    if (nsurf_ > 0) {
      anet::Context &ctx = anet::Context::thread_default();
      ctx.check(anet_dev_download(ctx.get(), pts_host_.data(), (const double *)pts_, pts_host_.size()));
    }
    pts_host_valid_ = true;
    return pts_host_;
  }
};

}  // namespace voxel_map
