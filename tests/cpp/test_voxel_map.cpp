// voxel_map::VoxelMap through the C++ header, the way the ROS node drives it: a PointCloud2-shaped float buffer filled
// one point at a time (mapCallBack), dilate, query, getSurf, getSurfInBox, and convexCover with the map against the points
// overload with map.getSurf().  Writes what it saw under argv[1] (the test compares it with the numpy restatement) and
// prints "OK" when the two convexCover overloads agree bit for bit.
//   test_voxel_map <out_dir>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <stdint.h>
#include "allocnet_amd/sfc_gen_map.hpp"
#include "allocnet_amd/voxel_map.hpp"

struct V3 {  // Eigen::Vector3d-like
  double v[3] = {0.0, 0.0, 0.0};
  V3() = default;
  V3(double x, double y, double z) : v{x, y, z} {}
  double operator()(int i) const { return v[i]; }
  double &operator()(int i) { return v[i]; }
};
struct V3i {  // Eigen::Vector3i-like
  int v[3] = {0, 0, 0};
  V3i() = default;
  V3i(int x, int y, int z) : v{x, y, z} {}
  int operator()(int i) const { return v[i]; }
};
struct DynMat {  // Eigen::MatrixX4d-like
  int R = 0, C = 0;
  std::vector<double> a;
  void resize(long r, long c) { R = (int)r; C = (int)c; a.assign((size_t)r * c, 0.0); }
  double &operator()(int r, int c) { return a[(size_t)r * C + c]; }
  double operator()(int r, int c) const { return a[(size_t)r * C + c]; }
  int rows() const { return R; }
};

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

static bool dump(const std::string &path, const void *p, size_t bytes) {
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
  return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: test_voxel_map <out_dir>\n");
    return 2;
  }
  const std::string out = argv[1];
  try {
    // 60 x 50 x 12 voxels of 0.1 m from (-3, -2.5, 0); PointCloud2 records of 16 bytes (x y z intensity)
    voxel_map::VoxelMap vm(V3i(60, 50, 12), V3(-3.0, -2.5, 0.0), 0.1);
    const size_t n = 4000, step = 16;
    std::vector<float> cloud(n * step / sizeof(float), 0.0f);
    uint32_t s = 7u;
    for (size_t i = 0; i < n; ++i) {
      float *r = &cloud[i * step / sizeof(float)];
      const bool pillar = i % 2 == 0;  // half on two pillars, half scattered, some outside the map, a few NaN
      r[0] = pillar ? (i % 4 == 0 ? 1.0f : -1.2f) + 0.15f * std::cos(6.2831853f * unit(s)) : -3.5f + 7.0f * unit(s);
      r[1] = pillar ? 0.3f + 0.15f * std::sin(6.2831853f * unit(s)) : -3.0f + 6.0f * unit(s);
      r[2] = -0.1f + 1.4f * unit(s);
      r[3] = 1.0f;
      if (i % 97 == 5) r[1] = std::nanf("");
    }
    // mapCallBack: one setOccupied per finite record
    for (size_t i = 0; i < n; ++i) {
      const float *r = &cloud[i * step / sizeof(float)];
      if (std::isnan(r[0]) || std::isnan(r[1]) || std::isnan(r[2]) || std::isinf(r[0]) || std::isinf(r[1]) || std::isinf(r[2]))
        continue;
      vm.setOccupied(V3(r[0], r[1], r[2]));
    }
    // setOccupied(Eigen::Vector3i): the index itself, out-of-bounds ones dropped (test_voxel_map_gpu.py CPP_INDEX_FILLS)
    const int idfill[6][3] = {{0, 0, 0}, {59, 49, 11}, {60, 0, 0}, {-1, 3, 3}, {10, 50, 2}, {30, 20, 11}};
    for (const auto &id : idfill) vm.setOccupied(V3i(id[0], id[1], id[2]));
    vm.dilate(2);
    const std::vector<uint8_t> &vox = vm.getVoxels();
    std::vector<V3> surf;
    vm.getSurf(surf);
    std::vector<double> sflat;
    for (const V3 &p : surf) sflat.insert(sflat.end(), p.v, p.v + 3);
    std::vector<V3> inbox;
    vm.getSurfInBox(V3i(40, 28, 3), 4, inbox);
    std::vector<double> bflat;
    for (const V3 &p : inbox) bflat.insert(bflat.end(), p.v, p.v + 3);
    // single queries from the host mirror and the batched device query, on a lattice reaching outside the map
    std::vector<double> qpos;
    for (int i = 0; i < 500; ++i) {
      qpos.push_back(-3.3 + 6.6 * unit(s)); qpos.push_back(-2.8 + 5.6 * unit(s)); qpos.push_back(-0.2 + 1.6 * unit(s));
    }
    std::vector<uint8_t> q1(500), q2(500);
    for (int i = 0; i < 500; ++i) q1[i] = vm.query(V3(qpos[i * 3], qpos[i * 3 + 1], qpos[i * 3 + 2])) ? 1 : 0;
    vm.query(qpos.data(), 500, q2.data());
    if (q1 != q2) {
      std::printf("FAIL single and batched query differ\n");
      return 1;
    }
    if (!(dump(out + "/cloud.bin", cloud.data(), cloud.size() * 4) && dump(out + "/voxels.bin", vox.data(), vox.size()) &&
          dump(out + "/surf.bin", sflat.data(), sflat.size() * 8) && dump(out + "/inbox.bin", bflat.data(), bflat.size() * 8) &&
          dump(out + "/qpos.bin", qpos.data(), qpos.size() * 8) && dump(out + "/query.bin", q1.data(), q1.size()))) {
      std::printf("FAIL writing under %s\n", out.c_str());
      return 1;
    }
    // convexCover: the map overload against the points overload on getSurf's points
    std::vector<V3> route = {V3(-2.5, -2.0, 0.6), V3(-0.1, -1.2, 0.6), V3(0.2, 1.5, 0.6), V3(2.5, 2.0, 0.6)};
    const V3 lo = vm.getOrigin(), hi = vm.getCorner();
    std::vector<DynMat> hm, hp;
    sfc_gen::convexCover(route, vm, lo, hi, 1.0, 0.8, hm);
    sfc_gen::convexCover(route, surf, lo, hi, 1.0, 0.8, hp);
    if (hm.size() != hp.size() || hm.empty()) {
      std::printf("FAIL convexCover: %zu polytopes from the map, %zu from the points\n", hm.size(), hp.size());
      return 1;
    }
    for (size_t i = 0; i < hm.size(); ++i)
      if (hm[i].rows() != hp[i].rows() || std::memcmp(hm[i].a.data(), hp[i].a.data(), hm[i].a.size() * 8) != 0) {
        std::printf("FAIL convexCover polytope %zu differs\n", i);
        return 1;
      }
    std::printf("surface %zu points, %zu in the box, %zu polytopes\nOK\n", surf.size(), inbox.size(), hm.size());
  } catch (const std::exception &e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
  return 0;
}
