// sfc_gen::planPath through the C++ headers, the way LearningPlanner::plan calls it when the route is empty: a map filled
// with walls one index at a time, dilate(1), a plan from s to g over [getOrigin(), getCorner()], and a start inside a wall.
// Writes the voxels and the path under argv[1] (the test plans the same map from Python and compares bit for bit) and
// prints "OK" when the invalid start returned INFINITY and left the route as it was.
//   test_voxel_path <out_dir>
#include <cmath>
#include <cstdio>
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

static bool dump(const std::string &path, const void *p, size_t bytes) {
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
  return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: test_voxel_path <out_dir>\n");
    return 2;
  }
  const std::string out = argv[1];
  try {
    // 60 x 50 x 12 voxels of 0.1 m from (-3, -2.5, 0): three walls across y with gaps at alternating ends
    voxel_map::VoxelMap vm(V3i(60, 50, 12), V3(-3.0, -2.5, 0.0), 0.1);
    for (int w = 0; w < 3; ++w) {
      const int x = 15 + 15 * w, gap0 = w % 2 == 0 ? 40 : 0;
      for (int y = 0; y < 50; ++y)
        for (int z = 0; z < 12; ++z)
          if (y < gap0 || y >= gap0 + 10) vm.setOccupied(V3i(x, y, z));
    }
    vm.dilate(1);
    const V3 s(-2.73, -2.21, 0.55), g(2.61, 2.07, 0.43);
    std::vector<V3> route;
    const double cost = sfc_gen::planPath(s, g, vm.getOrigin(), vm.getCorner(), &vm, 0.01, route);
    std::vector<double> flat;
    for (const V3 &p : route) flat.insert(flat.end(), p.v, p.v + 3);
    flat.push_back(cost);
    const std::vector<uint8_t> &vox = vm.getVoxels();
    if (!dump(out + "/voxels.bin", vox.data(), vox.size()) || !dump(out + "/path.bin", flat.data(), flat.size() * 8)) {
      std::printf("FAIL writing under %s\n", out.c_str());
      return 1;
    }
    if (route.size() < 3 || !(cost > 0.0)) {
      std::printf("FAIL route of %zu points, cost %g\n", route.size(), cost);
      return 1;
    }
    // a start inside a wall: INFINITY, and p keeps what it held
    std::vector<V3> kept = route;
    const double bad = sfc_gen::planPath<V3>(V3(-1.45, -2.0, 0.5), g, vm.getOrigin(), vm.getCorner(), &vm, 0.01, kept);
    if (!std::isinf(bad) || kept.size() != route.size()) {
      std::printf("FAIL invalid start: cost %g, %zu points\n", bad, kept.size());
      return 1;
    }
    for (size_t i = 0; i < route.size(); ++i)
      for (int c = 0; c < 3; ++c)
        if (kept[i](c) != route[i](c)) {
          std::printf("FAIL invalid start changed the route\n");
          return 1;
        }
  } catch (const std::exception &e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
