// distanceField / getDistance of include/allocnet_amd/voxel_map.hpp.
//     test_voxel_distance
// A 6 x 5 x 4 map at scale 0.5 with one blocked voxel: prints the field's value at three voxels and the distance and gradient at
// a point, as one JSON object, numbers with %.17g.
#include <cstdio>
#include <cstring>
#include <vector>

#include "allocnet_amd/voxel_map.hpp"

struct V3 {
  double v[3];
  double operator()(int i) const { return v[i]; }
  double &operator()(int i) { return v[i]; }
};

int main() {
  try {
    const voxel_map::Vec3i size(6, 5, 4);
    const V3 origin{{-1.0, 0.0, 0.25}};
    voxel_map::VoxelMap map(size, origin, 0.5);
    map.setOccupied(voxel_map::Vec3i(2, 2, 1));
    const int n = 6 * 5 * 4;
    anet::Context &ctx = anet::Context::thread_default();
    std::vector<double> buf((size_t)(n + 1) / 2);
    std::vector<int32_t> sd2((size_t)n);
    printf("{");
    for (int walls = 0; walls < 2; ++walls) {
      ctx.check(anet_dev_download(ctx.get(), buf.data(), (const double *)map.distanceField(walls != 0), buf.size()));
      std::memcpy(sd2.data(), buf.data(), (size_t)n * 4);
      printf("\"sd2_%d\": [%d, %d, %d], ", walls, sd2[0], sd2[2 + 6 * (2 + 5 * 1)], sd2[(size_t)n - 1]);
    }
    const V3 p{{0.1, 1.3, 0.9}};
    V3 g{{0.0, 0.0, 0.0}};
    const bool no_walls = false;  // a bool lvalue is `walls`, not a gradient
    const double d = map.getDistance(p, g), d0 = map.getDistance(p, no_walls);
    printf("\"dist\": %.17g, \"dist_no_walls\": %.17g, \"grad\": [%.17g, %.17g, %.17g]}\n", d, d0, g(0), g(1), g(2));
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
