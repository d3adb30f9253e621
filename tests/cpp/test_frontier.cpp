// Exploration goals through the C++ header: the frontier of a saved log-odds grid, its clusters, the reachable components of the
// hand-over's free voxels and the view gain of a few poses.  Reads logodds.bin (int16), views.bin (R [V][9] then t [V][3]) and
// pts.bin ([n][3]) under argv[1] and prints the counts; the test compares them with the Python path's.
//   test_frontier <dir>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include <stdint.h>
#include "allocnet_amd/occupancy_map.hpp"
#include "allocnet_amd/voxel_map.hpp"

struct V3 {
  double v[3];
  V3(double x, double y, double z) : v{x, y, z} {}
  double operator()(int i) const { return v[i]; }
};
struct V3i {
  int v[3];
  V3i(int x, int y, int z) : v{x, y, z} {}
  int operator()(int i) const { return v[i]; }
};

template <class T>
static std::vector<T> slurp(const std::string &path) {
  std::vector<T> out;
  FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) return out;
  T buf[1024];
  size_t k;
  while ((k = std::fread(buf, sizeof(T), 1024, f)) > 0) out.insert(out.end(), buf, buf + k);
  std::fclose(f);
  return out;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: test_frontier <dir>\n");
    return 2;
  }
  const std::string dir = argv[1];
  try {
    anet_occupancy_params prm = voxel_map::occupancyParams();
    prm.hit = 847; prm.miss = -405; prm.lo = -1100; prm.hi = 2000;
    prm.min_range = 0.2; prm.max_range = 3.0;
    voxel_map::OccupancyMap om(V3i(24, 20, 12), V3(-1.3, 0.7, -0.25), 0.25, prm);
    om.setLogOdds(slurp<int16_t>(dir + "/logodds.bin"));
    int64_t count = -1;
    const std::vector<uint8_t> mask = om.frontier(0, &count);
    int64_t ones = 0;
    for (uint8_t b : mask) ones += b;
    if (ones != count) {
      std::printf("FAIL the count %lld is not the number of ones %lld\n", (long long)count, (long long)ones);
      return 1;
    }
    const std::vector<voxel_map::FrontierCluster> cl = om.frontierClusters(0, 4, 26);
    int largest = 0;
    for (const voxel_map::FrontierCluster &c : cl) largest = c.count > largest ? c.count : largest;
    voxel_map::VoxelMap vm(V3i(24, 20, 12), V3(-1.3, 0.7, -0.25), 0.25);
    om.toVoxelMap(vm, 0, true);
    const std::vector<int32_t> labels = voxel_map::components(vm, 6);
    std::set<int32_t> roots;
    for (int32_t l : labels)
      if (l >= 0) roots.insert(l);
    const std::vector<double> views = slurp<double>(dir + "/views.bin"), pts = slurp<double>(dir + "/pts.bin");
    const size_t V = views.size() / 12;
    const std::vector<double> R(views.begin(), views.begin() + V * 9), t(views.begin() + V * 9, views.end());
    const std::vector<int32_t> gain = om.viewGain(R, t, pts, 0);
    std::printf("frontier=%lld clusters=%zu largest=%d free_components=%zu gain=", (long long)count, cl.size(), largest, roots.size());
    for (size_t i = 0; i < gain.size(); ++i) std::printf("%s%d", i ? "," : "", (int)gain[i]);
    std::printf("\nOK\n");
  } catch (const std::exception &e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
  return 0;
}
