// LearningPlanner (include/allocnet_amd/learning_planner.hpp) through the C ABI: loadModel from the flat weights file, then
// callModel on a corridor read from a text file, the way the planner node calls it after plan() has built the corridor.
// Prints one JSON object; tests/test_timenet_gpu.py checks it against the Python facade on the same weights and corridor.
//   test_learning_planner <weights file> <case file> [plan]
// case file: seg, then iniPVA (9 numbers, row = axis, columns p v a), finPVA (9), then per polytope m and m rows a b c d
// (planner form).  With a third argument the program also runs plan() on a 10 x 10 x 5 m map with one obstacle in a corner and
// reports what it returned (the test does not pass it: plan<Map> is instantiated, so compile-checked, by this file).
// `V3` / `Mat3` stand in for Eigen::Vector3d / Eigen::MatrixXd (duck typing only).
#include <cstdio>
#include <string>
#include <vector>

#include "allocnet_amd/learning_planner.hpp"

struct V3 {
  double v[3] = {0.0, 0.0, 0.0};
  V3() = default;
  V3(double x, double y, double z) : v{x, y, z} {}
  double &operator()(int i) { return v[i]; }
  double operator()(int i) const { return v[i]; }
};
struct V3i {
  int v[3] = {0, 0, 0};
  V3i(int x, int y, int z) : v{x, y, z} {}
  int operator()(int i) const { return v[i]; }
};
struct Mat3 {
  double a[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double &operator()(int r, int c) { return a[r * 3 + c]; }
  double operator()(int r, int c) const { return a[r * 3 + c]; }
};

int main(int argc, char **argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: test_learning_planner <weights file> <case file> [plan]\n");
    return 2;
  }
  try {
    FILE *f = std::fopen(argv[2], "r");
    if (!f) return 2;
    int seg = 0;
    Mat3 ini, fin;
    bool ok = std::fscanf(f, "%d", &seg) == 1 && seg >= 1 && seg <= 10;
    for (int i = 0; ok && i < 9; ++i) ok = std::fscanf(f, "%lf", &ini.a[i]) == 1;
    for (int i = 0; ok && i < 9; ++i) ok = std::fscanf(f, "%lf", &fin.a[i]) == 1;
    std::vector<LearningPlanner::HPoly> polys((size_t)(ok ? seg : 0));
    for (int i = 0; ok && i < seg; ++i) {
      int m = 0;
      ok = std::fscanf(f, "%d", &m) == 1 && m >= 1 && m <= 1000;
      if (ok) polys[i].resize(m, 4);
      for (int r = 0; ok && r < m; ++r)
        for (int c = 0; ok && c < 4; ++c) ok = std::fscanf(f, "%lf", &polys[i](r, c)) == 1;
    }
    std::fclose(f);
    if (!ok) {
      std::fprintf(stderr, "malformed case file\n");
      return 2;
    }
    LearningPlanner planner(LearningPlannerConfig(5, 4, QPConfig(4.0, 6.0, 20)));
    if (planner.loadModel(std::string(argv[1]) + ".missing")) return 3;  // a missing file is reported, not thrown
    if (!planner.loadModel(argv[1])) return 4;
    planner.setCorridor(polys);
    const bool solved = planner.callModel(ini, fin);
    std::printf("{\"ok\": %s, \"times\": [", solved ? "true" : "false");
    const std::vector<float> &times = planner.getTimes();
    for (size_t i = 0; i < times.size(); ++i) std::printf("%.9g%s", (double)times[i], i + 1 < times.size() ? ", " : "");
    std::printf("], \"coeffs\": [");
    if (solved) {
      Trajectory<7> traj;
      planner.getTraj(traj);
      for (int i = 0; i < traj.getPieceNum(); ++i)
        for (int j = 0; j < 3; ++j)
          for (int k = 0; k < 8; ++k)
            std::printf("%.17g%s", traj[i].getCoeffMat()(j, k), (i + 1 == traj.getPieceNum() && j == 2 && k == 7) ? "" : ", ");
    }
    std::printf("]");
    if (argc > 3) {
      voxel_map::VoxelMap vm(V3i(40, 40, 20), V3(-5.0, -5.0, 0.0), 0.25);
      vm.setOccupied(V3i(2, 37, 2));
      vm.dilate(1);
      std::vector<V3> route;
      Mat3 a = ini, b = fin;
      for (int c = 0; c < 3; ++c) {
        a(c, 0) = c == 2 ? 1.0 : -3.0;
        b(c, 0) = c == 2 ? 2.0 : 3.0;
      }
      const bool planned = planner.plan(a, b, route, vm);
      std::vector<LearningPlanner::HPoly> vis;
      planner.gethPolys(vis);
      std::printf(", \"plan\": {\"ok\": %s, \"route\": %zu, \"polys\": %zu, \"end\": [%.17g, %.17g, %.17g]", planned ? "true" : "false",
                  route.size(), vis.size(), b(0, 0), b(1, 0), b(2, 0));
      if (planned) {
        Trajectory<7> traj;
        planner.getTraj(traj);
        const double T = traj.getTotalDuration();
        const V3 p0 = traj.getPos(0.0), p1 = traj.getPos(T);
        std::printf(", \"p0\": [%.17g, %.17g, %.17g], \"p1\": [%.17g, %.17g, %.17g]", p0(0), p0(1), p0(2), p1(0), p1(1), p1(2));
      }
      std::printf("}");
    }
    std::printf("}\n");
  } catch (const anet::Error &e) {
    std::fprintf(stderr, "allocnet_amd error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
