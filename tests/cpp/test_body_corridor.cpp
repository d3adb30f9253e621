// getBodyMargin / checkBodyCorridor (include/allocnet_amd/trajectory_map.hpp) through the C ABI: a plate on SURVEY config 1's
// 8-segment min-snap trajectory against one box per piece (every other piece with a tilted seventh row).  Prints one JSON object
// with the polytopes it used; tests/test_body_corridor_gpu.py feeds them to the Python facade and compares bit for bit.
#include <cstdio>
#include <vector>

#include "allocnet_amd/flatness.hpp"
#include "allocnet_amd/minco.hpp"
#include "allocnet_amd/trajectory.hpp"
#include "allocnet_amd/trajectory_map.hpp"

struct Mat {
  int R, C;
  std::vector<double> a;
  Mat(int r = 3, int c = 8) : R(r), C(c), a((size_t)r * c, 0.0) {}
  double &operator()(int r, int c) { return a[(size_t)r * C + c]; }
  double operator()(int r, int c) const { return a[(size_t)r * C + c]; }
  int rows() const { return R; }
};
struct Vec {
  std::vector<double> a;
  explicit Vec(int n) : a(n, 0.0) {}
  double &operator()(int i) { return a[i]; }
  double operator()(int i) const { return a[i]; }
};

int main() {
  try {
    const int N = 8;
    Mat head(3, 3), tail(3, 3), inPs(3, N - 1);
    Vec ts(N);
    const double goal[3] = {8.0, 3.0, 1.0};
    for (int a = 0; a < 3; ++a) tail(a, 0) = goal[a];
    for (int k = 0; k < N - 1; ++k)
      for (int a = 0; a < 3; ++a) inPs(a, k) = goal[a] * (k + 1) / (double)N;
    for (int i = 0; i < N; ++i) ts(i) = 1.0;
    minco::MINCO_S4NU opt;
    opt.setConditions(head, tail, N, 3);
    opt.setParameters(inPs, ts);
    Trajectory<7> traj;
    opt.getTrajectory(traj);

    flatness::FlatnessMap fm;
    fm.reset(1.0, 9.8, 0.7, 0.8, 0.01, 1e-4);
    std::vector<anet::Vec3> verts;
    for (int sx = -1; sx <= 1; sx += 2)
      for (int sy = -1; sy <= 1; sy += 2)
        for (int sz = -1; sz <= 1; sz += 2) verts.push_back(anet::Vec3(0.25 * sx, 0.25 * sy, 0.05 * sz));
    const double hw[3] = {0.6, 0.3, 0.2};
    std::vector<Mat> hPolys;
    for (int i = 0; i < N; ++i) {
      Mat h(i % 2 ? 7 : 6, 4);
      double c[3];
      for (int a = 0; a < 3; ++a) c[a] = goal[a] * (i + 0.5) / (double)N;
      for (int a = 0; a < 3; ++a) {
        h(2 * a, a) = 1.0;      h(2 * a, 3) = hw[a] + c[a];
        h(2 * a + 1, a) = -1.0; h(2 * a + 1, 3) = hw[a] - c[a];
      }
      if (i % 2) {
        h(6, 1) = 0.6; h(6, 2) = 0.8;
        h(6, 3) = 0.6 * c[1] + 0.8 * c[2] + 0.15;
      }
      hPolys.push_back(h);
    }
    std::vector<double> per((size_t)N);
    const double m = getBodyMargin(traj, fm, verts, hPolys, 20, per.data());
    const bool ok_tight = checkBodyCorridor(traj, fm, verts, hPolys, 20), ok_loose = checkBodyCorridor(traj, fm, verts, hPolys, 20, m);
    printf("{\"margin\": %.17g, \"check\": [%d, %d], \"per_piece\": [", m, ok_tight ? 1 : 0, ok_loose ? 1 : 0);
    for (int i = 0; i < N; ++i) printf("%.17g%s", per[(size_t)i], i == N - 1 ? "" : ", ");
    printf("],\n \"hpolys\": [");
    for (int i = 0; i < N; ++i) {
      printf("[");
      for (int r = 0; r < hPolys[(size_t)i].rows(); ++r)
        printf("[%.17g, %.17g, %.17g, %.17g]%s", hPolys[(size_t)i](r, 0), hPolys[(size_t)i](r, 1), hPolys[(size_t)i](r, 2),
               hPolys[(size_t)i](r, 3), r == hPolys[(size_t)i].rows() - 1 ? "" : ", ");
      printf("]%s", i == N - 1 ? "" : ",\n  ");
    }
    printf("]}\n");
  } catch (const anet::Error &e) {
    fprintf(stderr, "allocnet_amd error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
