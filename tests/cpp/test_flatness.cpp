// flatness::FlatnessMap (include/allocnet_amd/flatness.hpp) through the C ABI, the way the reference's process() loop uses it
// (learning_planning.cpp:236-251): velocity, acceleration and jerk of a solved trajectory pushed through forward, then backward
// with fixed upstream gradients.  Prints one JSON object; tests/test_flatness_gpu.py checks it against the Python facade.
// `V3` / `V4` stand in for Eigen::Vector3d / Eigen::Vector4d (duck typing only).
#include <cstdio>
#include <vector>

#include "allocnet_amd/flatness.hpp"
#include "allocnet_amd/minco.hpp"
#include "allocnet_amd/trajectory.hpp"

struct Mat {
  int R, C;
  std::vector<double> a;
  Mat(int r = 3, int c = 8) : R(r), C(c), a((size_t)r * c, 0.0) {}
  double &operator()(int r, int c) { return a[(size_t)r * C + c]; }
  double operator()(int r, int c) const { return a[(size_t)r * C + c]; }
};
struct Vec {
  std::vector<double> a;
  explicit Vec(int n) : a(n, 0.0) {}
  double &operator()(int i) { return a[i]; }
  double operator()(int i) const { return a[i]; }
};
struct V3 {
  double v[3] = {0.0, 0.0, 0.0};
  V3() = default;
  V3(double x, double y, double z) : v{x, y, z} {}
  double &operator()(int i) { return v[i]; }
  double operator()(int i) const { return v[i]; }
};
struct V4 {
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  double &operator()(int i) { return v[i]; }
  double operator()(int i) const { return v[i]; }
};

template <class V>
static void print_row(const V &x, int n, bool last = false) {
  for (int k = 0; k < n; ++k) printf("%.17g%s", x(k), (last && k == n - 1) ? "" : ", ");
}

int main() {
  try {
    // one 8-segment min-snap trajectory, fixed waypoints on the chord, T_i = 1
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
    const double times[5] = {0.0, 0.4, 3.5, 6.75, 8.0};
    // one row per time: t, psi, dpsi | vel acc jer | thr quat omg | pos_total vel_total acc_total jer_total psi_total dpsi_total
    printf("{\"rows\": [\n");
    for (int q = 0; q < 5; ++q) {
      const double t = times[q], psi = 0.3 * q - 0.5, dpsi = 0.1 * q;
      const V3 vel = traj.getVel(t), acc = traj.getAcc(t), jer = traj.getJer(t);
      double thr = 0.0, psi_t = 0.0, dpsi_t = 0.0;
      V4 quat, qg;
      V3 omg, pt, vt, at, jt;
      fm.forward(vel, acc, jer, psi, dpsi, thr, quat, omg);
      const V3 pg(0.25, -0.5, 0.75), vg(-1.0, 0.5, 0.125), og(0.3, -0.7, 1.1);
      qg(0) = 0.5; qg(1) = -1.5; qg(2) = 0.75; qg(3) = 2.0;
      fm.backward(pg, vg, 1.25, qg, og, pt, vt, at, jt, psi_t, dpsi_t);
      printf("[%.17g, %.17g, %.17g, ", t, psi, dpsi);
      print_row(vel, 3); print_row(acc, 3); print_row(jer, 3);
      printf("%.17g, ", thr);
      print_row(quat, 4); print_row(omg, 3);
      print_row(pt, 3); print_row(vt, 3); print_row(at, 3); print_row(jt, 3);
      printf("%.17g, %.17g]%s\n", psi_t, dpsi_t, q == 4 ? "" : ",");
    }
    printf("]}\n");
  } catch (const anet::Error &e) {
    fprintf(stderr, "allocnet_amd error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
