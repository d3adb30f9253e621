// MincoYaw<2>, YawTrajectory, getYawMargin and checkYaw of include/allocnet_amd/yaw.hpp.
//     test_yaw CASE.txt margin t piece energy yaw_at_tq rate_at_tq
// The file holds, as text: half_fov, max_rate, v_min, res, the query time tq; the piece count N; per piece its duration and 18
// coefficients (3 x 6, row-major, highest power first); the yaw's head (psi, dpsi), tail (psi, dpsi) and N - 1 interior headings.
// The six numbers after it are what the numpy restatement (tests/yaw_np.py) gives for the same case; each is compared within 1e-9,
// scaled by max(1, |expected|).  Printed: one JSON object, numbers with %.17g.  Exit status 3: a number differs.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "allocnet_amd/yaw.hpp"

struct Vec {
  std::vector<double> v;
  double operator()(int i) const { return v[(size_t)i]; }
};

static bool close_to(double got, double want) { return std::fabs(got - want) <= 1e-9 * std::fmax(1.0, std::fabs(want)); }

int main(int argc, char **argv) {
  if (argc != 8) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  double half_fov = 0.0, max_rate = 0.0, v_min = 0.0, tq = 0.0;
  int res = 0, N = 0;
  if (fscanf(f, "%lf %lf %lf %d %lf %d", &half_fov, &max_rate, &v_min, &res, &tq, &N) != 6 || N < 1) return 2;
  try {
    Trajectory<5> traj;
    Vec durs;
    for (int i = 0; i < N; ++i) {
      double T = 0.0;
      anet::Matrix<3, 6> cm;
      if (fscanf(f, "%lf", &T) != 1) return 2;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 6; ++c)
          if (fscanf(f, "%lf", &cm(r, c)) != 1) return 2;
      traj.emplace_back(T, cm);
      durs.v.push_back(T);
    }
    Vec head, tail, wps;
    head.v.resize(2);
    tail.v.resize(2);
    wps.v.resize((size_t)(N - 1));
    if (fscanf(f, "%lf %lf %lf %lf", &head.v[0], &head.v[1], &tail.v[0], &tail.v[1]) != 4) return 2;
    for (int k = 0; k + 1 < N; ++k)
      if (fscanf(f, "%lf", &wps.v[(size_t)k]) != 1) return 2;
    fclose(f);
    minco::MincoYaw<2> my;
    my.setConditions(head, tail, N);
    my.setParameters(wps, durs);
    YawTrajectory yaw;
    my.getTrajectory(yaw);
    double t = 0.0;
    int piece = 0;
    const double margin = getYawMargin(traj, yaw, half_fov, v_min, res, &t, &piece);
    const double psi = yaw.getYaw(tq), dpsi = yaw.getYawRate(tq);
    // a field of view that the trajectory surely keeps, and one it surely does not; a rate limit it surely breaks
    const bool ok = checkYaw(traj, yaw, half_fov, max_rate, v_min, res);
    const bool ok_loose = half_fov - margin + 1e-3 <= 1.5707963267948966 && checkYaw(traj, yaw, half_fov - margin + 1e-3, INFINITY, v_min, res);
    const bool ok_tight = checkYaw(traj, yaw, half_fov - margin - 1e-3, INFINITY, v_min, res);
    const bool ok_slow = checkYaw(traj, yaw, 1.5707963267948966, 1e-6, 0.0, res);
    printf("{\"margin\": %.17g, \"t\": %.17g, \"piece\": %d, \"energy\": %.17g, \"yaw\": %.17g, \"rate\": %.17g, \"ok\": %d, "
           "\"ok_loose\": %d, \"ok_tight\": %d, \"ok_slow\": %d, \"total\": %.17g}\n",
           margin, t, piece, my.getEnergy(), psi, dpsi, (int)ok, (int)ok_loose, (int)ok_tight, (int)ok_slow, yaw.getTotalDuration());
    const bool same = close_to(margin, atof(argv[2])) && close_to(t, atof(argv[3])) && piece == atoi(argv[4]) &&
                      close_to(my.getEnergy(), atof(argv[5])) && close_to(psi, atof(argv[6])) && close_to(dpsi, atof(argv[7]));
    return same ? 0 : 3;
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
