// getStopMargin / checkStoppable of include/allocnet_amd/trajectory_map.hpp.
//     test_stop_margin CASE.txt
// The file holds, as text: the grid (three sizes, three origin coordinates, the scale); a count m and m voxel index triples to
// set; a_brake, t_react, clearance, res; the piece count N; per piece its duration and 18 coefficients (3 x 6, row-major, highest
// power first).  Printed: one JSON object, numbers with %.17g.  tests/test_stop_penalty_gpu.py compares it with the Python facade.
#include <cstdio>
#include <vector>

#include "allocnet_amd/trajectory_map.hpp"

struct V3 {
  double v[3];
  double operator()(int i) const { return v[i]; }
};

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  voxel_map::Vec3i size;
  V3 origin;
  double scale = 0.0, a_brake = 0.0, t_react = 0.0, clearance = 0.0;
  int m = 0, N = 0, res = 0;
  if (fscanf(f, "%d %d %d %lf %lf %lf %lf %d", &size(0), &size(1), &size(2), &origin.v[0], &origin.v[1], &origin.v[2], &scale, &m) != 8)
    return 2;
  try {
    voxel_map::VoxelMap map(size, origin, scale);
    for (int i = 0; i < m; ++i) {
      voxel_map::Vec3i id;
      if (fscanf(f, "%d %d %d", &id(0), &id(1), &id(2)) != 3) return 2;
      map.setOccupied(id);
    }
    if (fscanf(f, "%lf %lf %lf %d %d", &a_brake, &t_react, &clearance, &res, &N) != 5 || N < 1) return 2;
    Trajectory<5> traj;
    for (int i = 0; i < N; ++i) {
      double T = 0.0;
      anet::Matrix<3, 6> cm;
      if (fscanf(f, "%lf", &T) != 1) return 2;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 6; ++c)
          if (fscanf(f, "%lf", &cm(r, c)) != 1) return 2;
      traj.emplace_back(T, cm);
    }
    fclose(f);
    double t = 0.0;
    int piece = 0;
    const double margin = getStopMargin(traj, map, a_brake, t_react, clearance, res, t, piece);
    // a clearance that the trajectory surely keeps, and one it surely does not
    printf("{\"margin\": %.17g, \"t\": %.17g, \"piece\": %d, \"stoppable\": %d, \"stoppable_loose\": %d, \"stoppable_tight\": %d}\n",
           margin, t, piece, (int)checkStoppable(traj, map, a_brake, t_react, clearance, res),
           (int)checkStoppable(traj, map, a_brake, t_react, clearance + margin - 1e-3, res),
           (int)checkStoppable(traj, map, a_brake, t_react, clearance + margin + 1e-3, res));
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
