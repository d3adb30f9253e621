// getClearance / checkClearance of include/allocnet_amd/trajectory_map.hpp.
//     test_traj_clearance CASE.txt
// The file holds, as text: the grid (three sizes, three origin coordinates, the scale); a count m and m voxel index triples to
// set; the number of dilation rounds; a count k and k points (three coordinates each); a distance; the piece count N; per piece
// its duration and 18 coefficients (3 x 6, row-major, highest power first).  Printed: one JSON object, numbers with %.17g.
// tests/test_traj_clearance_gpu.py compares it with the Python facade.
#include <cstdio>
#include <vector>

#include "allocnet_amd/trajectory_map.hpp"

struct V3 {
  double v[3];
  double operator()(int i) const { return v[i]; }
};

// %.17g, with the spellings JSON readers accept for the non-finite values
static void num(double x) {
  if (x != x) printf("NaN");
  else if (x - x != 0.0) printf(x > 0.0 ? "Infinity" : "-Infinity");
  else printf("%.17g", x);
}

template <class P>
static void report(const char *name, const Trajectory<5> &traj, const P &points, double min_dist) {
  double t = 0.0;
  int piece = 0, point = 0;
  const double d = getClearance(traj, points, t, piece, point);
  printf("\"%s\": {\"d\": ", name);
  num(d);
  printf(", \"t\": ");
  num(t);
  printf(", \"piece\": %d, \"point\": %d, \"ok\": %d, \"pieces\": [", piece, point, (int)checkClearance(traj, points, min_dist));
  for (int i = 0; i < traj.getPieceNum(); ++i) {
    double tp = 0.0;
    int pp = 0;
    const double dp = getClearance(traj[i], points, tp, pp);
    printf("%s[", i ? ", " : "");
    num(dp);
    printf(", ");
    num(tp);
    printf(", %d, %d]", pp, (int)checkClearance(traj[i], points, min_dist));
  }
  printf("]}");
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  voxel_map::Vec3i size;
  V3 origin;
  double scale = 0.0, min_dist = 0.0;
  int m = 0, N = 0, rounds = 0, k = 0;
  if (fscanf(f, "%d %d %d %lf %lf %lf %lf %d", &size(0), &size(1), &size(2), &origin.v[0], &origin.v[1], &origin.v[2], &scale, &m) != 8)
    return 2;
  try {
    voxel_map::VoxelMap map(size, origin, scale);
    for (int i = 0; i < m; ++i) {
      voxel_map::Vec3i id;
      if (fscanf(f, "%d %d %d", &id(0), &id(1), &id(2)) != 3) return 2;
      map.setOccupied(id);
    }
    if (fscanf(f, "%d %d", &rounds, &k) != 2 || k < 0) return 2;
    map.dilate(rounds);
    std::vector<anet::Vec3> points((size_t)k);
    for (int i = 0; i < k; ++i)
      if (fscanf(f, "%lf %lf %lf", &points[(size_t)i](0), &points[(size_t)i](1), &points[(size_t)i](2)) != 3) return 2;
    if (fscanf(f, "%lf %d", &min_dist, &N) != 2 || N < 1) return 2;
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
    printf("{");
    report("points", traj, points, min_dist);
    printf(", ");
    report("map", traj, map, min_dist);
    printf(", ");
    report("none", traj, std::vector<anet::Vec3>(), min_dist);
    printf("}\n");
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
