// Piece<D>::getCorridorMargin, Trajectory<D>::getCorridorMargin / checkCorridor (include/allocnet_amd/trajectory.hpp).
//     test_corridor_margin CASE.txt
// The file holds one trajectory of degree 5 as text: the piece count N; per piece its duration, 18 coefficients (3 x 6, row-major,
// highest power first), a row count m and m rows of four numbers; then a tolerance.  Printed: one JSON object, numbers with %.17g.
// tests/test_corridor_margin_gpu.py compares it with the Python facade.  `HPoly` stands in for Eigen::MatrixX4d (duck typing only).
#include <cstdio>
#include <vector>

#include "allocnet_amd/trajectory.hpp"

struct HPoly {
  int R = 0;
  std::vector<double> a;
  double operator()(int r, int c) const { return a[(size_t)r * 4 + c]; }
  int rows() const { return R; }
};

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int N = 0;
  if (fscanf(f, "%d", &N) != 1 || N < 1) return 2;
  Trajectory<5> traj;
  std::vector<HPoly> polys(N);
  for (int i = 0; i < N; ++i) {
    double T = 0.0;
    anet::Matrix<3, 6> cm;
    if (fscanf(f, "%lf", &T) != 1) return 2;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 6; ++c)
        if (fscanf(f, "%lf", &cm(r, c)) != 1) return 2;
    traj.emplace_back(T, cm);
    if (fscanf(f, "%d", &polys[i].R) != 1) return 2;
    polys[i].a.resize((size_t)polys[i].R * 4);
    for (double &x : polys[i].a)
      if (fscanf(f, "%lf", &x) != 1) return 2;
  }
  double tol = 0.0;
  if (fscanf(f, "%lf", &tol) != 1) return 2;
  fclose(f);
  try {
    std::vector<double> per(N);
    const double all = traj.getCorridorMargin(polys, per.data());
    // the plain-array overload on the same rows, padded to the widest polytope
    int M = 1;
    for (const auto &h : polys) M = h.R > M ? h.R : M;
    std::vector<double> rows((size_t)N * M * 4, 0.0);
    for (int i = 0; i < N; ++i)
      for (int r = 0; r < polys[i].R; ++r)
        for (int c = 0; c < 4; ++c) rows[((size_t)i * M + r) * 4 + c] = polys[i](r, c);
    const double all_plain = traj.getCorridorMargin(rows.data(), M);
    printf("{\"margin\": %.17g, \"margin_plain\": %.17g, \"per_piece\": [", all, all_plain);
    for (int i = 0; i < N; ++i) printf("%s%.17g", i ? ", " : "", per[i]);
    printf("], \"pieces\": [");
    for (int i = 0; i < N; ++i)
      printf("%s[%.17g, %.17g]", i ? ", " : "", traj[i].getCorridorMargin(polys[i]),
             traj[i].getCorridorMargin(polys[i].a.data(), polys[i].R));
    printf("], \"check_default\": %d, \"check_tol\": %d, \"check_plain_tol\": %d}\n", (int)traj.checkCorridor(polys),
           (int)traj.checkCorridor(polys, tol), (int)traj.checkCorridor(rows.data(), M, tol));
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
