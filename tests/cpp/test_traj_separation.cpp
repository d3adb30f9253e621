// getSeparation / checkSeparation / getSeparations of include/allocnet_amd/trajectory_pair.hpp.
//     test_traj_separation CASE.txt
// The file holds, as text: a distance; the number of trajectories B; per trajectory its start time, its piece count N and per piece
// its duration and 18 coefficients (3 x 6, row-major, highest power first); a count P and P index pairs.  Printed: one JSON
// object, numbers with %.17g.  tests/test_traj_separation_gpu.py compares it with the Python facade.
#include <cstdio>
#include <utility>
#include <vector>

#include "allocnet_amd/trajectory_pair.hpp"

// %.17g, with the spellings JSON readers accept for the non-finite values
static void num(double x) {
  if (x != x) printf("NaN");
  else if (x - x != 0.0) printf(x > 0.0 ? "Infinity" : "-Infinity");
  else printf("%.17g", x);
}

static void row(double d, double t, int pa, int pb) {
  printf("[");
  num(d);
  printf(", ");
  num(t);
  printf(", %d, %d]", pa, pb);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  double min_dist = 0.0;
  int B = 0, P = 0;
  if (fscanf(f, "%lf %d", &min_dist, &B) != 2 || B < 1) return 2;
  std::vector<Trajectory<5>> fleet((size_t)B);
  std::vector<double> t0((size_t)B);
  for (int b = 0; b < B; ++b) {
    int N = 0;
    if (fscanf(f, "%lf %d", &t0[(size_t)b], &N) != 2 || N < 1) return 2;
    for (int i = 0; i < N; ++i) {
      double T = 0.0;
      anet::Matrix<3, 6> cm;
      if (fscanf(f, "%lf", &T) != 1) return 2;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 6; ++c)
          if (fscanf(f, "%lf", &cm(r, c)) != 1) return 2;
      fleet[(size_t)b].emplace_back(T, cm);
    }
  }
  if (fscanf(f, "%d", &P) != 1 || P < 0) return 2;
  std::vector<std::pair<int, int>> pairs((size_t)P);
  for (int p = 0; p < P; ++p)
    if (fscanf(f, "%d %d", &pairs[(size_t)p].first, &pairs[(size_t)p].second) != 2) return 2;
  fclose(f);
  try {
    printf("{\"batch\": [");
    const std::vector<anet::PairSeparation> all = anet::getSeparations(fleet, t0, pairs);
    for (int p = 0; p < P; ++p) {
      printf("%s", p ? ", " : "");
      row(all[(size_t)p].d, all[(size_t)p].t, all[(size_t)p].pieceA, all[(size_t)p].pieceB);
    }
    printf("], \"single\": [");
    for (int p = 0; p < P; ++p) {
      const Trajectory<5> &A = fleet[(size_t)pairs[(size_t)p].first], &Bt = fleet[(size_t)pairs[(size_t)p].second];
      const double ta = t0[(size_t)pairs[(size_t)p].first], tb = t0[(size_t)pairs[(size_t)p].second];
      double t = 0.0;
      int pa = 0, pb = 0;
      const double d = getSeparation(A, Bt, ta, tb, t, pa, pb);
      printf("%s", p ? ", " : "");
      row(d, t, pa, pb);
    }
    printf("], \"ok\": [");
    for (int p = 0; p < P; ++p) {
      const Trajectory<5> &A = fleet[(size_t)pairs[(size_t)p].first], &Bt = fleet[(size_t)pairs[(size_t)p].second];
      printf("%s%d", p ? ", " : "",
             (int)checkSeparation(A, Bt, min_dist, t0[(size_t)pairs[(size_t)p].first], t0[(size_t)pairs[(size_t)p].second]));
    }
    printf("]}\n");
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
