// sfc_opt::getShortestPath / allotPieces / expandCorridor (include/allocnet_amd/sfc_opt.hpp) on one corridor.
//     test_sfc_path PROBLEM.txt
// The file: "N M K lengthPerPiece", then one line each (%.17g): start (3), goal (3), the N polytopes of M rows a.x <= b (zero rows
// padding).  Printed, one "key: values" line each with %.17g: points (the route, start and goal included), length, status (status,
// iterations, evaluations), pieces, expanded (the number of polytopes of the expanded corridor).  tests/test_sfc_path_gpu.py
// compares every number bit for bit with the Python facade.  `Mat` stands in for Eigen::MatrixXd, `Vec` for Eigen::Vector3d.
#include <cstdio>
#include <vector>

#include "allocnet_amd/sfc_opt.hpp"

struct Mat {
  int R = 0, C = 0;
  std::vector<double> a;
  Mat() = default;
  Mat(int r, int c) : R(r), C(c), a((size_t)r * c, 0.0) {}
  double &operator()(int r, int c) { return a[(size_t)r * C + c]; }
  double operator()(int r, int c) const { return a[(size_t)r * C + c]; }
  int rows() const { return R; }
};
struct Vec {
  std::vector<double> a;
  double operator()(int i) const { return a[(size_t)i]; }
};

static bool read(FILE *f, std::vector<double> &v) {
  for (double &x : v)
    if (fscanf(f, "%lf", &x) != 1) return false;
  return true;
}
static void print(const char *key, const std::vector<double> &v) {
  printf("%s:", key);
  for (double x : v) printf(" %.17g", x);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int N = 0, M = 0, K = 0, rc = 0;
  double lpp = 0.0;
  try {
    if (fscanf(f, "%d %d %d %lf", &N, &M, &K, &lpp) != 4 || N < 2) { fclose(f); return 2; }
    Vec start, goal;
    start.a.resize(3); goal.a.resize(3);
    std::vector<double> hp((size_t)N * M * 4);
    if (!read(f, start.a) || !read(f, goal.a) || !read(f, hp)) { fclose(f); return 2; }
    std::vector<Mat> polys;  // raw form h.[x;1] <= 0, the padding rows kept
    for (int i = 0; i < N; ++i) {
      Mat m(M, 4);
      for (int r = 0; r < M; ++r) {
        const double *h = &hp[((size_t)i * M + r) * 4];
        for (int c = 0; c < 3; ++c) m(r, c) = h[c];
        m(r, 3) = -h[3];
      }
      polys.push_back(m);
    }
    const sfc_opt::Route route = sfc_opt::getShortestPath(start, goal, polys, 1.0e-2, K);
    print("points", route.points);
    print("length", {route.length});
    printf("status: %d %d %d\n", route.status, route.iters, route.evals);
    const std::vector<int> pieces = sfc_opt::allotPieces(route.points, lpp);
    print("pieces", std::vector<double>(pieces.begin(), pieces.end()));
    printf("expanded: %d\n", (int)sfc_opt::expandCorridor(polys, pieces).size());
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  fclose(f);
  return rc;
}
