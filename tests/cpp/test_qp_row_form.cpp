// QPSolver::setRowForm of the C++ facade (include/allocnet_amd/qp_solver.hpp): reads one problem from a text file -- order,
// pieces, Bernstein segments per piece; iniPVA and finPVA (row = axis); the durations; per piece its row count and rows -- solves it
// with the rows on control values and prints status, objective and coefficients (%.17g) as one JSON object;
// tests/test_qp_control_points_gpu.py compares them with allocnet_amd.qp_solve on the same problem.
#include <cstdio>
#include <exception>
#include <vector>

#include <stdint.h>
#include "allocnet_amd/qp_solver.hpp"

struct Mat3 {
  double a[9];
  double operator()(int r, int c) const { return a[r * 3 + c]; }
};
struct Poly {  // Eigen::MatrixX4d-like
  int R;
  std::vector<double> a;
  long rows() const { return R; }
  double operator()(int r, int c) const { return a[(size_t)r * 4 + c]; }
};
struct Times {
  std::vector<double> a;
  double operator()(int i) const { return a[(size_t)i]; }
};
struct VecX {  // Eigen::VectorXd-like
  std::vector<double> a;
  void resize(long n) { a.assign((size_t)n, 0.0); }
  double &operator()(long i) { return a[(size_t)i]; }
};

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int order = 0, seg = 0, segments = 0;
  if (std::fscanf(f, "%d %d %d", &order, &seg, &segments) != 3) return 2;
  Mat3 ini, fin;
  for (int k = 0; k < 9; ++k)
    if (std::fscanf(f, "%lf", &ini.a[k]) != 1) return 2;
  for (int k = 0; k < 9; ++k)
    if (std::fscanf(f, "%lf", &fin.a[k]) != 1) return 2;
  Times T;
  T.a.resize((size_t)seg);
  for (int i = 0; i < seg; ++i)
    if (std::fscanf(f, "%lf", &T.a[(size_t)i]) != 1) return 2;
  std::vector<Poly> polys((size_t)seg);
  for (int i = 0; i < seg; ++i) {
    if (std::fscanf(f, "%d", &polys[(size_t)i].R) != 1) return 2;
    polys[(size_t)i].a.resize((size_t)polys[(size_t)i].R * 4);
    for (double &v : polys[(size_t)i].a)
      if (std::fscanf(f, "%lf", &v) != 1) return 2;
  }
  std::fclose(f);
  try {
    QPSolver solver(QPConfig(3.0, 4.0, 20));
    solver.setOrder(order);
    solver.setRowForm(ANET_QP_ROWS_CONTROL_POINTS, segments);
    VecX sol;
    const bool ok = solver.solve(ini, fin, polys, T, sol);
    std::printf("{\"ok\": %d, \"obj\": %.17g, \"iters\": %d, \"coeffs\": [", ok ? 1 : 0, solver.getObjCost(), solver.getIterations());
    for (size_t i = 0; i < sol.a.size(); ++i) std::printf("%s%.17g", i ? ", " : "", sol.a[i]);
    std::printf("]}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
