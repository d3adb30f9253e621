// geo_utils::enumerateVs / filterVs (include/allocnet_amd/geo_utils.hpp) the way visualizer.hpp:191 calls them.
//     test_geo_vertices POLYTOPES.txt
// The file holds polytopes as text: a row count m, then m rows of four numbers (%.17g), repeated.  For each polytope the three
// overloads run; one JSON object is printed, vertices with %.17g.  tests/test_polytope_vertices_gpu.py compares it bit for bit
// with the Python facade.  `HPoly` / `VPoly` / `V3` stand in for Eigen::MatrixX4d / Matrix3Xd / Vector3d (duck typing only).
#include <array>
#include <cstdio>
#include <vector>

#include "allocnet_amd/geo_utils.hpp"

struct HPoly {
  int R = 0;
  std::vector<double> a;
  double operator()(int r, int c) const { return a[(size_t)r * 4 + c]; }
  int rows() const { return R; }
};
struct VPoly {
  int R = 0, C = 0;
  std::vector<double> a;
  void resize(int r, int c) { R = r; C = c; a.assign((size_t)r * c, 0.0); }
  double &operator()(int r, int c) { return a[(size_t)r * C + c]; }
  double operator()(int r, int c) const { return a[(size_t)r * C + c]; }
  int cols() const { return C; }
};
struct V3 {
  double v[3] = {0.0, 0.0, 0.0};
  double &operator()(int i) { return v[i]; }
  double operator()(int i) const { return v[i]; }
};

static void print_points(const char *key, const VPoly &v, bool last = false) {
  printf("\"%s\": [", key);
  for (int c = 0; c < v.cols(); ++c) printf("%s[%.17g, %.17g, %.17g]", c ? ", " : "", v(0, c), v(1, c), v(2, c));
  printf("]%s", last ? "" : ", ");
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  try {
    printf("{\"polytopes\": [");
    int m = 0, n_poly = 0;
    while (fscanf(f, "%d", &m) == 1) {
      HPoly h;
      h.R = m;
      h.a.resize((size_t)m * 4);
      for (double &x : h.a)
        if (fscanf(f, "%lf", &x) != 1) return 2;
      VPoly two, four, raw, filtered;
      std::vector<std::array<double, 3>> vec;
      const bool ok = geo_utils::enumerateVs(h, two);
      V3 inner;
      const bool has_inner = geo_utils::findInterior(h, inner);
      geo_utils::enumerateVs(h, inner, four, 1.0e-6);
      const bool ok_vec = geo_utils::enumerateVs(h, vec, 1.0e-6);
      VPoly as_vec;
      as_vec.resize(3, (int)vec.size());
      for (size_t q = 0; q < vec.size(); ++q)
        for (int r = 0; r < 3; ++r) as_vec(r, (int)q) = vec[q][r];
      // filterVs: every vertex three times, the second copy moved by half the resolution -> the vertices again
      const int n = two.cols();
      raw.resize(3, 3 * n);
      for (int c = 0; c < n; ++c)
        for (int r = 0; r < 3; ++r) {
          raw(r, c) = two(r, c);
          raw(r, n + c) = two(r, c) + 5.0e-7;
          raw(r, 2 * n + c) = two(r, c);
        }
      geo_utils::filterVs(raw, 1.0e-6, filtered);
      printf("%s{\"ok\": %s, \"ok_vector\": %s, \"interior\": %s, ", n_poly ? ", " : "", ok ? "true" : "false", ok_vec ? "true" : "false",
             has_inner ? "true" : "false");
      print_points("two", two);
      print_points("four", four);
      print_points("vector", as_vec);
      print_points("filtered", filtered, true);
      printf("}");
      ++n_poly;
    }
    printf("]}\n");
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    fclose(f);
    return 1;
  }
  fclose(f);
  return 0;
}
