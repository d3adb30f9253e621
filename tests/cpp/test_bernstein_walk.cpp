// The shared pieces of csrc/bernstein_walk.h on the host, in exact arithmetic: control values are small integers times a power
// of two, so every halving is exact and every comparison below is ==.  No HIP runtime call; built by
// tests/test_bernstein_walk_cpu.py for the host only.
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../allocnet_amd/csrc/bernstein_walk.h"

using namespace anet::bern;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      ++failures;                                                          \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
    }                                                                      \
  } while (0)

static int64_t ibinom(int n, int k) {
  int64_t r = 1;
  for (int j = 0; j < k; ++j) r = r * (n - j) / (j + 1);
  return r;
}

// integers in [-9, 9] with sign changes and zeros, the same for every run
static int value(int M, int k) { return ((k * 7 + M * 3) % 19) - 9; }

// halve<M> against the sub-polygons computed directly: L_j = 2^-j sum_i C(j, i) w_i, R_j = 2^-(M-1-j) sum_i C(M-1-j, i) w_(j+i)
template <int M>
static void test_halve() {
  const double unit = ldexp(1.0, 20);
  double w[M], le[M], ri[M];
  for (int k = 0; k < M; ++k) w[k] = le[k] = ri[k] = (double)value(M, k) * unit;
  halve<M>(le, false);
  halve<M>(ri, true);
  for (int j = 0; j < M; ++j) {
    int64_t sl = 0, sr = 0;
    for (int i = 0; i <= j; ++i) sl += ibinom(j, i) * value(M, i);
    for (int i = 0; i <= M - 1 - j; ++i) sr += ibinom(M - 1 - j, i) * value(M, j + i);
    CHECK(le[j] == ldexp((double)sl, 20 - j));
    CHECK(ri[j] == ldexp((double)sr, 20 - (M - 1 - j)));
  }
  CHECK(le[M - 1] == ri[0] && le[0] == w[0] && ri[M - 1] == w[M - 1]);
}

// descend at (3, 5) = right, left, right
template <int M, class Index>
static void test_descend() {
  double root[M], w[M], v[M];
  for (int k = 0; k < M; ++k) root[k] = v[k] = (double)value(M, k) * ldexp(1.0, 40);
  Dyadic<20, Index> d;
  d.lev = 3;
  d.idx = 5;
  d.template descend<M>(root, w);
  halve<M>(v, true);
  halve<M>(v, false);
  halve<M>(v, true);
  for (int k = 0; k < M; ++k) CHECK(w[k] == v[k]);
  CHECK(d.width() == 0.125 && d.lo() == 0.625);
  Dyadic<20, Index> r;
  r.template descend<M>(root, w);
  for (int k = 0; k < M; ++k) CHECK(w[k] == root[k]);
  CHECK(r.width() == 1.0 && r.lo() == 0.0);
}

static void test_signs() {
  {
    const double w[6] = {0.0, 2.0, 0.0, -1.0, 3.0, 0.0};  // zeros at both ends and inside: + - +
    const Signs s = signs<6>(w);
    CHECK(s.var == 2 && s.first == 1 && s.mx == 3.0);
  }
  {
    const double w[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const Signs s = signs<5>(w);
    CHECK(s.var == 0 && s.first == 0 && s.mx == 0.0);
  }
  {
    const double w[5] = {-4.0, 0.0, 0.0, -1.0, 0.5};
    const Signs s = signs<5>(w);
    CHECK(s.var == 1 && s.first == -1 && s.mx == 4.0);
  }
  {
    const double w[3] = {0.0, 0.0, -2.0};
    const Signs s = signs<3>(w);
    CHECK(s.var == 0 && s.first == -1 && s.mx == 2.0);
  }
  {
    const double w[4] = {1.0, -1.0, 1.0, -1.0};
    const Signs s = signs<4>(w);
    CHECK(s.var == 3 && s.first == 1 && s.mx == 1.0);
  }
}

static void preorder(int lev, uint64_t idx, int depth, std::vector<std::pair<int, uint64_t>> &out) {
  out.push_back({lev, idx});
  if (lev < depth) {
    preorder(lev + 1, 2 * idx, depth, out);
    preorder(lev + 1, 2 * idx + 1, depth, out);
  }
}

template <int MaxDepth, class Index>
static void test_walk() {
  // always splitting down to depth 3: the 15 intervals, left first, parents before children, then the end
  std::vector<std::pair<int, uint64_t>> want;
  preorder(0, 0, 3, want);
  CHECK(want.size() == 15);
  Dyadic<MaxDepth, Index> d;
  size_t seen = 0;
  bool more = true;
  for (int guard = 0; guard < 100 && more; ++guard) {
    CHECK(seen < want.size() && d.lev == want[seen].first && (uint64_t)d.idx == want[seen].second);
    ++seen;
    more = d.advance(d.lev < 3);
  }
  CHECK(seen == 15 && !more && d.lev == 0);
  // never splitting: one visit
  Dyadic<MaxDepth, Index> one;
  CHECK(one.can_split() && !one.advance(false) && one.lev == 0 && one.idx == 0);
  // the depth bound: no split there, and the climb from the right-most leaf ends the walk
  Dyadic<MaxDepth, Index> leaf;
  leaf.lev = MaxDepth;
  leaf.idx = (Index)((((uint64_t)1 << (MaxDepth - 1)) - 1) * 2 + 1);  // 2^MaxDepth - 1
  CHECK(!leaf.can_split());
  CHECK(leaf.width() == ldexp(1.0, -MaxDepth) && leaf.lo() + leaf.width() == 1.0);
  CHECK(!leaf.advance(false) && leaf.lev == 0 && leaf.idx == 0);
  // from the left-most leaf the next interval is its sibling
  Dyadic<MaxDepth, Index> left;
  left.lev = MaxDepth;
  left.idx = 0;
  CHECK(left.advance(false) && left.lev == MaxDepth && left.idx == 1);
  // the last leaf of the left half climbs to the right half of the root
  left.idx = (Index)(((uint64_t)1 << (MaxDepth - 1)) - 1);
  CHECK(left.advance(false) && left.lev == 1 && left.idx == 1);
}

static void test_forms() {
  CHECK(binom(7, 3) == 35.0 && binom(13, 6) == 1716.0 && binom(5, 0) == 1.0);
  // 1 + 2 t + t^2 = (1 + t)^2: control values 1, 2, 4
  const double u[3] = {1.0, 2.0, 1.0};
  double z[3];
  to_bernstein<3>(u, z);
  CHECK(z[0] == 1.0 && z[1] == 2.0 && z[2] == 4.0);
  CHECK(horner<3>(u, 0.5) == 2.25);
  // x = (t, 0, 0) and y = (t^2, 0, 0) in degree 2: x . y' / 2 = t^2, degree 3: control values 0, 0, 1/3, 1
  const double x[3][3] = {{0.0, 0.5, 1.0}, {0, 0, 0}, {0, 0, 0}}, y[3][3] = {{0.0, 0.0, 1.0}, {0, 0, 0}, {0, 0, 0}};
  double dv[4];
  product_cv<2>(x, y, dv);
  CHECK(dv[0] == 0.0 && dv[1] == 0.0 && dv[3] == 1.0 && fabs(dv[2] - 1.0 / 3.0) <= 1e-16);
  // the largest step of y's control polygon is 1: L h / 2 = 2 * 1 * (1 / 8) / 2 for 9 values
  CHECK(lipschitz_half_step<2>(y, 9) == 0.125);
}

int main() {
  test_halve<3>();
  test_halve<6>();
  test_halve<10>();
  test_halve<14>();
  test_descend<3, uint32_t>();
  test_descend<6, uint32_t>();
  test_descend<10, uint64_t>();
  test_descend<14, uint64_t>();
  test_signs();
  test_walk<20, uint32_t>();
  test_walk<20, uint64_t>();
  test_walk<32, uint32_t>();
  test_walk<32, uint64_t>();
  test_forms();
  std::printf("bernstein walk: %d failures\n", failures);
  return failures ? 1 : 0;
}
