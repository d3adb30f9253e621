// The Bernstein subdivision walk of the exact trajectory queries (corridor_margin_kernels.h, voxel_hit_kernels.h,
// clearance_kernels.h, separation_kernels.h), stated once.
//
// THE WALK.  A polynomial is held as its Bernstein control values on [0, 1].  The sign changes of the control values bound the
// number of its roots in the interval (variation diminishing), and the control values of either half follow from those of the
// whole by de Casteljau at 1/2: averages only, no monomial is ever re-expanded.  So a query halves [0, 1] until an interval holds
// at most one sign change (or, for voxel-hit, until the curve's box is small), and treats that interval by a rule of its own.
// The intervals are dyadic, [idx, idx + 1] / 2^lev, and are visited left first WITHOUT A STACK: the state is the pair
// (lev, idx), and the control values of a visit are rebuilt from the root by `lev` halvings chosen by the bits of idx
// (Dyadic::descend).  That costs `lev` halvings per visit instead of one, at the depth 2 or 3 that separated roots need, and
// keeps the lane free of private memory: every array here has compile-time indices (k_piece_max_rate's stack of control values
// is scratch).  After a visit the walk either splits -- (lev + 1, 2 idx) -- or climbs while the interval is a right child and
// steps to the sibling on the right; back at the root it is over (Dyadic::advance).
// BUDGETS.  The halvings of a visit and the climb run MaxDepth times at most, whatever (lev, idx) holds; can_split() is false
// at MaxDepth, where the kernel lets the midpoint stand for the cluster; the number of visits is bounded by the kernel's own
// loop.  All structural: no input can spin a wave.
// SPLIT POINTS ARE CANDIDATES.  A kernel that looks for extrema takes the midpoint of every interval it splits as a candidate,
// so a root that falls exactly on a split point is not lost between two halves that each see no sign change.
//
// Everything is __host__ __device__ __forceinline__ or constexpr (tests/cpp/test_bernstein_walk.cpp runs the walk on the host in
// exact arithmetic): no LDS, no atomics, no array indexed at run time.  The arithmetic is what the four kernels wrote out before
// this header existed, operation by operation -- the fused multiply-adds where they stood, 0.5 * (a + b) for a midpoint -- and
// tools/hash_traj_queries.py is how a change here is shown to keep every output bit.
// k_traj_voxel_hit keeps the (lev, idx) state of Dyadic written out (through the struct it measured 0.8 % slower at 131 072
// trajectories) and does not use halve: it blossoms straight to [a, b].
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace anet {
namespace bern {

#define ANET_BERN __host__ __device__ __forceinline__

constexpr double binom(int n, int k) {
  double r = 1.0;
  for (int j = 0; j < k; ++j) r = r * (double)(n - j) / (double)(j + 1);
  return r;
}

// ascending coefficients u of a polynomial of degree D - 1 -> its control values on [0, 1], z_i = sum_{k<=i} C(i,k)/C(n,k) u_k
template <int D>
ANET_BERN void to_bernstein(const double (&u)[D], double (&z)[D]) {
  constexpr int n = D - 1;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double acc = u[0];
#pragma unroll
    for (int k = 1; k <= i; ++k) acc = __builtin_fma(binom(i, k) / binom(n, k), u[k], acc);
    z[i] = acc;
  }
}

// Piece i of column b (coefficients highest power first, [(i*3+ax)*D + k][ld]) in normalised time: u[ax][k] = c_k T^k, so that
// p(T tau) = sum_k u_k tau^k.  A = sum |u|; false: a coefficient or a product is not finite.
template <int D>
ANET_BERN bool normalised(const double *coeffs, int i, int64_t b, int64_t ld, double Ti, double (&u)[3][D], double &A) {
  constexpr int n = D - 1;
  bool ok = true;
  double tk[D];
  tk[0] = 1.0;
#pragma unroll
  for (int k = 1; k < D; ++k) tk[k] = tk[k - 1] * Ti;
  A = 0.0;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double c = coeffs[(int64_t)((i * 3 + ax) * D + (n - k)) * ld + b];
      u[ax][k] = c * tk[k];
      ok = ok && fabs(c) < INFINITY && fabs(u[ax][k]) < INFINITY;
      A += fabs(u[ax][k]);
    }
  }
  return ok;
}

// Horner
template <int D>
ANET_BERN double horner(const double (&g)[D], double tau) {
  double v = g[D - 1];
#pragma unroll
  for (int k = D - 2; k >= 0; --k) v = __builtin_fma(v, tau, g[k]);
  return v;
}
template <int D>
ANET_BERN void horner3(const double (&u)[3][D], double tau, double (&v)[3]) {
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) v[ax] = horner<D>(u[ax], tau);
}

// control values on an interval -> those on its left or right half (de Casteljau at 1/2)
template <int M>
ANET_BERN void halve(double (&w)[M], bool right) {
  double le[M];
  le[0] = w[0];
#pragma unroll
  for (int r = 1; r < M; ++r) {
#pragma unroll
    for (int k = 0; k < M - r; ++k) w[k] = 0.5 * (w[k] + w[k + 1]);
    le[r] = w[0];
  }  // in place, w has ended as the right half
#pragma unroll
  for (int k = 0; k < M; ++k) w[k] = right ? w[k] : le[k];
}

// var: sign changes of the control values, zeros skipped; first: the first sign that is not zero (0: none); mx: largest modulus
struct Signs {
  int var, first;
  double mx;
};
template <int M>
ANET_BERN Signs signs(const double (&w)[M]) {
  int var = 0, last = 0, first = 0;
  double mx = 0.0;
#pragma unroll
  for (int k = 0; k < M; ++k) {
    const int sg = (w[k] > 0.0) - (w[k] < 0.0);
    mx = fmax(mx, fabs(w[k]));
    if (sg != 0) {
      if (first == 0) first = sg;
      if (last != 0 && sg != last) ++var;
      last = sg;
    }
  }
  return {var, first, mx};
}

// the state of the walk: the interval [idx, idx + 1] / 2^lev
template <int MaxDepth, class Index>
struct Dyadic {
  int lev = 0;
  Index idx = 0;
  // the control values of this interval from those of [0, 1]
  template <int M>
  ANET_BERN void descend(const double (&root)[M], double (&w)[M]) const {
#pragma unroll
    for (int k = 0; k < M; ++k) w[k] = root[k];
    for (int l = 0; l < lev && l < MaxDepth; ++l) halve<M>(w, (idx >> (lev - 1 - l)) & 1u);
  }
  ANET_BERN double width() const { return ldexp(1.0, -lev); }
  ANET_BERN double lo() const { return (double)idx * width(); }
  ANET_BERN bool can_split() const { return lev < MaxDepth; }
  // to the left half (split), or to the next interval on the right; false: the walk is over
  ANET_BERN bool advance(bool split) {
    if (split) {
      ++lev;
      idx <<= 1;
      return true;
    }
    for (int q = 0; q < MaxDepth && lev > 0 && (idx & 1u); ++q) { idx >>= 1; --lev; }
    if (lev == 0) return false;
    idx += 1;
    return true;
  }
};

// Control values (degree 2n - 1) of x . y' / n from the control values of x and y (degree n, three components): a product of
// Bernstein polynomials is a sum of positive weights times products of control values -- nothing is expanded into monomials and
// nothing cancels that does not cancel in the product itself.
template <int n>
ANET_BERN void product_cv(const double (&x)[3][n + 1], const double (&y)[3][n + 1], double (&dv)[2 * n]) {
#pragma unroll
  for (int k = 0; k < 2 * n; ++k) dv[k] = 0.0;
#pragma unroll
  for (int i = 0; i <= n; ++i) {
#pragma unroll
    for (int j = 0; j < n; ++j) {
      double dot = 0.0;
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) dot = __builtin_fma(x[ax][i], y[ax][j + 1] - y[ax][j], dot);
      dv[i + j] = __builtin_fma(binom(n, i) * binom(n - 1, j) / binom(2 * n - 1, i + j), dot, dv[i + j]);
    }
  }
}

// L h / 2 for K values of tau at k / (K - 1): every tau is within h / 2 of one of them, and L = n max_k || z_(k+1) - z_k ||
// bounds the speed of the curve with control values z from above
template <int n>
ANET_BERN double lipschitz_half_step(const double (&z)[3][n + 1], int K) {
  double m = 0.0;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    const double dx = z[0][k + 1] - z[0][k], dy = z[1][k + 1] - z[1][k], dz = z[2][k + 1] - z[2][k];
    m = fmax(m, __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)));
  }
  return sqrt(m) * ((double)n * 0.5 / (double)(K - 1));
}

#undef ANET_BERN

}  // namespace bern
}  // namespace anet
