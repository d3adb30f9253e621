// Source-compatible stand-ins for the polytope tests of the reference's geo_utils
// (src/planner/include/gcopter/geo_utils.hpp:43-111):
//     bool geo_utils::findInterior(hPoly, interior);
//     bool geo_utils::overlap(hPoly0, hPoly1, eps = 1.0e-6);
//     bool geo_utils::overlapPt(hPoly0, hPoly1, inner_pt, eps = 1.0e-6);     (geo_utils.hpp:88-111: the same test + its point)
// Both are the 4-variable linear programme  max t  s.t.  n.x + t <= -h3  the reference hands to sdlp::linprog<4>;
// here it runs on the MI355X behind anet_polytope_depth (batched; one polytope per call from this header,
// sfc_gen::shortCut in sfc_gen.hpp sends all its pairs at once).  Rows h of a polytope: h.[x;1] <= 0.
// Matrix arguments are duck-typed ((r,c) access, rows()); `interior` needs (i) access: Eigen types work unchanged.
//
// Vertex enumeration (geo_utils.hpp:128-202):
//     void geo_utils::filterVs(rV, epsilon, fV);
//     void geo_utils::enumerateVs(hPoly, inner, vPoly, epsilon = 1.0e-6);
//     bool geo_utils::enumerateVs(hPoly, vPoly, epsilon = 1.0e-6);
// behind anet_polytope_vertices: the feasible intersections of row triples, merged (the semantics are stated at that entry
// point in allocnet_amd.h), not the reference's quickhull of the polar dual -- the same vertex set in another order, and `inner`
// is accepted but not needed.  vPoly is filled through resize(3, n) and (r, c) (Eigen::Matrix3Xd, anet::MatrixX), or is a
// std::vector<std::array<double, 3>>.  A polytope without an interior point (empty, flat, unbounded) gives no vertices; the
// two-argument overload returns false for it.
// Deviation: filterVs merges by distance -- a point is dropped when one kept before it lies within max(epsilon, mag * DBL_EPSILON)
// of it in the max-norm -- where the reference rounds to a grid of that resolution and compares cells (two points 1e-12 apart on
// both sides of a cell edge stay distinct there).
#pragma once
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "core.hpp"

namespace geo_utils {

namespace detail {
template <typename Poly>
inline void append_rows(const Poly &h, std::vector<double> &out) {
  const int m = (int)h.rows();
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < 4; ++c) out.push_back(h(r, c));
}
}  // namespace detail

template <typename Poly, typename V3>
inline bool findInterior(const Poly &hPoly, V3 &interior) {
  std::vector<double> rows;
  detail::append_rows(hPoly, rows);
  const int m = (int)(rows.size() / 4);
  double depth = -INFINITY, pt[3] = {0.0, 0.0, 0.0};
  anet::Context &ctx = anet::Context::thread_default();
  ctx.check(anet_polytope_depth(ctx.get(), 1, m > 0 ? m : 1, rows.data(), 1, &depth, pt));
  for (int c = 0; c < 3; ++c) interior(c) = pt[c];
  return depth > 0.0 && !std::isinf(depth);
}

template <typename Poly0, typename Poly1>
inline bool overlap(const Poly0 &hPoly0, const Poly1 &hPoly1, const double eps = 1.0e-6) {
  std::vector<double> rows;
  detail::append_rows(hPoly0, rows);
  detail::append_rows(hPoly1, rows);
  const int m = (int)(rows.size() / 4);
  double depth = -INFINITY;
  anet::Context &ctx = anet::Context::thread_default();
  ctx.check(anet_polytope_depth(ctx.get(), 1, m > 0 ? m : 1, rows.data(), 0, &depth, nullptr));
  return depth > eps && !std::isinf(depth);
}

template <typename Poly0, typename Poly1, typename V3>
inline bool overlapPt(const Poly0 &hPoly0, const Poly1 &hPoly1, V3 &inner_pt, const double eps = 1.0e-6) {
  std::vector<double> rows;
  detail::append_rows(hPoly0, rows);
  detail::append_rows(hPoly1, rows);
  const int m = (int)(rows.size() / 4);
  double depth = -INFINITY, pt[3] = {0.0, 0.0, 0.0};
  anet::Context &ctx = anet::Context::thread_default();
  ctx.check(anet_polytope_depth(ctx.get(), 1, m > 0 ? m : 1, rows.data(), 0, &depth, pt));
  for (int c = 0; c < 3; ++c) inner_pt(c) = pt[c];
  return depth > eps && !std::isinf(depth);
}

namespace detail {
// the merge rule of anet_polytope_vertices on the host: keep[i] of n points p[3 i ..]
inline std::vector<int> merge_points(const std::vector<double> &p, const double epsilon) {
  std::vector<int> kept;
  double mag = 0.0;
  const int n = (int)(p.size() / 3);
  for (int i = 0; i < n; ++i) {
    const double *c = &p[(size_t)3 * i];
    const double m = std::fmax(mag, std::fmax(std::fabs(c[0]), std::fmax(std::fabs(c[1]), std::fabs(c[2]))));
    const double res = std::fmax(epsilon, m * DBL_EPSILON);
    bool dup = false;
    for (size_t q = 0; q < kept.size() && !dup; ++q) {
      const double *k = &p[(size_t)3 * kept[q]];
      dup = std::fabs(k[0] - c[0]) <= res && std::fabs(k[1] - c[1]) <= res && std::fabs(k[2] - c[2]) <= res;
    }
    if (!dup) {
      kept.push_back(i);
      mag = m;
    }
  }
  return kept;
}

// the vertices of one polytope, [n][3]; false: no interior point
template <typename Poly>
inline bool vertices_of(const Poly &hPoly, const double epsilon, std::vector<double> &verts) {
  std::vector<double> rows;
  append_rows(hPoly, rows);
  const int m = (int)(rows.size() / 4);
  if (m == 0) rows.assign(4, 0.0);
  int max_v = m > 4 ? 2 * m - 4 : 4;
  int32_t count = 0, status = 0;
  anet::Context &ctx = anet::Context::thread_default();
  for (int pass = 0; pass < 2; ++pass) {
    verts.assign((size_t)max_v * 3, 0.0);
    ctx.check(anet_polytope_vertices(ctx.get(), 1, m > 0 ? m : 1, rows.data(), epsilon, max_v, verts.data(), &count, nullptr, &status));
    if (status != ANET_POLYTOPE_TRUNCATED || count <= max_v) break;
    max_v = count;  // a degenerate polytope with more than 2 rows - 4 vertices: once more with room for all
  }
  verts.resize((size_t)(count < max_v ? count : max_v) * 3);
  return status != ANET_POLYTOPE_SKIPPED;
}
}  // namespace detail

template <typename M0, typename M1>
inline void filterVs(const M0 &rV, const double &epsilon, M1 &fV) {
  const int n = (int)rV.cols();
  std::vector<double> p((size_t)n * 3);
  for (int i = 0; i < n; ++i)
    for (int r = 0; r < 3; ++r) p[(size_t)3 * i + r] = rV(r, i);
  const std::vector<int> kept = detail::merge_points(p, epsilon);
  fV.resize(3, (int)kept.size());
  for (size_t q = 0; q < kept.size(); ++q)
    for (int r = 0; r < 3; ++r) fV(r, (int)q) = p[(size_t)3 * kept[q] + r];
}

template <typename Poly>
inline bool enumerateVs(const Poly &hPoly, std::vector<std::array<double, 3>> &vPoly, const double epsilon = 1.0e-6) {
  std::vector<double> v;
  const bool ok = detail::vertices_of(hPoly, epsilon, v);
  vPoly.resize(v.size() / 3);
  for (size_t q = 0; q < vPoly.size(); ++q) vPoly[q] = {{v[3 * q], v[3 * q + 1], v[3 * q + 2]}};
  return ok;
}

template <typename Poly, typename VP, typename = typename std::enable_if<!std::is_arithmetic<VP>::value>::type>
inline bool enumerateVs(const Poly &hPoly, VP &vPoly, const double epsilon = 1.0e-6) {
  std::vector<double> v;
  const bool ok = detail::vertices_of(hPoly, epsilon, v);
  const int n = (int)(v.size() / 3);
  vPoly.resize(3, n);
  for (int q = 0; q < n; ++q)
    for (int r = 0; r < 3; ++r) vPoly(r, q) = v[(size_t)3 * q + r];
  return ok;
}

template <typename Poly, typename V3, typename VP, typename = typename std::enable_if<!std::is_arithmetic<VP>::value>::type>
inline void enumerateVs(const Poly &hPoly, const V3 &inner, VP &vPoly, const double epsilon = 1.0e-6) {
  (void)inner;
  (void)enumerateVs(hPoly, vPoly, epsilon);
}

}  // namespace geo_utils
