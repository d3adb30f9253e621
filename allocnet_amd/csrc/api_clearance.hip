// Exact clearance of trajectories to obstacle points (include/allocnet_amd.h; semantics, procedure and accuracy in
// clearance_kernels.h).
#include "api_internal.h"
#include "minco_core.h"
#include "clearance_kernels.h"

namespace {

int check_args(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int n_sets, int64_t max_points) {
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (n_sets != 1 && n_sets != n_pieces)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_clearance: n_sets must be 1 (a shared cloud) or n_pieces (one set per piece)");
  if (max_points < 0 || max_points > INT32_MAX)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_clearance: max_points must be in [0, 2^31)");
  return ANET_OK;
}

}  // namespace

extern "C" {

int anet_traj_clearance_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                            int n_sets, int64_t max_points, const double *points, const int32_t *counts, double *clearance,
                            int32_t *point, double *t, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_args(ctx, s, n_pieces, batch, n_sets, max_points);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !clearance || (!points && max_points > 0) || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_clearance_dev: NULL pointer or ld < batch");
  anet::ClearanceArgs a{coeffs, T, points, counts, clearance, point, t, batch, ld, max_points, n_pieces, n_sets == n_pieces && n_pieces > 1};
  const dim3 grid((unsigned)((batch + 63) / 64), (unsigned)n_pieces), block(64);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_traj_clearance<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_clearance(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs, const double *T, int n_sets,
                        int64_t max_points, const double *points, const int32_t *counts, double *clearance, int32_t *point,
                        double *t) {
  ANET_ON_DEVICE(ctx);
  int rc = check_args(ctx, s, n_pieces, batch, n_sets, max_points);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !clearance || (!points && max_points > 0)) return fail(ctx, ANET_ERR_INVALID, "anet_traj_clearance: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s, npt = (int64_t)n_sets * max_points * 3;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_pts, *d_c, *d_t, *d_counts;
  int32_t *d_point;
  // the counts travel as whole doubles, two int32 each, through the same checked copy as the points
  std::vector<double> packed_counts(counts ? (size_t)(n_sets + 1) / 2 : 0, 0.0);
  if (counts) memcpy(packed_counts.data(), counts, sizeof(int32_t) * (size_t)n_sets);
  rc = st.stage([&](Stager::Pass &p) {
    p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T);
    p.out(n_pieces, &d_c); p.out(n_pieces, &d_t); p.rows(n_pieces, &d_point);
    p.shared(points, npt, &d_pts);
    p.shared(packed_counts.data(), (int64_t)packed_counts.size(), &d_counts);
  });
  if (rc) return rc;
  rc = anet_traj_clearance_dev(ctx, s, n_pieces, batch, st.ld, d_co, d_T, n_sets, max_points, d_pts,
                               counts ? (const int32_t *)d_counts : nullptr, d_c, point ? d_point : nullptr, t ? d_t : nullptr, ctx->stream);
  if (rc) return rc;
  if ((rc = st.download(d_c, n_pieces, clearance))) return rc;
  if (t && (rc = st.download(d_t, n_pieces, t))) return rc;
  if (point && (rc = st.download_rows(d_point, n_pieces, point))) return rc;
  return ANET_OK;
}

}  // extern "C"
