// Exact margins of trajectories against corridor and box-limit rows (include/allocnet_amd.h; semantics, pruning and tolerance in
// corridor_margin_kernels.h).
#include "api_internal.h"
#include "minco_core.h"
#include "corridor_margin_kernels.h"

namespace {

int check_args(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int deriv, int poly_rows) {
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (deriv < 0 || deriv > 2) return fail(ctx, ANET_ERR_INVALID, "anet_traj_row_margin: deriv must be 0, 1 or 2");
  if (poly_rows < 1 || poly_rows > ANET_MAX_POLY_ROWS)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_row_margin: poly_rows must be in [1, ANET_MAX_POLY_ROWS]");
  return ANET_OK;
}

}  // namespace

extern "C" {

int anet_traj_row_margin_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                             int deriv, int poly_rows, const double *rows, double *margin, int32_t *row, double *t, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_args(ctx, s, n_pieces, batch, deriv, poly_rows);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !rows || !margin || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_row_margin_dev: NULL pointer or ld < batch");
  anet::MarginArgs a{coeffs, T, rows, margin, row, t, batch, ld, n_pieces, poly_rows, deriv};
  const dim3 grid((unsigned)((batch + 63) / 64), (unsigned)n_pieces), block(64);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_traj_row_margin<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_row_margin(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs, const double *T, int deriv,
                         int poly_rows, const double *rows, double *margin, int32_t *row, double *t) {
  ANET_ON_DEVICE(ctx);
  int rc = check_args(ctx, s, n_pieces, batch, deriv, poly_rows);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !rows || !margin) return fail(ctx, ANET_ERR_INVALID, "anet_traj_row_margin: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s, nrow = (int64_t)n_pieces * poly_rows * 4;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_rows, *d_m, *d_t;
  int32_t *d_row;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T); p.in(rows, nrow, &d_rows);
    p.out(n_pieces, &d_m); p.out(n_pieces, &d_t); p.rows(n_pieces, &d_row);
  });
  if (rc) return rc;
  rc = anet_traj_row_margin_dev(ctx, s, n_pieces, batch, st.ld, d_co, d_T, deriv, poly_rows, d_rows, d_m, row ? d_row : nullptr,
                                t ? d_t : nullptr, ctx->stream);
  if (rc) return rc;
  if ((rc = st.download(d_m, n_pieces, margin))) return rc;
  if (t && (rc = st.download(d_t, n_pieces, t))) return rc;
  if (row && (rc = st.download_rows(d_row, n_pieces, row))) return rc;
  return ANET_OK;
}

}  // extern "C"
