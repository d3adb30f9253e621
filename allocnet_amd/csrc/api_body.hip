// Whole-body corridor terms: the vertices of a body-fixed polytope, rotated by the attitude of the flatness map, against the
// corridor rows -- partial gradients of the penalty and the sampled margin (include/allocnet_amd.h; kernels in body_kernels.h).
#include "api_internal.h"
#include "body_kernels.h"

namespace {

int check_body(anet_ctx *ctx, const anet_flat_params *p, const anet_body_penalty *q, bool penalty) {
  if (!p) return fail(ctx, ANET_ERR_INVALID, "anet_flat_params is NULL");
  if (!(p->mass > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_flat_params.mass must be > 0");
  if (!(p->speed_eps > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_flat_params.speed_eps must be > 0");
  if (!q) return fail(ctx, ANET_ERR_INVALID, "anet_body_penalty is NULL");
  if (q->n_verts < 1 || q->n_verts > ANET_MAX_BODY_VERTS)
    return fail(ctx, ANET_ERR_INVALID, "anet_body_penalty.n_verts must be in [1, ANET_MAX_BODY_VERTS]");
  if (q->res < 1 || q->res > kBasisTableMaxRes)
    return fail(ctx, ANET_ERR_INVALID, "anet_body_penalty.res must be in [1, 4096]");
  if (q->poly_rows < 1 || q->poly_rows > ANET_MAX_POLY_ROWS)
    return fail(ctx, ANET_ERR_INVALID, "anet_body_penalty.poly_rows must be in [1, ANET_MAX_POLY_ROWS]");
  for (int k = 0; k < q->n_verts; ++k)
    for (int c = 0; c < 3; ++c)
      if (!(fabs(q->verts[k][c]) < INFINITY)) return fail(ctx, ANET_ERR_INVALID, "anet_body_penalty.verts must be finite");
  if (penalty && !(q->smooth_mu > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_body_penalty.smooth_mu must be > 0");
  return ANET_OK;
}

anet::FlatParams to_dev(const anet_flat_params *p) {
  return anet::FlatParams{p->mass, p->grav, p->horiz_drag, p->vert_drag, p->paras_drag, p->speed_eps};
}

anet::BodyVerts to_dev(const anet_body_penalty *q) {
  anet::BodyVerts v;
  v.K = q->n_verts;
  double r2 = 0.0;
  for (int k = 0; k < anet::kMaxBodyVerts; ++k)
    for (int c = 0; c < 3; ++c) v.b[k][c] = k < q->n_verts ? q->verts[k][c] : 0.0;
  for (int k = 0; k < q->n_verts; ++k) r2 = fmax(r2, v.b[k][0] * v.b[k][0] + v.b[k][1] * v.b[k][1] + v.b[k][2] * v.b[k][2]);
  // rounded up by a few ulps: the row test of k_body_piece_grad must never drop a term that is active
  v.rmax = sqrt(r2) * (1.0 + 8.0 * 2.220446049250313e-16);
  return v;
}

}  // namespace

extern "C" {

int anet_minco_body_partial_grads_dev(anet_ctx *ctx, const anet_flat_params *params, const anet_body_penalty *pen, int s,
                                      int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                                      const double *hpolys, int accumulate, double *gdC, double *gdT, double *piece_cost,
                                      void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_body(ctx, params, pen, true))) return rc;
  if (s != 3 && s != 4)
    return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_minco_body_partial_grads_dev: order s must be 3 or 4 (the map needs the jerk)");
  if (!hpolys) return fail(ctx, ANET_ERR_INVALID, "anet_minco_body_partial_grads_dev: hpolys is NULL");
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !gdC || !gdT || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_body_partial_grads_dev: NULL pointer or ld < batch");
  hipStream_t st = (hipStream_t)stream;
  const double *tab = nullptr;
  if ((rc = basis_table(ctx, s, pen->res, st, &tab))) return rc;
  anet::BodyPieceGradArgs a{coeffs, T, hpolys, gdC, gdT, piece_cost, batch, ld, n_pieces, accumulate ? 1 : 0, pen->res,
                            pen->poly_rows, pen->w_body, pen->smooth_mu, to_dev(params), to_dev(pen)};
  const dim3 grid((unsigned)((batch + 255) / 256), (unsigned)n_pieces), block(256);
  if (s == 3) hipLaunchKernelGGL(anet::k_body_piece_grad<3>, grid, block, 0, st, a, tab);
  else hipLaunchKernelGGL(anet::k_body_piece_grad<4>, grid, block, 0, st, a, tab);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_body_margin_dev(anet_ctx *ctx, const anet_flat_params *params, const anet_body_penalty *pen, int s, int n_pieces,
                              int64_t batch, int64_t ld, const double *coeffs, const double *T, const double *hpolys,
                              double *margin, double *t, int32_t *row, int32_t *vert, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_body(ctx, params, pen, false))) return rc;
  if (!hpolys) return fail(ctx, ANET_ERR_INVALID, "anet_traj_body_margin_dev: hpolys is NULL");
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !margin || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_body_margin_dev: NULL pointer or ld < batch");
  anet::BodyMarginArgs a{coeffs, T, hpolys, margin, t, row, vert, batch, ld, n_pieces, pen->res, pen->poly_rows, to_dev(params),
                         to_dev(pen)};
  const dim3 grid((unsigned)((batch + 63) / 64), (unsigned)n_pieces), block(64);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_traj_body_margin<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_body_margin(anet_ctx *ctx, const anet_flat_params *params, const anet_body_penalty *pen, int s, int n_pieces,
                          int64_t batch, const double *coeffs, const double *T, const double *hpolys, double *margin, double *t,
                          int32_t *row, int32_t *vert) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_body(ctx, params, pen, false))) return rc;
  if (!hpolys) return fail(ctx, ANET_ERR_INVALID, "anet_traj_body_margin: hpolys is NULL");
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !margin) return fail(ctx, ANET_ERR_INVALID, "anet_traj_body_margin: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s, nrow = (int64_t)n_pieces * pen->poly_rows * 4;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_hp, *d_m, *d_t;
  int32_t *d_row, *d_vert;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T); p.in(hpolys, nrow, &d_hp);
    p.out(n_pieces, &d_m); p.out(n_pieces, &d_t); p.rows(n_pieces, &d_row); p.rows(n_pieces, &d_vert);
  });
  if (rc) return rc;
  rc = anet_traj_body_margin_dev(ctx, params, pen, s, n_pieces, batch, st.ld, d_co, d_T, d_hp, d_m, t ? d_t : nullptr,
                                 row ? d_row : nullptr, vert ? d_vert : nullptr, ctx->stream);
  if (rc) return rc;
  if ((rc = st.download(d_m, n_pieces, margin))) return rc;
  if (t && (rc = st.download(d_t, n_pieces, t))) return rc;
  if (row && (rc = st.download_rows(d_row, n_pieces, row))) return rc;
  if (vert && (rc = st.download_rows(d_vert, n_pieces, vert))) return rc;
  return ANET_OK;
}

}  // extern "C"
