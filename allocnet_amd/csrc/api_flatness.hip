// Differential flatness: pointwise map and adjoint, states and sampled limits along trajectories, the thrust / tilt / body-rate
// penalty of the MINCO objective (include/allocnet_amd.h).
#include "api_internal.h"
#include "flatness_kernels.h"

namespace {

constexpr double kPi = 3.14159265358979323846;

int check_flat_params(anet_ctx *ctx, const anet_flat_params *p) {
  if (!p) return fail(ctx, ANET_ERR_INVALID, "anet_flat_params is NULL");
  if (!(p->mass > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_flat_params.mass must be > 0");
  if (!(p->speed_eps > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_flat_params.speed_eps must be > 0");
  return ANET_OK;
}

int check_flat_penalty(anet_ctx *ctx, const anet_flat_penalty *q) {
  if (!q) return fail(ctx, ANET_ERR_INVALID, "anet_flat_penalty is NULL");
  if (!(q->smooth_mu > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_flat_penalty.smooth_mu must be > 0");
  if (q->res < 1) return fail(ctx, ANET_ERR_INVALID, "anet_flat_penalty.res must be >= 1");
  if (!(q->min_thrust < q->max_thrust)) return fail(ctx, ANET_ERR_INVALID, "anet_flat_penalty: min_thrust < max_thrust required");
  if (!(q->max_tilt > 0.0 && q->max_tilt < kPi)) return fail(ctx, ANET_ERR_INVALID, "anet_flat_penalty.max_tilt must be in (0, pi)");
  return ANET_OK;
}

anet::FlatParams to_dev(const anet_flat_params *p) {
  return anet::FlatParams{p->mass, p->grav, p->horiz_drag, p->vert_drag, p->paras_drag, p->speed_eps};
}

int check_traj(anet_ctx *ctx, const anet_flat_params *p, int s, int n_pieces, int64_t batch) {
  const int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  return rc ? rc : check_flat_params(ctx, p);
}

}  // namespace

extern "C" {

int anet_flat_forward_dev(anet_ctx *ctx, const anet_flat_params *params, int64_t batch, int64_t ld, const double *vel,
                          const double *acc, const double *jer, const double *psi, const double *dpsi, double *thr, double *quat,
                          double *omg, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_flat_params(ctx, params);
  if (rc) return rc;
  if (batch < 0) return fail(ctx, ANET_ERR_INVALID, "negative batch");
  if (batch == 0) return ANET_OK;
  if (!vel || !acc || !jer || !thr || !quat || !omg || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_flat_forward_dev: NULL pointer or ld < batch");
  anet::FlatFwdArgs a{vel, acc, jer, psi, dpsi, thr, quat, omg, batch, ld, to_dev(params)};
  const dim3 grid((unsigned)((batch + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (psi || dpsi) hipLaunchKernelGGL(anet::k_flat_forward<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(anet::k_flat_forward<false>, grid, block, 0, st, a);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_flat_backward_dev(anet_ctx *ctx, const anet_flat_params *params, int64_t batch, int64_t ld, const double *vel,
                           const double *acc, const double *jer, const double *psi, const double *dpsi, const double *pos_grad,
                           const double *vel_grad, const double *thr_grad, const double *quat_grad, const double *omg_grad,
                           double *pos_total, double *vel_total, double *acc_total, double *jer_total, double *psi_total,
                           double *dpsi_total, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_flat_params(ctx, params);
  if (rc) return rc;
  if (batch < 0) return fail(ctx, ANET_ERR_INVALID, "negative batch");
  if (batch == 0) return ANET_OK;
  if (!vel || !acc || !jer || !thr_grad || !quat_grad || !omg_grad || !vel_total || !acc_total || !jer_total || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_flat_backward_dev: NULL pointer or ld < batch");
  anet::FlatBwdArgs a{vel, acc, jer, psi, dpsi, pos_grad, vel_grad, thr_grad, quat_grad, omg_grad, pos_total, vel_total,
                      acc_total, jer_total, psi_total, dpsi_total, batch, ld, to_dev(params)};
  const dim3 grid((unsigned)((batch + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (psi || dpsi) hipLaunchKernelGGL(anet::k_flat_backward<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(anet::k_flat_backward<false>, grid, block, 0, st, a);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_flat_states_dev(anet_ctx *ctx, const anet_flat_params *params, int s, int n_pieces, int64_t batch, int64_t ld,
                              const double *coeffs, const double *T, int nq, const double *tq, double *out, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_traj(ctx, params, s, n_pieces, batch);
  if (rc) return rc;
  if (nq < 0) return fail(ctx, ANET_ERR_INVALID, "anet_traj_flat_states: nq >= 0");
  if (batch == 0 || nq == 0) return ANET_OK;
  if (!coeffs || !T || !tq || !out || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_flat_states_dev: NULL pointer or ld < batch");
  anet::FlatStatesArgs a{coeffs, T, tq, out, batch, ld, n_pieces, nq, to_dev(params)};
  const dim3 grid((unsigned)((batch + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_traj_flat_states<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_flat_extrema_dev(anet_ctx *ctx, const anet_flat_params *params, int s, int n_pieces, int64_t batch, int64_t ld,
                               const double *coeffs, const double *T, int res, double *out, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_traj(ctx, params, s, n_pieces, batch);
  if (rc) return rc;
  if (res < 1) return fail(ctx, ANET_ERR_INVALID, "anet_traj_flat_extrema: res >= 1");
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !out || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_flat_extrema_dev: NULL pointer or ld < batch");
  anet::FlatExtremaArgs a{coeffs, T, out, batch, ld, n_pieces, res, to_dev(params)};
  const dim3 grid((unsigned)((batch + 63) / 64)), block(64, anet::kFlatExtremaRows);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_traj_flat_extrema<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_minco_flat_partial_grads_dev(anet_ctx *ctx, const anet_flat_params *params, const anet_flat_penalty *pen, int s,
                                      int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                                      int accumulate, double *gdC, double *gdT, double *piece_cost, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_traj(ctx, params, s, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_flat_penalty(ctx, pen))) return rc;
  if (s != 3 && s != 4)
    return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_minco_flat_partial_grads_dev: order s must be 3 or 4 (the map needs the jerk)");
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !gdC || !gdT || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_flat_partial_grads_dev: NULL pointer or ld < batch");
  hipStream_t st = (hipStream_t)stream;
  const double *tab = nullptr;
  if ((rc = basis_table(ctx, s, pen->res, st, &tab))) return rc;
  anet::FlatPieceGradArgs a{coeffs, T, gdC, gdT, piece_cost, batch, ld, n_pieces, accumulate ? 1 : 0, to_dev(params),
                            anet::FlatPenalty{pen->w_thrust, pen->w_tilt, pen->w_bdr, pen->smooth_mu, pen->min_thrust,
                                              pen->max_thrust, cos(pen->max_tilt), pen->max_bdr * pen->max_bdr, pen->res}};
  const dim3 grid((unsigned)((batch + 255) / 256), (unsigned)n_pieces), block(256);
  if (s == 3) hipLaunchKernelGGL(anet::k_flat_piece_grad<3>, grid, block, 0, st, a, tab);
  else hipLaunchKernelGGL(anet::k_flat_piece_grad<4>, grid, block, 0, st, a, tab);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

// ---- host (element- / trajectory-major) variants ------------------------------------------------

int anet_flat_forward(anet_ctx *ctx, const anet_flat_params *params, int64_t batch, const double *vel, const double *acc,
                      const double *jer, const double *psi, const double *dpsi, double *thr, double *quat, double *omg) {
  ANET_ON_DEVICE(ctx);
  int rc = check_flat_params(ctx, params);
  if (rc) return rc;
  if (batch < 0) return fail(ctx, ANET_ERR_INVALID, "negative batch");
  if (batch == 0) return ANET_OK;
  if (!vel || !acc || !jer || !thr || !quat || !omg) return fail(ctx, ANET_ERR_INVALID, "anet_flat_forward: NULL pointer");
  Stager st(ctx, batch);
  double *d_v, *d_a, *d_j, *d_psi = nullptr, *d_dpsi = nullptr, *d_thr, *d_q, *d_o;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(vel, 3, &d_v); p.in(acc, 3, &d_a); p.in(jer, 3, &d_j);
    if (psi) p.in(psi, 1, &d_psi);
    if (dpsi) p.in(dpsi, 1, &d_dpsi);
    p.out(1, &d_thr); p.out(4, &d_q); p.out(3, &d_o);
  });
  if (rc) return rc;
  rc = anet_flat_forward_dev(ctx, params, batch, st.ld, d_v, d_a, d_j, d_psi, d_dpsi, d_thr, d_q, d_o, ctx->stream);
  if (rc) return rc;
  if ((rc = st.download(d_thr, 1, thr))) return rc;
  if ((rc = st.download(d_q, 4, quat))) return rc;
  return st.download(d_o, 3, omg);
}

int anet_flat_backward(anet_ctx *ctx, const anet_flat_params *params, int64_t batch, const double *vel, const double *acc,
                       const double *jer, const double *psi, const double *dpsi, const double *pos_grad, const double *vel_grad,
                       const double *thr_grad, const double *quat_grad, const double *omg_grad, double *pos_total,
                       double *vel_total, double *acc_total, double *jer_total, double *psi_total, double *dpsi_total) {
  ANET_ON_DEVICE(ctx);
  int rc = check_flat_params(ctx, params);
  if (rc) return rc;
  if (batch < 0) return fail(ctx, ANET_ERR_INVALID, "negative batch");
  if (batch == 0) return ANET_OK;
  if (!vel || !acc || !jer || !thr_grad || !quat_grad || !omg_grad || !vel_total || !acc_total || !jer_total)
    return fail(ctx, ANET_ERR_INVALID, "anet_flat_backward: NULL pointer");
  Stager st(ctx, batch);
  double *d_v, *d_a, *d_j, *d_psi = nullptr, *d_dpsi = nullptr, *d_pg = nullptr, *d_vg = nullptr, *d_tg, *d_qg, *d_og;
  double *d_pt, *d_vt, *d_at, *d_jt, *d_pst, *d_dpt;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(vel, 3, &d_v); p.in(acc, 3, &d_a); p.in(jer, 3, &d_j);
    if (psi) p.in(psi, 1, &d_psi);
    if (dpsi) p.in(dpsi, 1, &d_dpsi);
    if (pos_grad) p.in(pos_grad, 3, &d_pg);
    if (vel_grad) p.in(vel_grad, 3, &d_vg);
    p.in(thr_grad, 1, &d_tg); p.in(quat_grad, 4, &d_qg); p.in(omg_grad, 3, &d_og);
    p.out(3, &d_pt); p.out(3, &d_vt); p.out(3, &d_at); p.out(3, &d_jt); p.out(1, &d_pst); p.out(1, &d_dpt);
  });
  if (rc) return rc;
  rc = anet_flat_backward_dev(ctx, params, batch, st.ld, d_v, d_a, d_j, d_psi, d_dpsi, d_pg, d_vg, d_tg, d_qg, d_og, d_pt, d_vt,
                              d_at, d_jt, d_pst, d_dpt, ctx->stream);
  if (rc) return rc;
  if (pos_total && (rc = st.download(d_pt, 3, pos_total))) return rc;
  if ((rc = st.download(d_vt, 3, vel_total))) return rc;
  if ((rc = st.download(d_at, 3, acc_total))) return rc;
  if ((rc = st.download(d_jt, 3, jer_total))) return rc;
  if (psi_total && (rc = st.download(d_pst, 1, psi_total))) return rc;
  if (dpsi_total && (rc = st.download(d_dpt, 1, dpsi_total))) return rc;
  return ANET_OK;
}

int anet_traj_flat_states(anet_ctx *ctx, const anet_flat_params *params, int s, int n_pieces, int64_t batch, const double *coeffs,
                          const double *T, int nq, const double *tq, double *out) {
  ANET_ON_DEVICE(ctx);
  int rc = check_traj(ctx, params, s, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0 || nq <= 0) return nq < 0 ? fail(ctx, ANET_ERR_INVALID, "nq < 0") : ANET_OK;
  if (!coeffs || !T || !tq || !out) return fail(ctx, ANET_ERR_INVALID, "anet_traj_flat_states: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s, nout = (int64_t)nq * anet::kFlatStateFields;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_tq, *d_out;
  rc = st.stage([&](Stager::Pass &p) { p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T); p.in(tq, nq, &d_tq); p.out(nout, &d_out); });
  if (rc) return rc;
  rc = anet_traj_flat_states_dev(ctx, params, s, n_pieces, batch, st.ld, d_co, d_T, nq, d_tq, d_out, ctx->stream);
  if (rc) return rc;
  return st.download(d_out, nout, out);
}

int anet_traj_flat_extrema(anet_ctx *ctx, const anet_flat_params *params, int s, int n_pieces, int64_t batch, const double *coeffs,
                           const double *T, int res, double *out) {
  ANET_ON_DEVICE(ctx);
  int rc = check_traj(ctx, params, s, n_pieces, batch);
  if (rc) return rc;
  if (res < 1) return fail(ctx, ANET_ERR_INVALID, "anet_traj_flat_extrema: res >= 1");
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !out) return fail(ctx, ANET_ERR_INVALID, "anet_traj_flat_extrema: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_out;
  rc = st.stage([&](Stager::Pass &p) { p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T); p.out(4, &d_out); });
  if (rc) return rc;
  rc = anet_traj_flat_extrema_dev(ctx, params, s, n_pieces, batch, st.ld, d_co, d_T, res, d_out, ctx->stream);
  if (rc) return rc;
  return st.download(d_out, 4, out);
}

}  // extern "C"
