// Yaw trajectories: the one-axis MINCO (solve and adjoint), the field-of-view / yaw-rate / yaw-effort penalty that couples it to
// the position trajectory, its sampled margin, and flat states that use the yaw (include/allocnet_amd.h; kernels in yaw_kernels.h).
#include "api_internal.h"
#include "minco_core.h"  // with_order
#include "yaw_kernels.h"

static_assert(anet::kYawMaxPieces == ANET_MAX_PIECES, "the LDS image of k_minco_yaw and the one-axis MINCO hold ANET_MAX_PIECES pieces");

namespace {

constexpr double kHalfPi = 1.57079632679489661923;

// `penalty`: the weights, mu and speed_eps are read (the margin reads half_fov and res only)
int check_yaw_penalty(anet_ctx *ctx, const anet_yaw_penalty *q, bool penalty) {
  if (!q) return fail(ctx, ANET_ERR_INVALID, "anet_yaw_penalty is NULL");
  if (!(q->half_fov > 0.0) || !(q->half_fov <= kHalfPi)) return fail(ctx, ANET_ERR_INVALID, "anet_yaw_penalty.half_fov must be in (0, pi/2]");
  if (q->res < 1) return fail(ctx, ANET_ERR_INVALID, "anet_yaw_penalty.res must be >= 1");
  if (!penalty) return ANET_OK;
  auto weight = [](double w) { return w >= 0.0 && w < INFINITY; };
  if (!weight(q->w_look) || !weight(q->w_rate) || !weight(q->w_energy))
    return fail(ctx, ANET_ERR_INVALID, "anet_yaw_penalty: the weights must be finite and >= 0");
  if (q->w_look > 0.0 && (!(q->mu_look > 0.0) || !(q->mu_look < INFINITY) || !(q->speed_eps > 0.0) || !(q->speed_eps < INFINITY)))
    return fail(ctx, ANET_ERR_INVALID, "anet_yaw_penalty: mu_look and speed_eps must be finite and > 0 when w_look > 0");
  if (q->w_rate > 0.0 && (!(q->mu_rate > 0.0) || !(q->mu_rate < INFINITY)))
    return fail(ctx, ANET_ERR_INVALID, "anet_yaw_penalty.mu_rate must be finite and > 0 when w_rate > 0");
  if (!(q->max_rate > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_yaw_penalty.max_rate must be > 0 (+inf allowed)");
  return ANET_OK;
}

// what the trajectory entry points share: both orders, piece count, batch
int check_orders(anet_ctx *ctx, const char *who, int s, int sy, int n_pieces, int64_t batch) {
  if (s < 2 || s > 4 || sy < 2 || sy > 4) return fail(ctx, ANET_ERR_UNSUPPORTED, std::string(who) + ": orders s and sy must be 2, 3 or 4");
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (batch > INT32_MAX) return fail(ctx, ANET_ERR_INVALID, std::string(who) + ": batch too large");
  return ANET_OK;
}

// f(integral_constant<S>, integral_constant<SY>)
template <class F>
void with_orders(int s, int sy, F &&f) {
  anet::with_order(s, [&](auto o) { anet::with_order(sy, [&](auto oy) { f(o, oy); }); });
}

int check_flat_params(anet_ctx *ctx, const anet_flat_params *p) {
  if (!p) return fail(ctx, ANET_ERR_INVALID, "anet_flat_params is NULL");
  if (!(p->mass > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_flat_params.mass must be > 0");
  if (!(p->speed_eps > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_flat_params.speed_eps must be > 0");
  return ANET_OK;
}

}  // namespace

extern "C" {

int anet_minco_solve_scalar_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld, const double *head,
                                const double *tail, const double *wps, const double *T, double *coeffs, double *energy, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!head || !tail || !T || (n_pieces > 1 && !wps) || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_solve_scalar_dev: NULL input or ld < batch");
  anet::SolveArgs a{head, tail, wps, T, coeffs, energy, batch, ld, n_pieces, c};
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) {
    constexpr int S = decltype(o)::value, kBlock = anet::kScalarBlock<S>;
    hipLaunchKernelGGL(anet::k_minco_solve_scalar<S>, dim3((unsigned)((batch + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a);
  });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_minco_solve_scalar(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head, const double *tail,
                            const double *wps, const double *T, double *coeffs, double *energy) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!head || !tail || !T || (n_pieces > 1 && !wps)) return fail(ctx, ANET_ERR_INVALID, "anet_minco_solve_scalar: NULL input");
  const int N = n_pieces;
  const int64_t n_co = (int64_t)N * 2 * s;
  Stager st(ctx, batch);
  double *d_head, *d_tail, *d_wps, *d_T, *d_co, *d_en;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(head, c, &d_head); p.in(tail, c, &d_tail); p.in(wps, (int64_t)(N - 1), &d_wps); p.in(T, N, &d_T);
    p.out(n_co, &d_co); p.rows(1, &d_en);
  });
  if (rc) return rc;
  rc = anet_minco_solve_scalar_dev(ctx, s, c, N, batch, st.ld, d_head, d_tail, d_wps, d_T, coeffs ? d_co : nullptr, d_en, ctx->stream);
  if (rc) return rc;
  if (energy) ANET_HIP(ctx, hipMemcpyAsync(energy, d_en, sizeof(double) * batch, hipMemcpyDeviceToHost, ctx->stream));
  if (coeffs) return st.download(d_co, n_co, coeffs);
  ANET_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANET_OK;
}

int anet_minco_propagate_grad_scalar_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld, const double *T,
                                         const double *coeffs, const double *gdC, const double *gdT, double *gradP, double *gradT,
                                         void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!T || !coeffs || !gdC || !gradT || (n_pieces > 1 && !gradP) || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_propagate_grad_scalar_dev: NULL pointer or ld < batch");
  anet::PropArgs a{T, coeffs, gdC, gdT, gradP, gradT, nullptr, nullptr, nullptr, 0.0, batch, ld, n_pieces, c};
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) {
    constexpr int S = decltype(o)::value, kBlock = anet::kScalarBlock<S>;
    hipLaunchKernelGGL(anet::k_minco_propagate_scalar<S>, dim3((unsigned)((batch + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a);
  });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_minco_yaw_partial_grads_dev(anet_ctx *ctx, const anet_yaw_penalty *pen, int s, int sy, int n_pieces, int64_t batch, int64_t ld,
                                     const double *coeffs, const double *ycoeffs, const double *T, int accumulate, double *gdC,
                                     double *gdCy, double *gdT, double *piece_cost, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_orders(ctx, "anet_minco_yaw_partial_grads_dev", s, sy, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_yaw_penalty(ctx, pen, true))) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !ycoeffs || !T || !gdC || !gdCy || !gdT || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_yaw_partial_grads_dev: NULL pointer or ld < batch");
  const anet::YawTerm k{pen->w_look, pen->mu_look, cos(pen->half_fov), pen->speed_eps * pen->speed_eps,
                        pen->w_rate, pen->mu_rate, pen->max_rate * pen->max_rate, pen->w_energy};
  anet::YawArgs a{coeffs, ycoeffs, T, gdC, gdCy, gdT, piece_cost, batch, ld, n_pieces, pen->res, accumulate ? 1 : 0, k};
  const dim3 grd((unsigned)batch), block(anet::kYawBlock);
  hipStream_t st = (hipStream_t)stream;
  with_orders(s, sy, [&](auto o, auto oy) {
    hipLaunchKernelGGL((anet::k_minco_yaw<decltype(o)::value, decltype(oy)::value>), grd, block, 0, st, a);
  });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_yaw_margin_dev(anet_ctx *ctx, const anet_yaw_penalty *pen, double v_min, int s, int sy, int n_pieces, int64_t batch,
                             int64_t ld, const double *coeffs, const double *ycoeffs, const double *T, double *margin, double *t,
                             double *rate, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_orders(ctx, "anet_traj_yaw_margin_dev", s, sy, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_yaw_penalty(ctx, pen, false))) return rc;
  if (!(v_min >= 0.0) || !(v_min < INFINITY)) return fail(ctx, ANET_ERR_INVALID, "anet_traj_yaw_margin_dev: v_min must be finite and >= 0");
  if (batch == 0) return ANET_OK;
  if (!coeffs || !ycoeffs || !T || !margin || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_yaw_margin_dev: NULL pointer or ld < batch");
  anet::YawMarginArgs a{coeffs, ycoeffs, T, margin, t, rate, batch, ld, n_pieces, pen->res, pen->half_fov, v_min};
  const dim3 grd((unsigned)((batch + anet::kYawMarginBlock - 1) / anet::kYawMarginBlock), (unsigned)n_pieces),
      block(anet::kYawMarginBlock);
  hipStream_t st = (hipStream_t)stream;
  with_orders(s, sy, [&](auto o, auto oy) {
    hipLaunchKernelGGL((anet::k_traj_yaw_margin<decltype(o)::value, decltype(oy)::value>), grd, block, 0, st, a);
  });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_yaw_margin(anet_ctx *ctx, const anet_yaw_penalty *pen, double v_min, int s, int sy, int n_pieces, int64_t batch,
                         const double *coeffs, const double *ycoeffs, const double *T, double *margin, double *t, double *rate) {
  ANET_ON_DEVICE(ctx);
  int rc = check_orders(ctx, "anet_traj_yaw_margin", s, sy, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !ycoeffs || !T || !margin) return fail(ctx, ANET_ERR_INVALID, "anet_traj_yaw_margin: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s, ncy = (int64_t)n_pieces * 2 * sy;
  Stager st(ctx, batch);
  double *d_co, *d_cy, *d_T, *d_m, *d_t, *d_r;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(coeffs, nco, &d_co); p.in(ycoeffs, ncy, &d_cy); p.in(T, n_pieces, &d_T);
    p.out(n_pieces, &d_m); p.out(n_pieces, &d_t); p.out(n_pieces, &d_r);
  });
  if (rc) return rc;
  rc = anet_traj_yaw_margin_dev(ctx, pen, v_min, s, sy, n_pieces, batch, st.ld, d_co, d_cy, d_T, d_m, t ? d_t : nullptr,
                                rate ? d_r : nullptr, ctx->stream);
  if (rc) return rc;
  if ((rc = st.download(d_m, n_pieces, margin))) return rc;
  if (t && (rc = st.download(d_t, n_pieces, t))) return rc;
  if (rate && (rc = st.download(d_r, n_pieces, rate))) return rc;
  return ANET_OK;
}

int anet_traj_states_yaw_dev(anet_ctx *ctx, const anet_flat_params *params, int s, int sy, int n_pieces, int64_t batch, int64_t ld,
                                  const double *coeffs, const double *ycoeffs, const double *T, int nq, const double *tq, double *out,
                                  void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_orders(ctx, "anet_traj_states_yaw_dev", s, sy, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_flat_params(ctx, params))) return rc;
  if (nq < 0) return fail(ctx, ANET_ERR_INVALID, "anet_traj_states_yaw: nq >= 0");
  if (batch == 0 || nq == 0) return ANET_OK;
  if (!coeffs || !ycoeffs || !T || !tq || !out || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_states_yaw_dev: NULL pointer or ld < batch");
  const anet::FlatParams fp{params->mass, params->grav, params->horiz_drag, params->vert_drag, params->paras_drag, params->speed_eps};
  anet::FlatStatesYawArgs a{coeffs, ycoeffs, T, tq, out, batch, ld, n_pieces, nq, fp};
  const dim3 grid((unsigned)((batch + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  with_orders(s, sy, [&](auto o, auto oy) {
    hipLaunchKernelGGL((anet::k_traj_flat_states_yaw<decltype(o)::value, decltype(oy)::value>), grid, block, 0, st, a);
  });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_states_yaw(anet_ctx *ctx, const anet_flat_params *params, int s, int sy, int n_pieces, int64_t batch,
                              const double *coeffs, const double *ycoeffs, const double *T, int nq, const double *tq, double *out) {
  ANET_ON_DEVICE(ctx);
  int rc = check_orders(ctx, "anet_traj_states_yaw", s, sy, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0 || nq <= 0) return nq < 0 ? fail(ctx, ANET_ERR_INVALID, "nq < 0") : ANET_OK;
  if (!coeffs || !ycoeffs || !T || !tq || !out) return fail(ctx, ANET_ERR_INVALID, "anet_traj_states_yaw: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s, ncy = (int64_t)n_pieces * 2 * sy, nout = (int64_t)nq * anet::kFlatStateFields;
  Stager st(ctx, batch);
  double *d_co, *d_cy, *d_T, *d_tq, *d_out;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(coeffs, nco, &d_co); p.in(ycoeffs, ncy, &d_cy); p.in(T, n_pieces, &d_T); p.in(tq, nq, &d_tq); p.out(nout, &d_out);
  });
  if (rc) return rc;
  rc = anet_traj_states_yaw_dev(ctx, params, s, sy, n_pieces, batch, st.ld, d_co, d_cy, d_T, nq, d_tq, d_out, ctx->stream);
  if (rc) return rc;
  return st.download(d_out, nout, out);
}

}  // extern "C"
