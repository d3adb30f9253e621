// Stop within known space: the penalty that couples speed with the distance field of the voxel map, and its sampled margin
// (include/allocnet_amd.h; kernels in stop_kernels.h).
#include "api_internal.h"
#include "minco_core.h"  // with_order
#include "stop_kernels.h"

static_assert(anet::kStopMaxPieces == ANET_MAX_PIECES, "the LDS image of k_minco_stop holds ANET_MAX_PIECES pieces");
static_assert(anet::kDistNone == ANET_DIST_NONE, "the sentinel of the kernels is the header's");

namespace {

// oc = origin + 0.5 scale, as voxel_map.hpp's constructor forms it (and api_distance.hip for the same field)
bool dist_grid_of(const anet_voxel_grid *g, anet::DistGrid *out) {
#pragma clang fp contract(off)
  if (!voxel_grid_ok(g)) return false;
  for (int c = 0; c < 3; ++c) {
    out->size[c] = g->size[c];
    out->oc[c] = g->origin[c] + 0.5 * g->scale;
  }
  out->scale = g->scale;
  return true;
}

// `penalty`: w and smooth_mu are read (the margin forms do not read them)
int check_stop_penalty(anet_ctx *ctx, const anet_stop_penalty *q, bool penalty) {
  if (!q) return fail(ctx, ANET_ERR_INVALID, "anet_stop_penalty is NULL");
  if (penalty && (!(q->w >= 0.0) || !(q->w < INFINITY))) return fail(ctx, ANET_ERR_INVALID, "anet_stop_penalty.w must be finite and >= 0");
  if (penalty && (!(q->smooth_mu > 0.0) || !(q->smooth_mu < INFINITY)))
    return fail(ctx, ANET_ERR_INVALID, "anet_stop_penalty.smooth_mu must be finite and > 0");
  if (!(fabs(q->clearance) < INFINITY)) return fail(ctx, ANET_ERR_INVALID, "anet_stop_penalty.clearance must be finite");
  if (!(q->a_brake > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_stop_penalty.a_brake must be > 0 (+inf allowed)");
  if (!(q->t_react >= 0.0) || !(q->t_react < INFINITY)) return fail(ctx, ANET_ERR_INVALID, "anet_stop_penalty.t_react must be finite and >= 0");
  if (!(q->speed_eps >= 0.0) || !(q->speed_eps < INFINITY))
    return fail(ctx, ANET_ERR_INVALID, "anet_stop_penalty.speed_eps must be finite and >= 0");
  if (penalty && q->t_react > 0.0 && !(q->speed_eps > 0.0))
    return fail(ctx, ANET_ERR_INVALID, "anet_stop_penalty.speed_eps must be > 0 when t_react > 0");
  if (q->res < 1) return fail(ctx, ANET_ERR_INVALID, "anet_stop_penalty.res must be >= 1");
  return ANET_OK;
}

anet::StopTerm to_dev(const anet_stop_penalty *q) {
  return anet::StopTerm{q->clearance, q->t_react, q->speed_eps * q->speed_eps, 0.5 / q->a_brake, 1.0 / q->a_brake};
}

// what the three entry points share: order, piece count, batch, penalty, grid
int check_args(anet_ctx *ctx, const char *who, const anet_stop_penalty *pen, bool penalty, int s, int n_pieces, int64_t batch,
               const anet_voxel_grid *grid, anet::DistGrid *g) {
  if (s < 2 || s > 4) return fail(ctx, ANET_ERR_UNSUPPORTED, std::string(who) + ": order s must be 2, 3 or 4");
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_stop_penalty(ctx, pen, penalty))) return rc;
  if (!dist_grid_of(grid, g)) return fail(ctx, ANET_ERR_INVALID, std::string(who) + ": bad grid (size >= 1, voxels < 2^31, scale > 0)");
  if (batch > INT32_MAX) return fail(ctx, ANET_ERR_INVALID, std::string(who) + ": batch too large");
  return ANET_OK;
}

}  // namespace

extern "C" {

int anet_minco_stop_partial_grads_dev(anet_ctx *ctx, const anet_stop_penalty *pen, int s, int n_pieces, int64_t batch, int64_t ld,
                                      const double *coeffs, const double *T, const anet_voxel_grid *grid, const int32_t *sd2,
                                      int accumulate, double *gdC, double *gdT, double *piece_cost, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::DistGrid g;
  int rc = check_args(ctx, "anet_minco_stop_partial_grads_dev", pen, true, s, n_pieces, batch, grid, &g);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !sd2 || !gdC || !gdT || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_stop_partial_grads_dev: NULL pointer or ld < batch");
  anet::StopArgs a{coeffs, T, sd2, gdC, gdT, piece_cost, batch, ld, n_pieces, pen->res, accumulate ? 1 : 0, pen->w, pen->smooth_mu,
                   to_dev(pen), g};
  const dim3 grd((unsigned)batch), block(anet::kStopBlock);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_minco_stop<decltype(o)::value>, grd, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_stop_margin_dev(anet_ctx *ctx, const anet_stop_penalty *pen, int s, int n_pieces, int64_t batch, int64_t ld,
                              const double *coeffs, const double *T, const anet_voxel_grid *grid, const int32_t *sd2, double *margin,
                              double *t, double *speed, double *dist, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet::DistGrid g;
  int rc = check_args(ctx, "anet_traj_stop_margin_dev", pen, false, s, n_pieces, batch, grid, &g);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !sd2 || !margin || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_stop_margin_dev: NULL pointer or ld < batch");
  anet::StopMarginArgs a{coeffs, T, sd2, margin, t, speed, dist, batch, ld, n_pieces, pen->res, to_dev(pen), g};
  const dim3 grd((unsigned)((batch + anet::kStopMarginBlock - 1) / anet::kStopMarginBlock), (unsigned)n_pieces),
      block(anet::kStopMarginBlock);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_traj_stop_margin<decltype(o)::value>, grd, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_stop_margin(anet_ctx *ctx, const anet_stop_penalty *pen, int s, int n_pieces, int64_t batch, const double *coeffs,
                          const double *T, const anet_voxel_grid *grid, const int32_t *sd2, double *margin, double *t, double *speed,
                          double *dist) {
  ANET_ON_DEVICE(ctx);
  anet::DistGrid g;
  int rc = check_args(ctx, "anet_traj_stop_margin", pen, false, s, n_pieces, batch, grid, &g);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !sd2 || !margin) return fail(ctx, ANET_ERR_INVALID, "anet_traj_stop_margin: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_m, *d_t, *d_s, *d_d;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T);
    p.out(n_pieces, &d_m); p.out(n_pieces, &d_t); p.out(n_pieces, &d_s); p.out(n_pieces, &d_d);
  });
  if (rc) return rc;
  rc = anet_traj_stop_margin_dev(ctx, pen, s, n_pieces, batch, st.ld, d_co, d_T, grid, sd2, d_m, t ? d_t : nullptr,
                                 speed ? d_s : nullptr, dist ? d_d : nullptr, ctx->stream);
  if (rc) return rc;
  if ((rc = st.download(d_m, n_pieces, margin))) return rc;
  if (t && (rc = st.download(d_t, n_pieces, t))) return rc;
  if (speed && (rc = st.download(d_s, n_pieces, speed))) return rc;
  if (dist && (rc = st.download(d_d, n_pieces, dist))) return rc;
  return ANET_OK;
}

}  // extern "C"
