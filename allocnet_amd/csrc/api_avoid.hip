// Trajectory-avoidance penalty of the MINCO objective against neighbours of another set of trajectories (include/allocnet_amd.h).
#include "api_internal.h"
#include "minco_core.h"  // with_order
#include "avoid_kernels.h"

static_assert(anet::kAvoidMaxPieces == ANET_MAX_PIECES, "the LDS images of k_minco_avoid hold ANET_MAX_PIECES pieces");

namespace {

int check_avoid_penalty(anet_ctx *ctx, const anet_avoid_penalty *q) {
  if (!q) return fail(ctx, ANET_ERR_INVALID, "anet_avoid_penalty is NULL");
  if (!(q->w >= 0.0) || !(q->w < INFINITY)) return fail(ctx, ANET_ERR_INVALID, "anet_avoid_penalty.w must be finite and >= 0");
  if (!(q->smooth_mu > 0.0) || !(q->smooth_mu < INFINITY))
    return fail(ctx, ANET_ERR_INVALID, "anet_avoid_penalty.smooth_mu must be finite and > 0");
  if (!(q->min_dist > 0.0) || !(q->min_dist < INFINITY))
    return fail(ctx, ANET_ERR_INVALID, "anet_avoid_penalty.min_dist must be finite and > 0");
  if (!(q->z_scale > 0.0) || !(q->z_scale < INFINITY))
    return fail(ctx, ANET_ERR_INVALID, "anet_avoid_penalty.z_scale must be finite and > 0");
  if (q->res < 1) return fail(ctx, ANET_ERR_INVALID, "anet_avoid_penalty.res must be >= 1");
  return ANET_OK;
}

}  // namespace

extern "C" {

int anet_minco_avoid_partial_grads_dev(anet_ctx *ctx, const anet_avoid_penalty *pen, int s, int n_pieces, int64_t batch, int64_t ld,
                                       const double *coeffs, const double *T, const double *t0, int o_pieces, int64_t o_batch,
                                       int64_t o_ld, const double *o_coeffs, const double *o_T, const double *o_t0,
                                       const int32_t *nbr_start, const int32_t *nbr, int accumulate, double *gdC, double *gdT,
                                       double *piece_cost, double *gd_t0, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (s < 2 || s > 4) return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_minco_avoid_partial_grads_dev: order s must be 2, 3 or 4");
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_avoid_penalty(ctx, pen))) return rc;
  if (o_pieces < 1 || o_pieces > ANET_MAX_PIECES)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_avoid_partial_grads_dev: o_pieces must be in [1, ANET_MAX_PIECES]");
  if (o_batch < 0 || batch > INT32_MAX) return fail(ctx, ANET_ERR_INVALID, "anet_minco_avoid_partial_grads_dev: bad batch or o_batch");
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !o_coeffs || !o_T || !nbr_start || !nbr || !gdC || !gdT || ld < batch || o_ld < o_batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_avoid_partial_grads_dev: NULL pointer, ld < batch or o_ld < o_batch");
  anet::AvoidArgs a{coeffs, T, t0, o_coeffs, o_T, o_t0, nbr_start, nbr, gdC, gdT, piece_cost, gd_t0, batch, ld, o_batch, o_ld,
                    n_pieces, o_pieces, pen->res, accumulate ? 1 : 0, pen->w, pen->smooth_mu, pen->min_dist * pen->min_dist,
                    1.0 / (pen->z_scale * pen->z_scale)};
  const dim3 grid((unsigned)batch), block(anet::kAvoidBlock);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_minco_avoid<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

}  // extern "C"
