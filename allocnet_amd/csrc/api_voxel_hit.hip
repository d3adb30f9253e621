// Exact first collision of trajectories with the device voxel map (include/allocnet_amd.h; semantics, procedure and accuracy in
// voxel_hit_kernels.h).
#include "api_internal.h"
#include "minco_core.h"
#include "voxel_hit_kernels.h"

namespace {

int check_args(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const anet_voxel_grid *grid) {
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (!voxel_grid_ok(grid)) return fail(ctx, ANET_ERR_INVALID, "anet_traj_voxel_hit: bad grid (size >= 1, voxels < 2^31, finite origin, scale > 0)");
  return ANET_OK;
}

}  // namespace

extern "C" {

int anet_traj_voxel_hit_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                            const anet_voxel_grid *grid, const uint8_t *voxels, double *t_hit, int32_t *voxel, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_args(ctx, s, n_pieces, batch, grid);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !voxels || !t_hit || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_voxel_hit_dev: NULL pointer or ld < batch");
  anet::HitArgs a{coeffs, T, voxels, t_hit, voxel, batch, ld, n_pieces, {grid->size[0], grid->size[1], grid->size[2]},
                  {grid->origin[0], grid->origin[1], grid->origin[2]}, grid->scale};
  const dim3 blocks((unsigned)((batch + 63) / 64), (unsigned)n_pieces), block(64);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_traj_voxel_hit<decltype(o)::value>, blocks, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_voxel_hit(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs, const double *T,
                        const anet_voxel_grid *grid, const uint8_t *voxels, double *t_hit, int32_t *voxel) {
  ANET_ON_DEVICE(ctx);
  int rc = check_args(ctx, s, n_pieces, batch, grid);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !voxels || !t_hit) return fail(ctx, ANET_ERR_INVALID, "anet_traj_voxel_hit: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_t;
  int32_t *d_vox;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T);
    p.out(n_pieces, &d_t); p.rows(n_pieces, &d_vox);
  });
  if (rc) return rc;
  rc = anet_traj_voxel_hit_dev(ctx, s, n_pieces, batch, st.ld, d_co, d_T, grid, voxels, d_t, voxel ? d_vox : nullptr, ctx->stream);
  if (rc) return rc;
  if ((rc = st.download(d_t, n_pieces, t_hit))) return rc;
  if (voxel && (rc = st.download_rows(d_vox, n_pieces, voxel))) return rc;
  return ANET_OK;
}

}  // extern "C"
