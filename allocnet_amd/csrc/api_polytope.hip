// Vertex enumeration of corridor polytopes: geo_utils::enumerateVs, batched (include/allocnet_amd.h; semantics and launch shapes
// in polytope_kernels.h).  The depths that decide which polytopes are enumerated come from anet_polytope_depth_dev (api_lbfgs.hip).
#include "api_internal.h"
#include "polytope_kernels.h"

#include <cmath>

namespace {

int check_args(anet_ctx *ctx, int64_t batch, int max_rows, double epsilon, int max_vertices) {
  if (batch < 0 || max_rows < 1) return fail(ctx, ANET_ERR_INVALID, "anet_polytope_vertices: bad batch or max_rows");
  if (max_vertices < 1) return fail(ctx, ANET_ERR_INVALID, "anet_polytope_vertices: max_vertices must be >= 1");
  if (!std::isfinite(epsilon) || !(epsilon > 0.0))
    return fail(ctx, ANET_ERR_INVALID, "anet_polytope_vertices: epsilon must be finite and > 0");
  if (max_rows > anet::kPolyMaxRows)
    return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_polytope_vertices: more than 128 rows per polytope");
  return ANET_OK;
}

// ANET_POLYTOPE_VERTICES_WPP = 1 | 4 forces the waves per polytope (read at every call: the tests compare both shapes)
int waves_per_polytope(const anet_ctx *ctx, int64_t batch, int max_rows) {
  if (const char *e = getenv(anet::Tuning::polytope_vertices_wpp)) return atoi(e) == 1 ? 1 : anet::kPolyWaves;
  const anet::Tuning &t = anet::tuning();
  return batch >= t.polytope_vertices_wave_min_batch.at(ctx->cus) && max_rows <= t.polytope_vertices_wave_max_rows ? 1 : anet::kPolyWaves;
}

// depth: [batch] doubles of device scratch
int vertices_impl(anet_ctx *ctx, int64_t batch, int max_rows, const double *hpoly, double epsilon, int max_vertices, double *verts,
                  int32_t *count, uint64_t *active, int32_t *status, double *depth, hipStream_t st) {
  int rc = anet_polytope_depth_dev(ctx, batch, max_rows, hpoly, 1, depth, nullptr, st);
  if (rc) return rc;
  anet::PolyVertsArgs a{hpoly, depth, verts, count, active, status, batch, max_rows, max_vertices, epsilon};
  if (waves_per_polytope(ctx, batch, max_rows) == 1) {
    const size_t lds = sizeof(double) * anet::kPolyWaves * anet::poly_lds_doubles(max_rows, 1);
    hipLaunchKernelGGL(anet::k_polytope_vertices<1>, dim3((unsigned)((batch + anet::kPolyWaves - 1) / anet::kPolyWaves)),
                       dim3(64 * anet::kPolyWaves), lds, st, a);
  } else {
    const size_t lds = sizeof(double) * anet::poly_lds_doubles(max_rows, anet::kPolyWaves);
    hipLaunchKernelGGL(anet::k_polytope_vertices<anet::kPolyWaves>, dim3((unsigned)batch), dim3(64 * anet::kPolyWaves), lds, st, a);
  }
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

}  // namespace

extern "C" {

int anet_polytope_vertices_dev(anet_ctx *ctx, int64_t batch, int max_rows, const double *hpoly, double epsilon, int max_vertices,
                               double *verts, int32_t *count, uint64_t *active, int32_t *status, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_args(ctx, batch, max_rows, epsilon, max_vertices);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!hpoly || !verts || !count) return fail(ctx, ANET_ERR_INVALID, "anet_polytope_vertices_dev: NULL pointer");
  // the depths go to the head of the context's workspace (the host entry point below keeps that region for them)
  if ((rc = ensure_scratch(ctx, sizeof(double) * (size_t)batch))) return rc;
  return vertices_impl(ctx, batch, max_rows, hpoly, epsilon, max_vertices, verts, count, active, status, (double *)ctx->scratch,
                       (hipStream_t)stream);
}

int anet_polytope_vertices(anet_ctx *ctx, int64_t batch, int max_rows, const double *hpoly, double epsilon, int max_vertices,
                           double *verts, int32_t *count, uint64_t *active, int32_t *status) {
  ANET_ON_DEVICE(ctx);
  int rc = check_args(ctx, batch, max_rows, epsilon, max_vertices);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!hpoly || !verts || !count) return fail(ctx, ANET_ERR_INVALID, "anet_polytope_vertices: NULL pointer");
  const size_t n_hp = (size_t)batch * max_rows * 4, n_v = (size_t)batch * max_vertices * 3, n_a = (size_t)batch * max_vertices * 2;
  double *d_depth, *d_hp, *d_v;
  uint64_t *d_act;
  int32_t *d_cnt, *d_st;
  rc = stage_scratch(ctx, [&](void *w) {  // (the depths lead: anet_polytope_vertices_dev keeps them there; active directly behind verts)
    anet::Cursor c(w);
    d_depth = c.take<double>(batch); d_hp = c.take<double>(n_hp); d_v = c.take<double>(n_v); d_act = c.take<uint64_t>(n_a);
    d_cnt = c.take<int32_t>(batch); d_st = c.take<int32_t>(batch); (void)c.spare(2);
    return c.bytes;
  });
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  ANET_HIP(ctx, hipMemcpyAsync(d_hp, hpoly, sizeof(double) * n_hp, hipMemcpyHostToDevice, st));
  // (slots behind count[b] are not written by the kernel: the caller reads zeros there)
  ANET_HIP(ctx, hipMemsetAsync(d_v, 0, sizeof(double) * (n_v + n_a), st));
  rc = vertices_impl(ctx, batch, max_rows, d_hp, epsilon, max_vertices, d_v, d_cnt, active ? d_act : nullptr, status ? d_st : nullptr,
                     d_depth, st);
  if (rc) return rc;
  ANET_HIP(ctx, hipMemcpyAsync(verts, d_v, sizeof(double) * n_v, hipMemcpyDeviceToHost, st));
  ANET_HIP(ctx, hipMemcpyAsync(count, d_cnt, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
  if (active) ANET_HIP(ctx, hipMemcpyAsync(active, d_act, sizeof(uint64_t) * n_a, hipMemcpyDeviceToHost, st));
  if (status) ANET_HIP(ctx, hipMemcpyAsync(status, d_st, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
  ANET_HIP(ctx, hipStreamSynchronize(st));
  return ANET_OK;
}

}  // extern "C"
