// Waypoints as vertex weights of corridor overlaps (sfc_param_kernels.h): overlap enumeration, the transform and its gradient,
// backward_p, the corridor-constrained MINCO L-BFGS over (xi, tau) and the shortest route through a corridor
// (sfc_path_kernels.h), both on the lockstep driver of api_lbfgs.hip (include/allocnet_amd.h).
#include "api_internal.h"
#include "sfc_param_kernels.h"
#include "sfc_path_kernels.h"

#include <cmath>

namespace {

using anet::kSfcBlock;

dim3 sfc_grid(int64_t B, int rows) { return dim3((unsigned)((B + kSfcBlock - 1) / kSfcBlock), (unsigned)rows); }

int check_shape(anet_ctx *ctx, const char *who, int N, int64_t batch, int64_t ld, int K) {
  if (N < 2 || N > ANET_MAX_PIECES) return fail(ctx, ANET_ERR_INVALID, std::string(who) + ": piece count must be in [2, ANET_MAX_PIECES]");
  if (K < 1 || K > 256) return fail(ctx, ANET_ERR_INVALID, std::string(who) + ": max_verts must be in [1, 256]");
  if (batch < 0 || (batch > 0 && ld < batch)) return fail(ctx, ANET_ERR_INVALID, std::string(who) + ": batch < 0 or ld < batch");
  return ANET_OK;
}

int forward_p(anet_ctx *ctx, int N, int64_t B, int64_t ld, int K, const double *xi, const double *verts, double w_norm, double *wps,
              double *norm, hipStream_t st) {
  hipLaunchKernelGGL(anet::k_sfc_forward_p, sfc_grid(B, N - 1), dim3(kSfcBlock), 0, st, xi, verts, B, ld, K, w_norm, wps, norm);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int backward_grad(anet_ctx *ctx, int N, int64_t B, int64_t ld, int K, const double *xi, const double *verts, const double *wps,
                  const double *norm, const double *grad_p, double *grad_xi, double *cost, hipStream_t st) {
  hipLaunchKernelGGL(anet::k_sfc_backward_grad, sfc_grid(B, N - 1), dim3(kSfcBlock), 0, st, xi, verts, wps, norm, grad_p, B, ld, K,
                     grad_xi, cost);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

struct TinyEval {
  anet_ctx *ctx;
  anet::LbfgsLayout *L;
  const double *verts, *p;
  int64_t B, ld;
  int N, K;
  hipStream_t st;
};
int tiny_eval(void *inst) {
  const TinyEval &e = *(const TinyEval *)inst;
  hipLaunchKernelGGL(anet::k_sfc_tiny_nls, sfc_grid(e.B, e.N - 1), dim3(kSfcBlock), 0, e.st, e.L->x, e.verts, e.p, e.B, e.ld, e.K,
                     e.L->feval, e.L->g);
  ANET_HIP(e.ctx, hipGetLastError());
  return ANET_OK;
}

struct OptEval {
  anet_ctx *ctx;
  const anet::SfcWs *W;
  int s, c, N, K;
  int64_t B, ld;
  const double *head, *tail, *T, *verts, *hpolys, *tau;
  const anet_penalty *pen;
  double w_norm;
  double *gT_out;
  hipStream_t st;
};
// forward_p -> cost + gradient at the workspace's waypoint rows -> backward_grad into the optimiser's gradient rows
int opt_eval(void *inst) {
  const OptEval &e = *(const OptEval *)inst;
  const anet::LbfgsLayout &L = e.W->opt;
  int rc = forward_p(e.ctx, e.N, e.B, e.ld, e.K, L.x, e.verts, e.w_norm, e.W->wps, e.W->norm, e.st);
  if (rc) return rc;
  rc = cost_grad_dev_impl(e.ctx, e.s, e.c, e.N, e.B, e.ld, e.head, e.tail, e.W->wps, e.T, e.hpolys, e.pen, e.W->cg.co, L.feval, e.W->gP,
                          e.gT_out, nullptr, e.st, e.tau);
  if (rc) return rc;
  return backward_grad(e.ctx, e.N, e.B, e.ld, e.K, L.x, e.verts, e.W->wps, e.W->norm, e.W->gP, L.g, L.feval, e.st);
}

// one evaluation of the route length: one launch (sfc_path_kernels.h)
struct PathEval {
  anet_ctx *ctx;
  const anet::LbfgsLayout *L;
  const double *verts, *start, *goal;
  int64_t B, ld;
  int N, K;
  double eps2, w_norm;
  hipStream_t st;
};
int path_eval(void *inst) {
  const PathEval &e = *(const PathEval *)inst;
  hipLaunchKernelGGL(anet::k_sfc_path_eval, sfc_grid(e.B, 1), dim3(anet::kSfcPathBlock), 0, e.st, e.L->x, e.verts, e.start, e.goal, e.B,
                     e.ld, e.N - 1, e.K, e.eps2, e.w_norm, e.L->feval, e.L->g);
  ANET_HIP(e.ctx, hipGetLastError());
  return ANET_OK;
}

// the parameters of a route solve: the caller's, or the defaults (mem_size 8, past 3, delta 1e-6, g_epsilon 1e-5)
anet_lbfgs_params path_params(const anet_lbfgs_params *params) {
  anet_lbfgs_params prm;
  anet_lbfgs_default_params(&prm);
  return params ? *params : prm;
}

}  // namespace

extern "C" {

int64_t anet_sfc_overlap_workspace(int n_pieces, int64_t batch, int poly_rows, int max_verts) {
  if (n_pieces < 2 || batch < 0 || poly_rows < 1 || max_verts < 1) return -1;
  return anet::sfc_overlap_ws(nullptr, n_pieces, batch, poly_rows, max_verts).doubles;
}

int anet_sfc_overlap_vertices_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int poly_rows, const double *hpolys,
                                  double epsilon, int max_verts, double *verts, int32_t *count, int32_t *status, double *work,
                                  void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_shape(ctx, "anet_sfc_overlap_vertices_dev", n_pieces, batch, ld, max_verts);
  if (rc) return rc;
  if (poly_rows < 1 || 2 * poly_rows > 128)
    return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_sfc_overlap_vertices_dev: 1 <= poly_rows <= 64 (two stacked polytopes of 128 rows)");
  if (batch == 0) return ANET_OK;
  if (!hpolys || !verts || !count || !work) return fail(ctx, ANET_ERR_INVALID, "anet_sfc_overlap_vertices_dev: NULL pointer");
  const int N = n_pieces, M = poly_rows, K = max_verts;
  hipStream_t st = (hipStream_t)stream;
  const anet::SfcOverlapWs W = anet::sfc_overlap_ws(work, N, batch, M, K);
  hipLaunchKernelGGL(anet::k_sfc_pack_overlaps, sfc_grid(batch, (N - 1) * 2 * M), dim3(kSfcBlock), 0, st, hpolys, batch, ld, M, W.stacked);
  ANET_HIP(ctx, hipGetLastError());
  rc = anet_polytope_vertices_dev(ctx, (int64_t)(N - 1) * batch, 2 * M, W.stacked, epsilon, K, W.verts, W.count, nullptr, W.status, st);
  if (rc) return rc;
  hipLaunchKernelGGL(anet::k_sfc_pack_vertices, sfc_grid(batch, N - 1), dim3(kSfcBlock), 0, st, W.verts, W.count, W.status, batch, ld, K,
                     verts, count, status);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_sfc_forward_p_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int max_verts, const double *xi,
                           const double *verts, double w_norm, double *wps, double *norm, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_shape(ctx, "anet_sfc_forward_p_dev", n_pieces, batch, ld, max_verts);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!xi || !verts || !wps || !norm) return fail(ctx, ANET_ERR_INVALID, "anet_sfc_forward_p_dev: NULL pointer");
  return forward_p(ctx, n_pieces, batch, ld, max_verts, xi, verts, w_norm, wps, norm, (hipStream_t)stream);
}

int anet_sfc_backward_grad_p_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int max_verts, const double *xi,
                                 const double *verts, const double *wps, const double *norm, const double *grad_p,
                                 double *grad_xi, double *cost, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_shape(ctx, "anet_sfc_backward_grad_p_dev", n_pieces, batch, ld, max_verts);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!xi || !verts || !wps || !norm || !grad_p || !grad_xi) return fail(ctx, ANET_ERR_INVALID, "anet_sfc_backward_grad_p_dev: NULL pointer");
  return backward_grad(ctx, n_pieces, batch, ld, max_verts, xi, verts, wps, norm, grad_p, grad_xi, cost, (hipStream_t)stream);
}

int64_t anet_sfc_backward_p_workspace(int n_pieces, int max_verts, int64_t ld) {
  if (n_pieces < 2 || max_verts < 1 || ld < 1) return -1;
  return anet::sfc_backward_p_ws(nullptr, n_pieces, max_verts, ld).doubles;
}

int anet_sfc_backward_p_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int max_verts, const double *verts,
                            const int32_t *count, const double *wps, double *xi, double *residual, double *work, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_shape(ctx, "anet_sfc_backward_p_dev", n_pieces, batch, ld, max_verts);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!verts || !count || !wps || !xi || !residual || !work) return fail(ctx, ANET_ERR_INVALID, "anet_sfc_backward_p_dev: NULL pointer");
  const int N = n_pieces, K = max_verts;
  hipStream_t st = (hipStream_t)stream;
  anet::LbfgsLayout L = anet::sfc_backward_p_ws(work, N, K, ld);
  anet_lbfgs_params prm;
  anet_lbfgs_default_params(&prm);
  prm.mem_size = anet::kSfcTinyMem; prm.g_epsilon = 0.0; prm.past = anet::kSfcTinyPast; prm.delta = 1.0e-16;
  if ((rc = lbfgs_reset_shared(ctx, L, st))) return rc;
  hipLaunchKernelGGL(anet::k_sfc_tiny_start, sfc_grid(ld, N - 1), dim3(kSfcBlock), 0, st, count, batch, ld, K, L.x, L.is);
  ANET_HIP(ctx, hipGetLastError());
  TinyEval ev{ctx, &L, verts, wps, batch, ld, N, K, st};
  rc = lbfgs_drive_shared(ctx, L, (int64_t)(N - 1) * ld, prm, 200, st, tiny_eval, &ev, nullptr, 0, false, 0, 0.0, nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(anet::k_sfc_tiny_finish, sfc_grid(batch, N - 1), dim3(kSfcBlock), 0, st, L.x, verts, wps, count, batch, ld, K, xi,
                     residual);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int64_t anet_sfc_workspace(int s, int n_pieces, int max_verts, int64_t ld, const anet_lbfgs_params *params) {
  if (!params || params->mem_size <= 0 || s < 2 || s > 4 || n_pieces < 2 || max_verts < 1 || ld < 1) return -1;
  const int n = (n_pieces - 1) * max_verts + n_pieces, npf = params->past > 1 ? params->past : 1;
  return anet::sfc_ws(nullptr, s, n_pieces, max_verts, ld, params->mem_size, npf, n).doubles;
}

int anet_lbfgs_minco_sfc_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld, const double *head,
                             const double *tail, double *xi, double *T, const double *verts, const int32_t *count,
                             const int32_t *overlap_status, int max_verts, const double *hpolys, const anet_penalty *pen,
                             const anet_lbfgs_params *params, int opt_flags, int max_evals, double min_duration, double w_norm,
                             double *work, double *cost, double *wps_out, double *coeffs_out, int32_t *status, int32_t *iters,
                             int32_t *evals, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_penalty(ctx, pen))) return rc;
  if ((rc = check_shape(ctx, "anet_lbfgs_minco_sfc_dev", n_pieces, batch, ld, max_verts))) return rc;
  if (!(min_duration >= 0.0) || !(w_norm >= 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco_sfc_dev: min_duration and w_norm must be >= 0");
  const int N = n_pieces, K = max_verts, nxi = (N - 1) * K, nt = (opt_flags & ANET_OPT_TIMES) ? N : 0, n = nxi + nt;
  if (!params) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco_sfc_dev: params is NULL");
  if ((rc = check_lbfgs(ctx, n, params, max_evals))) return rc;
  if (batch == 0) return ANET_OK;
  if (!head || !tail || !xi || !T || !verts || !count || !work || !wps_out)
    return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco_sfc_dev: NULL pointer");
  const int m = params->mem_size, npf = params->past > 1 ? params->past : 1;
  anet::SfcWs W = anet::sfc_ws(work, s, N, K, ld, m, npf, n);
  anet::LbfgsLayout &L = W.opt;
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(kSfcBlock);
  // the state rows, the problems that must not run, the start point
  if ((rc = lbfgs_reset_shared(ctx, L, st))) return rc;
  hipLaunchKernelGGL(anet::k_sfc_mark_no_overlap, sfc_grid(batch, 1), blk, 0, st, count, overlap_status, batch, ld, N - 1,
                     (int)ANET_SFC_NO_OVERLAP, L.is);
  hipLaunchKernelGGL(anet::k_sfc_map, sfc_grid(batch, n), blk, 0, st, L.x, xi, T, L.is, batch, ld, nxi, (int)ANET_SFC_NO_OVERLAP, 0);
  ANET_HIP(ctx, hipGetLastError());
  const int step_bound = (min_duration > 0.0 && nt > 0) ? 1 : 0;
  OptEval ev{ctx, &W, s, c, N, K, batch, ld, head, tail, T, verts, hpolys, nt ? L.x + (int64_t)nxi * ld : nullptr, pen, w_norm,
             nt ? L.g + (int64_t)nxi * ld : W.gT, st};
  rc = lbfgs_drive_shared(ctx, L, batch, *params, max_evals, st, opt_eval, &ev, nt ? T : nullptr, nxi, false, step_bound,
                          minco_tau_min(min_duration), ctx->cancel_flag);
  if (rc) return rc;
  // the result (x may have been put back by a failed line search) for the problems that ran
  hipLaunchKernelGGL(anet::k_sfc_map, sfc_grid(batch, n), blk, 0, st, L.x, xi, T, L.is, batch, ld, nxi, (int)ANET_SFC_NO_OVERLAP, 1);
  ANET_HIP(ctx, hipGetLastError());
  if ((rc = forward_p(ctx, N, batch, ld, K, xi, verts, w_norm, wps_out, W.norm, st))) return rc;
  if ((rc = lbfgs_results_shared(ctx, L, batch, status, iters, evals, cost, st))) return rc;
  if (cost) {
    hipLaunchKernelGGL(anet::k_sfc_no_cost, sfc_grid(batch, 1), blk, 0, st, L.is, batch, ld, (int)ANET_SFC_NO_OVERLAP, cost);
    ANET_HIP(ctx, hipGetLastError());
  }
  return coeffs_out ? minco_final_coeffs(ctx, s, c, N, batch, ld, head, tail, wps_out, T, coeffs_out, st) : ANET_OK;
}

int anet_lbfgs_minco_sfc(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head, const double *tail,
                         const double *wps_start, double *T, const double *hpolys, const anet_penalty *pen,
                         const anet_lbfgs_params *params, int opt_flags, int max_evals, double min_duration, double w_norm,
                         double epsilon, int max_verts, double *wps_out, double *cost, double *coeffs_out, int32_t *status,
                         int32_t *iters, int32_t *evals, double *residual, int32_t *overlap_status, double *xi_out) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if (!pen || !params) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco_sfc: pen and params are required");
  if ((rc = check_penalty(ctx, pen))) return rc;
  if ((rc = check_shape(ctx, "anet_lbfgs_minco_sfc", n_pieces, batch, batch, max_verts))) return rc;
  if (batch == 0) return ANET_OK;
  if (!head || !tail || !T || !hpolys || !wps_out) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco_sfc: NULL pointer");
  const int N = n_pieces, K = max_verts, M = pen->poly_rows;
  if (M < 1) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco_sfc: pen->poly_rows must be >= 1");
  const int64_t nco = (int64_t)N * 3 * 2 * s, nhp = (int64_t)N * M * 4, nwp = (int64_t)3 * (N - 1), nxi = (int64_t)(N - 1) * K;
  Stager sg(ctx, batch);
  const int64_t ld = sg.ld;
  const int64_t w_opt = anet_sfc_workspace(s, N, K, ld, params), w_ov = anet_sfc_overlap_workspace(N, batch, M, K),
                w_bp = anet_sfc_backward_p_workspace(N, K, ld);
  if (w_opt < 0 || w_ov < 0 || w_bp < 0) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco_sfc: bad lbfgs parameters or shape");
  // the three workspaces are used one after the other: one region of the largest
  int64_t wmax = w_opt > w_ov ? w_opt : w_ov;
  if (w_bp > wmax) wmax = w_bp;
  double *d_head, *d_tail, *d_wp0 = nullptr, *d_T, *d_hp, *d_xi, *d_verts, *d_res, *d_wps, *d_co, *d_cost, *d_work;
  int32_t *count, *ostat;
  anet::LbfgsResultRows R;
  rc = sg.stage([&](Stager::Pass &p) {
    p.in(head, 3 * c, &d_head); p.in(tail, 3 * c, &d_tail);
    if (wps_start) p.in(wps_start, nwp, &d_wp0);
    p.in(T, N, &d_T); p.in(hpolys, nhp, &d_hp);
    p.out(nxi, &d_xi); p.rows(3 * nxi, &d_verts);
    // count | overlap status | residual: one row per waypoint each
    p.rows(N - 1, &count); p.rows(N - 1, &ostat); p.out(N - 1, &d_res);
    p.out(nwp, &d_wps); p.out(nco, &d_co); p.rows(1, &d_cost); p.doubles(wmax, &d_work);
    R = anet::lbfgs_result_rows(p.c, ld);
    // anet_polytope_vertices_dev keeps its (N - 1) batch depths at the head of the context's scratch, which is the stager's staging
    // area: every upload has left it in stream order by the time the enumeration runs, and it must be large enough to hold them
    p.at_least(N - 1);
  });
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  if ((rc = anet_sfc_overlap_vertices_dev(ctx, N, batch, ld, M, d_hp, epsilon, K, d_verts, count, ostat, d_work, st))) return rc;
  if (d_wp0) {
    if ((rc = anet_sfc_backward_p_dev(ctx, N, batch, ld, K, d_verts, count, d_wp0, d_xi, d_res, d_work, st))) return rc;
  } else {
    hipLaunchKernelGGL(anet::k_sfc_mean_start, sfc_grid(batch, N - 1), dim3(kSfcBlock), 0, st, count, batch, ld, K, d_xi, d_res);
    ANET_HIP(ctx, hipGetLastError());
  }
  rc = anet_lbfgs_minco_sfc_dev(ctx, s, c, N, batch, ld, d_head, d_tail, d_xi, d_T, d_verts, count, ostat, K, d_hp, pen, params,
                                opt_flags, max_evals, min_duration, w_norm, d_work, d_cost, d_wps, coeffs_out ? d_co : nullptr,
                                R.status, R.iters, R.evals, st);
  if (rc) return rc;
  if ((rc = download_results(ctx, batch, R, d_cost, status, iters, evals, cost, st))) return rc;
  if (overlap_status) {  // [(N-1)][ld] on the device -> [batch][N-1]
    std::vector<int32_t> h((size_t)(N - 1) * ld);
    for (int w = 0; w < N - 1; ++w)
      ANET_HIP(ctx, hipMemcpyAsync(h.data() + (size_t)w * ld, ostat + (int64_t)w * ld, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
    ANET_HIP(ctx, hipStreamSynchronize(st));
    for (int64_t b = 0; b < batch; ++b)
      for (int w = 0; w < N - 1; ++w) overlap_status[b * (N - 1) + w] = h[(size_t)w * ld + b];
  }
  if ((rc = sg.download(d_wps, nwp, wps_out))) return rc;
  if ((rc = sg.download(d_T, N, T))) return rc;
  if (residual && (rc = sg.download(d_res, N - 1, residual))) return rc;
  if (xi_out && (rc = sg.download(d_xi, nxi, xi_out))) return rc;
  if (coeffs_out && (rc = sg.download(d_co, nco, coeffs_out))) return rc;
  ANET_HIP(ctx, hipStreamSynchronize(st));
  return ANET_OK;
}

int64_t anet_sfc_shortest_path_workspace(int n_pieces, int max_verts, int64_t ld, const anet_lbfgs_params *params) {
  const anet_lbfgs_params prm = path_params(params);
  if (prm.mem_size <= 0 || n_pieces < 2 || max_verts < 1 || ld < 1) return -1;
  return anet::sfc_path_ws(nullptr, n_pieces, max_verts, ld, prm.mem_size, prm.past > 1 ? prm.past : 1).doubles;
}

int anet_sfc_path_cost_grad_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int max_verts, const double *start,
                                const double *goal, const double *xi, const double *verts, double eps, double w_norm, double *cost,
                                double *grad_xi, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_shape(ctx, "anet_sfc_path_cost_grad_dev", n_pieces, batch, ld, max_verts);
  if (rc) return rc;
  if (!(eps >= 0.0) || !(w_norm >= 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_sfc_path_cost_grad_dev: eps and w_norm must be >= 0");
  if (batch == 0) return ANET_OK;
  if (!start || !goal || !xi || !verts || !cost || !grad_xi) return fail(ctx, ANET_ERR_INVALID, "anet_sfc_path_cost_grad_dev: NULL pointer");
  hipLaunchKernelGGL(anet::k_sfc_path_eval, sfc_grid(batch, 1), dim3(anet::kSfcPathBlock), 0, (hipStream_t)stream, xi, verts, start, goal,
                     batch, ld, n_pieces - 1, max_verts, eps * eps, w_norm, cost, grad_xi);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_sfc_shortest_path_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int max_verts, const double *start,
                               const double *goal, const double *verts, const int32_t *count, const int32_t *overlap_status,
                               double *xi, int from_mean, double eps, double w_norm, const anet_lbfgs_params *params, int max_evals,
                               double *work, double *wps_out, double *length_out, double *cost_out, int32_t *status, int32_t *iters,
                               int32_t *evals, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_shape(ctx, "anet_sfc_shortest_path_dev", n_pieces, batch, ld, max_verts);
  if (rc) return rc;
  if (!(eps >= 0.0) || !(w_norm >= 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_sfc_shortest_path_dev: eps and w_norm must be >= 0");
  const int N = n_pieces, K = max_verts, n = (N - 1) * K;
  const anet_lbfgs_params prm = path_params(params);
  if (max_evals <= 0) max_evals = ANET_SFC_PATH_MAX_EVALS;
  if ((rc = check_lbfgs(ctx, n, &prm, max_evals))) return rc;
  if (batch == 0) return ANET_OK;
  if (!start || !goal || !verts || !count || !xi || !work || !wps_out)
    return fail(ctx, ANET_ERR_INVALID, "anet_sfc_shortest_path_dev: NULL pointer");
  static_assert(anet::kSfcPathBlock == kSfcBlock, "sfc_grid serves both headers");
  anet::SfcPathWs W = anet::sfc_path_ws(work, N, K, ld, prm.mem_size, prm.past > 1 ? prm.past : 1);
  anet::LbfgsLayout &L = W.opt;
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(kSfcBlock);
  const int code = (int)ANET_SFC_NO_OVERLAP;
  // the state rows, the problems that must not run, the start point
  if ((rc = lbfgs_reset_shared(ctx, L, st))) return rc;
  hipLaunchKernelGGL(anet::k_sfc_mark_no_overlap, sfc_grid(batch, 1), blk, 0, st, count, overlap_status, batch, ld, N - 1, code, L.is);
  if (from_mean)
    hipLaunchKernelGGL(anet::k_sfc_path_mean_start, sfc_grid(batch, N - 1), blk, 0, st, count, L.is, batch, ld, K, code, xi);
  hipLaunchKernelGGL(anet::k_sfc_path_map, sfc_grid(batch, n), blk, 0, st, L.x, xi, L.is, batch, ld, code, 0);
  ANET_HIP(ctx, hipGetLastError());
  PathEval ev{ctx, &L, verts, start, goal, batch, ld, N, K, eps * eps, w_norm, st};
  rc = lbfgs_drive_shared(ctx, L, batch, prm, max_evals, st, path_eval, &ev, nullptr, 0, false, 0, 0.0, ctx->cancel_flag);
  if (rc) return rc;
  // the result (x may have been put back by a failed line search) for the problems that ran
  hipLaunchKernelGGL(anet::k_sfc_path_map, sfc_grid(batch, n), blk, 0, st, L.x, xi, L.is, batch, ld, code, 1);
  ANET_HIP(ctx, hipGetLastError());
  if ((rc = forward_p(ctx, N, batch, ld, K, xi, verts, w_norm, wps_out, W.norm, st))) return rc;
  if (length_out) {
    hipLaunchKernelGGL(anet::k_sfc_path_length, sfc_grid(batch, 1), blk, 0, st, start, goal, wps_out, L.is, batch, ld, N - 1, code,
                       length_out);
    ANET_HIP(ctx, hipGetLastError());
  }
  if ((rc = lbfgs_results_shared(ctx, L, batch, status, iters, evals, cost_out, st))) return rc;
  if (cost_out) {
    hipLaunchKernelGGL(anet::k_sfc_no_cost, sfc_grid(batch, 1), blk, 0, st, L.is, batch, ld, code, cost_out);
    ANET_HIP(ctx, hipGetLastError());
  }
  return ANET_OK;
}

int anet_sfc_shortest_path(anet_ctx *ctx, int n_pieces, int64_t batch, int poly_rows, const double *hpolys, const double *start,
                           const double *goal, double epsilon, int max_verts, double eps, double w_norm,
                           const anet_lbfgs_params *params, int max_evals, double *wps_out, double *length_out, int32_t *status,
                           int32_t *iters, int32_t *evals, int32_t *overlap_status, double *xi_out) {
  ANET_ON_DEVICE(ctx);
  int rc = check_shape(ctx, "anet_sfc_shortest_path", n_pieces, batch, batch, max_verts);
  if (rc) return rc;
  if (poly_rows < 1) return fail(ctx, ANET_ERR_INVALID, "anet_sfc_shortest_path: poly_rows must be >= 1");
  if (batch == 0) return ANET_OK;
  if (!hpolys || !start || !goal || !wps_out) return fail(ctx, ANET_ERR_INVALID, "anet_sfc_shortest_path: NULL pointer");
  const int N = n_pieces, K = max_verts, M = poly_rows;
  const int64_t nhp = (int64_t)N * M * 4, nwp = (int64_t)3 * (N - 1), nxi = (int64_t)(N - 1) * K;
  Stager sg(ctx, batch);
  const int64_t ld = sg.ld;
  const int64_t w_opt = anet_sfc_shortest_path_workspace(N, K, ld, params), w_ov = anet_sfc_overlap_workspace(N, batch, M, K);
  if (w_opt < 0 || w_ov < 0) return fail(ctx, ANET_ERR_INVALID, "anet_sfc_shortest_path: bad lbfgs parameters or shape");
  double *d_start, *d_goal, *d_hp, *d_xi, *d_verts, *d_wps, *d_len, *d_work;
  int32_t *count, *ostat;
  anet::LbfgsResultRows R;
  rc = sg.stage([&](Stager::Pass &p) {
    p.in(start, 3, &d_start); p.in(goal, 3, &d_goal); p.in(hpolys, nhp, &d_hp);
    p.out(nxi, &d_xi); p.rows(3 * nxi, &d_verts);
    // count | overlap status: one row per waypoint each
    p.rows(N - 1, &count); p.rows(N - 1, &ostat);
    // the enumeration and the route solve use the workspace one after the other: one region of the larger
    p.out(nwp, &d_wps); p.rows(1, &d_len); p.doubles(w_opt > w_ov ? w_opt : w_ov, &d_work);
    R = anet::lbfgs_result_rows(p.c, ld);
    // anet_polytope_vertices_dev keeps its (N - 1) batch depths at the head of the staging area (as in anet_lbfgs_minco_sfc)
    p.at_least(N - 1);
  });
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  // a problem that does not run keeps its xi: zeros
  ANET_HIP(ctx, hipMemsetAsync(d_xi, 0, sizeof(double) * (size_t)(nxi * ld), st));
  if ((rc = anet_sfc_overlap_vertices_dev(ctx, N, batch, ld, M, d_hp, epsilon, K, d_verts, count, ostat, d_work, st))) return rc;
  rc = anet_sfc_shortest_path_dev(ctx, N, batch, ld, K, d_start, d_goal, d_verts, count, ostat, d_xi, 1, eps, w_norm, params, max_evals,
                                  d_work, d_wps, d_len, nullptr, R.status, R.iters, R.evals, st);
  if (rc) return rc;
  if ((rc = download_results(ctx, batch, R, d_len, status, iters, evals, length_out, st))) return rc;
  if (overlap_status) {  // [(N-1)][ld] on the device -> [batch][N-1]
    std::vector<int32_t> h((size_t)(N - 1) * ld);
    for (int w = 0; w < N - 1; ++w)
      ANET_HIP(ctx, hipMemcpyAsync(h.data() + (size_t)w * ld, ostat + (int64_t)w * ld, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
    ANET_HIP(ctx, hipStreamSynchronize(st));
    for (int64_t b = 0; b < batch; ++b)
      for (int w = 0; w < N - 1; ++w) overlap_status[b * (N - 1) + w] = h[(size_t)w * ld + b];
  }
  if ((rc = sg.download(d_wps, nwp, wps_out))) return rc;
  if (xi_out && (rc = sg.download(d_xi, nxi, xi_out))) return rc;
  ANET_HIP(ctx, hipStreamSynchronize(st));
  return ANET_OK;
}

}  // extern "C"
