// Coefficient solve, cost sampling and the wide-spread solve; trajectory evaluation, cost, its duration gradient, normalised
// piece coefficients and maximum rates (include/allocnet_amd.h).
#include "api_internal.h"
#include "minco_kernels.h"
#include "minco_sample_kernel.h"
#include "minco_dense_kernels.h"
#include "traj_kernels.h"
#include "rate_kernels.h"

namespace {

// Small batches (tuning().axis_max_batch) solve and propagate with a lane per (trajectory, axis) -- three times the waves, ~2.4x
// shorter dependent chains --, larger ones with a lane per trajectory
template <int S>
int launch_solve(anet_ctx *ctx, const anet::SolveArgs &a, hipStream_t st) {
  const dim3 block(anet::kSolveBlock);
  if (a.B <= anet::tuning().axis_max_batch.at(ctx->cus)) {
    // (exact shapes with an even number of pieces, batches that leave SIMDs empty: the chain from both ends, two lanes per axis)
    if (a.B <= anet::tuning().axis_two_max_batch.at(ctx->cus) && a.c == 3 && ((S == 4 && a.N == 8) || (S == 3 && a.N == 16))) {
      const dim3 g6((unsigned)((a.B + 9) / 10));
      if constexpr (S == 4) hipLaunchKernelGGL((anet::k_minco_solve_axis_two<4, 8, 2>), g6, block, 0, st, a);
      else if constexpr (S == 3) hipLaunchKernelGGL((anet::k_minco_solve_axis_two<3, 16, 2>), g6, block, 0, st, a);
    } else {
      const dim3 g3((unsigned)((a.B + 20) / 21));
      anet::with_minco_shape<S>(a.N, a.c, [&](auto sh) {
        using Sh = decltype(sh);
        hipLaunchKernelGGL((anet::k_minco_solve_axis<S, Sh::NB, Sh::EXACT, Sh::NPC>), g3, block, 0, st, a);
      });
    }
  } else {
    const dim3 grid((unsigned)((a.B + anet::kSolveBlock - 1) / anet::kSolveBlock));
    anet::with_minco_shape<S>(a.N, a.c, [&](auto sh) {
      using Sh = decltype(sh);
      hipLaunchKernelGGL((anet::k_minco_solve<S, Sh::NB, Sh::EXACT, Sh::NPC>), grid, block, 0, st, a);
    });
  }
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

// (no fully specialised instantiation for 8-piece snap with c = 4)
template <int S>
static int launch_sample(anet_ctx *ctx, const anet::SampleArgs &a, hipStream_t st) {
  const dim3 grid((unsigned)((a.B + anet::kSolveBlock - 1) / anet::kSolveBlock)), block(anet::kSolveBlock);
  anet::with_minco_shape<S, false>(a.N, a.c, [&](auto sh) {
    using Sh = decltype(sh);
    hipLaunchKernelGGL((anet::k_minco_sample<S, Sh::NB, Sh::EXACT, Sh::NPC>), grid, block, 0, st, a);
  });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

// k_traj_cost: the cost (a.cost) and / or its gradient in the durations (a.gradT) of every trajectory
int launch_traj_cost(anet_ctx *ctx, int s, const anet::CostArgs &a, hipStream_t st) {
  const dim3 grid((unsigned)((a.B + 255) / 256)), block(256);
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_traj_cost<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}
}  // namespace

extern "C" {

int anet_minco_solve_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                         const double *head, const double *tail, const double *wps, const double *T,
                         double *coeffs, double *energy, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!head || !tail || !T || (n_pieces > 1 && !wps) || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_solve_dev: NULL input or ld < batch");
  anet::SolveArgs a{head, tail, wps, T, coeffs, energy, batch, ld, n_pieces, c};
  hipStream_t st = (hipStream_t)stream;
  return anet::with_order(s, [&](auto o) { return launch_solve<decltype(o)::value>(ctx, a, st); });
}

int anet_minco_sample_costs_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t problems, int64_t samples_per_problem,
                                int64_t ld, int64_t ldp, const double *head, const double *tail, const double *wps,
                                const double *T, double rho, double *cost, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (problems < 0 || samples_per_problem < 1) return fail(ctx, ANET_ERR_INVALID, "anet_minco_sample_costs: problems >= 0, samples_per_problem >= 1");
  const int64_t total = problems * samples_per_problem;
  int rc = check_solve_args(ctx, s, c, n_pieces, total);
  if (rc) return rc;
  if (total == 0) return ANET_OK;
  if (!head || !tail || !T || !cost || (n_pieces > 1 && !wps) || ld < total || ldp < problems)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_sample_costs_dev: NULL pointer, ld < problems * samples_per_problem or ldp < problems");
  anet::SampleArgs a{head, tail, wps, T, cost, total, ld, ldp, samples_per_problem, n_pieces, c, rho};
  hipStream_t st = (hipStream_t)stream;
  return anet::with_order(s, [&](auto o) { return launch_sample<decltype(o)::value>(ctx, a, st); });
}

int anet_minco_solve_wide_spread_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                                     const double *head, const double *tail, const double *wps, const double *T,
                                     double min_spread, double *coeffs, double *energy, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!head || !tail || !T || (n_pieces > 1 && !wps) || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_solve_wide_spread_dev: NULL input or ld < batch");
  if (!coeffs && !energy) return fail(ctx, ANET_ERR_INVALID, "anet_minco_solve_wide_spread_dev: no output requested");
  anet::DenseSolveArgs a{head, tail, wps, T, coeffs, energy, batch, ld, n_pieces, c, min_spread};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)batch), block(64);
  return anet::with_order(s, [&](auto o) -> int {
    constexpr int S = decltype(o)::value;
    const size_t lds = anet::minco_dense_lds_bytes<S>(n_pieces);
    if (lds > 64 * 1024)
      ANET_HIP(ctx, hipFuncSetAttribute((const void *)anet::k_minco_solve_dense<S>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(anet::k_minco_solve_dense<S>, grid, block, lds, st, a);
    ANET_HIP(ctx, hipGetLastError());
    return ANET_OK;
  });
}

int anet_traj_eval_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld,
                       const double *coeffs, const double *T, int nq, const double *tq, int deriv,
                       double *out, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (deriv < 0 || deriv > 3 || nq < 0) return fail(ctx, ANET_ERR_INVALID, "anet_traj_eval: deriv in [0,3], nq >= 0");
  if (batch == 0 || nq == 0) return ANET_OK;
  if (!coeffs || !T || !tq || !out || ld < batch) return fail(ctx, ANET_ERR_INVALID, "anet_traj_eval_dev: NULL pointer or ld < batch");
  anet::EvalArgs a{coeffs, T, tq, out, batch, ld, n_pieces, nq, deriv};
  const dim3 grid((unsigned)((batch + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_traj_eval<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_cost_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld,
                       const double *coeffs, const double *T, double m34, double *cost, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !cost || ld < batch) return fail(ctx, ANET_ERR_INVALID, "anet_traj_cost_dev: NULL pointer or ld < batch");
  return launch_traj_cost(ctx, s, anet::CostArgs{coeffs, T, cost, nullptr, batch, ld, n_pieces, m34}, (hipStream_t)stream);
}

int anet_minco_solve(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head,
                     const double *tail, const double *wps, const double *T, double *coeffs,
                     double *energy) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!head || !tail || !T || (n_pieces > 1 && !wps))
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_solve: NULL input");
  const int N = n_pieces;
  const int64_t n_co = (int64_t)N * 3 * 2 * s;
  Stager st(ctx, batch);
  double *d_head, *d_tail, *d_wps, *d_T, *d_co, *d_en;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(head, 3 * c, &d_head); p.in(tail, 3 * c, &d_tail); p.in(wps, (int64_t)(N - 1) * 3, &d_wps); p.in(T, N, &d_T);
    p.out(n_co, &d_co); p.rows(1, &d_en);
  });
  if (rc) return rc;
  rc = anet_minco_solve_dev(ctx, s, c, N, batch, st.ld, d_head, d_tail, d_wps, d_T, coeffs ? d_co : nullptr, d_en,
                            ctx->stream);
  if (rc) return rc;
  {
    // The durations are in host memory here, so the check is free: trajectories whose durations spread over more
    // than kWideSpread are redone by the pivoted collocation solve (the reduced form of the fast kernel loses the
    // north star's 1e-6 on the coefficients beyond a spread of ~100).  Device callers decide for
    // themselves (anet_minco_solve_wide_spread_dev): the fast path never pays for the check.
    bool wide = false;
    for (int64_t b = 0; b < batch && !wide; ++b) {
      double lo = T[b * N], hi = lo;
      for (int i = 1; i < N; ++i) {
        lo = T[b * N + i] < lo ? T[b * N + i] : lo;
        hi = T[b * N + i] > hi ? T[b * N + i] : hi;
      }
      wide = hi > kWideSpread * lo;
    }
    if (wide) {
      rc = anet_minco_solve_wide_spread_dev(ctx, s, c, N, batch, st.ld, d_head, d_tail, d_wps, d_T, kWideSpread,
                                            coeffs ? d_co : nullptr, d_en, ctx->stream);
      if (rc) return rc;
    }
  }
  if (energy) ANET_HIP(ctx, hipMemcpyAsync(energy, d_en, sizeof(double) * batch, hipMemcpyDeviceToHost, ctx->stream));
  if (coeffs) return st.download(d_co, n_co, coeffs);
  ANET_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANET_OK;
}

int anet_minco_sample_costs(anet_ctx *ctx, int s, int c, int n_pieces, int64_t samples, const double *head,
                            const double *tail, const double *wps, const double *T, double rho, double *cost) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, samples);
  if (rc) return rc;
  if (samples == 0) return ANET_OK;
  if (!head || !tail || !T || !cost || (n_pieces > 1 && !wps)) return fail(ctx, ANET_ERR_INVALID, "anet_minco_sample_costs: NULL pointer");
  const int N = n_pieces;
  // (the one problem -- head, tail, waypoints -- is shared by every sample: ldp = 1)
  Stager st(ctx, samples);
  double *d_T, *d_cost, *d_head, *d_tail, *d_wps;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(T, N, &d_T); p.rows(1, &d_cost);
    p.shared(head, 3 * c, &d_head); p.shared(tail, 3 * c, &d_tail); p.shared(wps, 3 * (int64_t)(N - 1), &d_wps);
  });
  if (rc) return rc;
  rc = anet_minco_sample_costs_dev(ctx, s, c, N, 1, samples, st.ld, 1, d_head, d_tail, d_wps, d_T, rho, d_cost, ctx->stream);
  if (rc) return rc;
  ANET_HIP(ctx, hipMemcpyAsync(cost, d_cost, sizeof(double) * samples, hipMemcpyDeviceToHost, ctx->stream));
  ANET_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANET_OK;
}

int anet_traj_eval(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs,
                   const double *T, int nq, const double *tq, int deriv, double *out) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0 || nq <= 0) return nq < 0 ? fail(ctx, ANET_ERR_INVALID, "nq < 0") : ANET_OK;
  if (!coeffs || !T || !tq || !out) return fail(ctx, ANET_ERR_INVALID, "anet_traj_eval: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_tq, *d_out;
  rc = st.stage([&](Stager::Pass &p) { p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T); p.in(tq, nq, &d_tq); p.out(3 * (int64_t)nq, &d_out); });
  if (rc) return rc;
  rc = anet_traj_eval_dev(ctx, s, n_pieces, batch, st.ld, d_co, d_T, nq, d_tq, deriv, d_out, ctx->stream);
  if (rc) return rc;
  return st.download(d_out, 3 * (int64_t)nq, out);
}

int anet_traj_cost(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs,
                   const double *T, double m34, double *cost) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !cost) return fail(ctx, ANET_ERR_INVALID, "anet_traj_cost: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_cost;
  rc = st.stage([&](Stager::Pass &p) { p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T); p.rows(1, &d_cost); });
  if (rc) return rc;
  rc = anet_traj_cost_dev(ctx, s, n_pieces, batch, st.ld, d_co, d_T, m34, d_cost, ctx->stream);
  if (rc) return rc;
  ANET_HIP(ctx, hipMemcpyAsync(cost, d_cost, sizeof(double) * batch, hipMemcpyDeviceToHost, ctx->stream));
  ANET_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANET_OK;
}

int anet_piece_normalized_coeffs_dev(anet_ctx *ctx, int s, int64_t pieces, const double *coeffs, const double *T, int deriv,
                                     double *out, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (s < 2 || s > 4 || pieces < 0 || deriv < 0 || deriv > 2)
    return fail(ctx, ANET_ERR_INVALID, "anet_piece_normalized_coeffs: order in [2, 4], pieces >= 0, deriv in [0, 2]");
  if (pieces == 0) return ANET_OK;
  if (!coeffs || !T || !out) return fail(ctx, ANET_ERR_INVALID, "anet_piece_normalized_coeffs: NULL pointer");
  anet::NormArgs a{coeffs, T, out, pieces, deriv};
  const dim3 grid((unsigned)((pieces + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_piece_normalize<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_piece_normalized_coeffs(anet_ctx *ctx, int s, int64_t pieces, const double *coeffs, const double *T, int deriv,
                                 double *out) {
  ANET_ON_DEVICE(ctx);
  if (s < 2 || s > 4 || pieces < 0 || deriv < 0 || deriv > 2)
    return fail(ctx, ANET_ERR_INVALID, "anet_piece_normalized_coeffs: order in [2, 4], pieces >= 0, deriv in [0, 2]");
  if (pieces == 0) return ANET_OK;
  if (!coeffs || !T || !out) return fail(ctx, ANET_ERR_INVALID, "anet_piece_normalized_coeffs: NULL pointer");
  const size_t nin = (size_t)pieces * 3 * 2 * s, nout = (size_t)pieces * 3 * (2 * s - deriv);
  double *d_co, *d_T, *d_out;
  int rc = stage_scratch(ctx, [&](void *w) {
    anet::Cursor c(w);
    d_co = c.take<double>(nin); d_T = c.take<double>(pieces); d_out = c.take<double>(nout);
    return c.bytes;
  });
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  ANET_HIP(ctx, hipMemcpyAsync(d_co, coeffs, sizeof(double) * nin, hipMemcpyHostToDevice, st));
  ANET_HIP(ctx, hipMemcpyAsync(d_T, T, sizeof(double) * pieces, hipMemcpyHostToDevice, st));
  if ((rc = anet_piece_normalized_coeffs_dev(ctx, s, pieces, d_co, d_T, deriv, d_out, st))) return rc;
  ANET_HIP(ctx, hipMemcpyAsync(out, d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, st));
  ANET_HIP(ctx, hipStreamSynchronize(st));
  return ANET_OK;
}

int anet_traj_cost_grad_T_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld,
                              const double *coeffs, const double *T, double m34, double *gradT, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !gradT || ld < batch) return fail(ctx, ANET_ERR_INVALID, "anet_traj_cost_grad_T_dev: NULL pointer or ld < batch");
  return launch_traj_cost(ctx, s, anet::CostArgs{coeffs, T, nullptr, gradT, batch, ld, n_pieces, m34}, (hipStream_t)stream);
}

int anet_traj_cost_grad_T(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs,
                          const double *T, double m34, double *gradT) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !gradT) return fail(ctx, ANET_ERR_INVALID, "anet_traj_cost_grad_T: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_g;
  rc = st.stage([&](Stager::Pass &p) { p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T); p.out(n_pieces, &d_g); });
  if (rc) return rc;
  rc = anet_traj_cost_grad_T_dev(ctx, s, n_pieces, batch, st.ld, d_co, d_T, m34, d_g, ctx->stream);
  if (rc) return rc;
  return st.download(d_g, n_pieces, gradT);
}

int anet_traj_max_rate_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld,
                           const double *coeffs, const double *T, int which, double *rate, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (which != 1 && which != 2) return fail(ctx, ANET_ERR_INVALID, "anet_traj_max_rate: which must be 1 (velocity) or 2 (acceleration)");
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !rate || ld < batch) return fail(ctx, ANET_ERR_INVALID, "anet_traj_max_rate_dev: NULL pointer or ld < batch");
  anet::RateArgs a{coeffs, T, rate, batch, ld, n_pieces, which};
  const dim3 grid((unsigned)((batch + 63) / 64), (unsigned)n_pieces), block(64);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_piece_max_rate<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_max_rate(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs,
                       const double *T, int which, double *rate) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !rate) return fail(ctx, ANET_ERR_INVALID, "anet_traj_max_rate: NULL pointer");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_r;
  rc = st.stage([&](Stager::Pass &p) { p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T); p.out(n_pieces, &d_r); });
  if (rc) return rc;
  rc = anet_traj_max_rate_dev(ctx, s, n_pieces, batch, st.ld, d_co, d_T, which, d_r, ctx->stream);
  if (rc) return rc;
  return st.download(d_r, n_pieces, rate);
}

}  // extern "C"
