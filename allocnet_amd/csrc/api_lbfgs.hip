// L-BFGS: parameters, the host and device optimisers, MVIE, the MINCO optimisation, launch order, spread flags, cancel flag;
// FIRI and polytope depth, which launch the MVIE kernels of this unit (include/allocnet_amd.h).
#include "api_internal.h"
#include "lbfgs_kernels.h"
#include "mvie_kernels.h"
#include "lbfgs_minco_persistent.h"
#include "firi_kernels.h"

namespace {

// ---- L-BFGS driver ----------------------------------------------------------------------------
static anet::LbfgsP to_kernel_params(const anet_lbfgs_params &p) {
  return anet::LbfgsP{p.mem_size, p.g_epsilon, p.past, p.delta, p.max_iterations, p.max_linesearch,
                      p.min_step, p.max_step, p.f_dec_coeff, p.s_curv_coeff, p.cautious_factor, p.machine_prec};
}

using anet::LbfgsLayout;  // (workspace.h)

// The kernels' view of a layout for B problems.  wave: the internal vectors (xp, gp, d, lm_s, lm_y) problem-major (element i
// of problem b at [i + b*n]: one wave per problem), else batch-minor (one lane per problem).  What a call site has beyond
// this -- variable map, step bound, cancel word, host callbacks -- it sets by field name.
static anet::LbfgsArgs lbfgs_args(const LbfgsLayout &L, int64_t B, const anet_lbfgs_params &p, bool wave) {
  anet::LbfgsArgs a{};
  a.n = L.n; a.B = B; a.ld = L.ld;
  a.x = L.x; a.g = L.g; a.xp = L.xp; a.gp = L.gp; a.d = L.d; a.lm_s = L.lm_s; a.lm_y = L.lm_y; a.lm_ys = L.lm_ys;
  a.lm_alpha = L.lm_alpha; a.pf = L.pf; a.ds = L.ds; a.feval = L.feval; a.is = L.is;
  a.p = to_kernel_params(p);
  a.vs = wave ? 1 : L.ld; a.ps = wave ? L.n : 1;
  return a;
}
// a fresh run: every IS_* / DS_* row zero
static hipError_t lbfgs_reset(const LbfgsLayout &L, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(L.is, 0, sizeof(int) * anet::IS_COUNT_ * L.ld, st);
  return e != hipSuccess ? e : hipMemsetAsync(L.ds, 0, sizeof(double) * anet::DS_COUNT_ * L.ld, st);
}

// eval(): enqueue the objective at L.x -> L.feval, L.g (for all problems).  The loop advances every
// problem by one evaluation per pass and polls an "any problem still running" flag every `poll` passes.
// The poll is one group behind the enqueue: the flag of group g is read only after group g+1 is in the
// stream, so the device never idles while the host looks.  The price is up to `poll` extra passes after the
// last problem stopped; they change nothing (finished problems ignore evaluations).
template <class Eval>
static int lbfgs_drive(anet_ctx *ctx, LbfgsLayout &L, int64_t B, const anet_lbfgs_params &prm, int max_evals,
                       hipStream_t st, Eval &&eval, double *map_T = nullptr, int map_nw = 0, bool reset = true,
                       int sb_on = 0, double sb_xmin = 0.0, const int32_t *cancel = nullptr) {
  int rc = ensure_counter(ctx);
  if (rc) return rc;
  if (reset) ANET_HIP(ctx, lbfgs_reset(L, st));  // (a caller that pre-marks problems as finished resets the state itself)
  // one wave per problem (DPP reductions, internal vectors problem-major) whenever the problem fits a wave's registers, at every
  // batch size -- at 131072 x 29 variables the lane-per-problem update kernel took 1.67 ms per tick (three times the objective
  // evaluation), the wave kernel 0.4 ms --; otherwise one lane per problem (internal vectors batch-minor)
  const bool wave = L.n <= 128 && prm.mem_size <= 64;
  anet::LbfgsArgs a = lbfgs_args(L, B, prm, wave);
  a.map_T = map_T; a.map_nw = map_nw;
  a.sb_on = sb_on; a.sb_lo = map_nw; a.sb_xmin = sb_xmin;
  a.cancel = (const int *)cancel;
  const dim3 grid(wave ? (unsigned)B : (unsigned)((B + 63) / 64)), block(64);
  const int poll = 8;
  int group = 0;
  for (int it = 0; it < max_evals; ++it) {
    if ((rc = eval())) return rc;
    const bool check = ((it + 1) % poll == 0) || it + 1 == max_evals;
    if (check) ANET_HIP(ctx, hipMemsetAsync(ctx->d_counter, 0, sizeof(int), st));
    a.n_active = check ? ctx->d_counter : nullptr;
    // `waves` waves per workgroup, `per` problems per wave
    auto launch = [&](auto kernel, int waves, int per) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)((B + per * waves - 1) / (per * waves))), dim3(64u * waves), 0, st, a);
    };
    const int m = a.p.mem_size;
    const bool one = L.n <= 64;  // one variable per lane: half the registers
    constexpr int W8 = anet::LbfgsWaveShape<8>::kWaves, W20 = anet::LbfgsWaveShape<20>::kWaves, W0 = anet::LbfgsWaveShape<0>::kWaves;
    if (!wave) hipLaunchKernelGGL(anet::k_lbfgs_update, grid, block, 0, st, a);
    else if (m <= 8 && L.n <= 32) launch(anet::k_lbfgs_update_wave<8, 1, true>, W8, 2);  // two problems per wave
    else if (m <= 8 && one) launch(anet::k_lbfgs_update_wave<8, 1>, W8, 1);
    else if (m <= 8) launch(anet::k_lbfgs_update_wave<8, 2>, W8, 1);
    else if (m <= 20 && one) launch(anet::k_lbfgs_update_wave<20, 1>, W20, 1);
    else if (m <= 20) launch(anet::k_lbfgs_update_wave<20, 2>, W20, 1);
    else if (one) launch(anet::k_lbfgs_update_wave<0, 1>, W0, 1);
    else launch(anet::k_lbfgs_update_wave<0, 2>, W0, 1);
    ANET_HIP(ctx, hipGetLastError());
    if (check) {
      const int slot = group & 1;
      ANET_HIP(ctx, hipMemcpyAsync(ctx->h_counter + slot, ctx->d_counter, sizeof(int), hipMemcpyDeviceToHost, st));
      ANET_HIP(ctx, hipEventRecord(ctx->poll_ev[slot], st));
      if (group > 0) {
        ANET_HIP(ctx, hipEventSynchronize(ctx->poll_ev[slot ^ 1]));
        if (ctx->h_counter[slot ^ 1] == 0) break;
      }
      ++group;
    }
  }
  ANET_HIP(ctx, hipStreamSynchronize(st));
  return ANET_OK;
}

// The whole MVIE optimisation (nine variables, M rows) in one launch, one wave per problem: everything in registers when it
// fits (<= 128 rows, mem_size <= 20, past <= 64; k_lbfgs_mvie_resident), else the state goes through memory
// (k_lbfgs_mvie_persistent, mem_size <= 64).  FIRI's call is the mem_size = 18 row of this ladder.
static void launch_mvie_one_launch(const anet::LbfgsArgs &la, const anet::MvieArgs &ma, int max_evals, hipStream_t st) {
  const int m = la.p.mem_size, M = ma.M;
  const int64_t batch = la.B;
  auto launch = [&](auto kernel, int waves) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((batch + waves - 1) / waves)), dim3(64u * waves), 0, st, la, ma, max_evals);
  };
  const bool resident = M <= 128 && m <= 20 && la.p.past <= 64 && !anet::env_set(anet::Tuning::mvie_state_in_memory);
  if (resident && m <= 8 && M <= 64) launch(anet::k_lbfgs_mvie_resident<8, 1>, 1);
  else if (resident && m <= 8) launch(anet::k_lbfgs_mvie_resident<8, 2>, 1);
  else if (resident && M <= 64) launch(anet::k_lbfgs_mvie_resident<20, 1>, 1);
  else if (resident) launch(anet::k_lbfgs_mvie_resident<20, 2>, 1);
  else if (m <= 8) launch(anet::k_lbfgs_mvie_persistent<8>, anet::LbfgsWaveShape<8>::kWaves);
  else if (m <= 20) launch(anet::k_lbfgs_mvie_persistent<20>, anet::LbfgsWaveShape<20>::kWaves);
  else launch(anet::k_lbfgs_mvie_persistent<0>, anet::LbfgsWaveShape<0>::kWaves);
}

// (shift 4: evaluation counts of an L-BFGS run, up to 65535; shift 0: Newton-step counts of the interior point, up to 4095)
__device__ __forceinline__ int order_bucket(int v, int shift) {
  const int top = (anet::kOrderBuckets << shift) - 1;
  v = v < 0 ? 0 : (v > top ? top : v);
  return anet::kOrderBuckets - 1 - (v >> shift);  // descending
}
__global__ void k_order_hist(const int *counts, int64_t B, int *hist, int shift) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b < B) atomicAdd(&hist[order_bucket(counts[b], shift)], 1);
}
__global__ void __launch_bounds__(1024) k_order_scan(int *hist) {  // exclusive scan of the 4096 bucket sizes, one workgroup
  __shared__ int part[1024];
  const int t = threadIdx.x;
  int v[4], sum = 0;
  for (int q = 0; q < 4; ++q) { v[q] = hist[4 * t + q]; sum += v[q]; }
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int run = part[t] - sum;
  for (int q = 0; q < 4; ++q) { hist[4 * t + q] = run; run += v[q]; }
}
__global__ void k_order_scatter(const int *counts, int64_t B, int *hist, int *order, int shift) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b < B) order[atomicAdd(&hist[order_bucket(counts[b], shift)], 1)] = (int)b;
}

// 1 where the durations of a trajectory spread over more than min_spread (max T > min_spread min T)
__global__ void k_spread_flags(const double *T, int64_t B, int64_t ld, int N, double min_spread, int32_t *flags) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double lo = T[b], hi = lo;
  for (int i = 1; i < N; ++i) {
    const double t = T[(int64_t)i * ld + b];
    lo = fmin(lo, t);
    hi = fmax(hi, t);
  }
  flags[b] = hi > min_spread * lo ? 1 : 0;
}

// status / iters / evals rows -> caller arrays (device or host destination)
__global__ void k_lbfgs_results(const int *is, const double *ds, int64_t B, int64_t ld, int *status, int *iters,
                                int *evals, double *f) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  if (status) status[b] = is[anet::IS_DONE * ld + b] ? is[anet::IS_RET * ld + b] : ANET_LBFGS_RUNNING;
  if (iters) iters[b] = is[anet::IS_K * ld + b];
  if (evals) evals[b] = is[anet::IS_EVALS * ld + b];
  // a problem no workgroup took (a launch order that skips it) has no cost: NaN, not whatever the workspace held
  if (f) f[b] = (is[anet::IS_DONE * ld + b] == 0 && is[anet::IS_EVALS * ld + b] == 0) ? __builtin_nan("") : ds[anet::DS_FX * ld + b];
}

}  // namespace

int launch_order_impl(anet_ctx *ctx, int64_t batch, const int32_t *counts, int32_t *launch_order, int32_t *work, void *stream,
                      int shift) {
  ANET_ON_DEVICE(ctx);
  if (batch < 0 || batch > 0x7fffffff) return fail(ctx, ANET_ERR_INVALID, "anet_launch_order_from_counts: bad batch");
  if (batch == 0) return ANET_OK;
  if (!counts || !launch_order || !work) return fail(ctx, ANET_ERR_INVALID, "anet_launch_order_from_counts_dev: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((batch + 255) / 256)), block(256);
  ANET_HIP(ctx, hipMemsetAsync(work, 0, sizeof(int) * anet::kOrderBuckets, st));
  hipLaunchKernelGGL(k_order_hist, grid, block, 0, st, counts, batch, work, shift);
  hipLaunchKernelGGL(k_order_scan, dim3(1), dim3(1024), 0, st, work);
  hipLaunchKernelGGL(k_order_scatter, grid, block, 0, st, counts, batch, work, launch_order, shift);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

extern "C" {

// ---- L-BFGS entry points -------------------------------------------------------------------------
void anet_lbfgs_default_params(anet_lbfgs_params *p) {
  if (!p) return;
  p->mem_size = 8; p->g_epsilon = 1.0e-5; p->past = 3; p->delta = 1.0e-6; p->max_iterations = 0;
  p->max_linesearch = 64; p->min_step = 1.0e-20; p->max_step = 1.0e+20; p->f_dec_coeff = 1.0e-4;
  p->s_curv_coeff = 0.9; p->cautious_factor = 1.0e-6; p->machine_prec = 1.0e-16;
}

int anet_lbfgs_check_params(int n, const anet_lbfgs_params *p) {
  if (!p) return -1024;
  if (n <= 0) return -1023;
  if (p->mem_size <= 0) return -1022;
  if (p->g_epsilon < 0.0) return -1021;
  if (p->past < 0) return -1020;
  if (p->delta < 0.0) return -1019;
  if (p->min_step < 0.0) return -1018;
  if (p->max_step < p->min_step) return -1017;
  if (!(p->f_dec_coeff > 0.0 && p->f_dec_coeff < 1.0)) return -1016;
  if (!(p->s_curv_coeff < 1.0 && p->s_curv_coeff > p->f_dec_coeff)) return -1015;
  if (!(p->machine_prec > 0.0)) return -1014;
  if (p->max_linesearch <= 0) return -1013;
  return 0;
}

const char *anet_lbfgs_strerror(int code) {
  switch (code) {
    case 0: return "Success: reached convergence (g_epsilon).";
    case 1: return "Success: met stopping criteria (past f decrease less than delta).";
    case 2: return "The iteration has been canceled by the monitor callback.";
    case -1024: return "Unknown error.";
    case -1023: return "Invalid number of variables specified.";
    case -1022: return "Invalid parameter lbfgs_parameter_t::mem_size specified.";
    case -1021: return "Invalid parameter lbfgs_parameter_t::g_epsilon specified.";
    case -1020: return "Invalid parameter lbfgs_parameter_t::past specified.";
    case -1019: return "Invalid parameter lbfgs_parameter_t::delta specified.";
    case -1018: return "Invalid parameter lbfgs_parameter_t::min_step specified.";
    case -1017: return "Invalid parameter lbfgs_parameter_t::max_step specified.";
    case -1016: return "Invalid parameter lbfgs_parameter_t::f_dec_coeff specified.";
    case -1015: return "Invalid parameter lbfgs_parameter_t::s_curv_coeff specified.";
    case -1014: return "Invalid parameter lbfgs_parameter_t::machine_prec specified.";
    case -1013: return "Invalid parameter lbfgs_parameter_t::max_linesearch specified.";
    case -1012: return "The function value became NaN or Inf.";
    case -1011: return "The line-search step became smaller than lbfgs_parameter_t::min_step.";
    case -1010: return "The line-search step became larger than lbfgs_parameter_t::max_step.";
    case -1009: return "Line search reaches the maximum try number, assumptions not satisfied or precision not achievable.";
    case -1008: return "The algorithm routine reaches the maximum number of iterations.";
    case -1007: return "Relative search interval width is at least lbfgs_parameter_t::machine_prec.";
    case -1006: return "A logic error (negative line-search step) occurred.";
    case -1005: return "The current search direction increases the cost function value.";
    case ANET_SFC_NO_OVERLAP: return "A waypoint's two polytopes have no overlap with an interior: the problem was not run.";
    case ANET_LBFGS_RUNNING: return "Still running: the evaluation budget (max_evals) was exhausted.";
    default: return "(unknown)";
  }
}

int anet_lbfgs_mvie(anet_ctx *ctx, int64_t batch, int M, const double *A, double smooth_eps,
                    double penalty_wt, double *x, double *f, const anet_lbfgs_params *params,
                    int max_evals, int32_t *status, int32_t *iters, int32_t *evals) {
  ANET_ON_DEVICE(ctx);
  int rc = check_lbfgs(ctx, 9, params, max_evals);
  if (rc) return rc;
  if (batch < 0 || M < 1 || !(smooth_eps > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_mvie: bad batch, M or smooth_eps");
  if (batch == 0) return ANET_OK;
  if (!A || !x) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_mvie: NULL pointer");
  const int n = 9, m = params->mem_size, npf = params->past > 1 ? params->past : 1;
  Stager st(ctx, batch);
  double *d_A, *d_x0;
  LbfgsLayout L;
  anet::LbfgsResultRows R;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(A, 3 * (int64_t)M, &d_A); p.in(x, n, &d_x0);  // (x comes back from L.x: the same width)
    L = anet::lbfgs_layout(p.c, n, m, npf, st.ld);
    R = anet::lbfgs_result_rows(p.c, st.ld);
  });
  if (rc) return rc;
  hipStream_t s0 = ctx->stream;
  ANET_HIP(ctx, hipMemcpyAsync(L.x, d_x0, sizeof(double) * n * st.ld, hipMemcpyDeviceToDevice, s0));
  anet::MvieArgs ma{d_A, L.x, L.feval, L.g, L.is, batch, st.ld, M, smooth_eps, penalty_wt};
  const dim3 grid((unsigned)((batch + 63) / 64)), block(64);
  if (params->mem_size <= 64) {
    // one wave per problem, the whole optimisation in one launch (k_lbfgs_mvie_persistent)
    ANET_HIP(ctx, lbfgs_reset(L, s0));
    launch_mvie_one_launch(lbfgs_args(L, batch, *params, true), ma, max_evals, s0);
    ANET_HIP(ctx, hipGetLastError());
  } else {
    rc = lbfgs_drive(ctx, L, batch, *params, max_evals, s0, [&]() -> int {
      hipLaunchKernelGGL(anet::k_mvie_eval, grid, block, 0, s0, ma);
      ANET_HIP(ctx, hipGetLastError());
      return ANET_OK;
    });
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_lbfgs_results, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s0, L.is, L.ds, batch,
                     st.ld, R.status, R.iters, R.evals, L.feval);
  ANET_HIP(ctx, hipGetLastError());
  if ((rc = download_results(ctx, batch, R, L.feval, status, iters, evals, f, s0))) return rc;
  return st.download(L.x, n, x);
}

int64_t anet_lbfgs_workspace(int n, int64_t ld, const anet_lbfgs_params *params) {
  if (!params || n < 1 || ld < 1) return 0;
  return anet::lbfgs_layout(nullptr, n, params->mem_size, params->past > 1 ? params->past : 1, ld).doubles;
}

int anet_lbfgs_optimize_dev(anet_ctx *ctx, int n, int64_t batch, int64_t ld, double *x, double *f, double *g,
                            anet_lbfgs_evaluate_t proc_evaluate, void *instance, const anet_lbfgs_params *params,
                            int max_evals, int bound_from, double bound_min, double *work, int32_t *status,
                            int32_t *iters, int32_t *evals, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_lbfgs(ctx, n, params, max_evals);
  if (rc) return rc;
  if (batch < 0 || ld < batch) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_optimize_dev: batch < 0 or ld < batch");
  if (batch == 0) return ANET_OK;
  if (!x || !f || !g || !proc_evaluate || !work) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_optimize_dev: NULL pointer");
  const int m = params->mem_size, npf = params->past > 1 ? params->past : 1;
  LbfgsLayout L = anet::lbfgs_layout(work, n, m, npf, ld);
  L.x = x;      // the caller's buffers: what its callback reads and fills
  L.g = g;
  L.feval = f;
  hipStream_t st = (hipStream_t)stream;
  int cb_rc = 0;
  rc = lbfgs_drive(ctx, L, batch, *params, max_evals, st, [&]() -> int {
    cb_rc = proc_evaluate(instance, L.x, L.feval, L.g, batch, ld, n, stream);
    return cb_rc ? fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_optimize_dev: proc_evaluate returned non-zero") : ANET_OK;
  }, nullptr, bound_from < n ? (bound_from > 0 ? bound_from : 0) : n, true, bound_from < n ? 1 : 0, bound_min, ctx->cancel_flag);
  if (rc) return rc;
  hipLaunchKernelGGL(k_lbfgs_results, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, L.is, L.ds, batch, ld, status,
                     iters, evals, f);
  ANET_HIP(ctx, hipGetLastError());
  // the run synchronises `stream` as it goes (completion polls); so does its end: status / iters / evals / f are complete
  // when this returns, whatever stream the caller reads them on
  ANET_HIP(ctx, hipStreamSynchronize(st));
  return ANET_OK;
}

int anet_lbfgs_optimize_host(anet_ctx *ctx, int n, double *x, double *f, anet_lbfgs_host_evaluate_t proc_evaluate,
                             anet_lbfgs_host_stepbound_t proc_stepbound, anet_lbfgs_host_progress_t proc_progress,
                             void *instance, const anet_lbfgs_params *params, int32_t *ret, int32_t *iters, int32_t *evals) {
  ANET_ON_DEVICE(ctx);
  if (!x || !f || !proc_evaluate || !ret) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_optimize_host: NULL argument");
  if (iters) *iters = 0;
  if (evals) *evals = 0;
  // lbfgs_optimize's own parameter validation, in its order, is its return value (lbfgs.hpp:449-495)
  const int code = anet_lbfgs_check_params(n, params);
  if (code) {
    *ret = code;
    return ANET_OK;
  }
  const int m = params->mem_size, npf = params->past > 1 ? params->past : 1;
  // device: the optimiser's state (row stride 1: one problem) + f + the cancel word; host: g, xp, d.  An allocation of THIS
  // call, not the context's scratch: the callbacks run while the state is live and may call any host-staged entry point on
  // the same context (anet_minco_cost_grad, anet_traj_*, another anet_lbfgs_optimize_host ...), which re-carve -- or free and
  // re-allocate -- that scratch (lbfgs::lbfgs_optimize<V>, Piece and Trajectory all use Context::thread_default()).
  LbfgsLayout L{};
  int *d_cancel = nullptr;
  auto layout = [&](void *w) { anet::Cursor c(w); L = anet::lbfgs_layout(c, n, m, npf, 1); d_cancel = c.take<int>(1); return c.bytes; };
  struct OwnBuffer {
    void *p = nullptr;
    ~OwnBuffer() { if (p) (void)hipFree(p); }
  } own;
  {
    hipError_t e = hipMalloc(&own.p, (size_t)layout(nullptr));
    if (e != hipSuccess) {
      own.p = nullptr;
      return fail(ctx, ANET_ERR_NOMEM, std::string("anet_lbfgs_optimize_host: hipMalloc: ") + hipGetErrorString(e));
    }
  }
  int rc = ANET_OK;
  (void)layout(own.p);
  hipStream_t st = ctx->stream;
  std::vector<double> hg((size_t)n), hxp((size_t)n), hd((size_t)n);
  ANET_HIP(ctx, lbfgs_reset(L, st));
  ANET_HIP(ctx, hipMemsetAsync(d_cancel, 0, sizeof(int), st));
  ANET_HIP(ctx, hipMemcpyAsync(L.x, x, sizeof(double) * n, hipMemcpyHostToDevice, st));
  anet::LbfgsArgs a = lbfgs_args(L, 1, *params, false);
  a.cancel = d_cancel;
  a.host_pg = proc_progress ? 1 : 0;
  a.host_sb = proc_stepbound ? 1 : 0;
  int his[anet::IS_COUNT_];
  double hds[anet::DS_COUNT_];
  // sources of the small host-to-device copies below: they live until the stream is synchronised in tick()
  double fv = 0.0, bound = 0.0;
  int word = 0;
  auto tick = [&]() -> int {  // one launch of the state machine, then its state on the host
    hipLaunchKernelGGL(anet::k_lbfgs_update, dim3(1), dim3(64), 0, st, a);
    ANET_HIP(ctx, hipGetLastError());
    ANET_HIP(ctx, hipMemcpyAsync(his, L.is, sizeof(his), hipMemcpyDeviceToHost, st));
    ANET_HIP(ctx, hipMemcpyAsync(hds, L.ds, sizeof(hds), hipMemcpyDeviceToHost, st));
    ANET_HIP(ctx, hipStreamSynchronize(st));
    return ANET_OK;
  };
  for (;;) {
    // the point to evaluate is in L.x (the host's copy in x: the start point, or what the last tick left)
    fv = proc_evaluate(instance, x, hg.data(), n);
    ANET_HIP(ctx, hipMemcpyAsync(L.g, hg.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
    ANET_HIP(ctx, hipMemcpyAsync(L.feval, &fv, sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = tick())) return rc;
    while (!his[anet::IS_DONE] && (his[anet::IS_PHASE] == anet::LB_PHASE_AWAIT_PROGRESS || his[anet::IS_PHASE] == anet::LB_PHASE_AWAIT_STEPBOUND)) {
      if (his[anet::IS_PHASE] == anet::LB_PHASE_AWAIT_PROGRESS) {
        // lbfgs.hpp:580-587: x is the accepted point (the one just evaluated), g its gradient
        const int verdict = proc_progress(instance, x, hg.data(), hds[anet::DS_FX], hds[anet::DS_STEP], his[anet::IS_K], his[anet::IS_COUNT], n);
        word = verdict ? 1 : 0;
        ANET_HIP(ctx, hipMemcpyAsync(d_cancel, &word, sizeof(int), hipMemcpyHostToDevice, st));
      } else {
        // lbfgs.hpp:557-565: xp (= the current point) and the search direction
        ANET_HIP(ctx, hipMemcpyAsync(hxp.data(), L.xp, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        ANET_HIP(ctx, hipMemcpyAsync(hd.data(), L.d, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        ANET_HIP(ctx, hipStreamSynchronize(st));
        bound = proc_stepbound(instance, hxp.data(), hd.data(), n);
        ANET_HIP(ctx, hipMemcpyAsync(L.ds + anet::DS_SMAX, &bound, sizeof(double), hipMemcpyHostToDevice, st));
      }
      if ((rc = tick())) return rc;
    }
    // the next point to evaluate -- or, when the run has ended, the result (a failed line search put xp back)
    ANET_HIP(ctx, hipMemcpyAsync(x, L.x, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    ANET_HIP(ctx, hipStreamSynchronize(st));
    if (his[anet::IS_DONE]) break;
  }
  *ret = his[anet::IS_RET];
  *f = hds[anet::DS_FX];
  if (iters) *iters = his[anet::IS_K];
  if (evals) *evals = his[anet::IS_EVALS];
  return ANET_OK;
}

// Does the workspace of N pieces end in the tail the two launches hand the parked optimisers over in?  Where the two-launch form
// of the one-launch shape can run: enough variables.  Whether a BATCH takes it is the context's decision -- lbfgs_minco_dev_impl,
// by the device's compute units -- and does not enter the size: the workspace is enough for either form at any batch <= ld.
static bool minco_ws_has_tail(int N) {
  return anet::tuning().lbfgs_split_evals > 1 && 3 * (N - 1) + N >= anet::tuning().lbfgs_split_min_vars;
}

int64_t anet_lbfgs_minco_workspace(int s, int n_pieces, int64_t ld, const anet_lbfgs_params *params) {
  if (!params || params->mem_size <= 0) return -1;
  const int n = 3 * (n_pieces - 1) + n_pieces, npf = params->past > 1 ? params->past : 1;
  return anet::lbfgs_minco_ws(nullptr, s, n_pieces, ld, params->mem_size, npf, n, minco_ws_has_tail(n_pieces)).doubles;
}

// Order of the second launch of a two-launch L-BFGS run (lbfgs_minco_persistent.h PersistArgs::park): larger = expected to need more
// evaluations.  What predicts it at the split point (4096 problems of BASELINE configs[3], parked after 1000 evaluations;
// Spearman 0.61 with the evaluations left, and the order it gives simulates to the longest-first makespan): the gradient norm
// relative to the cost and the relative decrease of the cost over the last half of the first part, in decades.  Problems that
// ended in the first part score 0 and come last (their waves leave at once).
__global__ void k_lbfgs_resume_score(const int *is, const double *cont, int64_t B, int64_t ld, int *score) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int sc = 0;
  if (is[(int64_t)anet::IS_DONE * ld + b] == 0) {
    const double *u = anet::parked_uniform(cont + b * (int64_t)anet::kPersistContDoubles);
    const double fx = fabs(u[anet::PARK_U_FX]) + 1e-300, dec = fmax((u[anet::PARK_U_F_HALF] - u[anet::PARK_U_FX]) / fx, 1e-16),
                 gn = sqrt(fmax(u[anet::PARK_U_GN2], 0.0)) / fx;
    double v = 4000.0 + 150.0 * (log10(fmax(gn, 1e-16)) + log10(dec));
    if (!(v == v)) v = 4000.0;
    sc = (int)fmin(fmax(v, 1.0), 4000.0);
  }
  score[b] = sc;
}

int anet_launch_order_from_counts_dev(anet_ctx *ctx, int64_t batch, const int32_t *counts, int32_t *launch_order,
                                      int32_t *work, void *stream) {
  return launch_order_impl(ctx, batch, counts, launch_order, work, stream, 4);
}

int anet_launch_order_from_steps_dev(anet_ctx *ctx, int64_t batch, const int32_t *steps, int32_t *launch_order,
                                     int32_t *work, void *stream) {
  return launch_order_impl(ctx, batch, steps, launch_order, work, stream, 0);
}

int anet_minco_spread_flags_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, const double *T, double min_spread,
                                int32_t *flags, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (n_pieces < 1 || batch < 0) return fail(ctx, ANET_ERR_INVALID, "anet_minco_spread_flags_dev: n_pieces >= 1, batch >= 0");
  if (batch == 0) return ANET_OK;
  if (!T || !flags || ld < batch) return fail(ctx, ANET_ERR_INVALID, "anet_minco_spread_flags_dev: NULL pointer or ld < batch");
  hipLaunchKernelGGL(k_spread_flags, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, T, batch, ld,
                     n_pieces, min_spread > 0.0 ? min_spread : kWideSpread, flags);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

// Coefficients of the RETURNED waypoints / durations: the fast (reduced-system) solve, then the pivoted collocation solve
// for the trajectories whose optimised durations spread over more than kWideSpread -- inside the optimisation loop the
// cost and its gradient keep the reduced system's accuracy envelope, what is handed back does not.
static int final_coeffs(anet_ctx *ctx, int s, int c, int N, int64_t batch, int64_t ld, const double *head, const double *tail,
                        const double *wps, const double *T, double *coeffs_out, hipStream_t st) {
  int rc = anet_minco_solve_dev(ctx, s, c, N, batch, ld, head, tail, wps, T, coeffs_out, nullptr, st);
  if (rc) return rc;
  return anet_minco_solve_wide_spread_dev(ctx, s, c, N, batch, ld, head, tail, wps, T, kWideSpread, coeffs_out, nullptr, st);
}

int anet_set_cancel_flag(anet_ctx *ctx, const int32_t *flag) {
  if (!ctx) return ANET_ERR_INVALID;
  ctx->cancel_flag = flag;
  return ANET_OK;
}

int anet_lbfgs_minco_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                         const double *head, const double *tail, double *wps, double *T,
                         const double *hpolys, const anet_penalty *pen, const anet_lbfgs_params *params,
                         int opt_flags, int max_evals, double *work, double *cost, double *coeffs_out,
                         int32_t *status, int32_t *iters, int32_t *evals, void *stream) {
  return anet_lbfgs_minco_ordered_dev(ctx, s, c, n_pieces, batch, ld, head, tail, wps, T, hpolys, pen, params, opt_flags,
                                      max_evals, nullptr, work, cost, coeffs_out, status, iters, evals, stream);
}

static int lbfgs_minco_dev_impl(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                               const double *head, const double *tail, double *wps, double *T,
                               const double *hpolys, const anet_penalty *pen, const anet_lbfgs_params *params,
                               int opt_flags, int max_evals, double min_duration, const int32_t *launch_order, double *work,
                               double *cost, double *coeffs_out, int32_t *status, int32_t *iters, int32_t *evals, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_penalty(ctx, pen))) return rc;
  const int N = n_pieces;
  const int nw = (opt_flags & ANET_OPT_WAYPOINTS) ? 3 * (N - 1) : 0;
  const int nt = (opt_flags & ANET_OPT_TIMES) ? N : 0;
  const int n = nw + nt;
  if (n <= 0) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco: nothing to optimise (opt_flags / N)");
  if ((rc = check_lbfgs(ctx, n, params, max_evals))) return rc;
  if (batch == 0) return ANET_OK;
  if (!head || !tail || !T || (N > 1 && !wps) || !work || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco_dev: NULL pointer or ld < batch");
  const int m = params->mem_size, npf = params->past > 1 ? params->past : 1;
  const anet::LbfgsMincoWs W = anet::lbfgs_minco_ws(work, s, N, ld, m, npf, n, minco_ws_has_tail(N));
  LbfgsLayout L = W.opt;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g256((unsigned)((batch + 255) / 256)), b256(256);
  anet::MapArgs mp{L.x, wps, T, batch, ld, nw, nt, 0};
  const dim3 gmap(g256.x, (unsigned)n);
  hipLaunchKernelGGL(anet::k_minco_map, gmap, b256, 0, st, mp);
  ANET_HIP(ctx, hipGetLastError());
  // No per-evaluation mapping launches: the optimised waypoints ARE the first nw rows of x (same layout),
  // their gradient goes straight into g, the update kernel writes T = forward_T(tau) next to x, and the
  // propagate kernel applies dT/dtau to the duration gradient.
  const double *wps_eval = nw ? L.x : wps;
  double *gP_out = nw ? L.g : W.gP, *gT_out = nt ? L.g + (int64_t)nw * ld : W.gT;
  const double *tau = nt ? L.x + (int64_t)nw * ld : nullptr;
  // One launch, one wave per problem (lbfgs_minco_persistent.h) whenever the problem fits a wave: every problem runs
  // until ITS OWN stop instead of the batch advancing in lockstep, four launches per evaluation.  The launch-per-
  // evaluation kernels (all 64 lanes busy in the chains) have up to twice the throughput per evaluation STEP at batches
  // of 10^5, but a run to convergence is as long as its slowest member times the whole batch there: 131072 x 8-segment
  // snap 2.3 s in one launch against 4.1 s in lockstep, 131072 x 16-segment jerk 3.5 s against 10.0 s.  So one launch
  // at any batch; callers with a small fixed evaluation budget at a huge batch ask for the lockstep shape (ANET_OPT_LOCKSTEP).
  const int Mrows = (pen && hpolys) ? pen->poly_rows : 0;
  // the minimum-duration bound of either shape, in the variable tau (gcopter's backwardT, minco_core.h backward_T)
  const int step_bound = (min_duration > 0.0 && nt > 0) ? 1 : 0;
  const double tau_min = minco_tau_min(min_duration);
  // final parameters (x may have been reverted by a failed line search) and outputs
  auto finish = [&]() -> int {
    mp.mode = 1;
    hipLaunchKernelGGL(anet::k_minco_map, gmap, b256, 0, st, mp);
    ANET_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lbfgs_results, g256, b256, 0, st, L.is, L.ds, batch, ld, status, iters, evals, cost);
    ANET_HIP(ctx, hipGetLastError());
    return coeffs_out ? final_coeffs(ctx, s, c, N, batch, ld, head, tail, wps, T, coeffs_out, st) : ANET_OK;
  };
  const size_t row_bytes = sizeof(double) * anet::persist_lds_row_doubles(N, Mrows);
  if (!(opt_flags & ANET_OPT_LOCKSTEP) && (s == 3 || s == 4) && n <= 64 &&
      params->mem_size <= 8 && params->past <= 64) {
    anet::PersistArgs pa{};
    pa.head = head; pa.tail = tail; pa.wps = wps; pa.T = T; pa.hpolys = Mrows ? hpolys : nullptr;
    pa.x = L.x; pa.is = L.is; pa.ds = L.ds; pa.order = launch_order; pa.B = batch; pa.ld = ld;
    pa.N = N; pa.c = c; pa.nw = nw; pa.nt = nt; pa.M = Mrows; pa.max_evals = max_evals; pa.with_penalty = pen ? 1 : 0;
    if (pen) pa.pp = anet::to_kernel_penalty(*pen, Mrows);
    else pa.pp = anet::Penalty{0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1, 0};
    pa.inv_mu = 1.0 / pa.pp.mu; pa.inv_res = 1.0 / (double)pa.pp.res;
    pa.p = to_kernel_params(*params);
    pa.step_bound = step_bound;
    pa.cancel = (const int *)ctx->cancel_flag;
    pa.tau_min = tau_min;
#ifdef ANET_PERSIST_PROF
    static long long *d_prof = nullptr;
    if (!d_prof) ANET_HIP(ctx, hipMalloc((void **)&d_prof, 16 * sizeof(long long)));
    ANET_HIP(ctx, hipMemsetAsync(d_prof, 0, 16 * sizeof(long long), st));
    pa.prof = d_prof;
#endif
    // a caller-supplied launch order is not checked: a problem it skips (out-of-range or repeated entries) must report
    // ANET_LBFGS_RUNNING with zero counters, not whatever the workspace held
    if (launch_order) ANET_HIP(ctx, hipMemsetAsync(L.is, 0, sizeof(int) * anet::IS_COUNT_ * ld, st));
    // Batches well beyond the 2048 resident waves in TWO launches: the first takes every problem through the same number of
    // evaluations (equally long waves: no late starters), the second resumes the unfinished ones longest-expected first.  The
    // batch of BASELINE configs[3] (4096 problems, 300..7400 evaluations) otherwise ends with whichever long problem happened to
    // start in the second round: 0.160 s against 0.117 s with the problems longest first by their true counts.
    // ... where it was measured to pay (tools/time_lbfgs_batch.py, 4096 problems unless noted, one launch -> two): 16 jerk pieces
    // 165 -> 140 ms (bench: 0.169 -> 0.133 s), 16 snap pieces 424 -> 389, 12 jerk pieces 107 -> 98, 10 jerk pieces 79 -> 77, 16 jerk
    // pieces x 8192 235 -> 216, x 16384 415 -> 403, x 3072 no change; 8 snap pieces 102 -> 100..109, 5 jerk pieces 23.5 -> 25, 5
    // snap pieces 37 -> 39 (their runs are a few hundred evaluations long: the split point lies behind most of them, and at 250..700
    // evaluations the parked state does not tell the long problems yet).  Hence: problems of at least 36 variables (ten pieces).
    // (A SECOND park / re-sort was measured in round 5 and not kept: profiles/r05_lbfgs_second_park.txt -- every stage boundary is
    //  a barrier for the whole batch, and what the better order of a third stage gains is less than what the second stage's own
    //  tail loses: configs[3] 136 -> 147 / 157 / 165 ms with the second boundary at 2000 / 2500 / 3000 evaluations.)
    const anet::Tuning &t = anet::tuning();
    const int split_evals = t.lbfgs_split_evals;
    const bool two_launches = split_evals > 1 && batch >= t.lbfgs_split_min_batch.at(ctx->cus) && n >= t.lbfgs_split_min_vars &&
                              !launch_order && max_evals > split_evals;
    const anet::ResumeTail &rt = W.tail;  // (two_launches implies minco_ws_has_tail)
    auto launch = [&](auto kernel, size_t fixed_bytes) -> int {
      const size_t lds = fixed_bytes + row_bytes;
      if (!two_launches) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(64), lds, st, pa);
        return ANET_OK;
      }
      // every problem through the first split_evals evaluations, parked; then the ones still running, longest-expected first
      pa.cont = rt.cont;
      pa.park = 1;
      pa.half_mark = split_evals / 2;
      pa.max_evals = split_evals;
      hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(64), lds, st, pa);
      return resume_parked(
          ctx, batch, rt, st,
          [&](int32_t *score) { hipLaunchKernelGGL(k_lbfgs_resume_score, g256, b256, 0, st, L.is, rt.cont, batch, ld, score); },
          [&](const int32_t *order) {
            pa.park = 0;
            pa.resume = 1;
            pa.half_mark = (split_evals + max_evals) / 2;
            pa.max_evals = max_evals;
            pa.order = order;
            hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(64), lds, st, pa);
            return ANET_OK;
          });
    };
    const size_t lds_cap = 64 * 1024;
    bool launched = true;
    if (s == 3 && N <= 8 && anet::persist_lds_fixed_bytes<3, 8>() + row_bytes <= lds_cap)
      rc = launch(anet::k_lbfgs_minco_persistent<3, 8, 8>, anet::persist_lds_fixed_bytes<3, 8>());
    else if (s == 3 && anet::persist_lds_fixed_bytes<3, 16>() + row_bytes <= lds_cap)
      rc = launch(anet::k_lbfgs_minco_persistent<3, 16, 8>, anet::persist_lds_fixed_bytes<3, 16>());
    else if (s == 4 && N <= 8 && anet::persist_lds_fixed_bytes<4, 8>() + row_bytes <= lds_cap)
      rc = launch(anet::k_lbfgs_minco_persistent<4, 8, 8>, anet::persist_lds_fixed_bytes<4, 8>());
    else if (s == 4 && anet::persist_lds_fixed_bytes<4, 16>() + row_bytes <= lds_cap)
      rc = launch(anet::k_lbfgs_minco_persistent<4, 16, 8>, anet::persist_lds_fixed_bytes<4, 16>());
    else
      launched = false;
    if (rc) return rc;  // (the counting sort between two launches cannot fail with these arguments; if it ever does: its error)
    if (launched) {
      ANET_HIP(ctx, hipGetLastError());
#ifdef ANET_PERSIST_PROF
      {
        long long h[16];
        ANET_HIP(ctx, hipMemcpyAsync(h, d_prof, sizeof(h), hipMemcpyDeviceToHost, st));
        ANET_HIP(ctx, hipStreamSynchronize(st));
        fprintf(stderr, "persist_prof cycles (problem 0): E1 %lld E2 %lld E3 %lld E4 %lld E5 %lld E6 %lld E7 %lld E8 %lld update %lld\n",
                h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9]);
      }
#endif
      return finish();
    }
  }
  // the lockstep shape: the same minimum-duration bound (one maximum over the duration variables per iteration) and the
  // same cancel word, looked at after every successful line search (lbfgs.hpp:557-565, 580-587)
  rc = lbfgs_drive(ctx, L, batch, *params, max_evals, st, [&]() -> int {
    return cost_grad_dev_impl(ctx, s, c, N, batch, ld, head, tail, wps_eval, T, hpolys, pen, W.cg.co, L.feval, gP_out,
                              gT_out, nullptr, st, tau);
  }, nt ? T : nullptr, nw, true, step_bound, tau_min, ctx->cancel_flag);
  return rc ? rc : finish();
}

int anet_lbfgs_minco_ordered_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                                 const double *head, const double *tail, double *wps, double *T,
                                 const double *hpolys, const anet_penalty *pen, const anet_lbfgs_params *params,
                                 int opt_flags, int max_evals, const int32_t *launch_order, double *work, double *cost,
                                 double *coeffs_out, int32_t *status, int32_t *iters, int32_t *evals, void *stream) {
  return lbfgs_minco_dev_impl(ctx, s, c, n_pieces, batch, ld, head, tail, wps, T, hpolys, pen, params, opt_flags, max_evals, 0.0,
                              launch_order, work, cost, coeffs_out, status, iters, evals, stream);
}

int anet_lbfgs_minco_bounded_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                                 const double *head, const double *tail, double *wps, double *T,
                                 const double *hpolys, const anet_penalty *pen, const anet_lbfgs_params *params,
                                 int opt_flags, int max_evals, double min_duration, const int32_t *launch_order, double *work,
                                 double *cost, double *coeffs_out, int32_t *status, int32_t *iters, int32_t *evals, void *stream) {
  if (ctx && !(min_duration >= 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco_bounded_dev: min_duration must be >= 0");
  return lbfgs_minco_dev_impl(ctx, s, c, n_pieces, batch, ld, head, tail, wps, T, hpolys, pen, params, opt_flags, max_evals,
                              min_duration, launch_order, work, cost, coeffs_out, status, iters, evals, stream);
}

static int lbfgs_minco_host_impl(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head,
                                 const double *tail, double *wps, double *T, const double *hpolys,
                                 const anet_penalty *pen, const anet_lbfgs_params *params, int opt_flags,
                                 int max_evals, double min_duration, double *cost, double *coeffs_out, int32_t *status,
                                 int32_t *iters, int32_t *evals) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_penalty(ctx, pen))) return rc;
  if (!params) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco: params is NULL");
  if (batch == 0) return ANET_OK;
  if (!head || !tail || !T || (n_pieces > 1 && !wps)) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco: NULL pointer");
  const int N = n_pieces;
  const int64_t nco = (int64_t)N * 3 * 2 * s;
  const int64_t M = (pen && hpolys) ? pen->poly_rows : 0;
  const int64_t nhp = (int64_t)N * M * 4;
  Stager st(ctx, batch);
  // (the workspace has terms that do not scale with ld: asked for with the stager's own row stride)
  const int64_t wtotal = anet_lbfgs_minco_workspace(s, N, st.ld, params);
  if (wtotal < 0) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco: bad lbfgs parameters");
  double *d_head, *d_tail, *d_wps, *d_T, *d_hp = nullptr, *d_co, *d_work, *d_cost;
  anet::LbfgsResultRows R;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(head, 3 * c, &d_head); p.in(tail, 3 * c, &d_tail); p.in(wps, (int64_t)(N - 1) * 3, &d_wps); p.in(T, N, &d_T);
    if (nhp) p.in(hpolys, nhp, &d_hp);
    p.out(nco, &d_co); p.doubles(wtotal, &d_work); p.rows(1, &d_cost);
    R = anet::lbfgs_result_rows(p.c, st.ld);
  });
  if (rc) return rc;
  rc = lbfgs_minco_dev_impl(ctx, s, c, N, batch, st.ld, d_head, d_tail, d_wps, d_T, d_hp, pen, params, opt_flags,
                            max_evals, min_duration, nullptr, d_work, d_cost, coeffs_out ? d_co : nullptr, R.status, R.iters, R.evals,
                            ctx->stream);
  if (rc) return rc;
  hipStream_t s0 = ctx->stream;
  if ((rc = download_results(ctx, batch, R, d_cost, status, iters, evals, cost, s0))) return rc;
  if (N > 1 && (rc = st.download(d_wps, (int64_t)(N - 1) * 3, wps))) return rc;
  if ((rc = st.download(d_T, N, T))) return rc;
  if (coeffs_out && (rc = st.download(d_co, nco, coeffs_out))) return rc;
  ANET_HIP(ctx, hipStreamSynchronize(s0));
  return ANET_OK;
}

int anet_lbfgs_minco(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head,
                     const double *tail, double *wps, double *T, const double *hpolys,
                     const anet_penalty *pen, const anet_lbfgs_params *params, int opt_flags,
                     int max_evals, double *cost, double *coeffs_out, int32_t *status, int32_t *iters,
                     int32_t *evals) {
  return lbfgs_minco_host_impl(ctx, s, c, n_pieces, batch, head, tail, wps, T, hpolys, pen, params, opt_flags, max_evals, 0.0,
                               cost, coeffs_out, status, iters, evals);
}

int anet_lbfgs_minco_bounded(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head,
                             const double *tail, double *wps, double *T, const double *hpolys,
                             const anet_penalty *pen, const anet_lbfgs_params *params, int opt_flags,
                             int max_evals, double min_duration, double *cost, double *coeffs_out, int32_t *status,
                             int32_t *iters, int32_t *evals) {
  if (ctx && !(min_duration >= 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_lbfgs_minco_bounded: min_duration must be >= 0");
  return lbfgs_minco_host_impl(ctx, s, c, n_pieces, batch, head, tail, wps, T, hpolys, pen, params, opt_flags, max_evals,
                               min_duration, cost, coeffs_out, status, iters, evals);
}

// ---- batched FIRI -------------------------------------------------------------------------------
void anet_firi_default_params(anet_firi_params *p) {
  if (!p) return;
  p->iterations = 4;       // firi.hpp:273
  p->epsilon = 1.0e-6;     // firi.hpp:274
  p->smooth_eps = 1.0e-2;  // firi.hpp:218
  p->penalty_wt = 1.0e+3;  // firi.hpp:219
  p->mvie_max_evals = 20000;  // a cap, not a tolerance: the reference has none; corridors cut off by it report ok = 2
}

static int firi_check(anet_ctx *ctx, int64_t batch, int n_bd, int max_points, int max_rows, const anet_firi_params &P) {
  if (batch < 0 || n_bd < 1 || n_bd > 64 || max_points < 0 || max_rows < 4 || P.iterations < 1 || !(P.epsilon >= 0.0) ||
      !(P.smooth_eps > 0.0) || P.mvie_max_evals < 1)
    return fail(ctx, ANET_ERR_INVALID, "anet_firi: bad argument (1 <= n_bd <= 64, max_rows >= 4, iterations >= 1)");
  if ((size_t)max_rows * 4 * sizeof(double) > 60 * 1024) return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_firi: max_rows too large");
  return ANET_OK;
}

// doubles of device workspace of anet_firi_dev: ellipsoid state, forward points, MVIE rows, L-BFGS state, flags
int64_t anet_firi_workspace(int64_t batch, int max_points, int max_rows) {
  if (batch < 0 || max_points < 0 || max_rows < 4) return -1;
  return anet::firi_ws(nullptr, batch, anet_recommended_ld(batch), max_points > 0 ? max_points : 1, max_rows).doubles;
}

int anet_firi_dev(anet_ctx *ctx, int64_t batch, int n_bd, int max_points, int max_rows, const double *bd,
                  const double *pc, const int32_t *n_points, const double *a, const double *b,
                  const anet_firi_params *params, double *work, double *hpoly, int32_t *n_rows, int32_t *ok,
                  double *ellipsoid, void *stream) {
  return anet_firi_var_dev(ctx, batch, n_bd, max_points, max_rows, bd, pc, n_points, a, b, nullptr, params, work, hpoly, n_rows,
                           ok, ellipsoid, stream);
}

int anet_firi_var_dev(anet_ctx *ctx, int64_t batch, int n_bd, int max_points, int max_rows, const double *bd,
                      const double *pc, const int32_t *n_points, const double *a, const double *b,
                      const int32_t *iterations, const anet_firi_params *params, double *work, double *hpoly,
                      int32_t *n_rows, int32_t *ok, double *ellipsoid, void *stream) {
  ANET_ON_DEVICE(ctx);
  anet_firi_params P;
  anet_firi_default_params(&P);
  if (params) P = *params;
  int rc = firi_check(ctx, batch, n_bd, max_points, max_rows, P);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!bd || (max_points > 0 && (!pc || !n_points)) || !a || !b || !work || !hpoly || !n_rows || !ok)
    return fail(ctx, ANET_ERR_INVALID, "anet_firi_dev: NULL pointer");
  const int H = max_rows, Np = max_points > 0 ? max_points : 1;
  // firi.hpp:212-217
  anet_lbfgs_params lp;
  anet_lbfgs_default_params(&lp);
  lp.mem_size = anet::kFiriLbfgsMem; lp.g_epsilon = 0.0; lp.min_step = 1.0e-32; lp.past = anet::kFiriLbfgsPast; lp.delta = 1.0e-7;
  const int64_t ld = anet_recommended_ld(batch);
  const size_t n_hp = (size_t)batch * H * 4;
  const anet::FiriWs W = anet::firi_ws(work, batch, ld, Np, H);
  const LbfgsLayout &L = W.opt;
  double *d_ell = W.ell, *d_A = W.A;
  hipStream_t st = (hipStream_t)stream;
  const int *d_np = n_points;
  if (max_points == 0) {  // no obstacle points at all: a zero count per corridor
    ANET_HIP(ctx, hipMemsetAsync(W.np0, 0, sizeof(int) * batch, st));
    d_np = W.np0;
  }
  ANET_HIP(ctx, hipMemsetAsync(hpoly, 0, sizeof(double) * n_hp, st));
  anet::FiriArgs fa{bd, pc, d_np, a, b, d_ell, W.fpc, W.flag, hpoly, n_rows, ok, batch, n_bd, Np, H, P.epsilon};
  const dim3 g64((unsigned)((batch + 63) / 64)), b64(64), gB((unsigned)batch), b256(256);
  hipLaunchKernelGGL(anet::k_firi_init, g64, b64, 0, st, fa);
  ANET_HIP(ctx, hipGetLastError());
  anet::FiriMvieArgs ma{hpoly, n_rows, ok, d_ell, d_A, L.x, L.is + (int64_t)anet::IS_DONE * ld, L.is + (int64_t)anet::IS_RET * ld,
                        W.mok, batch, ld, H};
  anet::MvieArgs ev{d_A, L.x, L.feval, L.g, L.is, batch, ld, H, P.smooth_eps, P.penalty_wt};
  const anet::LbfgsArgs la = lbfgs_args(L, batch, lp, true);  // (one wave per corridor; no "still running" counter)
  fa.iters = iterations; ma.iters = iterations;
  for (int loop = 0; loop < P.iterations; ++loop) {
    fa.pass = loop; ma.pass = loop;
    hipLaunchKernelGGL(anet::k_firi_planes, gB, b256, 0, st, fa);
    ANET_HIP(ctx, hipGetLastError());
    if (loop == P.iterations - 1) break;
    ANET_HIP(ctx, lbfgs_reset(L, st));
    hipLaunchKernelGGL(anet::k_firi_mvie_setup, gB, b256, sizeof(double) * H * 4, st, ma);
    ANET_HIP(ctx, hipGetLastError());
    launch_mvie_one_launch(la, ev, P.mvie_max_evals, st);  // the whole MVIE optimisation in one launch, one wave per corridor
    ANET_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(anet::k_firi_mvie_finish, g64, b64, 0, st, ma);
    ANET_HIP(ctx, hipGetLastError());
  }
  if (ellipsoid)
    ANET_HIP(ctx, hipMemcpy2DAsync(ellipsoid, sizeof(double) * 15, d_ell, sizeof(double) * anet::kFiriEll, sizeof(double) * 15, batch,
                                   hipMemcpyDeviceToDevice, st));
  return ANET_OK;
}

int anet_firi(anet_ctx *ctx, int64_t batch, int n_bd, int max_points, int max_rows, const double *bd,
              const double *pc, const int32_t *n_points, const double *a, const double *b,
              const anet_firi_params *params, double *hpoly, int32_t *n_rows, int32_t *ok, double *ellipsoid) {
  return anet_firi_var(ctx, batch, n_bd, max_points, max_rows, bd, pc, n_points, a, b, nullptr, params, hpoly, n_rows, ok, ellipsoid);
}

int anet_firi_var(anet_ctx *ctx, int64_t batch, int n_bd, int max_points, int max_rows, const double *bd,
                  const double *pc, const int32_t *n_points, const double *a, const double *b, const int32_t *iterations,
                  const anet_firi_params *params, double *hpoly, int32_t *n_rows, int32_t *ok, double *ellipsoid) {
  if (!ctx) return fail(nullptr, ANET_ERR_INVALID, "ctx is NULL");
  anet_firi_params P;
  anet_firi_default_params(&P);
  if (params) P = *params;
  int rc = firi_check(ctx, batch, n_bd, max_points, max_rows, P);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!bd || (max_points > 0 && (!pc || !n_points)) || !a || !b || !hpoly || !n_rows)
    return fail(ctx, ANET_ERR_INVALID, "anet_firi: NULL pointer");
  ANET_ON_DEVICE(ctx);
  const int H = max_rows, Np = max_points > 0 ? max_points : 1;
  const size_t n_bdv = (size_t)batch * n_bd * 4, n_pc = (size_t)batch * Np * 3, n_ab = (size_t)batch * 3;
  const size_t n_hp = (size_t)batch * H * 4, n_ell = (size_t)batch * 15;
  const int64_t n_work = anet_firi_workspace(batch, max_points, max_rows);
  double *d_bd, *d_pc, *d_a, *d_b, *d_hp, *d_el, *d_work;
  int *d_np, *d_nh, *d_ok, *d_it;
  rc = stage_scratch(ctx, [&](void *w) {
    anet::Cursor c(w);
    d_bd = c.take<double>(n_bdv); d_pc = c.take<double>(n_pc); d_a = c.take<double>(n_ab); d_b = c.take<double>(n_ab);
    d_hp = c.take<double>(n_hp); d_el = c.take<double>(n_ell); d_work = c.take<double>(n_work);
    d_np = c.take<int>(batch); d_nh = c.take<int>(batch); d_ok = c.take<int>(batch); d_it = c.take<int>(batch);
    (void)c.spare(16);
    return c.bytes;
  });
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  if (iterations) {  // (host array: checked here; the device variant clamps instead, it cannot look without a synchronisation)
    for (int64_t b = 0; b < batch; ++b)
      if (iterations[b] < 1 || iterations[b] > P.iterations)
        return fail(ctx, ANET_ERR_INVALID, "anet_firi_var: iterations[b] must be in [1, params->iterations]");
    ANET_HIP(ctx, hipMemcpyAsync(d_it, iterations, sizeof(int) * batch, hipMemcpyHostToDevice, st));
  }
  ANET_HIP(ctx, hipMemcpyAsync(d_bd, bd, sizeof(double) * n_bdv, hipMemcpyHostToDevice, st));
  if (max_points > 0) {
    ANET_HIP(ctx, hipMemcpyAsync(d_pc, pc, sizeof(double) * n_pc, hipMemcpyHostToDevice, st));
    ANET_HIP(ctx, hipMemcpyAsync(d_np, n_points, sizeof(int) * batch, hipMemcpyHostToDevice, st));
  }
  ANET_HIP(ctx, hipMemcpyAsync(d_a, a, sizeof(double) * n_ab, hipMemcpyHostToDevice, st));
  ANET_HIP(ctx, hipMemcpyAsync(d_b, b, sizeof(double) * n_ab, hipMemcpyHostToDevice, st));
  rc = anet_firi_var_dev(ctx, batch, n_bd, max_points, max_rows, d_bd, d_pc, d_np, d_a, d_b, iterations ? d_it : nullptr, &P,
                         d_work, d_hp, d_nh, d_ok, ellipsoid ? d_el : nullptr, st);
  if (rc) return rc;
  ANET_HIP(ctx, hipMemcpyAsync(hpoly, d_hp, sizeof(double) * n_hp, hipMemcpyDeviceToHost, st));
  ANET_HIP(ctx, hipMemcpyAsync(n_rows, d_nh, sizeof(int) * batch, hipMemcpyDeviceToHost, st));
  if (ok) ANET_HIP(ctx, hipMemcpyAsync(ok, d_ok, sizeof(int) * batch, hipMemcpyDeviceToHost, st));
  if (ellipsoid) ANET_HIP(ctx, hipMemcpyAsync(ellipsoid, d_el, sizeof(double) * n_ell, hipMemcpyDeviceToHost, st));
  ANET_HIP(ctx, hipStreamSynchronize(st));
  return ANET_OK;
}

int anet_polytope_depth_dev(anet_ctx *ctx, int64_t batch, int max_rows, const double *hpoly, int normalise,
                            double *depth, double *point, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (batch < 0 || max_rows < 1) return fail(ctx, ANET_ERR_INVALID, "anet_polytope_depth: bad batch or max_rows");
  // (the vertex enumeration is C(rows, 4): 1.7e8 candidates at 256 rows -- corridor polytopes have a few dozen)
  if (max_rows > 256) return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_polytope_depth: more than 256 rows per polytope");
  if (batch == 0) return ANET_OK;
  if (!hpoly || !depth) return fail(ctx, ANET_ERR_INVALID, "anet_polytope_depth_dev: NULL pointer");
  // active-set ascent, one lane per polytope, certified; what it cannot certify (NaN) goes to the vertex enumeration
  const bool enumerate_all = anet::env_set(anet::Tuning::polytope_depth_enumerate);
  anet::DepthArgs a{hpoly, depth, point, batch, max_rows, normalise ? 1 : 0, enumerate_all ? 0 : 1};
  if (!enumerate_all) {
    hipLaunchKernelGGL(anet::k_polytope_depth_simplex, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    ANET_HIP(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(anet::k_polytope_depth, dim3((unsigned)batch), dim3(256), sizeof(double) * max_rows * 4, (hipStream_t)stream, a);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_polytope_depth(anet_ctx *ctx, int64_t batch, int max_rows, const double *hpoly, int normalise,
                        double *depth, double *point) {
  ANET_ON_DEVICE(ctx);
  if (batch < 0 || max_rows < 1) return fail(ctx, ANET_ERR_INVALID, "anet_polytope_depth: bad batch or max_rows");
  if (batch == 0) return ANET_OK;
  if (!hpoly || !depth) return fail(ctx, ANET_ERR_INVALID, "anet_polytope_depth: NULL pointer");
  const size_t n_hp = (size_t)batch * max_rows * 4;
  double *d_hp, *d_depth, *d_pt;
  int rc = stage_scratch(ctx, [&](void *w) {
    anet::Cursor c(w);
    d_hp = c.take<double>(n_hp); d_depth = c.take<double>(batch); d_pt = c.take<double>(3 * batch);
    return c.bytes;
  });
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  ANET_HIP(ctx, hipMemcpyAsync(d_hp, hpoly, sizeof(double) * n_hp, hipMemcpyHostToDevice, st));
  rc = anet_polytope_depth_dev(ctx, batch, max_rows, d_hp, normalise, d_depth, point ? d_pt : nullptr, st);
  if (rc) return rc;
  ANET_HIP(ctx, hipMemcpyAsync(depth, d_depth, sizeof(double) * batch, hipMemcpyDeviceToHost, st));
  if (point) ANET_HIP(ctx, hipMemcpyAsync(point, d_pt, sizeof(double) * 3 * batch, hipMemcpyDeviceToHost, st));
  ANET_HIP(ctx, hipStreamSynchronize(st));
  return ANET_OK;
}

}  // extern "C"

// ---- what api_sfc.hip shares with this unit (api_internal.h): the update kernels stay compiled here only ----------------------
int lbfgs_drive_shared(anet_ctx *ctx, anet::LbfgsLayout &L, int64_t B, const anet_lbfgs_params &prm, int max_evals, hipStream_t st,
                       int (*eval)(void *), void *instance, double *map_T, int map_nw, bool reset, int sb_on, double sb_xmin,
                       const int32_t *cancel) {
  return lbfgs_drive(ctx, L, B, prm, max_evals, st, [&]() -> int { return eval(instance); }, map_T, map_nw, reset, sb_on, sb_xmin,
                     cancel);
}

int lbfgs_reset_shared(anet_ctx *ctx, const anet::LbfgsLayout &L, hipStream_t st) {
  ANET_HIP(ctx, lbfgs_reset(L, st));
  return ANET_OK;
}

int lbfgs_results_shared(anet_ctx *ctx, const anet::LbfgsLayout &L, int64_t B, int32_t *status, int32_t *iters, int32_t *evals,
                         double *f, hipStream_t st) {
  hipLaunchKernelGGL(k_lbfgs_results, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, L.is, L.ds, B, L.ld, status, iters, evals, f);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int minco_final_coeffs(anet_ctx *ctx, int s, int c, int N, int64_t batch, int64_t ld, const double *head, const double *tail,
                       const double *wps, const double *T, double *coeffs_out, hipStream_t st) {
  return final_coeffs(ctx, s, c, N, batch, ld, head, tail, wps, T, coeffs_out, st);
}

