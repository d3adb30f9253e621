// Cost + gradient: partial gradients, the adjoint, the basis tables of k_piece_grad and the one-launch decision
// (include/allocnet_amd.h).
#include "api_internal.h"
#include "minco_kernels.h"
#include "minco_fused_kernel.h"

namespace anet {
// the basis-table rows k_piece_grad reads (their layout: minco_kernels.h, at k_piece_grad)
static __global__ void __launch_bounds__(256) k_build_basis_table(double *tab, int res, int D) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= res * 4 * D) return;
  const int j = e / (4 * D), d = (e / D) % 4, col = e % D, k = D - 1 - col;
  const double tau = (double)j / (double)res;
  double v = 0.0;
  if (k >= d) {
    v = 1.0;
    for (int q = 0; q < d; ++q) v *= (double)(k - q);
    for (int q = 0; q < k - d; ++q) v *= tau;
  }
  tab[e] = v;
}
}  // namespace anet

namespace {

template <int S>
int launch_prop(anet_ctx *ctx, const anet::PropArgs &a, hipStream_t st) {
  const dim3 block(anet::kSolveBlock);
  if (a.B <= anet::tuning().axis_max_batch.at(ctx->cus)) {  // same small-batch split as launch_solve
    const dim3 g3((unsigned)((a.B + 20) / 21));
    anet::launch_propagate_axis(S, a, g3, block, st);  // (piece_grad_unit.hip: scheduled for ILP)
  } else {
    const dim3 grid((unsigned)((a.B + anet::kSolveBlock - 1) / anet::kSolveBlock));
    anet::with_minco_shape<S>(a.N, a.c, [&](auto sh) {
      using Sh = decltype(sh);
      hipLaunchKernelGGL((anet::k_minco_propagate<S, Sh::NB, Sh::EXACT, Sh::NPC>), grid, block, 0, st, a);
    });
  }
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}
int do_propagate(anet_ctx *ctx, int s, const anet::PropArgs &a, hipStream_t st) {
  return anet::with_order(s, [&](auto o) { return launch_prop<decltype(o)::value>(ctx, a, st); });
}

}  // namespace

// The basis table of k_piece_grad for (order, res): built once per context on the stream that first needs it; other streams are
// ordered behind the build by its event.  (Declared in api_internal.h: k_flat_piece_grad reads the same table.)
int basis_table(anet_ctx *ctx, int s, int res, hipStream_t st, const double **out) {
  int rc = ANET_OK;
  *out = nullptr;
  if (res > kBasisTableMaxRes) return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_penalty.res too large for the basis table");
  for (auto &t : ctx->tabs)
    if (t.s == s && t.res == res) {
      // built on another stream: order this stream behind the build (no host or device-wide synchronisation)
      if (t.built_on != st) ANET_HIP(ctx, hipStreamWaitEvent(st, t.ready, 0));
      *out = t.d;
    }
  if (!*out) {
    // (never freed before anet_destroy -- a launch on another stream may still read one: a caller that sweeps res over
    //  hundreds of values is told so instead of growing the context without bound, as for the tables of k_qp_ipm)
    if (ctx->tabs.size() >= kMaxTablesPerContext)
      return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_minco_partial_grads: more than 256 distinct (order, res) on one context");
    anet_ctx::BasisTable t{s, res, nullptr, st, nullptr};
    const int need = res * 4 * 2 * s;
    if ((rc = new_table(ctx, sizeof(double) * need, &t.d, &t.ready))) return rc;
    hipLaunchKernelGGL(anet::k_build_basis_table, dim3((unsigned)((need + 255) / 256)), dim3(256), 0, st, t.d, res, 2 * s);
    hipError_t e1 = hipGetLastError();
    if (e1 == hipSuccess) e1 = hipEventRecord(t.ready, st);
    if (e1 != hipSuccess) {
      drop_table(t.d, t.ready);
      return hip_fail(ctx, e1, "k_build_basis_table");
    }
    ctx->tabs.push_back(t);
    *out = t.d;
  }
  return rc;
}

namespace {

// The large-batch penalty kernel with the basis-table contractions on the FP64 matrix instructions (csrc/piece_grad_mx.h): built for
// res = 20, orders 3 and 4 (131 072 x 8 snap pieces: 295 us against 344; 65 536 x 16 jerk pieces: 287 against 296 -- six coefficients
// fill three quarters of the instructions' k and column tiles --, profiles/r06_piece_grad_mx.txt).  ANET_PG_MX=0: never (A-B runs).
// The launch shape of the penalty / energy-gradient kernel (launch_piece_grad): 0 a lane per (trajectory, piece); 1 two lanes per
// pair (small batches); 2 two lanes and the samples over a workgroup's four waves (fewest pairs); 3 k_piece_grad_mx
static int piece_grad_shape(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const anet_penalty *pen) {
  const anet::Tuning &t = anet::tuning();
  if (pen && batch <= t.axis_max_batch.at(ctx->cus)) return batch * n_pieces <= t.piece_sw_max_pairs.at(ctx->cus) ? 2 : 1;
  if (pen && pen->res == anet::kMxRes && (s == 3 || s == 4) && t.pg_mx) return 3;
  return 0;
}

// Does this evaluation run as ONE launch (k_minco_cost_grad_fused) or as solve -> piece gradients -> adjoint?  (c: the boundary
// count, or -1 when the caller does not know it: the thresholds of the vector phase 2 then)
static bool cost_grad_in_one_launch(const anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const anet_penalty *pen) {
  // Small batches in ONE launch (minco_fused_kernel.h): up to THREE rounds of one workgroup per CU for problems of up to eight pieces,
  // two rounds for longer ones (measured with the chains eliminated from both ends, one launch against three: 8192 x 8-seg snap 54.0
  // against 64.9 us, 12000: 79.5 / 83.8, 16384 = four rounds: 105.5 / 102.4 -- not taken; 4096 x 16-seg jerk 51.8 / 61.0, 2500: 48.7 /
  // 59.3) -- beyond that the three streaming kernels have the chip full anyway and are the better shape.
  // Round 6: where phase 2 runs on the matrix instructions and eight waves (the exact shapes at 20 samples per piece: launch_fused_t)
  // a round of groups costs 17 us instead of 27 and the crossover moves out -- 16 384 x 8-seg snap (four rounds) 68.7 us against 102.9,
  // 24 576 (six) 100.5 / 107.4, 32 768 (eight) 133.4 / 125.5: SIX rounds; 16 384 x 16-seg jerk (eight rounds of groups of 8) 131.4 / 150.6:
  // EIGHT.  (ANET_FUSED_MAX_GROUPS overrides; 0 disables.)
  const bool mx = pen && anet::fused_phase2_mx(s, c, n_pieces, pen->res);
  const int rounds = mx ? (n_pieces <= 8 ? 6 : 8) : (n_pieces <= 8 ? 3 : 2);
  const int64_t env_groups = anet::tuning().fused_max_groups;
  const int64_t fused_max_groups = env_groups >= 0 ? env_groups : rounds * (int64_t)ctx->cus;
  const int fg = pen ? anet::cost_grad_fused_group(s, n_pieces) : 0;
  return fg > 0 && (batch + fg - 1) / fg <= fused_max_groups && pen->res <= anet::kFusedMaxRes;
}

}  // namespace

int cost_grad_dev_impl(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                       const double *head, const double *tail, const double *wps,
                       const double *T, const double *hpolys, const anet_penalty *pen,
                       double *work, double *cost, double *gradP, double *gradT,
                       double *coeffs_out, void *stream, const double *tau) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_penalty(ctx, pen))) return rc;
  if (batch == 0) return ANET_OK;
  if (!work || !cost || !gradT || (n_pieces > 1 && !gradP))
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_cost_grad_dev: NULL output or workspace");
  if (cost_grad_in_one_launch(ctx, s, c, n_pieces, batch, pen)) {
    if (!head || !tail || !T || (n_pieces > 1 && !wps) || ld < batch)
      return fail(ctx, ANET_ERR_INVALID, "anet_minco_cost_grad_dev: NULL input or ld < batch");
    const double *tab = nullptr;
    if ((rc = basis_table(ctx, s, pen->res, (hipStream_t)stream, &tab))) return rc;
    anet::FusedArgs fa{head, tail, wps, T, pen->poly_rows > 0 ? hpolys : nullptr, cost, gradP, gradT, coeffs_out, tau, batch, ld,
                       n_pieces, c, anet::to_kernel_penalty(*pen, pen->poly_rows), 0};
#ifdef ANET_FUSED_PROF
    static long long *d_fprof = nullptr;
    if (!d_fprof) ANET_HIP(ctx, hipMalloc((void **)&d_fprof, 16 * sizeof(long long)));
    fa.prof = d_fprof;
#endif
    if (anet::launch_cost_grad_fused(s, fa, tab, (hipStream_t)stream, ctx->cus)) {
      ANET_HIP(ctx, hipGetLastError());
#ifdef ANET_FUSED_PROF
      if (anet::env_set("ANET_FUSED_PROF_PRINT")) {
        long long h[16];
        ANET_HIP(ctx, hipMemcpyAsync(h, d_fprof, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream));
        ANET_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
        static const char *nm[13] = {"loads1", "factor", "solve", "stash", "barrier1", "lds-in", "penalty", "energy+pairsum+reduce", "nodeform",
                                     "barrier2", "lds-in3", "fwd", "bwd"};
        fprintf(stderr, "fused_prof cycles (workgroup 0, thread 0):");
        for (int k = 0; k < 13; ++k) fprintf(stderr, " %s %lld", nm[k], h[k + 1] - h[k]);
        fprintf(stderr, " | total %lld\n", h[13] - h[0]);
      }
#endif
      return ANET_OK;
    }
  }
  const anet::CostGradWs W = anet::cost_grad_ws(work, s, n_pieces, ld);
  double *w_co = coeffs_out ? coeffs_out : W.co;
  rc = anet_minco_solve_dev(ctx, s, c, n_pieces, batch, ld, head, tail, wps, T, w_co, W.en, stream);
  if (rc) return rc;
  rc = anet_minco_partial_grads_dev(ctx, s, n_pieces, batch, ld, w_co, T, hpolys, pen, 1, W.gdC, W.gdT, W.pc, stream);
  if (rc) return rc;
  anet::PropArgs a{T, w_co, W.gdC, W.gdT, gradP, gradT, W.en, pen ? W.pc : nullptr, cost,
                   pen ? pen->rho : 0.0, batch, ld, n_pieces, c, tau};
  return do_propagate(ctx, s, a, (hipStream_t)stream);
}

extern "C" {

int anet_minco_piece_grad_shape(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const anet_penalty *pen) {
  if (!ctx) return fail(nullptr, ANET_ERR_INVALID, "ctx is NULL");
  if (s < 2 || s > 4 || n_pieces < 1 || n_pieces > ANET_MAX_PIECES || batch < 0)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_piece_grad_shape: bad shape");
  return piece_grad_shape(ctx, s, n_pieces, batch, pen);
}

int anet_minco_partial_grads_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld,
                                 const double *coeffs, const double *T, const double *hpolys,
                                 const anet_penalty *pen, int with_energy, double *gdC, double *gdT,
                                 double *piece_cost, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_penalty(ctx, pen))) return rc;
  if (batch == 0) return ANET_OK;
  if (!coeffs || !T || !gdC || !gdT || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_partial_grads_dev: NULL pointer or ld < batch");
  anet::PieceGradArgs a{};
  a.coeffs = coeffs; a.T = T; a.hpolys = (pen && pen->poly_rows > 0) ? hpolys : nullptr;
  a.gdC = gdC; a.gdT = gdT; a.pcost = piece_cost;
  a.B = batch; a.ld = ld; a.N = n_pieces; a.with_energy = with_energy ? 1 : 0; a.with_penalty = pen ? 1 : 0;
  if (pen) a.pp = anet::to_kernel_penalty(*pen, pen->poly_rows);
  const dim3 grid((unsigned)((batch + 255) / 256), (unsigned)n_pieces), block(256);
  hipStream_t st = (hipStream_t)stream;
  const double *tab = nullptr;
  if (pen && (rc = basis_table(ctx, s, pen->res, st, &tab))) return rc;
  const int shape = piece_grad_shape(ctx, s, n_pieces, batch, pen);
  if (shape == 2) {
    // fewest waves: two lanes per (trajectory, piece) AND the samples spread over the four waves of a workgroup
    const dim3 g4((unsigned)((2 * batch + 63) / 64), (unsigned)n_pieces);
    anet::launch_piece_grad(s, 2, g4, block, st, a, tab);
  } else if (shape == 1) {  // small batches: two lanes per (trajectory, piece)
    const dim3 g2((unsigned)((2 * batch + 255) / 256), (unsigned)n_pieces);
    anet::launch_piece_grad(s, 1, g2, block, st, a, tab);
  } else {  // 0: a lane per (trajectory, piece); 3: four lanes per pair and the matrix instructions -- 64 pairs per wave either way
    anet::launch_piece_grad(s, shape, grid, block, st, a, tab, ctx->cus);
  }
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}


int anet_minco_propagate_grad_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                                  const double *T, const double *coeffs, const double *gdC,
                                  const double *gdT, double *gradP, double *gradT, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!T || !coeffs || !gdC || !gdT || !gradT || (n_pieces > 1 && !gradP) || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_propagate_grad_dev: NULL pointer or ld < batch");
  anet::PropArgs a{T, coeffs, gdC, gdT, gradP, gradT, nullptr, nullptr, nullptr, 0.0, batch, ld, n_pieces, c};
  return do_propagate(ctx, s, a, (hipStream_t)stream);
}

int64_t anet_minco_cost_grad_workspace(int s, int n_pieces, int64_t ld) {
  return anet::cost_grad_ws(nullptr, s, n_pieces, ld).doubles;
}

int anet_minco_cost_grad_launches(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const anet_penalty *pen) {
  if (!ctx) return fail(nullptr, ANET_ERR_INVALID, "ctx is NULL");
  if (s < 2 || s > 4 || c < 1 || c > s || n_pieces < 1 || n_pieces > ANET_MAX_PIECES || batch < 0)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_cost_grad_launches: bad shape");
  return cost_grad_in_one_launch(ctx, s, c, n_pieces, batch, pen) ? 1 : 3;
}

int anet_minco_cost_grad_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                             const double *head, const double *tail, const double *wps,
                             const double *T, const double *hpolys, const anet_penalty *pen,
                             double *work, double *cost, double *gradP, double *gradT,
                             double *coeffs_out, void *stream) {
  return cost_grad_dev_impl(ctx, s, c, n_pieces, batch, ld, head, tail, wps, T, hpolys, pen, work, cost, gradP, gradT,
                            coeffs_out, stream, nullptr);
}

int anet_minco_cost_grad(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head,
                         const double *tail, const double *wps, const double *T, const double *hpolys,
                         const anet_penalty *pen, double *cost, double *gradP, double *gradT,
                         double *coeffs_out) {
  ANET_ON_DEVICE(ctx);
  int rc = check_solve_args(ctx, s, c, n_pieces, batch);
  if (rc) return rc;
  if ((rc = check_penalty(ctx, pen))) return rc;
  if (batch == 0) return ANET_OK;
  if (!head || !tail || !T || (n_pieces > 1 && (!wps || !gradP)) || !cost || !gradT)
    return fail(ctx, ANET_ERR_INVALID, "anet_minco_cost_grad: NULL pointer");
  const int N = n_pieces;
  const int64_t nco = (int64_t)N * 3 * 2 * s;
  const int64_t M = (pen && hpolys) ? pen->poly_rows : 0;
  const int64_t nhp = (int64_t)N * M * 4;
  Stager st(ctx, batch);
  double *d_head, *d_tail, *d_wps, *d_T, *d_hp = nullptr, *d_cost, *d_gP, *d_gT, *d_co, *d_work;
  rc = st.stage([&](Stager::Pass &p) {
    p.in(head, 3 * c, &d_head); p.in(tail, 3 * c, &d_tail); p.in(wps, (int64_t)(N - 1) * 3, &d_wps); p.in(T, N, &d_T);
    if (nhp) p.in(hpolys, nhp, &d_hp);
    p.rows(1, &d_cost); p.out((int64_t)(N - 1) * 3, &d_gP); p.out(N, &d_gT); p.out(nco, &d_co);
    p.doubles(anet_minco_cost_grad_workspace(s, N, st.ld), &d_work);
  });
  if (rc) return rc;
  rc = anet_minco_cost_grad_dev(ctx, s, c, N, batch, st.ld, d_head, d_tail, d_wps, d_T, d_hp, pen, d_work,
                                d_cost, d_gP, d_gT, d_co, ctx->stream);
  if (rc) return rc;
  ANET_HIP(ctx, hipMemcpyAsync(cost, d_cost, sizeof(double) * batch, hipMemcpyDeviceToHost, ctx->stream));
  if (N > 1 && (rc = st.download(d_gP, (int64_t)(N - 1) * 3, gradP))) return rc;
  if ((rc = st.download(d_gT, N, gradT))) return rc;
  if (coeffs_out && (rc = st.download(d_co, nco, coeffs_out))) return rc;
  ANET_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANET_OK;
}

}  // extern "C"
