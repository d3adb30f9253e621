// The QP: assembly, settings, the interior-point and ADMM solves, the time gradient and the VJP (include/allocnet_amd.h).
#include "api_internal.h"
#include "qp_assemble.h"
#include "qp_admm.h"
#include "qp_ipm.h"

extern "C" {

// ---- QP assembly entry points --------------------------------------------------------------------
int anet_qp_dims_of(int s, int n_pieces, int res, const int32_t *rows, anet_qp_dims *out) {
  if (!out || !rows || (s != 3 && s != 4) || n_pieces < 1 || res < 1) return ANET_ERR_INVALID;
  int64_t tot = 0;
  for (int i = 0; i < n_pieces; ++i) {
    if (rows[i] < 0) return ANET_ERR_INVALID;
    tot += rows[i];
  }
  out->n = (int64_t)3 * 2 * s * n_pieces;
  out->m_e = 3 * (6 + (int64_t)s * (n_pieces - 1));
  out->m_g = (int64_t)res * (tot + 12 * (int64_t)n_pieces);
  return ANET_OK;
}

int anet_qp_assemble_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M,
                         double max_vel, double max_acc, double m34, int float_time, int row_order,
                         const double *state, const double *T, const double *hpolys, const int32_t *rows,
                         double *Q, double *A, double *b, double *G, double *h, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (s != 3 && s != 4) return fail(ctx, ANET_ERR_INVALID, "anet_qp_assemble: order must be 3 (jerk) or 4 (snap), qp_solver.hpp:61-83");
  const int control_points = (row_order & ANET_QP_ROWS_CONTROL_POINTS) ? 1 : 0;
  row_order &= ~ANET_QP_ROWS_CONTROL_POINTS;
  if (n_pieces < 1 || batch < 0 || res < 1 || M < 0 || (row_order != 0 && row_order != 1))
    return fail(ctx, ANET_ERR_INVALID, "anet_qp_assemble: bad argument");
  if (control_points && res % (2 * s) != 0)
    return fail(ctx, ANET_ERR_INVALID, "anet_qp_assemble: control-point rows need res = k * 2 * order (k Bernstein segments per piece)");
  if (control_points && float_time)
    return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_qp_assemble: control-point rows are assembled in double only (no float_time)");
  if (batch == 0) return ANET_OK;
  if (!state || !T || !rows || (M > 0 && !hpolys) || !Q || !A || !b || !G || !h)
    return fail(ctx, ANET_ERR_INVALID, "anet_qp_assemble: NULL pointer");
  // one shape for the whole batch: read the first trajectory's row counts (device -> host, tiny)
  std::vector<int32_t> r0((size_t)n_pieces * batch);
  ANET_HIP(ctx, hipMemcpy(r0.data(), rows, sizeof(int32_t) * n_pieces * batch, hipMemcpyDeviceToHost));
  anet_qp_dims dm;
  if (anet_qp_dims_of(s, n_pieces, res, r0.data(), &dm)) return fail(ctx, ANET_ERR_INVALID, "anet_qp_assemble: bad row counts");
  for (int64_t bb = 0; bb < batch; ++bb) {
    int64_t tot = 0;
    for (int i = 0; i < n_pieces; ++i) {
      const int32_t v = r0[(size_t)bb * n_pieces + i];
      if (v < 0 || v > M) return fail(ctx, ANET_ERR_INVALID, "anet_qp_assemble: rows[b][i] must be in [0, M]");
      tot += v;
    }
    if ((int64_t)res * (tot + 12 * (int64_t)n_pieces) != dm.m_g)
      return fail(ctx, ANET_ERR_INVALID, "anet_qp_assemble: every trajectory of a batch needs the same total polytope row count");
  }
  anet::QpArgs a{state, T, hpolys, rows, Q, A, b, G, h, batch, dm.n, dm.m_e, dm.m_g, n_pieces, res, M,
                 float_time ? 1 : 0, row_order, max_vel, max_acc, m34, control_points};
  hipStream_t st = (hipStream_t)stream;
  const int64_t ne = dm.n * dm.n + dm.m_e * dm.n + dm.m_e, ng = dm.m_g * dm.n;
  const dim3 blk(256), g1((unsigned)((ne + 255) / 256), (unsigned)batch), g2((unsigned)((ng + 255) / 256), (unsigned)batch);
  if (s == 4) {
    if (float_time) { hipLaunchKernelGGL((anet::k_qp_eq_obj<4, float>), g1, blk, 0, st, a); if (ng) hipLaunchKernelGGL((anet::k_qp_ineq<4, float>), g2, blk, 0, st, a); }
    else { hipLaunchKernelGGL((anet::k_qp_eq_obj<4, double>), g1, blk, 0, st, a); if (ng) hipLaunchKernelGGL((anet::k_qp_ineq<4, double>), g2, blk, 0, st, a); }
  } else {
    if (float_time) { hipLaunchKernelGGL((anet::k_qp_eq_obj<3, float>), g1, blk, 0, st, a); if (ng) hipLaunchKernelGGL((anet::k_qp_ineq<3, float>), g2, blk, 0, st, a); }
    else { hipLaunchKernelGGL((anet::k_qp_eq_obj<3, double>), g1, blk, 0, st, a); if (ng) hipLaunchKernelGGL((anet::k_qp_ineq<3, double>), g2, blk, 0, st, a); }
  }
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_qp_assemble(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                     double max_acc, double m34, int float_time, int row_order, const double *state,
                     const double *T, const double *hpolys, const int32_t *rows, double *Q, double *A,
                     double *b, double *G, double *h) {
  ANET_ON_DEVICE(ctx);
  if ((s != 3 && s != 4) || n_pieces < 1 || batch < 0 || res < 1 || M < 0 || !rows)
    return fail(ctx, ANET_ERR_INVALID, "anet_qp_assemble: bad argument");
  if (batch == 0) return ANET_OK;
  anet_qp_dims dm;
  if (anet_qp_dims_of(s, n_pieces, res, rows, &dm)) return fail(ctx, ANET_ERR_INVALID, "anet_qp_assemble: bad row counts");
  const size_t n_state = 18 * (size_t)batch, n_T = (size_t)n_pieces * batch, n_hp = (size_t)batch * n_pieces * M * 4;
  const size_t nQ = (size_t)(dm.n * dm.n) * batch, nA = (size_t)(dm.m_e * dm.n) * batch, nb = (size_t)dm.m_e * batch;
  const size_t nG = (size_t)(dm.m_g * dm.n) * batch, nh = (size_t)dm.m_g * batch;
  double *d_state, *d_T, *d_hp, *d_Q, *d_A, *d_b, *d_G, *d_h;
  int32_t *d_rows;
  int rc = stage_scratch(ctx, [&](void *w) {
    anet::Cursor c(w);
    d_state = c.take<double>(n_state); d_T = c.take<double>(n_T); d_hp = c.take<double>(n_hp); d_rows = c.take<int32_t>(n_T);
    d_Q = c.take<double>(nQ); d_A = c.take<double>(nA); d_b = c.take<double>(nb); d_G = c.take<double>(nG); d_h = c.take<double>(nh);
    (void)c.spare(8);
    return c.bytes;
  });
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  ANET_HIP(ctx, hipMemcpyAsync(d_state, state, sizeof(double) * n_state, hipMemcpyHostToDevice, st));
  ANET_HIP(ctx, hipMemcpyAsync(d_T, T, sizeof(double) * n_T, hipMemcpyHostToDevice, st));
  if (n_hp) ANET_HIP(ctx, hipMemcpyAsync(d_hp, hpolys, sizeof(double) * n_hp, hipMemcpyHostToDevice, st));
  ANET_HIP(ctx, hipMemcpyAsync(d_rows, rows, sizeof(int32_t) * n_pieces * batch, hipMemcpyHostToDevice, st));
  ANET_HIP(ctx, hipStreamSynchronize(st));
  rc = anet_qp_assemble_dev(ctx, s, n_pieces, batch, res, M, max_vel, max_acc, m34, float_time, row_order, d_state,
                            d_T, d_hp, d_rows, d_Q, d_A, d_b, d_G, d_h, st);
  if (rc) return rc;
  if (Q) ANET_HIP(ctx, hipMemcpyAsync(Q, d_Q, sizeof(double) * nQ, hipMemcpyDeviceToHost, st));
  if (A) ANET_HIP(ctx, hipMemcpyAsync(A, d_A, sizeof(double) * nA, hipMemcpyDeviceToHost, st));
  if (b) ANET_HIP(ctx, hipMemcpyAsync(b, d_b, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
  if (G && nG) ANET_HIP(ctx, hipMemcpyAsync(G, d_G, sizeof(double) * nG, hipMemcpyDeviceToHost, st));
  if (h && nh) ANET_HIP(ctx, hipMemcpyAsync(h, d_h, sizeof(double) * nh, hipMemcpyDeviceToHost, st));
  ANET_HIP(ctx, hipStreamSynchronize(st));
  return ANET_OK;
}

// ---- QP solve entry points (interior point and ADMM) ------------------------------------------------
void anet_qp_default_settings(anet_qp_settings *s) {
  if (!s) return;
  s->rho = 0.1; s->sigma = 1e-6; s->alpha = 1.6; s->eps_abs = 1e-3; s->eps_rel = 1e-3;
  s->max_iter = 4000; s->check_termination = 25; s->adaptive_rho_interval = 100; s->scaled_termination = 0;
  s->method = ANET_QP_METHOD_INTERIOR_POINT;
}

int64_t anet_qp_solve_workspace(int s, int n_pieces, int64_t batch, int res, int M) {
  return anet::qp_solve_ws(nullptr, s, n_pieces, batch, res, M).doubles;
}

// Second part of a two-launch interior-point solve: what order its workgroups take the problems in.  Score of a parked problem,
// larger = expected to take longer (tools/qp_split_features.py: the parked scalars of 3 x 4096 problems against the steps they still
// needed).  The problems a batch waits for -- the infeasible ones, told at step 30..50, and the hard feasible ones -- stand out
// after four steps already: their PRIMAL residual is still above 2e-4 (1e-3..4e-2 against <= 5e-5 for the rest) and their steps
// are short; they go first, by residual.  Behind them the rest by the decades their complementarity stands above the tolerance
// (Spearman 0.75..0.94 with the steps left: an interior point gains a fixed number of digits per step at the end).  Problems
// decided in the first part score 0 and come last (their workgroups leave at once).
__global__ void k_qp_resume_score(const int *status, const double *cont, int64_t B, int ny, double tol, int *score) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int sc = 0;
  if (status[b] == 0) {
    const double *c = cont + b * (int64_t)(ny + anet::kIpmContScalars) + ny;
    const double pres = c[8], gap = c[10];
    double v = 200.0 + 100.0 * log10(fmax(gap / tol, 1.0));
    if (!(pres <= 2e-4)) v = 2000.0 + 100.0 * log10(fmax(pres / 2e-4, 1.0));
    if (!(v == v)) v = 4000.0;
    sc = (int)fmin(fmax(v, 1.0), 4000.0);
  }
  score[b] = sc;
}

// A caller's launch order is not checked (device memory): whatever it skips -- out-of-range or repeated entries -- must say so
__global__ void k_qp_mark_not_run(int64_t B, int *status, int *iters, double *obj) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  status[b] = ANET_QP_UNSOLVED;
  iters[b] = 0;
  obj[b] = __builtin_nan("");
}

// The LDS of one interior-point workgroup; the shape is the caller's to check
static size_t qp_ipm_lds(int s, int n_pieces, int res, int M) {
  return (s == 4) ? anet::qp_ipm_lds_bytes<4>(n_pieces, res, M) : anet::qp_ipm_lds_bytes<3>(n_pieces, res, M);
}

// Which form of the interior point a batch takes on this context's device (ANET_QP_IPM_FORM_*: the workgroups per CU the kernel's
// registers are bounded for, | THROUGHPUT, | TWO_LAUNCHES): the ONE statement of the selection -- qp_solve_dev_impl launches by
// it, anet_qp_ipm_launch_form reports it.  max_iter is the step limit of the solve (after its cap at 200).  Negative = error
// (bad shape, or a problem that does not fit the LDS); no error text is set here, the callers have their own.
static int qp_ipm_launch_form(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, bool has_launch_order,
                              int max_iter) {
  if (!ctx || (s != 3 && s != 4) || n_pieces < 1 || batch < 0 || res < 1 || M < 0) return ANET_ERR_INVALID;
  const size_t ldsb = qp_ipm_lds(s, n_pieces, res, M);
  if (ldsb > 160 * 1024) return ANET_ERR_UNSUPPORTED;
  if (batch == 0) return 0;
  const anet::Tuning &t = anet::tuning();
  // two workgroups per CU (registers bounded to 256) from this batch on, when two fit the LDS: more than two rounds of one
  // workgroup per CU (measured on 256 CUs): below that a batch lasts as long as its slowest problem and a problem alone on its
  // CU is faster (512 problems are a draw -- 2.86 / 1.88 / 2.95 ms against 2.64 / 1.63 / 3.42 ms for 8 snap / 5 jerk / 5 snap
  // pieces --, 768 problems gain 15-20 % from two per CU, 320 lose 15 %)
  const bool two_per_cu = batch >= t.ipm_two_per_cu_min_batch.at(ctx->cus) && 2 * ldsb <= 160 * 1024;
  // Shapes that put two workgroups on a CU visit the rows once more per step instead of carrying the next step's sums
  // through the updating pass (registers: qp_ipm.h FUSE); a lone problem, a small batch or a problem whose LDS fills the
  // CU takes the fused form.  (jerk: the unbounded instantiation needs <= 256 registers as it is -- two workgroups per CU
  // -- and the compiler schedules it for latency; bounded to 256 it is 18 % slower per problem at the same occupancy)
  if (!two_per_cu) return 1;  // (qp_ipm_fuse_unit.hip: the FUSE instantiations, scheduled for ILP)
  // ... and THREE for jerk problems whose LDS allows it, from a batch on that fills them several times over (registers bounded
  // to 168: 464 B of scratch).  Measured (round 5, same box, 5 jerk pieces): 4096 problems 3.96-4.00 -> 3.77-3.85 ms; 3000:
  // 3.02-3.07 -> 3.21-3.25; 2048: 2.09-2.12 -> 2.42-2.43 (1024: 1.60 -> 1.91 in round 4) -- selected by batch like every other
  // shape here (ANET_IPM_THREE_PER_CU_MIN_BATCH overrides; 0 disables)
  const int64_t ipm_three_per_cu_min_batch = t.ipm_three_per_cu_min_batch.at(ctx->cus);
  const bool three_per_cu = s == 3 && ipm_three_per_cu_min_batch > 0 && batch >= ipm_three_per_cu_min_batch && 3 * ldsb <= 160 * 1024;
  // the shape of large batches: four row passes, registers bounded for 2 (snap) or 3 per CU (jerk: 1 where three do not apply)
  int form = ANET_QP_IPM_FORM_THROUGHPUT | (s == 4 ? 2 : three_per_cu ? 3 : 1);
  // Large batches in TWO launches (qp_ipm.h, IpmArgs::it_stop): the first takes every problem through the same number of Newton
  // steps -- no tail: all workgroups are equally long --, the second resumes the unfinished ones longest-expected first.  A batch
  // of 4096 in one launch ends 27 % above its balanced figure because its 30..50-step problems start whenever their turn comes.
  // (from 576 problems on 256 CUs: 520..560 problems lose 7-10 %, 600..1280 gain 10-19 %)
  if (t.ipm_split_steps > 0 && batch >= t.ipm_split_min_batch.at(ctx->cus) && !has_launch_order && max_iter > t.ipm_split_steps)
    form |= ANET_QP_IPM_FORM_TWO_LAUNCHES;
  return form;
}

// the step limit of an interior-point solve with these settings
static int qp_ipm_max_iter(const anet_qp_settings &st) { return st.max_iter < 200 ? st.max_iter : 200; }

int anet_qp_ipm_launch_form(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, int with_launch_order) {
  if (!ctx) return fail(nullptr, ANET_ERR_INVALID, "ctx is NULL");
  anet_qp_settings st_;
  anet_qp_default_settings(&st_);
  const int form = qp_ipm_launch_form(ctx, s, n_pieces, batch, res, M, with_launch_order != 0, qp_ipm_max_iter(st_));
  if (form == ANET_ERR_UNSUPPORTED)
    return fail(ctx, form, "anet_qp_ipm_launch_form: problem too large for the 160 KB LDS (interior-point method)");
  if (form < 0) return fail(ctx, form, "anet_qp_ipm_launch_form: bad shape");
  return form;
}

static int qp_solve_dev_impl(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                             double max_acc, double m34, const double *state, const double *T,
                             const double *hpolys, const anet_qp_settings *settings, double *work, double *coeffs,
                             double *obj, int32_t *status, int32_t *iters, double *residuals, double *grad_T,
                             void *stream, const double *grad_z = nullptr, double *vjp_T = nullptr,
                             const int32_t *launch_order = nullptr) {
  ANET_ON_DEVICE(ctx);
  if (s != 3 && s != 4) return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve: order must be 3 (jerk) or 4 (snap)");
  if (n_pieces < 1 || batch < 0 || res < 1 || M < 0) return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve: bad argument");
  if (batch == 0) return ANET_OK;
  if (!state || !T || (M > 0 && !hpolys) || !work || !coeffs || !obj || !status || !iters)
    return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve: NULL pointer");
  anet_qp_settings st_;
  anet_qp_default_settings(&st_);
  if (settings) st_ = *settings;
  if (!(st_.rho > 0) || !(st_.sigma > 0) || !(st_.alpha > 0 && st_.alpha < 2) || st_.max_iter < 1 ||
      st_.check_termination < 1 || st_.eps_abs < 0 || st_.eps_rel < 0 || st_.adaptive_rho_interval < 0)
    return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve: bad settings");
  // the row form rides on the method word (ANET_QP_ROWS_CONTROL_POINTS); every other unknown bit or value is refused
  const int control_points = (st_.method & ANET_QP_ROWS_CONTROL_POINTS) ? 1 : 0;
  st_.method &= ~ANET_QP_ROWS_CONTROL_POINTS;
  if (st_.method != ANET_QP_METHOD_ADMM && st_.method != ANET_QP_METHOD_INTERIOR_POINT)
    return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve: unknown method");
  if (control_points) {
    if (res % (2 * s) != 0)
      return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve: control-point rows need res = k * 2 * order (k Bernstein segments per piece)");
    if (st_.method != ANET_QP_METHOD_INTERIOR_POINT)
      return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_qp_solve: control-point rows need the interior-point method");
  }
  const anet::QpSolveWs W = anet::qp_solve_ws(work, s, n_pieces, batch, res, M);
  if (st_.method == ANET_QP_METHOD_INTERIOR_POINT) {
    const size_t ldsb = qp_ipm_lds(s, n_pieces, res, M);
    if (ldsb > 160 * 1024)
      return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_qp_solve: problem too large for the 160 KB LDS (interior-point method)");
    double tol = st_.eps_rel < st_.eps_abs ? st_.eps_rel : st_.eps_abs;
    if (!(tol > 0.0) || tol > 1e-6) tol = 1e-6;   // Newton's method: the last digits cost one or two steps
    if (tol < 1e-10) tol = 1e-10;                 // (below that the slacks of the touched rows underflow the factorisation)
    // the backward pass differentiates the central path at the barrier parameter the solve stopped at: its error is
    // of that order, so it asks for three more digits (one or two Newton steps)
    const double tol_plain = tol;
    if (grad_z && tol > 1e-9) tol = 1e-9;
    anet::IpmArgs ia{state, T, hpolys, W.ipm().z, W.ipm().y, coeffs, obj, status, iters,
                     residuals ? residuals : W.ipm().residuals, grad_T, grad_z, vjp_T, batch, n_pieces, res, M, max_vel,
                     max_acc, m34, tol, qp_ipm_max_iter(st_), tol_plain > tol ? tol_plain : 0.0, 0.1 * tol, 0, launch_order, 0, 0, nullptr, nullptr};
    const anet::Tuning &t = anet::tuning();
    ia.twist_min_pieces = t.ipm_twist_min_pieces;
    hipStream_t sti = (hipStream_t)stream;
    if (launch_order) {
      hipLaunchKernelGGL(k_qp_mark_not_run, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, sti, batch, status, iters, obj);
      ANET_HIP(ctx, hipGetLastError());
    }
    {  // the tables of (order, res, m34, row form): built once, on the stream that first needs them
      const double *tab = nullptr;
      for (auto &tb : ctx->ipm_tabs)
        if (tb.s == s && tb.res == res && tb.m34 == m34 && tb.control_points == control_points) {
          if (tb.built_on != sti) ANET_HIP(ctx, hipStreamWaitEvent(sti, tb.ready, 0));
          tab = tb.d;
        }
      if (!tab) {
        // (never freed before anet_destroy -- a launch on another stream may still read one: a caller that sweeps m34 or res over
        //  hundreds of values is told so instead of growing the context without bound)
        if (ctx->ipm_tabs.size() >= kMaxTablesPerContext)
          return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_qp_solve: more than 256 distinct (order, res, m34, row form) on one context");
        anet_ctx::IpmTable tb{s, res, m34, nullptr, sti, nullptr, control_points};
        const size_t need = (size_t)2 * (2 * s) * (2 * s) + (size_t)res * anet::ipm_ht_stride(2 * s);
        int rc_t = new_table(ctx, sizeof(double) * need, &tb.d, &tb.ready);
        if (rc_t) return rc_t;
        hipError_t e1 = hipMemsetAsync(tb.d, 0, sizeof(double) * need, sti);
        if (e1 == hipSuccess) {
          if (s == 4) hipLaunchKernelGGL(anet::k_qp_ipm_tables<4>, dim3(1), dim3(256), 0, sti, tb.d, res, m34, control_points);
          else hipLaunchKernelGGL(anet::k_qp_ipm_tables<3>, dim3(1), dim3(256), 0, sti, tb.d, res, m34, control_points);
          e1 = hipGetLastError();
        }
        if (e1 == hipSuccess) e1 = hipEventRecord(tb.ready, sti);
        if (e1 != hipSuccess) {  // nothing half-built stays behind
          drop_table(tb.d, tb.ready);
          return hip_fail(ctx, e1, "k_qp_ipm_tables");
        }
        ctx->ipm_tabs.push_back(tb);
        tab = tb.d;
      }
      ia.tab = tab;
    }
#ifdef ANET_IPM_PROF
    static long long *d_iprof = nullptr;
    if (!d_iprof) ANET_HIP(ctx, hipMalloc((void **)&d_iprof, 16 * sizeof(long long)));
    ANET_HIP(ctx, hipMemsetAsync(d_iprof, 0, 16 * sizeof(long long), sti));
    ia.prof = d_iprof;
    struct ProfDump {
      anet_ctx *c; long long *d; hipStream_t st;
      ~ProfDump() {
        long long h[16];
        if (hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return;
        fprintf(stderr, "ipm_prof cycles (problem 0): setup %lld | passA %lld resid %lld assemble %lld rhs %lld factor %lld solve1 %lld passB %lld passC %lld rhs2 %lld solve2 %lld passD %lld passE %lld | before the loop (tables, first iterate) %lld\n",
                h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11], h[12], h[13]);
      }
    } prof_dump{ctx, d_iprof, sti};
#endif
    const int form = qp_ipm_launch_form(ctx, s, n_pieces, batch, res, M, launch_order != nullptr, ia.max_iter);
    if (form < 0) return fail(ctx, form, "anet_qp_solve: no interior-point form for this shape");
    auto launch_ipm = [&](auto kern) -> int {
      ANET_HIP(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb));
      hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(256), ldsb, sti, ia);
      return ANET_OK;
    };
    auto launch_throughput = [&]() -> int {
      if (s == 4) return launch_ipm(anet::k_qp_ipm<4, 2, false>);
      return (form & ANET_QP_IPM_FORM_PER_CU_MASK) == 3 ? launch_ipm(anet::k_qp_ipm<3, 3, false>) : launch_ipm(anet::k_qp_ipm<3, 1, false>);
    };
    int rc_l;
    if (form & ANET_QP_IPM_FORM_TWO_LAUNCHES) {
      const int ny = 3 * s * (n_pieces + 1);
      const anet::ResumeTail &rt = W.tail;
      ia.cont = rt.cont;
      ia.it_stop = t.ipm_split_steps;
      rc_l = launch_throughput();
      if (rc_l != ANET_OK) return rc_l;
      rc_l = resume_parked(
          ctx, batch, rt, sti,
          [&](int32_t *score) {
            hipLaunchKernelGGL(k_qp_resume_score, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, sti, status, rt.cont, batch, ny,
                               tol, score);
          },
          [&](const int32_t *order) {
            ia.it_stop = 0;
            ia.resume = 1;
            ia.order = order;
            return launch_throughput();
          });
      if (rc_l != ANET_OK) return rc_l;
      ANET_HIP(ctx, hipGetLastError());
      return ANET_OK;
    }
    if (!(form & ANET_QP_IPM_FORM_THROUGHPUT)) {
      ANET_HIP(ctx, (hipError_t)anet::launch_qp_ipm_fuse(s, batch, ldsb, sti, ia));
      rc_l = ANET_OK;
    } else rc_l = launch_throughput();
    if (rc_l != ANET_OK) return rc_l;
    ANET_HIP(ctx, hipGetLastError());
    return ANET_OK;
  }
  if (grad_z) return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_qp_solve_vjp: the backward pass needs the interior-point method");
  size_t lds = (s == 4) ? anet::qp_admm_lds_bytes<4>(n_pieces, res, M, true) : anet::qp_admm_lds_bytes<3>(n_pieces, res, M, true);
  int zy_in_lds = 1;
  if (lds > 160 * 1024) {
    zy_in_lds = 0;
    lds = (s == 4) ? anet::qp_admm_lds_bytes<4>(n_pieces, res, M, false) : anet::qp_admm_lds_bytes<3>(n_pieces, res, M, false);
  }
  if (lds > 160 * 1024)
    return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_qp_solve: the block factor of this many pieces does not fit the 160 KB LDS");
  int adapt = st_.adaptive_rho_interval;
  if (adapt > 0) adapt = (adapt + st_.check_termination - 1) / st_.check_termination * st_.check_termination;
  anet::AdmmArgs a{state, T, hpolys, W.admm().z, W.admm().y, coeffs, obj, status, iters,
                   residuals ? residuals : W.admm().residuals, batch, n_pieces, res, M, max_vel, max_acc, m34,
                   anet::AdmmParams{st_.rho, st_.sigma, st_.alpha, st_.eps_abs, st_.eps_rel, st_.max_iter,
                                    st_.check_termination, adapt, st_.scaled_termination ? 1 : 0},
                   zy_in_lds, grad_T};
  hipStream_t st = (hipStream_t)stream;
  if (s == 4) {
    ANET_HIP(ctx, hipFuncSetAttribute((const void *)anet::k_qp_admm<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((anet::k_qp_admm<4>), dim3((unsigned)batch), dim3(256), lds, st, a);
  } else {
    ANET_HIP(ctx, hipFuncSetAttribute((const void *)anet::k_qp_admm<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((anet::k_qp_admm<3>), dim3((unsigned)batch), dim3(256), lds, st, a);
  }
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_qp_solve_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                      double max_acc, double m34, const double *state, const double *T,
                      const double *hpolys, const anet_qp_settings *settings, double *work, double *coeffs,
                      double *obj, int32_t *status, int32_t *iters, double *residuals, void *stream) {
  return qp_solve_dev_impl(ctx, s, n_pieces, batch, res, M, max_vel, max_acc, m34, state, T, hpolys, settings, work,
                           coeffs, obj, status, iters, residuals, nullptr, stream);
}

int anet_qp_solve_ordered_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                              double max_acc, double m34, const double *state, const double *T, const double *hpolys,
                              const anet_qp_settings *settings, const int32_t *launch_order, double *work, double *coeffs,
                              double *obj, int32_t *status, int32_t *iters, double *residuals, void *stream) {
  return qp_solve_dev_impl(ctx, s, n_pieces, batch, res, M, max_vel, max_acc, m34, state, T, hpolys, settings, work,
                           coeffs, obj, status, iters, residuals, nullptr, stream, nullptr, nullptr, launch_order);
}

int anet_qp_solve_time_grad_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                                double max_acc, double m34, const double *state, const double *T,
                                const double *hpolys, const anet_qp_settings *settings, double *work,
                                double *coeffs, double *obj, int32_t *status, int32_t *iters, double *residuals,
                                double *grad_T, void *stream) {
  if (ctx && batch > 0 && !grad_T) return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve_time_grad: grad_T is NULL");
  return qp_solve_dev_impl(ctx, s, n_pieces, batch, res, M, max_vel, max_acc, m34, state, T, hpolys, settings, work,
                           coeffs, obj, status, iters, residuals, grad_T, stream);
}

int anet_qp_solve_vjp_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                          double max_acc, double m34, const double *state, const double *T, const double *hpolys,
                          const anet_qp_settings *settings, const double *grad_z, double *work, double *coeffs,
                          double *obj, int32_t *status, int32_t *iters, double *residuals, double *grad_T,
                          void *stream) {
  if (ctx && batch > 0 && (!grad_z || !grad_T)) return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve_vjp: grad_z / grad_T is NULL");
  return qp_solve_dev_impl(ctx, s, n_pieces, batch, res, M, max_vel, max_acc, m34, state, T, hpolys, settings, work,
                           coeffs, obj, status, iters, residuals, nullptr, stream, grad_z, grad_T);
}

static int qp_solve_host_impl(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                              double max_acc, double m34, const double *state, const double *T,
                              const double *hpolys, const anet_qp_settings *settings, double *coeffs, double *obj,
                              int32_t *status, int32_t *iters, double *residuals, double *grad_T,
                              const double *grad_z = nullptr) {
  ANET_ON_DEVICE(ctx);
  if ((s != 3 && s != 4) || n_pieces < 1 || batch < 0 || res < 1 || M < 0)
    return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve: bad argument");
  if (batch == 0) return ANET_OK;
  if (!state || !T || (M > 0 && !hpolys) || !coeffs) return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve: NULL pointer");
  const size_t n = (size_t)3 * 2 * s * n_pieces;
  const size_t n_state = 18 * (size_t)batch, n_T = (size_t)n_pieces * batch, n_hp = (size_t)batch * n_pieces * M * 4;
  const int64_t n_work = anet_qp_solve_workspace(s, n_pieces, batch, res, M);
  double *d_state, *d_T, *d_hp, *d_work, *d_co, *d_obj, *d_res, *d_gT, *d_gz;
  int32_t *d_status, *d_iters;
  int rc = stage_scratch(ctx, [&](void *w) {
    anet::Cursor c(w);
    d_state = c.take<double>(n_state); d_T = c.take<double>(n_T); d_hp = c.take<double>(n_hp); d_work = c.take<double>(n_work);
    d_co = c.take<double>(n * batch); d_obj = c.take<double>(batch); d_res = c.take<double>(2 * batch);
    d_status = c.take<int32_t>(batch); d_iters = c.take<int32_t>(batch);
    d_gT = c.take<double>(n_T); d_gz = c.take<double>(n * batch); (void)c.spare(8);
    return c.bytes;
  });
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  ANET_HIP(ctx, hipMemcpyAsync(d_state, state, sizeof(double) * n_state, hipMemcpyHostToDevice, st));
  ANET_HIP(ctx, hipMemcpyAsync(d_T, T, sizeof(double) * n_T, hipMemcpyHostToDevice, st));
  if (n_hp) ANET_HIP(ctx, hipMemcpyAsync(d_hp, hpolys, sizeof(double) * n_hp, hipMemcpyHostToDevice, st));
  if (grad_z) ANET_HIP(ctx, hipMemcpyAsync(d_gz, grad_z, sizeof(double) * n * batch, hipMemcpyHostToDevice, st));
  rc = qp_solve_dev_impl(ctx, s, n_pieces, batch, res, M, max_vel, max_acc, m34, d_state, d_T, d_hp, settings, d_work,
                         d_co, d_obj, d_status, d_iters, d_res, (grad_T && !grad_z) ? d_gT : nullptr, st,
                         grad_z ? d_gz : nullptr, grad_z ? d_gT : nullptr);
  if (rc) return rc;
  if (grad_T) ANET_HIP(ctx, hipMemcpyAsync(grad_T, d_gT, sizeof(double) * n_T, hipMemcpyDeviceToHost, st));
  ANET_HIP(ctx, hipMemcpyAsync(coeffs, d_co, sizeof(double) * n * batch, hipMemcpyDeviceToHost, st));
  if (obj) ANET_HIP(ctx, hipMemcpyAsync(obj, d_obj, sizeof(double) * batch, hipMemcpyDeviceToHost, st));
  if (status) ANET_HIP(ctx, hipMemcpyAsync(status, d_status, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
  if (iters) ANET_HIP(ctx, hipMemcpyAsync(iters, d_iters, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
  if (residuals) ANET_HIP(ctx, hipMemcpyAsync(residuals, d_res, sizeof(double) * 2 * batch, hipMemcpyDeviceToHost, st));
  ANET_HIP(ctx, hipStreamSynchronize(st));
  return ANET_OK;
}

int anet_qp_solve(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                  double max_acc, double m34, const double *state, const double *T, const double *hpolys,
                  const anet_qp_settings *settings, double *coeffs, double *obj, int32_t *status,
                  int32_t *iters, double *residuals) {
  return qp_solve_host_impl(ctx, s, n_pieces, batch, res, M, max_vel, max_acc, m34, state, T, hpolys, settings, coeffs,
                            obj, status, iters, residuals, nullptr);
}

int anet_qp_solve_time_grad(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                            double max_acc, double m34, const double *state, const double *T,
                            const double *hpolys, const anet_qp_settings *settings, double *coeffs, double *obj,
                            int32_t *status, int32_t *iters, double *residuals, double *grad_T) {
  if (ctx && batch > 0 && !grad_T) return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve_time_grad: grad_T is NULL");
  return qp_solve_host_impl(ctx, s, n_pieces, batch, res, M, max_vel, max_acc, m34, state, T, hpolys, settings, coeffs,
                            obj, status, iters, residuals, grad_T);
}

int anet_qp_solve_vjp(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                      double max_acc, double m34, const double *state, const double *T, const double *hpolys,
                      const anet_qp_settings *settings, const double *grad_z, double *coeffs, double *obj,
                      int32_t *status, int32_t *iters, double *residuals, double *grad_T) {
  if (ctx && batch > 0 && (!grad_z || !grad_T)) return fail(ctx, ANET_ERR_INVALID, "anet_qp_solve_vjp: grad_z / grad_T is NULL");
  return qp_solve_host_impl(ctx, s, n_pieces, batch, res, M, max_vel, max_acc, m34, state, T, hpolys, settings, coeffs,
                            obj, status, iters, residuals, grad_T, grad_z);
}

}  // extern "C"
