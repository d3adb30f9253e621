// The shape of every device workspace of the library, each written ONCE: a function runs a bump cursor over the regions in order
// and returns typed pointers plus the total.  The anet_*_workspace() functions call it on a null base (measure only), the
// *_dev_impls on the buffer.  The host entry points shape their buffers with the same cursor: the trajectory-major ones that
// transpose state theirs in staging.h's terms (Stager::stage), the contiguous ones in api_internal.h's stage_scratch.  Host C++17 only, no HIP include, no device code: tests/cpp/test_workspace_layout.cpp carves every layout in
// host memory under a sanitizer.  DESIGN.md section 8i.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "workspace_constants.h"

namespace anet {

// take<T>(count) hands out the next region, rounded up to whole doubles, so no region starts inside a double.  The sizes the
// anet_*_workspace() functions have always returned count int32 rows packed, two per double, plus a few doubles on top;
// spare(n) is that addend as a region of its own: n doubles less what the roundings since the last spare() took of them.
struct Cursor {
  char *base;  // 8-byte aligned, or nullptr: measure only (every pointer handed out is nullptr)
  int64_t bytes = 0, padded = 0;
  explicit Cursor(void *b) : base((char *)b) {}
  template <class T>
  T *take(int64_t count) {
    T *p = base ? (T *)(base + bytes) : nullptr;
    const int64_t raw = (int64_t)sizeof(T) * count, whole = (raw + 7) / 8 * 8;
    bytes += whole;
    padded += whole - raw;
    return p;
  }
  double *spare(int64_t n) {
    n -= (padded + 7) / 8;
    padded = 0;
    return take<double>(n > 0 ? n : 0);
  }
  int64_t doubles() const { return bytes / 8; }
};

// ---- device workspaces (what the anet_*_workspace() functions size) ---------------------------------------------------------
// The batched L-BFGS state of n variables, history m, npf past costs, row stride ld: x g xp gp d | lm_s lm_y | lm_ys lm_alpha |
// pf | the DS_* rows | feval | the IS_* rows (int32)
struct LbfgsLayout {
  int n, m, npf;
  int64_t ld;
  double *x, *g, *xp, *gp, *d, *lm_s, *lm_y, *lm_ys, *lm_alpha, *pf, *ds, *feval;
  int *is;
  int64_t doubles;
};
inline LbfgsLayout lbfgs_layout(Cursor &c, int n, int m, int npf, int64_t ld) {
  LbfgsLayout L{};
  const int64_t at = c.doubles(), v = (int64_t)n * ld;
  L.n = n; L.m = m; L.npf = npf; L.ld = ld;
  L.x = c.take<double>(v); L.g = c.take<double>(v); L.xp = c.take<double>(v); L.gp = c.take<double>(v); L.d = c.take<double>(v);
  L.lm_s = c.take<double>(m * v); L.lm_y = c.take<double>(m * v);
  L.lm_ys = c.take<double>(m * ld); L.lm_alpha = c.take<double>(m * ld); L.pf = c.take<double>(npf * ld);
  L.ds = c.take<double>(DS_COUNT_ * ld); L.feval = c.take<double>(ld); L.is = c.take<int>(IS_COUNT_ * ld);
  L.doubles = c.doubles() - at;
  return L;
}
inline LbfgsLayout lbfgs_layout(double *w, int n, int m, int npf, int64_t ld) { Cursor c(w); return lbfgs_layout(c, n, m, npf, ld); }

// The tail of the workspace of a solve that can run in two launches (the one-launch L-BFGS, the interior-point QP): the parked
// state of every problem (`per` doubles each), its score and the order of the second launch (int32 rows of ld), the bins of the
// counting sort, and two doubles of spare.  cont == nullptr: the workspace has no tail.
struct ResumeTail { double *cont; int32_t *score, *order, *bins; double *spare; };
inline ResumeTail resume_tail(Cursor &c, int64_t per, int64_t ld) {
  ResumeTail t{};
  t.cont = c.take<double>(per * ld); t.score = c.take<int32_t>(ld); t.order = c.take<int32_t>(ld);
  t.bins = c.take<int32_t>(kOrderBuckets); t.spare = c.spare(2);
  return t;
}

// cost + gradient in three launches: coefficients | dJ/dc | dJ/dT | penalty per piece | energy
struct CostGradWs { double *co, *gdC, *gdT, *pc, *en; int64_t doubles; };
inline CostGradWs cost_grad_ws(Cursor &c, int s, int N, int64_t ld) {
  CostGradWs L{};
  const int64_t at = c.doubles(), nco = (int64_t)N * 3 * 2 * s;
  L.co = c.take<double>(nco * ld); L.gdC = c.take<double>(nco * ld); L.gdT = c.take<double>(N * ld);
  L.pc = c.take<double>(N * ld); L.en = c.take<double>(ld);
  L.doubles = c.doubles() - at;
  return L;
}
inline CostGradWs cost_grad_ws(double *w, int s, int N, int64_t ld) { Cursor c(w); return cost_grad_ws(c, s, N, ld); }

// The MINCO L-BFGS: optimiser state | cost + gradient | gradP rows | gradT rows | (with_tail) the two-launch tail.  The state
// region is sized for all 3(N-1) + N variables and carved for the n_run of this run (waypoints only, durations only), so
// everything behind it -- the tail above all -- lies where anet_lbfgs_minco_workspace() counted it, whatever opt_flags says.
struct LbfgsMincoWs { LbfgsLayout opt; CostGradWs cg; double *gP, *gT; ResumeTail tail; int64_t doubles; };
inline LbfgsMincoWs lbfgs_minco_ws(double *w, int s, int N, int64_t ld, int m, int npf, int n_run, bool with_tail) {
  Cursor c(w);
  LbfgsMincoWs L{};
  L.opt = lbfgs_layout(c.take<double>(lbfgs_layout(nullptr, 3 * (N - 1) + N, m, npf, ld).doubles), n_run, m, npf, ld);
  L.cg = cost_grad_ws(c, s, N, ld);
  L.gP = c.take<double>((int64_t)3 * (N - 1) * ld); L.gT = c.take<double>((int64_t)N * ld);
  if (with_tail) L.tail = resume_tail(c, kPersistContDoubles, ld);
  L.doubles = c.doubles();
  return L;
}

// a parked interior-point problem (qp_ipm.h IpmArgs::cont): the iterate's ny = 3 s (N + 1) doubles, then its scalars
inline int64_t qp_cont_doubles(int s, int N) { return (int64_t)3 * s * (N + 1) + kIpmContScalars; }
// The QP solve: the rows' slacks and multipliers (the front) | residuals | the two-launch tail of the interior point | six
// doubles of spare.  ADMM addresses the front by all m rows; the interior point by the mi inequality rows only, and keeps its
// residuals (when the caller passes none) behind those, inside the front.
struct QpSolveWs {
  struct View { double *z, *y, *residuals; };
  int64_t m, mi, batch;
  double *front, *residuals;
  ResumeTail tail;
  double *spare;
  int64_t doubles;
  View admm() const { return {front, front + m * batch, residuals}; }
  View ipm() const { return {front, front + mi * batch, front + 2 * mi * batch}; }
};
inline QpSolveWs qp_solve_ws(double *w, int s, int N, int64_t batch, int res, int M) {
  Cursor c(w);
  QpSolveWs L{};
  L.mi = (int64_t)N * res * (M + 12); L.m = 3 * (6 + (int64_t)s * (N - 1)) + L.mi; L.batch = batch;
  L.front = c.take<double>(2 * L.m * batch); L.residuals = c.take<double>(2 * batch);
  L.tail = resume_tail(c, qp_cont_doubles(s, N), batch); L.spare = c.spare(6);
  L.doubles = c.doubles();
  return L;
}

// FIRI: ellipsoid state | forward points | MVIE rows (batch-minor, stride ld) | the MVIE L-BFGS | per-point flags, MVIE verdicts,
// the zero point counts of a call without points (int32) | sixteen doubles of spare
constexpr int kFiriLbfgsVars = 9, kFiriLbfgsMem = 18, kFiriLbfgsPast = 3;  // firi.hpp:212-217
struct FiriWs { double *ell, *fpc, *A; LbfgsLayout opt; int32_t *flag, *mok, *np0; double *spare; int64_t doubles; };
inline FiriWs firi_ws(double *w, int64_t batch, int64_t ld, int Np, int H) {
  Cursor c(w);
  FiriWs L{};
  L.ell = c.take<double>(batch * kFiriEll); L.fpc = c.take<double>(batch * Np * 4); L.A = c.take<double>((int64_t)3 * H * ld);
  L.opt = lbfgs_layout(c, kFiriLbfgsVars, kFiriLbfgsMem, kFiriLbfgsPast, ld);
  L.flag = c.take<int32_t>(batch * Np); L.mok = c.take<int32_t>(batch); L.np0 = c.take<int32_t>(batch); L.spare = c.spare(16);
  L.doubles = c.doubles();
  return L;
}

// The corridor-constrained MINCO L-BFGS (sfc_param_kernels.h): optimiser state of (N-1) K + N variables, carved for the n_run of
// this run | cost + gradient | waypoint rows P(xi) | dJ/dP rows | dJ/dT rows | the three norm rows per waypoint
struct SfcWs { LbfgsLayout opt; CostGradWs cg; double *wps, *gP, *gT, *norm; int64_t doubles; };
inline SfcWs sfc_ws(double *w, int s, int N, int K, int64_t ld, int m, int npf, int n_run) {
  Cursor c(w);
  SfcWs L{};
  L.opt = lbfgs_layout(c.take<double>(lbfgs_layout(nullptr, (N - 1) * K + N, m, npf, ld).doubles), n_run, m, npf, ld);
  L.cg = cost_grad_ws(c, s, N, ld);
  L.wps = c.take<double>((int64_t)3 * (N - 1) * ld); L.gP = c.take<double>((int64_t)3 * (N - 1) * ld);
  L.gT = c.take<double>((int64_t)N * ld); L.norm = c.take<double>((int64_t)3 * (N - 1) * ld);
  L.doubles = c.doubles();
  return L;
}
// Overlap enumeration of a corridor: the (N-1) B stacked pairs of 2 M rows | their vertices, K each | count | status (int32)
struct SfcOverlapWs { double *stacked, *verts; int32_t *count, *status; int64_t doubles; };
inline SfcOverlapWs sfc_overlap_ws(double *w, int N, int64_t B, int M, int K) {
  Cursor c(w);
  SfcOverlapWs L{};
  const int64_t P = (int64_t)(N - 1) * B;
  L.stacked = c.take<double>(P * 2 * M * 4); L.verts = c.take<double>(P * K * 3);
  L.count = c.take<int32_t>(P); L.status = c.take<int32_t>(P);
  L.doubles = c.doubles();
  return L;
}
// backward_p: the L-BFGS state of the (N-1) ld problems of K variables (mem_size 8, past 3)
constexpr int kSfcTinyMem = 8, kSfcTinyPast = 3;
inline LbfgsLayout sfc_backward_p_ws(double *w, int N, int K, int64_t ld) {
  return lbfgs_layout(w, K, kSfcTinyMem, kSfcTinyPast, (int64_t)(N - 1) * ld);
}

// The shortest route through a corridor (sfc_path_kernels.h): optimiser state of (N-1) K variables | the three norm rows per
// waypoint that k_sfc_forward_p writes beside the returned waypoints
struct SfcPathWs { LbfgsLayout opt; double *norm; int64_t doubles; };
inline SfcPathWs sfc_path_ws(double *w, int N, int K, int64_t ld, int m, int npf) {
  Cursor c(w);
  SfcPathWs L{};
  L.opt = lbfgs_layout(c, (N - 1) * K, m, npf, ld);
  L.norm = c.take<double>((int64_t)3 * (N - 1) * ld);
  L.doubles = c.doubles();
  return L;
}

// status | iterations | evaluations of an L-BFGS run (k_lbfgs_results), int32 rows of ld
struct LbfgsResultRows { int32_t *status, *iters, *evals; int64_t doubles; };
inline LbfgsResultRows lbfgs_result_rows(Cursor &c, int64_t ld) {
  const int64_t at = c.doubles();
  LbfgsResultRows R{c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), 0};
  R.doubles = c.doubles() - at;
  return R;
}
inline LbfgsResultRows lbfgs_result_rows(double *w, int64_t ld) { Cursor c(w); return lbfgs_result_rows(c, ld); }

// Connected components of a byte grid of n voxels (frontier_kernels.h), labelling and statistics on one buffer: the rank of every
// root at its own index | the root count of every block of kCompScanBlock voxels, scanned in place | the round of the last merge
struct VoxCompWs { int32_t *rank, *blocks, *changed; int64_t n_blocks, bytes; };
inline VoxCompWs voxel_components_ws(void *w, int64_t n) {
  Cursor c(w);
  VoxCompWs L{};
  L.n_blocks = (n + kCompScanBlock - 1) / kCompScanBlock;
  L.rank = c.take<int32_t>(n);
  L.blocks = c.take<int32_t>(L.n_blocks);
  L.changed = c.take<int32_t>(2);
  L.bytes = c.bytes;
  return L;
}

// View gain (frontier_kernels.h): one slot of mark bytes per view of a chunk, each the largest sub-box a view can have -- at most
// 2 reach + 1 cells per axis, cut to the map -- rounded up to whole kViewSlotAlign bytes; all zero between calls
struct ViewGainWs { uint8_t *marks; int64_t slot, bytes; };
inline ViewGainWs view_gain_ws(void *w, const int32_t size[3], int64_t reach, int64_t n_views) {
  Cursor c(w);
  ViewGainWs L{};
  int64_t cells = 1;
  for (int a = 0; a < 3; ++a) cells *= (2 * reach + 1 < size[a]) ? 2 * reach + 1 : size[a];
  L.slot = (cells + kViewSlotAlign - 1) / kViewSlotAlign * kViewSlotAlign;
  L.marks = c.take<uint8_t>(L.slot * n_views);
  L.bytes = c.bytes;
  return L;
}

}  // namespace anet
