// Host plumbing shared by the translation units of the C ABI (include/allocnet_amd.h).  Built by allocnet_amd/build.py:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC
// No torch, no Eigen.  There is no CPU fallback in this library: without a device every entry point fails with
// ANET_ERR_NODEVICE.
//
// One unit per domain; each includes only the kernel headers it launches from, so every kernel is compiled in one unit:
//   api_context.hip    context, version, memory, layout transposes, RCCL
//   api_solve.hip      coefficient solve, sampling, wide-spread solve; trajectory evaluation, cost, normalisation, max rate
//   api_cost_grad.hip  cost + gradient: partial gradients, adjoint, basis tables, the one-launch decision
//   api_lbfgs.hip      L-BFGS (host, device, MVIE, MINCO), launch order, spread flags, cancel flag; FIRI and polytope depth
//                      (FIRI launches the MVIE kernels of mvie_kernels.h, which one unit only may include)
//   api_qp.hip         QP assembly, settings, solve, time gradient, VJP
//   api_voxel.hip      voxel map and route search
//   api_flatness.hip   differential flatness: states, sampled limits, penalty gradients
//   api_timenet.hip    the time-allocation network: weights handle, batched inference
//   api_polytope.hip   vertex enumeration of polytopes (geo_utils::enumerateVs)
//   api_sfc.hip        waypoints as vertex weights of corridor overlaps: the transform, its inverse, the constrained MINCO L-BFGS
//   api_margin.hip     exact margins of trajectories against corridor and box-limit rows
//   api_voxel_hit.hip  exact first collision of trajectories with the voxel map
//   api_clearance.hip  exact clearance of trajectories to obstacle points
//   api_separation.hip exact minimum separation between pairs of trajectories
//   api_avoid.hip      trajectory-avoidance penalty of the MINCO objective against neighbours of another set of trajectories
//   api_distance.hip   exact distance field of the voxel map, its query, the obstacle penalty of the MINCO objective
//   api_stop.hip       stop within known space: the penalty that couples speed with the distance field, and its sampled margin
//   api_yaw.hip        yaw trajectories: one-axis MINCO, the field-of-view / yaw-rate penalty, its sampled margin, flat states with yaw
//   api_body.hip       whole-body corridor terms: body vertices through the flatness attitude, penalty gradients and sampled margin
//   api_occupancy.hip  log-odds occupancy grid from sensor scans (ray carving), depth unprojection, first hit of a segment on the byte grid;
//                      exploration goals on it (frontier_kernels.h, which builds on occupancy_kernels.h): frontier, components, view gain
//   piece_grad_unit.hip, qp_ipm_fuse_unit.hip: kernels scheduled for ILP, reached through launch functions
// Only what two or more units use is here.  Nothing here is exported: the library's dynamic symbols stay the anet_* entry
// points (and the kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include <rccl/rccl.h>  // types only: the library is dlopen()ed

#include "../../include/allocnet_amd.h"
#include "tuning.h"
#include "workspace.h"  // the shape of every device workspace: the only place one is written
#include "staging.h"    // the staging buffers of the host entry points: one statement each, measured and carved by the same code

#pragma GCC visibility push(hidden)

// ------------------------------------------------------------------------------------------
// context + error plumbing
// ------------------------------------------------------------------------------------------
struct anet_ctx {
  int device = -1;
  // compute units of the device (hipDeviceAttributeMultiprocessorCount, read once in anet_create): the launch-shape thresholds
  // were measured on the 256 CUs of an MI355X in SPX mode and are scaled by cus / 256 (tuning.h, PerCu)
  int cus = 256;
  hipStream_t stream = nullptr;
  std::string err;
  // grow-only device scratch for the host (trajectory-major) entry points
  void *scratch = nullptr;
  size_t scratch_bytes = 0;
  // L-BFGS completion polling: device counter + pinned host mirror
  int *d_counter = nullptr;
  int *h_counter = nullptr;          // two pinned ints (polls alternate)
  hipEvent_t poll_ev[2] = {nullptr, nullptr};
  // pinned host staging for single-trajectory calls (inputs are packed and sent with ONE copy)
  double *h_pack = nullptr;
  size_t h_pack_doubles = 0;
  // cancel word of the one-launch L-BFGS (anet_set_cancel_flag), device-visible, owned by the caller
  const int32_t *cancel_flag = nullptr;
  // RCCL communicator for the all-gather of costs
  ncclComm_t comm = nullptr;
  int comm_ranks = 0;
  // basis tables of k_piece_grad, one per (order, res) ever used: never rebuilt, never freed before anet_destroy
  // (a launch on another stream may still be reading one), built on the caller's stream
  struct BasisTable {
    int s, res;
    double *d;
    hipStream_t built_on;
    hipEvent_t ready;
  };
  std::vector<BasisTable> tabs;
  // tables of k_qp_ipm, one per (order, res, m34, row form) ever used (csrc/qp_ipm.h k_qp_ipm_tables): same lifetime rules
  struct IpmTable {
    int s, res;
    double m34;
    double *d;
    hipStream_t built_on;
    hipEvent_t ready;
    int control_points;  // 0: rows at samples, 1: rows on Bernstein control values (ANET_QP_ROWS_CONTROL_POINTS)
  };
  std::vector<IpmTable> ipm_tabs;
};

extern thread_local std::string g_err;  // errors raised without a context (defined in api_context.hip)

inline int fail(anet_ctx *ctx, int code, const std::string &msg) {
  if (ctx) ctx->err = msg;
  g_err = msg;
  return code;
}
inline int hip_fail(anet_ctx *ctx, hipError_t e, const char *what) {
  return fail(ctx, ANET_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define ANET_HIP(ctx, call)                                   \
  do {                                                        \
    hipError_t e_ = (call);                                   \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, #call);    \
  } while (0)

// Every entry point makes the context's device current first: allocations made inside *_dev calls (counters, basis
// tables) and the launches must land on the context's GPU, not on whatever device the calling thread used last.  The
// caller's current device is put back on the way out (a multi-GPU torch process keeps allocating on ITS device), and
// nothing is switched when the context's device is current already.
struct DeviceGuard {
  int prev = -1;
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
#define ANET_ON_DEVICE(ctx)                                                   \
  DeviceGuard anet_device_guard_;                                             \
  do {                                                                        \
    if (!(ctx)) return fail(nullptr, ANET_ERR_INVALID, "ctx is NULL");        \
    int cur_ = -1;                                                            \
    ANET_HIP(ctx, hipGetDevice(&cur_));                                       \
    if (cur_ != (ctx)->device) {                                              \
      ANET_HIP(ctx, hipSetDevice((ctx)->device));                             \
      anet_device_guard_.prev = cur_;                                         \
    }                                                                         \
  } while (0)

inline int ensure_scratch(anet_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->scratch_bytes) return ANET_OK;
  if (ctx->scratch) {
    hipError_t e = hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    if (e != hipSuccess) return hip_fail(ctx, e, "hipFree(scratch)");
  }
  hipError_t e = hipMalloc(&ctx->scratch, bytes);
  if (e != hipSuccess) {
    ctx->scratch = nullptr;
    return fail(ctx, ANET_ERR_NOMEM, std::string("hipMalloc(scratch): ") + hipGetErrorString(e));
  }
  ctx->scratch_bytes = bytes;
  return ANET_OK;
}

// The scratch of a host (trajectory-major) entry point: layout(base) runs an anet::Cursor over base and returns the bytes taken --
// once on nullptr to size the scratch, once on the scratch to set the caller's pointers.
template <class Layout>
int stage_scratch(anet_ctx *ctx, Layout &&layout) {
  const int rc = ensure_scratch(ctx, (size_t)layout(nullptr));
  if (rc == ANET_OK) (void)layout(ctx->scratch);
  return rc;
}

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// Per-context tables (basis rows of k_piece_grad per (order, res); tables of k_qp_ipm per (order, res, m34)) live until
// anet_destroy; their number is bounded, and a table whose build fails half-way is released, not leaked.
constexpr size_t kMaxTablesPerContext = 256;
inline int new_table(anet_ctx *ctx, size_t bytes, double **d, hipEvent_t *ready) {
  *d = nullptr;
  *ready = nullptr;
  hipError_t e = hipMalloc((void **)d, bytes);
  if (e != hipSuccess) {
    *d = nullptr;
    return fail(ctx, ANET_ERR_NOMEM, std::string("hipMalloc(table): ") + hipGetErrorString(e));
  }
  e = hipEventCreateWithFlags(ready, hipEventDisableTiming);
  if (e != hipSuccess) {
    (void)hipFree(*d);
    *d = nullptr;
    *ready = nullptr;
    return hip_fail(ctx, e, "hipEventCreateWithFlags(table)");
  }
  return ANET_OK;
}
inline void drop_table(double *d, hipEvent_t ready) {
  if (d) (void)hipFree(d);
  if (ready) (void)hipEventDestroy(ready);
}

// max T / min T inside one trajectory above which the host entry point of the coefficient solve switches to the pivoted
// collocation solve (minco_dense_kernels.h)
constexpr double kWideSpread = 50.0;

int ensure_counter(anet_ctx *ctx);  // the L-BFGS / route-search completion poll: device counter, pinned mirror, events

// (callers make the context's device current first: ANET_ON_DEVICE in front of every call)
inline int check_solve_args(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch) {
  if (!ctx) return fail(nullptr, ANET_ERR_INVALID, "ctx is NULL");
  if (s < 2 || s > 4) return fail(ctx, ANET_ERR_INVALID, "order s must be 2, 3 or 4");
  if (c < 1 || c > s) return fail(ctx, ANET_ERR_INVALID, "boundary derivative count c must be in [1, s]");
  if (n_pieces < 1 || n_pieces > ANET_MAX_PIECES)
    return fail(ctx, ANET_ERR_INVALID, "piece count must be in [1, ANET_MAX_PIECES]");
  if (batch < 0) return fail(ctx, ANET_ERR_INVALID, "negative batch");
  return ANET_OK;
}

// the grid every voxel entry point accepts: sizes >= 1, fewer than 2^31 voxels, a finite origin, a finite scale > 0
inline bool voxel_grid_ok(const anet_voxel_grid *g) {
  if (!g || g->size[0] < 1 || g->size[1] < 1 || g->size[2] < 1) return false;
  if ((int64_t)g->size[0] * g->size[1] * g->size[2] >= ((int64_t)1 << 31)) return false;
  if (!(g->scale > 0.0) || !(fabs(g->scale) < INFINITY)) return false;
  for (int c = 0; c < 3; ++c)
    if (!(fabs(g->origin[c]) < INFINITY)) return false;
  return true;
}

inline int check_penalty(anet_ctx *ctx, const anet_penalty *pen) {
  if (!pen) return ANET_OK;
  if (!(pen->smooth_mu > 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_penalty.smooth_mu must be > 0");
  if (pen->res < 1) return fail(ctx, ANET_ERR_INVALID, "anet_penalty.res must be >= 1");
  if (pen->poly_rows < 0 || pen->poly_rows > ANET_MAX_POLY_ROWS)
    return fail(ctx, ANET_ERR_INVALID, "anet_penalty.poly_rows must be in [0, ANET_MAX_POLY_ROWS]");
  return ANET_OK;
}

// Host (trajectory-major) wrappers: stage -> batch-minor -> kernel -> back.  The layout of the staging buffer, the pack of a single
// trajectory and the width check of download() are staging.h's; this is its transport: the context's scratch, the pinned pack
// buffer, the copies on the context's stream and the transpose kernels.
// (the entry point that stages has made the context's device current: ANET_ON_DEVICE)
struct HipStaging {
  anet_ctx *ctx;
  int scratch(int64_t bytes, void **base) { const int rc = ensure_scratch(ctx, (size_t)bytes); *base = ctx->scratch; return rc; }
  int pack(int64_t off, const double *host, int64_t nf) {
    if ((size_t)(off + nf) > ctx->h_pack_doubles) {
      const size_t want = (size_t)(off + nf) * 2 + 1024;
      double *np_ = nullptr;
      hipError_t e1 = hipHostMalloc((void **)&np_, sizeof(double) * want, hipHostMallocDefault);
      if (e1 != hipSuccess) return hip_fail(ctx, e1, "hipHostMalloc(pack)");
      if (ctx->h_pack) {
        memcpy(np_, ctx->h_pack, sizeof(double) * off);
        (void)hipHostFree(ctx->h_pack);
      }
      ctx->h_pack = np_;
      ctx->h_pack_doubles = want;
    }
    memcpy(ctx->h_pack + off, host, sizeof(double) * nf);
    return ANET_OK;
  }
  const double *packed() const { return ctx->h_pack; }
  int put(double *dev, const double *host, int64_t n) {
    hipError_t e = hipMemcpyAsync(dev, host, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream);
    return e == hipSuccess ? ANET_OK : hip_fail(ctx, e, "hipMemcpyAsync(H2D)");
  }
  int scatter(const double *host, int64_t batch, int64_t nf, int64_t ld, double *area, double *dev) {
    const int rc = put(area, host, batch * nf);
    return rc ? rc : anet_to_batch_minor_dev(ctx, batch, nf, ld, area, dev, ctx->stream);
  }
  int fetch(const double *dev, int64_t n, double *host) {
    hipError_t e = hipMemcpyAsync(host, dev, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipMemcpyAsync(D2H)");
    e = hipStreamSynchronize(ctx->stream);  // (the staging area is reused by the next transfer)
    return e == hipSuccess ? ANET_OK : hip_fail(ctx, e, "hipStreamSynchronize");
  }
  int gather(const double *dev, int64_t batch, int64_t nf, int64_t ld, double *area, double *host) {
    const int rc = anet_to_traj_major_dev(ctx, batch, nf, ld, dev, area, ctx->stream);
    return rc ? rc : fetch(area, batch * nf, host);
  }
  int refuse(const char *why) { return fail(ctx, ANET_ERR_INVALID, why); }
};
struct Stager : anet::Staging<HipStaging> {
  Stager(anet_ctx *ctx, int64_t batch) : Staging{{ctx}, batch, batch == 1 ? 1 : anet_recommended_ld(batch)} {}
  // an int32 row plane [n][ld] on the device (Pass::rows) -> host [batch][n]: the plane comes back as it lies and is turned on
  // the host; the stream is idle on return
  int download_rows(const int32_t *dev, int64_t n, int32_t *host) {
    std::vector<int32_t> h((size_t)(n * ld));
    hipError_t e = hipMemcpyAsync(h.data(), dev, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, tr.ctx->stream);
    if (e != hipSuccess) return hip_fail(tr.ctx, e, "hipMemcpyAsync(D2H)");
    e = hipStreamSynchronize(tr.ctx->stream);
    if (e != hipSuccess) return hip_fail(tr.ctx, e, "hipStreamSynchronize");
    for (int64_t bb = 0; bb < batch; ++bb)
      for (int64_t i = 0; i < n; ++i) host[bb * n + i] = h[(size_t)(i * ld + bb)];
    return ANET_OK;
  }
};

// the parameter check of every L-BFGS entry point
inline int check_lbfgs(anet_ctx *ctx, int n, const anet_lbfgs_params *params, int max_evals) {
  const int code = anet_lbfgs_check_params(n, params);
  if (code) return fail(ctx, ANET_ERR_INVALID, std::string("lbfgs parameters rejected: ") + anet_lbfgs_strerror(code));
  if (max_evals <= 0) return fail(ctx, ANET_ERR_INVALID, "max_evals must be > 0");
  return ANET_OK;
}
// the status / iters / evals rows k_lbfgs_results filled and the cost -> the caller's host arrays
inline int download_results(anet_ctx *ctx, int64_t batch, const anet::LbfgsResultRows &r, const double *d_cost, int32_t *status,
                            int32_t *iters, int32_t *evals, double *cost, hipStream_t s0) {
  if (status) ANET_HIP(ctx, hipMemcpyAsync(status, r.status, sizeof(int) * batch, hipMemcpyDeviceToHost, s0));
  if (iters) ANET_HIP(ctx, hipMemcpyAsync(iters, r.iters, sizeof(int) * batch, hipMemcpyDeviceToHost, s0));
  if (evals) ANET_HIP(ctx, hipMemcpyAsync(evals, r.evals, sizeof(int) * batch, hipMemcpyDeviceToHost, s0));
  if (cost) ANET_HIP(ctx, hipMemcpyAsync(cost, d_cost, sizeof(double) * batch, hipMemcpyDeviceToHost, s0));
  return ANET_OK;
}

// the counting sort of the launch order (api_lbfgs.hip; anet::kOrderBuckets buckets, longest first): shift 4 for evaluation counts, 0 for Newton-step counts
int launch_order_impl(anet_ctx *ctx, int64_t batch, const int32_t *counts, int32_t *launch_order, int32_t *work, void *stream,
                      int shift);

// Between the two launches of a two-launch solve, whose first launch parked the unfinished problems in t.cont: score them
// (score(t.score) enqueues the solver's score kernel), counting-sort the scores into the order of the second launch, longest-
// expected first, and enqueue that launch (resume(t.order)).
template <class Score, class Resume>
int resume_parked(anet_ctx *ctx, int64_t batch, const anet::ResumeTail &t, hipStream_t st, Score &&score, Resume &&resume) {
  score(t.score);
  const int rc = launch_order_impl(ctx, batch, t.score, t.order, t.bins, st, 0);
  return rc ? rc : resume(t.order);
}

// The lockstep L-BFGS driver of api_lbfgs.hip for the other units (the update kernels are compiled there only): eval(instance)
// enqueues one objective evaluation of the batch at L.x -> L.feval, L.g.  reset = false: the caller has zeroed the IS_* / DS_* rows
// (lbfgs_reset_shared) and marked the problems that must not run as finished.  The other arguments are lbfgs_drive's.
int lbfgs_drive_shared(anet_ctx *ctx, anet::LbfgsLayout &L, int64_t B, const anet_lbfgs_params &prm, int max_evals, hipStream_t st,
                       int (*eval)(void *), void *instance, double *map_T, int map_nw, bool reset, int sb_on, double sb_xmin,
                       const int32_t *cancel);
int lbfgs_reset_shared(anet_ctx *ctx, const anet::LbfgsLayout &L, hipStream_t st);
// status / iters / evals / f of a run from its state rows (row stride L.ld); any of the four may be nullptr
int lbfgs_results_shared(anet_ctx *ctx, const anet::LbfgsLayout &L, int64_t B, int32_t *status, int32_t *iters, int32_t *evals,
                         double *f, hipStream_t st);
// coefficients of returned waypoints / durations: the reduced solve, then the pivoted one where the durations spread widely
int minco_final_coeffs(anet_ctx *ctx, int s, int c, int N, int64_t batch, int64_t ld, const double *head, const double *tail,
                       const double *wps, const double *T, double *coeffs_out, hipStream_t st);
// the minimum-duration bound in the variable tau (gcopter's backwardT, minco_core.h backward_T); 0: none
inline double minco_tau_min(double min_duration) {
  return min_duration > 1.0 ? sqrt(2.0 * min_duration - 1.0) - 1.0 : (min_duration > 0.0 ? 1.0 - sqrt(2.0 / min_duration - 1.0) : 0.0);
}

// cost + gradient of a batch (api_cost_grad.hip); tau != nullptr: the durations are T = forward_T(tau) and gradT is returned as
// dJ/dtau (the L-BFGS driver)
int cost_grad_dev_impl(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld, const double *head, const double *tail,
                       const double *wps, const double *T, const double *hpolys, const anet_penalty *pen, double *work, double *cost,
                       double *gradP, double *gradT, double *coeffs_out, void *stream, const double *tau);

// the basis table of k_piece_grad for (order, res) (api_cost_grad.hip owns and builds it; layout: minco_kernels.h, at k_piece_grad):
// k_flat_piece_grad reads its derivative rows 1..3, k_body_piece_grad rows 0..3.  The caller has made the context's device current.
constexpr int kBasisTableMaxRes = 4096;  // a larger res is refused (ANET_ERR_UNSUPPORTED)
int basis_table(anet_ctx *ctx, int s, int res, hipStream_t st, const double **out);

#pragma GCC visibility pop
