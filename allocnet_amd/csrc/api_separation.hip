// Exact minimum separation between pairs of trajectories (include/allocnet_amd.h; semantics, procedure and accuracy in
// separation_kernels.h).
#include "api_internal.h"
#include "minco_core.h"
#include "separation_kernels.h"

namespace {

int check_args(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t n_pairs, double cutoff) {
  int rc = check_solve_args(ctx, s, 1, n_pieces, batch);
  if (rc) return rc;
  if (n_pairs < 0) return fail(ctx, ANET_ERR_INVALID, "anet_traj_separation: negative n_pairs");
  if (!(cutoff >= 0.0)) return fail(ctx, ANET_ERR_INVALID, "anet_traj_separation: cutoff must be >= 0 (+inf: off)");
  return ANET_OK;
}

}  // namespace

extern "C" {

int anet_traj_separation_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                             const double *t0, int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double cutoff,
                             double *sep, double *t, int32_t *piece_a, int32_t *piece_b, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_args(ctx, s, n_pieces, batch, n_pairs, cutoff);
  if (rc) return rc;
  if (batch == 0 || n_pairs == 0) return ANET_OK;
  if (!coeffs || !T || !pair_a || !pair_b || !sep || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_traj_separation_dev: NULL pointer or ld < batch");
  if ((n_pairs + 63) / 64 > INT32_MAX) return fail(ctx, ANET_ERR_INVALID, "anet_traj_separation_dev: n_pairs must be below 2^37");
  anet::SeparationArgs a{coeffs, T, t0, pair_a, pair_b, sep, t, piece_a, piece_b, batch, ld, n_pairs, n_pieces, cutoff};
  const dim3 grid((unsigned)((n_pairs + 63) / 64)), block(64);
  hipStream_t st = (hipStream_t)stream;
  anet::with_order(s, [&](auto o) { hipLaunchKernelGGL(anet::k_traj_separation<decltype(o)::value>, grid, block, 0, st, a); });
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_traj_separation(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs, const double *T, const double *t0,
                         int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, double cutoff, double *sep, double *t,
                         int32_t *piece_a, int32_t *piece_b) {
  ANET_ON_DEVICE(ctx);
  int rc = check_args(ctx, s, n_pieces, batch, n_pairs, cutoff);
  if (rc) return rc;
  if (batch == 0 || n_pairs == 0) return ANET_OK;
  if (!coeffs || !T || !pair_a || !pair_b || !sep) return fail(ctx, ANET_ERR_INVALID, "anet_traj_separation: NULL pointer");
  for (int64_t p = 0; p < n_pairs; ++p)
    if (pair_a[p] < 0 || pair_a[p] >= batch || pair_b[p] < 0 || pair_b[p] >= batch)
      return fail(ctx, ANET_ERR_INVALID, "anet_traj_separation: pair index outside [0, batch)");
  const int64_t nco = (int64_t)n_pieces * 3 * 2 * s;
  Stager st(ctx, batch);
  double *d_co, *d_T, *d_t0, *d_pairs, *d_sep, *d_t, *d_pieces;
  // the two index planes travel as whole doubles, two int32 each, through the same checked copy: [pair_a | pair_b]
  std::vector<double> packed((size_t)n_pairs, 0.0);
  memcpy(packed.data(), pair_a, sizeof(int32_t) * (size_t)n_pairs);
  memcpy((int32_t *)packed.data() + n_pairs, pair_b, sizeof(int32_t) * (size_t)n_pairs);
  rc = st.stage([&](Stager::Pass &p) {
    p.in(coeffs, nco, &d_co); p.in(T, n_pieces, &d_T); p.in(t0, t0 ? 1 : 0, &d_t0);
    p.shared(packed.data(), n_pairs, &d_pairs);
    p.doubles(n_pairs, &d_sep); p.doubles(n_pairs, &d_t); p.doubles(n_pairs, &d_pieces);
  });
  if (rc) return rc;
  const int32_t *d_pa = (const int32_t *)d_pairs;
  int32_t *d_qa = (int32_t *)d_pieces;
  rc = anet_traj_separation_dev(ctx, s, n_pieces, batch, st.ld, d_co, d_T, t0 ? d_t0 : nullptr, n_pairs, d_pa, d_pa + n_pairs, cutoff,
                                d_sep, t ? d_t : nullptr, piece_a ? d_qa : nullptr, piece_b ? d_qa + n_pairs : nullptr, ctx->stream);
  if (rc) return rc;
  // the planes are contiguous on both sides: plain checked copies, the stream idle on return
  HipStaging &tr = st.tr;
  if ((rc = tr.fetch(d_sep, n_pairs, sep))) return rc;
  if (t && (rc = tr.fetch(d_t, n_pairs, t))) return rc;
  if (piece_a || piece_b) {
    std::vector<double> h((size_t)n_pairs);
    if ((rc = tr.fetch(d_pieces, n_pairs, h.data()))) return rc;
    if (piece_a) memcpy(piece_a, h.data(), sizeof(int32_t) * (size_t)n_pairs);
    if (piece_b) memcpy(piece_b, (const int32_t *)h.data() + n_pairs, sizeof(int32_t) * (size_t)n_pairs);
  }
  return ANET_OK;
}

}  // extern "C"
