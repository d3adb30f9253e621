// Control-point row form of the inequality QP (ANET_QP_ROWS_CONTROL_POINTS): the linear functional behind "group j" of a piece.
//
// The sample form holds a row at tau_j = j / res; this form holds it on the Bernstein control values instead.  With D = 2s and
// res = K D, group j = q D + r stands for segment q of the piece, [q / K, (q + 1) / K] in normalised time, and control index r:
// for derivative d in {0, 1, 2} the d-th derivative of the piece is restricted to the segment, written in the Bernstein basis of
// its own degree n = D - 1 - d, and degree-elevated d times to D values beta^d_0 .. beta^d_(D-1).  A polynomial lies in the hull
// of its control values and an elevated value is a convex combination of the originals, so a row every beta^d_r of a segment
// satisfies holds for every t of that segment.
//
// Everything after the monomial-to-Bernstein map is an average with weights in [0, 1] (de Casteljau to the left of (q + 1) / K,
// then to the right of q / (q + 1); elevation): no shifted monomial is expanded, nothing cancels.  The map itself has the positive
// weights C(i, k) / C(n, k).  One statement for the interior point's table (k_qp_ipm_tables, applied to the Hermite basis) and
// for the dense assembly (k_qp_ineq, applied to the monomials).
#pragma once
#include <hip/hip_runtime.h>

namespace anet {

// c[k]: ascending coefficients of P(tau) = sum_k c[k] tau^k (degree D - 1).  out[r] = beta^d_r of P on segment q of K.
template <int D>
__host__ __device__ inline void qp_control_values(const double (&c)[D], int d, int q, int K, double (&out)[D]) {
  const int n = D - 1 - d;  // degree of the derivative
  double u[D], b[D];
  for (int k = 0; k <= n; ++k) {  // P^(d) = sum_k u[k] tau^k
    double f = 1.0;
    for (int e = 0; e < d; ++e) f *= (double)(k + d - e);
    u[k] = f * c[k + d];
  }
  // Bernstein control values on [0, 1]: b_i = sum_(k <= i) C(i, k) / C(n, k) u_k, the ratio as a running product
  for (int i = 0; i <= n; ++i) {
    double v = 0.0, w = 1.0;
    for (int k = 0; k <= i; ++k) {
      v += w * u[k];
      w *= (double)(i - k) / (double)(n - k > 0 ? n - k : 1);
    }
    b[i] = v;
  }
  if (q + 1 < K) {  // keep [0, (q + 1) / K]: b[i] <- b_0^(i)
    const double t = (double)(q + 1) / (double)K, t1 = 1.0 - t;
    for (int l = 1; l <= n; ++l)
      for (int i = n; i >= l; --i) b[i] = t1 * b[i - 1] + t * b[i];
  }
  if (q > 0) {  // of that, keep [q / (q + 1), 1]: b[i] <- b_i^(n - i)
    const double t = (double)q / (double)(q + 1), t1 = 1.0 - t;
    for (int l = 1; l <= n; ++l)
      for (int i = 0; i <= n - l; ++i) b[i] = t1 * b[i] + t * b[i + 1];
  }
  for (int nn = n; nn < D - 1; ++nn) {  // degree nn -> nn + 1
    b[nn + 1] = b[nn];
    for (int i = nn; i >= 1; --i) {
      const double w = (double)i / (double)(nn + 1);
      b[i] = w * b[i - 1] + (1.0 - w) * b[i];
    }
  }
  for (int r = 0; r < D; ++r) out[r] = b[r];
}

}  // namespace anet
