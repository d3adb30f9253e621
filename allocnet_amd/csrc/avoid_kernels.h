// Trajectory-avoidance penalty of the MINCO objective: a batch of ego trajectories is kept min_dist away from listed neighbours of
// an OTHER set of piecewise polynomials (other vehicles of the fleet at a frozen iterate, moving obstacles), sampled in global time.
//
// SEMANTICS (on the doubles given, exactly; include/allocnet_amd.h states them in full).  Knots are float64 by definition:
// K_0 = t0 (0 without t0), K_(i+1) = K_i + T_i summed in piece order; the knots L_m of an other likewise from o_t0, o_T.  Sample
// j < res of ego piece i:
//     sigma = (double)j / (double)res,   tau = sigma * T_i,   t = K_i + tau        (one rounding each: sample_time, no FMA)
// and of other o the piece m with L_m <= t < L_(m+1) (which implies L_(m+1) > L_m: a piece of zero duration is never located),
// evaluated at u = t - L_m; t < L_0 or t >= L_No: the other is not there and contributes exactly nothing.
//     r = p_b,i(tau) - p_o,m(u),   q = r_x^2 + r_y^2 + (r_z / z_scale)^2,   Phi = w smoothed_l1_mu(min_dist^2 - q)
//     J_avoid(b) = sum_i (T_i / res) sum_j sum_(o in nbr(b)) Phi
// With rt = (r_x, r_y, r_z / z_scale^2), F = sum_o -2 w phi' rt and G = sum_o (-2 w phi' rt) . v_o,m(u):
//     dJ/dc[i][ax][k] = (T_i/res) sum_j F_ax tau^k
//     dJ/dT_i         = (1/res) sum_j sum Phi + (T_i/res) sum_j sigma (F . v_b,i(tau) - G) + sum_(i' > i) S_i'
//     S_i             = -(T_i/res) sum_j G,          dJ/dt0 = sum_i S_i
// NaN in every output of ego b, and of b only: a duration, t0 or knot of b that is not finite, a duration of b <= 0; a neighbour
// index outside [0, Bo) (nothing is read for it); a duration or knot of a listed neighbour that is not finite, a negative one.
//
// PROCEDURE.  One workgroup of kAvoidBlock lanes per ego trajectory; the lanes run over the flattened samples (i, j), in rounds of
// kAvoidBlock when N res exceeds the block.  The ego's durations and coefficients are staged in LDS once.  In a round a lane forms
// p_b, v_b, t of its sample once and then walks the neighbour list with Phi, F[3], G in registers -- the inner loop does not depend
// on the ego's order.  The list is taken in chunks of kAvoidBlock neighbours:
//   pre-pass   a lane per neighbour sums that neighbour's knots from global memory (No loads), raises the block's NaN flag for a bad
//              index or duration, and marks the neighbour dead when its window [L_0, L_No) misses the ego's [K_0, K_N]: a dead
//              neighbour is skipped by the whole block and its coefficients are never loaded;
//   staging    the live neighbour's start, No durations and No 3 D coefficients (strided gathers from a batch-minor buffer either
//              way) go through registers into one of two LDS images: the loads of the NEXT live neighbour are issued before the
//              arithmetic on the current one and stored after it, one barrier per neighbour;
//   location   every lane sums the knots from the image (wave-uniform addresses: broadcasts) and keeps the piece its t falls in;
//   evaluation p_o, v_o by Horner from the image.  Lanes of a wave sit in different pieces m, so these reads are lane-divergent:
//              a piece's row is padded to 3 D + 1 doubles, which puts any two pieces of the sixteen on different banks for
//              ds_read_b64 (stride 2 (3 D + 1) dwords = 26 / 38 / 50, a multiple of 64 only at 32 pieces apart).
// After the list a lane leaves Phi, F, G, H = sigma (F . v_b - G) and tau of its sample in LDS, and the contraction runs once per
// round: output row r = (i, ax, k) | (i, Phi) | (i, H) | (i, G) belongs to lane r mod kAvoidBlock, which adds the samples of piece i
// in this round in ascending j into an accumulator it keeps across the rounds (two rows per lane at most: N (3 D + 3) <= 432).
// The scale T_i / res, the suffix sum of S_i (from the last piece down) and the stores follow after the last round.
// DETERMINISM.  No atomics; every sum has a fixed order (neighbours in list order, samples in ascending j, pieces from the last
// down), and nothing depends on the launch: the outputs of ego b have the same bits alone or among many, whatever ld and o_ld.
// `accumulate`: the kernel's own share is complete before one unfused addition to the stored value (add_unfused).
// BOUNDS.  Loops run over N, No, res (through the rounds) or the list length; no input can spin a wave.  No scratch, no register
// array with a run-time index.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "penalty_terms.h"  // smoothed_l1, add_unfused

namespace anet {

constexpr int kAvoidBlock = 256;
constexpr int kAvoidMaxPieces = 16;  // ANET_MAX_PIECES (checked where the launch is)

struct AvoidArgs {
  const double *coeffs, *T, *t0;        // ego: [(i*3+ax)*2S + col][ld], [N][ld], [B] or nullptr
  const double *o_coeffs, *o_T, *o_t0;  // others: the same with ldo, No, Bo
  const int32_t *nbr_start, *nbr;       // CSR: [B + 1], [nbr_start[B]]
  double *gdC, *gdT, *pcost, *gt0;      // pcost, gt0 may be nullptr
  int64_t B, ld, Bo, ldo;
  int N, No, res, accumulate;
  double w, mu, d2, inv_z2;             // weight, smoothedL1 mu, min_dist^2, 1 / z_scale^2
};

// tau and t of a sample: one rounding each, never contracted -- the piece an other is located in depends on these bits
__device__ __forceinline__ void sample_time(const int j, const int res, const double Ti, const double Ki, double &sigma, double &tau,
                                            double &t) {
#pragma clang fp contract(off)
  sigma = (double)j / (double)res;
  tau = sigma * Ti;
  t = Ki + tau;
}

template <int S>
struct AvoidShared {
  static constexpr int D = 2 * S;
  static constexpr int kRow = 3 * D + 1;                 // a piece's coefficients, padded (see `evaluation` above)
  static constexpr int kRows = 3 * D + 3;                // output rows per piece: 3 D coefficients, Phi, H, G
  static constexpr int kImage = 1 + kAvoidMaxPieces + kAvoidMaxPieces * kRow;  // start, durations, coefficients
  double eT[kAvoidMaxPieces];
  double eC[kAvoidMaxPieces * 3 * D];
  double img[2][kImage];
  double smp[7][kAvoidBlock];                            // Phi, F[3], G, H, tau of this round's samples
  double sums[kAvoidMaxPieces * 3];                      // per piece: sum Phi, sum H, sum G
  int32_t live[kAvoidBlock];                             // this chunk's neighbours: the index, or -1 when skipped
  int32_t bad;
};

// the next live neighbour of the chunk after position e (cnt: none)
__device__ __forceinline__ int avoid_next_live(const int32_t *live, int e, const int cnt) {
  for (++e; e < cnt && live[e] < 0; ++e) {}
  return e;
}

template <int S>
__global__ void __launch_bounds__(kAvoidBlock) k_minco_avoid(AvoidArgs a) {
  using Sh = AvoidShared<S>;
  constexpr int D = Sh::D, kRow = Sh::kRow, kRows = Sh::kRows;
  __shared__ Sh sh;
  const int tid = threadIdx.x, N = a.N, No = a.No, res = a.res;
  const int64_t b = blockIdx.x, ld = a.ld, ldo = a.ldo;
  const double inv_mu = 1.0 / a.mu;

  // ---- the ego: durations and coefficients into LDS, its knots and window -----------------------------------------------------
  if (tid < N) sh.eT[tid] = a.T[(int64_t)tid * ld + b];
  for (int e = tid; e < N * 3 * D; e += kAvoidBlock) sh.eC[e] = a.coeffs[(int64_t)e * ld + b];
  if (tid == 0) sh.bad = 0;
  __syncthreads();
  const double K0 = a.t0 ? a.t0[b] : 0.0;
  double KN = K0;
  bool ego_bad = !(fabs(K0) < INFINITY);
  for (int i = 0; i < N; ++i) {
    const double Ti = sh.eT[i];
    ego_bad = ego_bad || !(fabs(Ti) < INFINITY) || !(Ti > 0.0);
    KN += Ti;
  }
  ego_bad = ego_bad || !(fabs(KN) < INFINITY);
  const int nb_lo = a.nbr_start[b], nb_hi = a.nbr_start[b + 1];

  // the output rows of this lane and their accumulators across the rounds
  const int total_rows = N * kRows;
  const int row0 = tid, row1 = tid + kAvoidBlock;
  const int pi0 = row0 / kRows, q0 = row0 % kRows, pi1 = row1 / kRows, q1 = row1 % kRows;
  double acc0 = 0.0, acc1 = 0.0;

  const int64_t M = (int64_t)N * res;
  for (int64_t base = 0; base < M && !ego_bad; base += kAvoidBlock) {
    // ---- this lane's sample ---------------------------------------------------------------------------------------------------
    const int64_t g = base + tid;
    const bool has = g < M;
    const int i = has ? (int)(g / res) : 0, j = has ? (int)(g % res) : 0;
    double Ki = K0;
    for (int k = 0; k < i; ++k) Ki += sh.eT[k];
    double sigma, tau, t;
    sample_time(j, res, sh.eT[i], Ki, sigma, tau, t);
    double pb[3], vb[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const double *c = sh.eC + (i * 3 + ax) * D;
      double p = c[0], v = 0.0;
#pragma unroll
      for (int col = 1; col < D; ++col) {
        v = __builtin_fma(v, tau, p);
        p = __builtin_fma(p, tau, c[col]);
      }
      pb[ax] = p;
      vb[ax] = v;
    }
    double Phi = 0.0, F0 = 0.0, F1 = 0.0, F2 = 0.0, G = 0.0;

    // ---- the neighbour list, in chunks ----------------------------------------------------------------------------------------
    for (int cs = nb_lo; cs < nb_hi; cs += kAvoidBlock) {
      const int cnt = min(kAvoidBlock, nb_hi - cs);
      __syncthreads();  // the previous chunk's (round's) readers of live[] and of the images are done
      {
        int32_t idx = -1;
        if (tid < cnt) {
          const int64_t o = a.nbr[cs + tid];
          if (o < 0 || o >= a.Bo) {
            sh.bad = 1;
          } else {
            const double L0 = a.o_t0 ? a.o_t0[o] : 0.0;
            double LN = L0;
            bool nb_bad = !(fabs(L0) < INFINITY);
            for (int m = 0; m < No; ++m) {
              const double Tm = a.o_T[(int64_t)m * ldo + o];
              nb_bad = nb_bad || !(fabs(Tm) < INFINITY) || Tm < 0.0;
              LN += Tm;
            }
            nb_bad = nb_bad || !(fabs(LN) < INFINITY);
            if (nb_bad) sh.bad = 1;
            else if (LN > K0 && !(L0 > KN)) idx = (int32_t)o;  // its window meets the ego's: t ranges over [K_0, K_N]
          }
        }
        sh.live[tid] = idx;
      }
      __syncthreads();
      // what this lane stages of a neighbour: its start or a duration, and up to two coefficients
      const int ne = No * 3 * D;
      const int e0 = tid, e1 = tid + kAvoidBlock;
      const int dst0 = 1 + kAvoidMaxPieces + (e0 / (3 * D)) * kRow + e0 % (3 * D);
      const int dst1 = 1 + kAvoidMaxPieces + (e1 / (3 * D)) * kRow + e1 % (3 * D);
      double rk = 0.0, rc0 = 0.0, rc1 = 0.0;
      auto fetch = [&](const int64_t o) {
        if (tid == 0) rk = a.o_t0 ? a.o_t0[o] : 0.0;
        else if (tid <= No) rk = a.o_T[(int64_t)(tid - 1) * ldo + o];
        if (e0 < ne) rc0 = a.o_coeffs[(int64_t)e0 * ldo + o];
        if (e1 < ne) rc1 = a.o_coeffs[(int64_t)e1 * ldo + o];
      };
      int nxt = avoid_next_live(sh.live, -1, cnt), buf = 0;
      if (nxt < cnt) fetch(sh.live[nxt]);
      while (nxt < cnt) {
        double *im = sh.img[buf];
        if (tid <= No) im[tid] = rk;
        if (e0 < ne) im[dst0] = rc0;
        if (e1 < ne) im[dst1] = rc1;
        __syncthreads();  // image `buf` is complete; the other one is free (its readers passed this barrier a neighbour ago)
        nxt = avoid_next_live(sh.live, nxt, cnt);
        if (nxt < cnt) fetch(sh.live[nxt]);  // in flight during the arithmetic below
        if (has) {
          // location: L_m <= t < L_(m+1)
          double L = im[0], Lm = 0.0;
          int m_at = -1;
          for (int m = 0; m < No; ++m) {
            const double Ln = L + im[1 + m];
            const bool in = t >= L && t < Ln;
            m_at = in ? m : m_at;
            Lm = in ? L : Lm;
            L = Ln;
          }
          if (m_at >= 0) {
            const double u = t - Lm;
            const double *c = im + 1 + kAvoidMaxPieces + m_at * kRow;
            double po[3], vo[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
              double p = c[ax * D], v = 0.0;
#pragma unroll
              for (int col = 1; col < D; ++col) {
                v = __builtin_fma(v, u, p);
                p = __builtin_fma(p, u, c[ax * D + col]);
              }
              po[ax] = p;
              vo[ax] = v;
            }
            const double rx = pb[0] - po[0], ry = pb[1] - po[1], rz = pb[2] - po[2], rzt = rz * a.inv_z2;
            const double q = __builtin_fma(rz, rzt, __builtin_fma(ry, ry, rx * rx));
            double f, df;
            smoothed_l1(a.mu, inv_mu, a.d2 - q, f, df);
            const double k = -2.0 * a.w * df;
            const double fx = k * rx, fy = k * ry, fz = k * rzt;
            Phi = __builtin_fma(a.w, f, Phi);
            F0 += fx;
            F1 += fy;
            F2 += fz;
            G += __builtin_fma(fz, vo[2], __builtin_fma(fy, vo[1], fx * vo[0]));
          }
        }
        buf ^= 1;
      }
    }

    // ---- the samples of this round into LDS, then the contraction per output row -------------------------------------------------
    __syncthreads();  // (smp[] of the previous round has been read)
    sh.smp[0][tid] = Phi;
    sh.smp[1][tid] = F0;
    sh.smp[2][tid] = F1;
    sh.smp[3][tid] = F2;
    sh.smp[4][tid] = G;
    sh.smp[5][tid] = sigma * (__builtin_fma(F2, vb[2], __builtin_fma(F1, vb[1], F0 * vb[0])) - G);
    sh.smp[6][tid] = tau;
    __syncthreads();
    auto contract = [&](const int row, const int pi, const int q, double &acc) {
      if (row >= total_rows) return;
      // the samples of piece pi in this round: g in [pi res, (pi + 1) res) cut to [base, base + kAvoidBlock)
      const int64_t lo = max((int64_t)pi * res, base), hi = min((int64_t)(pi + 1) * res, min(base + kAvoidBlock, M));
      const int src = q < 3 * D ? 1 + q / D : (q == 3 * D ? 0 : (q == 3 * D + 1 ? 5 : 4));
      const int pw = q < 3 * D ? D - 1 - q % D : 0;
      for (int64_t gg = lo; gg < hi; ++gg) {
        const int l = (int)(gg - base);
        double term = sh.smp[src][l];
        const double tl = sh.smp[6][l];
        for (int e = 0; e < pw; ++e) term *= tl;
        acc += term;
      }
    };
    contract(row0, pi0, q0, acc0);
    contract(row1, pi1, q1, acc1);
  }

  // ---- scales, the suffix sum of S, the stores ------------------------------------------------------------------------------------
  __syncthreads();
  const bool nan_out = ego_bad || sh.bad != 0;
  const double qnan = __builtin_nan("");
  auto put = [&](double *p, const double v) { *p = a.accumulate ? add_unfused(*p, v) : v; };
  auto finish = [&](const int row, const int pi, const int q, const double acc) {
    if (row >= total_rows) return;
    if (q < 3 * D) {
      const double step = sh.eT[pi] / (double)res;
      put(a.gdC + (int64_t)(pi * 3 * D + q) * ld + b, nan_out ? qnan : step * acc);
    } else {
      sh.sums[pi * 3 + (q - 3 * D)] = acc;
    }
  };
  finish(row0, pi0, q0, acc0);
  finish(row1, pi1, q1, acc1);
  __syncthreads();
  if (tid < N) {
    double suffix = 0.0, all = 0.0;  // sum of S_i' over i' > tid, over all i': from the last piece down
    for (int i = N - 1; i >= 0; --i) {
      const double Si = -(sh.eT[i] / (double)res) * sh.sums[i * 3 + 2];
      if (i == tid) suffix = all;
      all += Si;
    }
    const double Ti = sh.eT[tid], step = Ti / (double)res, sPhi = sh.sums[tid * 3];
    const double gT = (sPhi / (double)res + step * sh.sums[tid * 3 + 1]) + suffix;
    put(a.gdT + (int64_t)tid * ld + b, nan_out ? qnan : gT);
    if (a.pcost) put(a.pcost + (int64_t)tid * ld + b, nan_out ? qnan : step * sPhi);
    if (tid == 0 && a.gt0) put(a.gt0 + b, nan_out ? qnan : all);
  }
}

}  // namespace anet
