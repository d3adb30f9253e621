// firi::costMVIE as an objective (one lane or one wave per problem) and the whole MVIE optimisation in one launch, with the
// optimiser's state in memory (k_lbfgs_mvie_persistent) or in registers (k_lbfgs_mvie_resident).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "penalty_terms.h"  // smoothed_l1
#include "lbfgs_kernels.h"
#include "lbfgs_resident.h"

namespace anet {

// firi::costMVIE (gcopter/firi.hpp:86-157): x = [p, rtd, cde], A is M x 3 column-major per problem
// (field k*M + r), the reference's optData packing (firi.hpp:186-200).
struct MvieArgs {
  const double *A, *x;
  double *f, *g;
  const int *done;
  int64_t B, ld;
  int M;
  double eps, wt;
};
__device__ __forceinline__ void mvie_eval_lane(const MvieArgs &a, const int64_t b) {
  if (a.done && a.done[b]) return;
  const int64_t ld = a.ld;
  const double *x = a.x + b;
  double p[3], rtd[3], cde[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    p[q] = x[q * ld];
    rtd[q] = x[(3 + q) * ld];
    cde[q] = x[(6 + q) * ld];
  }
  const double L00 = rtd[0] * rtd[0] + 2.220446049250313e-16, L11 = rtd[1] * rtd[1] + 2.220446049250313e-16,
               L22 = rtd[2] * rtd[2] + 2.220446049250313e-16;
  const double L10 = cde[0], L21 = cde[1], L20 = cde[2];
  double cost = 0.0, gdp[3] = {0, 0, 0}, gdr[3] = {0, 0, 0}, gdc[3] = {0, 0, 0};
  const double inv_mu = 1.0 / a.eps;
  for (int r = 0; r < a.M; ++r) {
    const double a0 = a.A[(int64_t)r * ld + b], a1 = a.A[(int64_t)(a.M + r) * ld + b],
                 a2 = a.A[(int64_t)(2 * a.M + r) * ld + b];
    const double al0 = a0 * L00 + a1 * L10 + a2 * L20, al1 = a1 * L11 + a2 * L21, al2 = a2 * L22;
    const double nrm = sqrt(al0 * al0 + al1 * al1 + al2 * al2);
    const double viol = nrm + (a0 * p[0] + a1 * p[1] + a2 * p[2]) - 1.0;
    if (viol >= 0.0) {
      double c, dc;
      smoothed_l1(a.eps, inv_mu, viol, c, dc);
      const double inv = 1.0 / nrm;
      const double adj0 = al0 * inv, adj1 = al1 * inv, adj2 = al2 * inv;
      const double v0 = dc * a0, v1 = dc * a1, v2 = dc * a2;
      cost += c;
      gdp[0] += v0; gdp[1] += v1; gdp[2] += v2;
      gdr[0] += adj0 * v0; gdr[1] += adj1 * v1; gdr[2] += adj2 * v2;
      gdc[0] += adj0 * v1;
      gdc[1] += adj1 * v2;
      gdc[2] += adj0 * v2;
    }
  }
  cost *= a.wt;
  cost -= log(L00) + log(L11) + log(L22);
  const double Ld[3] = {L00, L11, L22};
  double *g = a.g + b;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    g[q * ld] = gdp[q] * a.wt;
    g[(3 + q) * ld] = (gdr[q] * a.wt - 1.0 / Ld[q]) * 2.0 * rtd[q];
    g[(6 + q) * ld] = gdc[q] * a.wt;
  }
  a.f[b] = cost;
}
__global__ void __launch_bounds__(64) k_mvie_eval(MvieArgs a) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b < a.B) mvie_eval_lane(a, b);
}

// costMVIE with one WAVE per problem: the rows of A are spread over the lanes, the ten sums (cost, nine gradient
// parts) are wave reductions.  Same quantities as mvie_eval_lane, summed in a different order.
__device__ __forceinline__ void mvie_eval_wave(const MvieArgs &a, const int64_t b, const int lane) {
  const int64_t ld = a.ld;
  const double *x = a.x + b;
  double p[3], rtd[3], cde[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    p[q] = x[q * ld];
    rtd[q] = x[(3 + q) * ld];
    cde[q] = x[(6 + q) * ld];
  }
  const double L00 = rtd[0] * rtd[0] + 2.220446049250313e-16, L11 = rtd[1] * rtd[1] + 2.220446049250313e-16,
               L22 = rtd[2] * rtd[2] + 2.220446049250313e-16;
  const double L10 = cde[0], L21 = cde[1], L20 = cde[2];
  double cost = 0.0, gdp[3] = {0, 0, 0}, gdr[3] = {0, 0, 0}, gdc[3] = {0, 0, 0};
  const double inv_mu = 1.0 / a.eps;
  for (int r = lane; r < a.M; r += 64) {
    const double a0 = a.A[(int64_t)r * ld + b], a1 = a.A[(int64_t)(a.M + r) * ld + b],
                 a2 = a.A[(int64_t)(2 * a.M + r) * ld + b];
    const double al0 = a0 * L00 + a1 * L10 + a2 * L20, al1 = a1 * L11 + a2 * L21, al2 = a2 * L22;
    const double nrm = sqrt(al0 * al0 + al1 * al1 + al2 * al2);
    const double viol = nrm + (a0 * p[0] + a1 * p[1] + a2 * p[2]) - 1.0;
    if (viol >= 0.0) {
      double c, dc;
      smoothed_l1(a.eps, inv_mu, viol, c, dc);
      const double inv = 1.0 / nrm;
      const double adj0 = al0 * inv, adj1 = al1 * inv, adj2 = al2 * inv;
      const double v0 = dc * a0, v1 = dc * a1, v2 = dc * a2;
      cost += c;
      gdp[0] += v0; gdp[1] += v1; gdp[2] += v2;
      gdr[0] += adj0 * v0; gdr[1] += adj1 * v1; gdr[2] += adj2 * v2;
      gdc[0] += adj0 * v1;
      gdc[1] += adj1 * v2;
      gdc[2] += adj0 * v2;
    }
  }
  cost = wave_sum(cost);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    gdp[q] = wave_sum(gdp[q]);
    gdr[q] = wave_sum(gdr[q]);
    gdc[q] = wave_sum(gdc[q]);
  }
  cost *= a.wt;
  cost -= log(L00) + log(L11) + log(L22);
  const double Ld[3] = {L00, L11, L22};
  if (lane == 0) {
    double *g = a.g + b;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      g[q * ld] = gdp[q] * a.wt;
      g[(3 + q) * ld] = (gdr[q] * a.wt - 1.0 / Ld[q]) * 2.0 * rtd[q];
      g[(6 + q) * ld] = gdc[q] * a.wt;
    }
    a.f[b] = cost;
  }
}

// A whole MVIE optimisation in ONE launch: one wave per problem loops evaluation + L-BFGS update (the same
// update body as k_lbfgs_update_wave, state in the same arrays).  The launch-per-evaluation driver spends a
// corridor search of a handful of segments almost entirely on launch latency (hundreds of evaluations of a
// 9-variable problem); here an evaluation costs a few memory round trips.  The fences order the cross-lane
// traffic through global memory inside the wave (workgroup scope: the lanes share one L1).
template <int LBFGS_WAVE_MREG>
__global__ void __launch_bounds__(64 * LbfgsWaveShape<LBFGS_WAVE_MREG>::kWaves)
k_lbfgs_mvie_persistent(LbfgsArgs la, MvieArgs ma, int max_evals) {
  const int64_t b = (int64_t)blockIdx.x * LbfgsWaveShape<LBFGS_WAVE_MREG>::kWaves + (threadIdx.x >> 6);
  if (b >= la.B) return;
  const int lane = threadIdx.x & 63;
  const int *done = la.is + (int64_t)IS_DONE * la.ld + b;
  // When mem_size fits, the history stays in registers across the iterations: the first one fills it from memory
  // as the per-launch kernel does (nothing to read in a fresh run), the later ones carry it.
  WaveHistory<(LBFGS_WAVE_MREG > 0 ? LBFGS_WAVE_MREG : 1), 1> H;
  H.clear();
  const bool carry = LBFGS_WAVE_MREG > 0 && la.p.mem_size <= LBFGS_WAVE_MREG;
  for (int e = 0; e < max_evals; ++e) {
    if (__builtin_amdgcn_readfirstlane(*(volatile const int *)done)) break;
    mvie_eval_wave(ma, b, lane);
    __threadfence_block();
    // nine variables: one per lane
    if (carry && e > 0) lbfgs_update_wave_body<LBFGS_WAVE_MREG, 1, true, 15>(la, b, lane, H);
    else lbfgs_update_wave_body<LBFGS_WAVE_MREG, 1, false, 15>(la, b, lane, H);
    __threadfence_block();
  }
}

// firi::maxVolInsEllipsoid's optimisation (firi.hpp:207-227) in one launch with NOTHING in memory between the iterations:
// one wave per polytope, the rows of A in registers (lane = row, RG groups of 64), the nine variables and the L-BFGS
// state in LbfgsResident (variable = lane), costMVIE (firi.hpp:86-157) as ten wave sums over the rows.  The variant with
// the state in memory (k_lbfgs_mvie_persistent: x, g, f and the optimiser state through L1 / L2 every iteration) spent
// about half of an iteration on those round trips.  Same arithmetic as mvie_eval_wave + lbfgs_update_wave_body.
template <int MR, int RG>
__global__ void __launch_bounds__(64) k_lbfgs_mvie_resident(LbfgsArgs la, MvieArgs ma, int max_evals) {
  const int64_t b = blockIdx.x, ld = la.ld;
  const int lane = threadIdx.x;
  if (la.is[(int64_t)IS_DONE * ld + b]) return;  // (corridors FIRI's set-up found empty)
  double a0[RG], a1[RG], a2[RG];
#pragma unroll
  for (int g = 0; g < RG; ++g) {
    const int r = lane + 64 * g;
    const bool v = r < ma.M;
    a0[g] = v ? ma.A[(int64_t)r * ld + b] : 0.0;
    a1[g] = v ? ma.A[(int64_t)(ma.M + r) * ld + b] : 0.0;
    a2[g] = v ? ma.A[(int64_t)(2 * ma.M + r) * ld + b] : 0.0;
  }
  LbfgsResident<MR, 15> st;
  st.init(lane < 9 ? la.x[(int64_t)lane * ld + b] : 0.0);
  const double inv_mu = 1.0 / ma.eps;
  int finish = 0x7fffffff;
#pragma unroll 1
  for (int e = 0; e < max_evals; ++e) {
    double xv[9];
#pragma unroll
    for (int q = 0; q < 9; ++q)
      xv[q] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(st.x), q), __builtin_amdgcn_readlane(__double2loint(st.x), q));
    const double L00 = xv[3] * xv[3] + 2.220446049250313e-16, L11 = xv[4] * xv[4] + 2.220446049250313e-16,
                 L22 = xv[5] * xv[5] + 2.220446049250313e-16;
    const double L10 = xv[6], L21 = xv[7], L20 = xv[8];
    double cost = 0.0, gdp[3] = {0, 0, 0}, gdr[3] = {0, 0, 0}, gdc[3] = {0, 0, 0};
#pragma unroll
    for (int g = 0; g < RG; ++g) {
      const double al0 = a0[g] * L00 + a1[g] * L10 + a2[g] * L20, al1 = a1[g] * L11 + a2[g] * L21, al2 = a2[g] * L22;
      const double nrm = sqrt(al0 * al0 + al1 * al1 + al2 * al2);
      const double viol = nrm + (a0[g] * xv[0] + a1[g] * xv[1] + a2[g] * xv[2]) - 1.0;
      if (viol >= 0.0) {
        double c, dc;
        smoothed_l1(ma.eps, inv_mu, viol, c, dc);
        const double inv = fast_rcp(nrm);  // (v_rcp_f64 + two Newton steps: 5 instructions where the IEEE division takes ~30)
        const double adj0 = al0 * inv, adj1 = al1 * inv, adj2 = al2 * inv;
        const double v0 = dc * a0[g], v1 = dc * a1[g], v2 = dc * a2[g];
        cost += c;
        gdp[0] += v0; gdp[1] += v1; gdp[2] += v2;
        gdr[0] += adj0 * v0; gdr[1] += adj1 * v1; gdr[2] += adj2 * v2;
        gdc[0] += adj0 * v1;
        gdc[1] += adj1 * v2;
        gdc[2] += adj0 * v2;
      }
    }
    cost = wave_sum(cost);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      gdp[q] = wave_sum(gdp[q]);
      gdr[q] = wave_sum(gdr[q]);
      gdc[q] = wave_sum(gdc[q]);
    }
    cost *= ma.wt;
    cost -= log(L00 * L11 * L22);  // (one logarithm instead of three: ~70 wave instructions each)
    const double Ld[3] = {L00, L11, L22};
    double g = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      g = (lane == q) ? gdp[q] * ma.wt : g;
      g = (lane == 3 + q) ? (gdr[q] * ma.wt - fast_rcp(Ld[q])) * 2.0 * xv[3 + q] : g;
      g = (lane == 6 + q) ? gdc[q] * ma.wt : g;
    }
    st.g = g;
    finish = __builtin_amdgcn_readfirstlane(st.update(la.p, lane, cost));
    if (finish != 0x7fffffff) break;
  }
  if (lane < 9) la.x[(int64_t)lane * ld + b] = st.x;
  if (lane == 0) {
    la.is[(int64_t)IS_DONE * ld + b] = finish != 0x7fffffff;
    la.is[(int64_t)IS_RET * ld + b] = finish;
    la.is[(int64_t)IS_K * ld + b] = st.k;
    la.is[(int64_t)IS_EVALS * ld + b] = st.evals;
    la.ds[(int64_t)DS_FX * ld + b] = st.fx;
  }
}

}  // namespace anet
