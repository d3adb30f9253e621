// The register-resident L-BFGS of one problem (one wave, one variable per lane) and the layout it is parked in between two launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lbfgs_step.h"
#include "workspace_constants.h"  // kPersistContLaneFields, kPersistContDoubles
#include "wave_ops.h"

namespace anet {

// A parked optimiser (PersistArgs::park / resume): kPersistContLaneFields per-lane values x 64 lanes ([field][lane]), then 64
// wave-uniform ones.  The slots are named here, next to park / unpark, for every reader (k_lbfgs_resume_score takes PARK_U_FX,
// PARK_U_F_HALF and PARK_U_GN2; tools/lbfgs_split_features.py reads the same layout from Python).
enum { PARK_X = 0, PARK_G, PARK_D, PARK_XP, PARK_GP, PARK_PF, PARK_HS, PARK_HY = PARK_HS + 8, PARK_LANE_FIELDS_ = PARK_HY + 8 };
enum {
  PARK_U_HYS = 0, PARK_U_FX = PARK_U_HYS + 8, PARK_U_STEP, PARK_U_FINIT, PARK_U_DGTEST, PARK_U_DSTEST, PARK_U_MU, PARK_U_NU,
  PARK_U_SMAX, PARK_U_K, PARK_U_BOUND, PARK_U_COUNT, PARK_U_BRACKT, PARK_U_TOUCHED, PARK_U_EVALS, PARK_U_PHASE,
  PARK_U_F_HALF,  // the cost at PersistArgs::half_mark (for the order of the second launch only)
  PARK_U_GN2,     // gp.gp (likewise)
  PARK_U_COUNT_
};
static_assert(PARK_LANE_FIELDS_ == kPersistContLaneFields && PARK_U_COUNT_ <= 64, "layout of the parked state");
__host__ __device__ __forceinline__ const double *parked_uniform(const double *c) { return c + kPersistContLaneFields * 64; }
__host__ __device__ __forceinline__ double *parked_uniform(double *c) { return c + kPersistContLaneFields * 64; }

// The register-resident L-BFGS of one problem: lbfgs_update_wave_body (one variable per lane, history carried)
// without its loads and stores.  pf: lane j holds pf[j] of the past-f ring.
// LAST: the highest lane that can hold a non-zero component (63: any n <= 64; 15: n <= 16, reductions stop after one row).
// lbfgs_optimize's proc_stepbound (lbfgs.hpp:221-224, 557-565) as a built-in: the largest step along d that keeps the variables
// of lanes [lo, hi) at or above xmin -- for the MINCO objective the duration variables tau and xmin = backward_T(minimum
// duration), so that no line search ever leaves T >= T_min.  on = 0: no bound (step_max = max_step, as with a NULL callback).
struct StepBound {
  int on, lo, hi;
  double xmin;
};

template <int MR, int LAST = 63>
struct LbfgsResident {
  double x, g, d, xp, gp;
  LineSearch ls;  // the running line search (ls.smax: min(step bound, max_step))
  double hs[MR], hy[MR], hys[MR];  // hys: 1 / (y.s) of the slot
  double fx, step, pf;
  int k, bound, evals, phase;

  __device__ __forceinline__ void init(double x0) {
    x = x0;
    g = d = xp = gp = 0.0;
#pragma unroll
    for (int it = 0; it < MR; ++it) {
      hs[it] = hy[it] = 0.0;
      hys[it] = 1.0;
    }
    fx = step = ls.finit = ls.dgtest = ls.dstest = ls.mu = ls.nu = pf = ls.smax = 0.0;
    k = bound = ls.count = ls.brackt = ls.touched = evals = phase = 0;
  }
  // the whole state to / from global memory ([field][lane], then 64 wave-uniform values): what a second launch needs to go on
  // exactly where this one stopped (PersistArgs::park / resume)
  __device__ __forceinline__ void park(double *c, const int lane, const double f_half) const {
    static_assert(MR <= 8, "layout of the parked state");
    double *pl = c + lane;
    pl[PARK_X * 64] = x; pl[PARK_G * 64] = g; pl[PARK_D * 64] = d; pl[PARK_XP * 64] = xp; pl[PARK_GP * 64] = gp; pl[PARK_PF * 64] = pf;
#pragma unroll
    for (int it = 0; it < MR; ++it) {
      pl[(PARK_HS + it) * 64] = hs[it];
      pl[(PARK_HY + it) * 64] = hy[it];
    }
    const double gn2 = dot(gp, gp);
    if (lane == 0) {
      double *u = parked_uniform(c);
#pragma unroll
      for (int it = 0; it < MR; ++it) u[PARK_U_HYS + it] = hys[it];
      u[PARK_U_FX] = fx; u[PARK_U_STEP] = step; u[PARK_U_FINIT] = ls.finit; u[PARK_U_DGTEST] = ls.dgtest;
      u[PARK_U_DSTEST] = ls.dstest; u[PARK_U_MU] = ls.mu; u[PARK_U_NU] = ls.nu; u[PARK_U_SMAX] = ls.smax;
      u[PARK_U_K] = (double)k; u[PARK_U_BOUND] = (double)bound; u[PARK_U_COUNT] = (double)ls.count;
      u[PARK_U_BRACKT] = (double)ls.brackt; u[PARK_U_TOUCHED] = (double)ls.touched;
      u[PARK_U_EVALS] = (double)evals; u[PARK_U_PHASE] = (double)phase;
      u[PARK_U_F_HALF] = f_half;
      u[PARK_U_GN2] = gn2;
    }
  }
  __device__ __forceinline__ void unpark(const double *c, const int lane) {
    const double *pl = c + lane;
    x = pl[PARK_X * 64]; g = pl[PARK_G * 64]; d = pl[PARK_D * 64]; xp = pl[PARK_XP * 64]; gp = pl[PARK_GP * 64]; pf = pl[PARK_PF * 64];
#pragma unroll
    for (int it = 0; it < MR; ++it) {
      hs[it] = pl[(PARK_HS + it) * 64];
      hy[it] = pl[(PARK_HY + it) * 64];
    }
    const double *u = parked_uniform(c);
#pragma unroll
    for (int it = 0; it < MR; ++it) hys[it] = u[PARK_U_HYS + it];
    fx = u[PARK_U_FX]; step = u[PARK_U_STEP]; ls.finit = u[PARK_U_FINIT]; ls.dgtest = u[PARK_U_DGTEST];
    ls.dstest = u[PARK_U_DSTEST]; ls.mu = u[PARK_U_MU]; ls.nu = u[PARK_U_NU]; ls.smax = u[PARK_U_SMAX];
    k = (int)u[PARK_U_K]; bound = (int)u[PARK_U_BOUND]; ls.count = (int)u[PARK_U_COUNT];
    ls.brackt = (int)u[PARK_U_BRACKT]; ls.touched = (int)u[PARK_U_TOUCHED];
    evals = (int)u[PARK_U_EVALS]; phase = (int)u[PARK_U_PHASE];
  }
  __device__ __forceinline__ static double dot(double u, double v) { return wave_sum<LAST>(u * v); }
  // |g|_inf / max(1, |x|_inf) < g_epsilon (lbfgs.hpp:520-524, 592-596), the quotient cleared
  // (g_epsilon = 0, the setting of the reference's only call site: a norm is never below zero, the two reductions are skipped)
  __device__ __forceinline__ bool conv_test(const LbfgsP &P) const {
    if (!(P.g_epsilon > 0.0)) return false;
    return wave_max_nonneg<LAST>(fabs(g)) < P.g_epsilon * fmax(1.0, wave_max_nonneg<LAST>(fabs(x)));
  }
  // consumes f = objective at x (gradient already in g); leaves the next point in x.  Returns the lbfgs.hpp
  // return code when the problem stops, 0x7fffffff while it runs.
  __device__ __forceinline__ int update(const LbfgsP &P, const int lane, const double f, const StepBound sb = StepBound{0, 0, 0, 0.0},
                                        const int cancel = 0) {
    const int m = P.mem_size;
    ++evals;
    bool start_ls = false;
    int finish = 0x7fffffff;
    if (phase == 0) {
      fx = f;
      pf = (lane == 0) ? fx : pf;
      d = -g;
      const double dd = dot(g, g);
      if (conv_test(P)) {
        finish = LB_CONVERGENCE;
      } else {
        step = 1.0 / sqrt(dd);
        k = 1;
        bound = 0;
        phase = 1;
        start_ls = true;
      }
    } else {
      bool success;
      const int err = ls_trial(P, ls, f, step, success, [&]() { return dot(g, d); });
      if (err) {  // revert; the reported f stays the last trial's (lbfgs.hpp:570-577,713)
        x = xp;
        g = gp;
        fx = f;
        finish = err;
      } else if (!success) {
        x = trial_point(step, d, xp);
      } else {
        fx = f;
        finish = stop_tests(
            P, cancel, k, fx, [&]() { return conv_test(P); },
            [&](int slot) {
              return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(pf), slot),
                                      __builtin_amdgcn_readlane(__double2loint(pf), slot));
            },
            [&](int slot) { pf = (lane == slot) ? fx : pf; });
        if (finish == 0x7fffffff) {
          ++k;
          const double sreg = x - xp, yreg = g - gp;
          double dv = -g;
          const double ys = dot(yreg, sreg), yy = dot(yreg, yreg), ss = dot(sreg, sreg), gpgp = dot(gp, gp);
          const double cau = ss * sqrt(gpgp) * P.cautious_factor;
          if (ys > cau) {
            ++bound;
            bound = m < bound ? m : bound;
            hs[0] = sreg;
            hy[0] = yreg;
            hys[0] = 1.0 / ys;  // one division per stored pair instead of two per slot and iteration
            double alpha[MR];
#pragma unroll
            for (int it = 0; it < MR; ++it) {
              alpha[it] = 0.0;
              if (it < bound) {
                alpha[it] = dot(hs[it], dv) * hys[it];
                dv = __builtin_fma(-alpha[it], hy[it], dv);
              }
            }
            dv *= ys / yy;
#pragma unroll
            for (int it = MR - 1; it >= 0; --it) {
              if (it < bound) {
                const double cf = alpha[it] - dot(hy[it], dv) * hys[it];
                dv = __builtin_fma(cf, hs[it], dv);
              }
            }
#pragma unroll
            for (int it = MR - 1; it > 0; --it) {  // the stored pair is one slot behind the next new pair
              hs[it] = hs[it - 1];
              hy[it] = hy[it - 1];
              hys[it] = hys[it - 1];
            }
          }
          d = dv;
          step = 1.0;
          start_ls = true;
        }
      }
    }
    if (start_ls) {  // lbfgs.hpp:553-565, then the entry of line_search_lewisoverton (lbfgs.hpp:287-305)
      xp = x;
      gp = g;
      ls.smax = P.max_step;
      if (sb.on) {  // proc_stepbound(xp, d)
        const bool mine = lane >= sb.lo && lane < sb.hi && d < 0.0;
        const double q = mine ? step_bound_ratio(d, x, sb.xmin) : 0.0;
        ls_bound_step(P, ls, step, step_bound_of(wave_max_nonneg<LAST>(q)));
      }
      const double dginit = dot(g, d);
      finish = ls_entry_check(step, dginit);
      if (finish == 0x7fffffff) {
        ls_fresh(P, ls, fx, dginit);
        x = trial_point(step, d, x);
      }
    }
    return finish;
  }
};

}  // namespace anet
