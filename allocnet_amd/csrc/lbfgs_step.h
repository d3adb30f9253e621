// The L-BFGS / Lewis-Overton step (lbfgs.hpp:276-384, 434-717) on scalars: parameters, state rows, return codes and the
// decision logic of one optimiser step, written once for the kernel forms that run it --
//   lbfgs_update_lane (lbfgs_kernels.h: lane per problem, state in memory),
//   LbfgsResident::update (lbfgs_resident.h: wave per problem, state in registers);
// the third form, lbfgs_update_wave_body (lbfgs_kernels.h: wave per problem, state in memory), keeps its own copy for a
// measured reason given there.
// A form owns its data movement (where x, g, d, xp, gp and the history live, how a dot product or a maximum is reduced,
// whether the scalars are wave-uniform, whether the host parks the machine); it hands its reductions in as callables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "workspace_constants.h"  // the DS_* / IS_* state rows

namespace anet {

// ------------------------------------------------------------------------------------------
// batched L-BFGS (lbfgs.hpp:276-384, 434-717) as a per-trajectory state machine
// ------------------------------------------------------------------------------------------
struct LbfgsP {
  int mem_size;
  double g_epsilon;
  int past;
  double delta;
  int max_iterations, max_linesearch;
  double min_step, max_step, f_dec_coeff, s_curv_coeff, cautious_factor, machine_prec;
};
enum {  // lbfgs.hpp:135-184
  LB_CONVERGENCE = 0, LB_STOP = 1, LB_CANCELED = 2,
  LBERR_INVALID_FUNCVAL = -1012, LBERR_MINIMUMSTEP = -1011, LBERR_MAXIMUMSTEP = -1010,
  LBERR_MAXIMUMLINESEARCH = -1009, LBERR_MAXIMUMITERATION = -1008, LBERR_WIDTHTOOSMALL = -1007,
  LBERR_INVALIDPARAMETERS = -1006, LBERR_INCREASEGRADIENT = -1005
};
enum { LB_PHASE_FIRST = 0, LB_PHASE_SEARCH = 1, LB_PHASE_AWAIT_PROGRESS = 2, LB_PHASE_AWAIT_STEPBOUND = 3 };
__device__ __forceinline__ int read_cancel_word(const int *w) {  // system scope: written while the kernels run
  return w ? __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0;
}
// x = xp + step * d as the reference computes it (lbfgs.hpp:308): the reference is built with -O3 and no -march
// (src/planner/CMakeLists.txt:4-6), i.e. for baseline x86-64, where this is a multiply and an add -- two roundings.  The
// trial point decides every later comparison of a line search, so the kernels round it the same way instead of fusing.
__device__ __forceinline__ double trial_point(double step, double d, double xp) {
#pragma clang fp contract(off)
  const double p = step * d;
  return xp + p;
}

// The scalars of a running line_search_lewisoverton (the DS_FINIT .. DS_SMAX and IS_COUNT .. IS_TOUCHED rows).
struct LineSearch {
  double finit, dgtest, dstest, mu, nu;
  double smax;  // stpmax: min(step bound, max_step)
  int count, brackt, touched;
};

// lbfgs_optimize's proc_stepbound (lbfgs.hpp:221-224) as the built-in bound "variable x may not fall below xmin": what a
// variable that moves down (d < 0) asks of the step, as 1 / step; the bound is one over the largest of these.
__device__ __forceinline__ double step_bound_ratio(double d, double x, double xmin) {
  const double room = x - xmin;
  return -d / (room > 1e-300 ? room : 1e-300);
}
__device__ __forceinline__ double step_bound_of(double worst_ratio) { return worst_ratio > 0.0 ? 1.0 / worst_ratio : INFINITY; }

// One trial of line_search_lewisoverton (lbfgs.hpp:307-383): f is the objective at the trial point xp + step d, dg() the
// directional derivative there (evaluated only when the decrease condition holds).  Returns the error that ends the search
// (0: none); otherwise `success` says whether the trial is accepted, and if it is not, `step` is the next one to try.
template <class Dg>
__device__ __forceinline__ int ls_trial(const LbfgsP &P, LineSearch &ls, const double f, double &step, bool &success, Dg &&dg) {
  ++ls.count;
  success = false;
  if (isinf(f) || isnan(f)) return LBERR_INVALID_FUNCVAL;
  if (f > ls.finit + step * ls.dgtest) {
    ls.nu = step;
    ls.brackt = 1;
  } else if (dg() < ls.dstest) {
    ls.mu = step;
  } else {
    success = true;
    return 0;
  }
  if (P.max_linesearch <= ls.count) return LBERR_MAXIMUMLINESEARCH;
  if (ls.brackt && (ls.nu - ls.mu) < P.machine_prec * ls.nu) return LBERR_WIDTHTOOSMALL;
  step = ls.brackt ? 0.5 * (ls.mu + ls.nu) : step * 2.0;
  if (step < P.min_step) return LBERR_MINIMUMSTEP;
  if (step > ls.smax) {
    if (ls.touched) return LBERR_MAXIMUMSTEP;
    ls.touched = 1;
    step = ls.smax;
  }
  return 0;
}

// Entry of a line search along a new direction, in the three pieces a form strings together around its own reductions:
//   ls.smax = P.max_step;  if (bounded) ls_bound_step(P, ls, step, proc_stepbound's value);
//   finish = ls_entry_check(step, g.d);  still running: ls_fresh(P, ls, fx, g.d), put the first trial point out
// lbfgs.hpp:557-565: step_max = min(proc_stepbound(xp, d), max_step); step = step < step_max ? step : step_max / 2
__device__ __forceinline__ void ls_bound_step(const LbfgsP &P, LineSearch &ls, double &step, const double bnd) {
  ls.smax = bnd < P.max_step ? bnd : P.max_step;
  step = step < ls.smax ? step : 0.5 * ls.smax;
}
// the two checks at the entry of line_search_lewisoverton (lbfgs.hpp:287-299): the code that stops the problem, 0x7fffffff to go on
__device__ __forceinline__ int ls_entry_check(const double step, const double dginit) {
  return !(step > 0.0) ? LBERR_INVALIDPARAMETERS : (0.0 < dginit ? LBERR_INCREASEGRADIENT : 0x7fffffff);
}
// the fresh state of a search that starts at cost fx with slope dginit (lbfgs.hpp:301-305)
__device__ __forceinline__ void ls_fresh(const LbfgsP &P, LineSearch &ls, const double fx, const double dginit) {
  ls.finit = fx;
  ls.dgtest = P.f_dec_coeff * dginit;
  ls.dstest = P.s_curv_coeff * dginit;
  ls.mu = 0.0;
  ls.nu = ls.smax;
  ls.count = 0;
  ls.brackt = 0;
  ls.touched = 0;
}

// The stopping tests of an accepted step in the reference's order (lbfgs.hpp:580-605): the progress report comes first
// after a line search (non-zero cancels), then g_epsilon, past / delta, max_iterations.  converged() is the g_epsilon test,
// pf_old(slot) the cost `past` iterations ago, pf_store(slot) keeps fx in its place.  Returns the code that stops the
// problem, 0x7fffffff while it runs.
template <class Conv, class PfOld, class PfStore>
__device__ __forceinline__ int stop_tests(const LbfgsP &P, const int cancel, const int k, const double fx, Conv &&converged,
                                          PfOld &&pf_old, PfStore &&pf_store) {
  if (cancel) return LB_CANCELED;
  if (converged()) return LB_CONVERGENCE;
  if (0 < P.past) {
    const int slot = k % P.past;
    if (P.past <= k) {
      const double rate = fabs(pf_old(slot) - fx) / fmax(1.0, fabs(fx));
      if (rate < P.delta) return LB_STOP;
    }
    pf_store(slot);
  }
  if (P.max_iterations != 0 && P.max_iterations <= k) return LBERR_MAXIMUMITERATION;
  return 0x7fffffff;
}

}  // namespace anet
