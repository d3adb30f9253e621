// The launch-shape overrides of the library: every environment switch that changes which kernel runs or how it is shaped, with
// its default and where that default comes from.  tuning() reads the environment once per process (both translation units call
// it); the two switches marked per call are read at every use (env_set), because tests flip them inside one process.  Each
// switch serves A-B runs and the tests that compare both sides; none is meant to be set in production.
// (Instrumentation -- -DANET_*_PROF builds, -DANET_IPM_TRACE, -DANET_IPM_CERT_TRACE -- is compile-time and not listed here, nor is
//  ANET_FUSED_PROF_PRINT, read only by a -DANET_FUSED_PROF build; ANET_RCCL_PATH is configuration: anet_comm_init.)
#pragma once
#include <stdint.h>
#include <stdlib.h>

namespace anet {

// A batch / pair / group-count threshold measured on the 256 compute units of an MI355X in SPX mode, for a device of `cus`
// compute units: at_256 * cus / 256 + plus -- a partitioned mode (CPX: 32 CUs per logical device) picks its shapes by rounds of
// workgroups per CU, not by literals.  A value the environment sets (>= 0) is taken as given, not scaled.
struct PerCu {
  int64_t at_256, plus;
  int64_t env;
  int64_t at(int cus) const { return env >= 0 ? env : at_256 * (int64_t)cus / 256 + plus; }
};

struct Tuning {
  // ---- coefficient solve / adjoint (minco_kernels.h)
  // ANET_AXIS_MAX_BATCH: lane per (trajectory, axis) solve / propagate, two lanes per (trajectory, piece) penalty up to this batch
  // (3 B / 63 waves still fill the chip's 1024 SIMDs about once)
  PerCu axis_max_batch{16384, 0, -1};
  // ANET_AXIS_TWO_MAX_BATCH: the exact shapes with an even piece count solve with two lanes per (trajectory, axis), the chain from
  // both ends, up to this batch; 0 disables (tools/time_solve_small.py)
  PerCu axis_two_max_batch{4096, 0, -1};
  // ---- penalty / energy gradient (launch_piece_grad)
  // ANET_PIECE_SW_MAX_PAIRS: the samples of a piece spread over a workgroup's four waves up to this many (trajectory, piece)
  // pairs (profiles/r05_cost_grad_small_batch.txt)
  PerCu piece_sw_max_pairs{16384, 0, -1};
  // ANET_PG_MX: 0 = k_piece_grad instead of k_piece_grad_mx at res = kMxRes (profiles/r06_piece_grad_mx.txt; tests compare both)
  int pg_mx = 1;
  // ANET_PGMX_DYNLDS: bytes of unused dynamic LDS per workgroup of k_piece_grad_mx, an occupancy probe (one workgroup per CU at
  // 61440: profiles/r06_piece_grad_mx.txt)
  int pgmx_dynlds = 0;
  // ---- the one-launch cost + gradient evaluation (minco_fused_kernel.h)
  // ANET_FUSED_MAX_GROUPS: one launch up to this many workgroups; 0 = always three launches.  Default (-1): 3 / 2 rounds of one
  // workgroup per CU for <= 8 / more pieces, 6 / 8 where phase 2 is MX (cost_grad_in_one_launch)
  int64_t fused_max_groups = -1;
  // ANET_FUSED_MX: 0 = the vector form of the one-launch kernel's phase 2 (fused_phase2_mx; tests compare both)
  int fused_mx = 1;
  // ---- the one-launch MINCO L-BFGS in two launches (lbfgs_minco_persistent.h; profiles/r04_lbfgs_two_launch.txt)
  // ANET_LBFGS_SPLIT_EVALS: evaluations of the first launch; 0 = one launch
  int lbfgs_split_evals = 1000;
  // ANET_LBFGS_SPLIT_MIN_BATCH: smallest batch that takes it (twice the resident waves)
  PerCu lbfgs_split_min_batch{4096, 0, -1};
  // ANET_LBFGS_SPLIT_MIN_VARS: fewest variables (ten pieces; shorter runs end before the split point tells the long ones)
  int lbfgs_split_min_vars = 36;
  // ---- the interior-point QP (qp_ipm.h)
  // ANET_IPM_TWIST_MIN_PIECES: chains of at least this many pieces are factored from both ends by two waves; a large value
  // restores the one-chain order (tests compare both)
  int ipm_twist_min_pieces = 2;
  // ANET_IPM_TWO_PER_CU_MIN_BATCH: the four-pass form with two workgroups per CU from this batch on, the FUSE form below it --
  // more than two rounds of one workgroup per CU (512 problems are a draw, 768 gain 15-20 %, 320 lose 15 %)
  PerCu ipm_two_per_cu_min_batch{512, 1, -1};
  // ANET_IPM_THREE_PER_CU_MIN_BATCH: jerk problems whose LDS allows it take three workgroups per CU from this batch on; 0
  // disables (round 5, 5 jerk pieces: 4096 problems 3.96-4.00 -> 3.77-3.85 ms, 2048: 2.09-2.12 -> 2.42-2.43)
  PerCu ipm_three_per_cu_min_batch{4096, 0, -1};
  // ANET_IPM_SPLIT_STEPS: Newton steps of the first of two launches; 0 = one launch (profiles/r04_qp_ipm_roofline.txt)
  int ipm_split_steps = 4;
  // ANET_IPM_SPLIT_MIN_BATCH: smallest batch that takes two launches (520..560 problems lose 7-10 %, 600..1280 gain 10-19 %)
  PerCu ipm_split_min_batch{576, 0, -1};
  // ---- vertex enumeration of polytopes (polytope_kernels.h)
  // ANET_POLYTOPE_VERTICES_WAVE_MIN_BATCH, ANET_POLYTOPE_VERTICES_WAVE_MAX_ROWS: one wave per polytope from this batch on when
  // max_rows is at most that many, else the workgroup's four waves per polytope.  Measured (one run): 131 072 x 16
  // rows 0.823 ms against 0.879, but 8 192 x 64 rows 8.95 ms against 8.11 (a wave's 6 KB kept list halves the residency there) and
  // one plan's 21 polytopes 0.452 against 0.320; 32 rows and 1024 polytopes (four per compute unit) lie between the measured points
  PerCu polytope_vertices_wave_min_batch{1024, 0, -1};
  int polytope_vertices_wave_max_rows = 32;

  // ---- per call (env_set at every use: tests set and unset them inside one process)
  // ANET_MVIE_STATE_IN_MEMORY: the MVIE L-BFGS with its state in memory (k_lbfgs_mvie_persistent), not in registers
  static constexpr const char *mvie_state_in_memory = "ANET_MVIE_STATE_IN_MEMORY";
  // ANET_POLYTOPE_DEPTH_ENUMERATE: polytope depths by vertex enumeration only, without the certified ascent in front
  static constexpr const char *polytope_depth_enumerate = "ANET_POLYTOPE_DEPTH_ENUMERATE";
  // ANET_POLYTOPE_VERTICES_WPP: 1 or 4 waves per polytope in k_polytope_vertices whatever the batch (the results are the same bits)
  static constexpr const char *polytope_vertices_wpp = "ANET_POLYTOPE_VERTICES_WPP";
  // ANET_OCC_MARKS_ATOMIC: the marks of a scan in one launch of atomicOr on flag bits (k_occ_mark_atomic), not the two launches of
  // plain byte stores (the grids are the same bits; DESIGN.md 8t has both timings)
  static constexpr const char *occ_marks_atomic = "ANET_OCC_MARKS_ATOMIC";
};

// a per-call switch: set (to anything) or not
inline bool env_set(const char *name) { return getenv(name) != nullptr; }

inline void env_override(const char *name, int &field) {
  if (const char *e = getenv(name)) field = atoi(e);
}
inline void env_override(const char *name, int64_t &field) {
  if (const char *e = getenv(name)) field = (int64_t)atoll(e);
}

// the table with the environment's overrides, read on the first call
inline const Tuning &tuning() {
  static const Tuning t = [] {
    Tuning v;
    env_override("ANET_AXIS_MAX_BATCH", v.axis_max_batch.env);
    env_override("ANET_AXIS_TWO_MAX_BATCH", v.axis_two_max_batch.env);
    env_override("ANET_PIECE_SW_MAX_PAIRS", v.piece_sw_max_pairs.env);
    env_override("ANET_PG_MX", v.pg_mx);
    env_override("ANET_PGMX_DYNLDS", v.pgmx_dynlds);
    env_override("ANET_FUSED_MAX_GROUPS", v.fused_max_groups);
    env_override("ANET_FUSED_MX", v.fused_mx);
    env_override("ANET_LBFGS_SPLIT_EVALS", v.lbfgs_split_evals);
    env_override("ANET_LBFGS_SPLIT_MIN_BATCH", v.lbfgs_split_min_batch.env);
    env_override("ANET_LBFGS_SPLIT_MIN_VARS", v.lbfgs_split_min_vars);
    env_override("ANET_IPM_TWIST_MIN_PIECES", v.ipm_twist_min_pieces);
    env_override("ANET_IPM_TWO_PER_CU_MIN_BATCH", v.ipm_two_per_cu_min_batch.env);
    env_override("ANET_IPM_THREE_PER_CU_MIN_BATCH", v.ipm_three_per_cu_min_batch.env);
    env_override("ANET_IPM_SPLIT_STEPS", v.ipm_split_steps);
    env_override("ANET_IPM_SPLIT_MIN_BATCH", v.ipm_split_min_batch.env);
    env_override("ANET_POLYTOPE_VERTICES_WAVE_MIN_BATCH", v.polytope_vertices_wave_min_batch.env);
    env_override("ANET_POLYTOPE_VERTICES_WAVE_MAX_ROWS", v.polytope_vertices_wave_max_rows);
    return v;
  }();
  return t;
}

}  // namespace anet
