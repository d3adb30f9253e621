/*
 * allocnet_amd -- C ABI of the MI355X-native batched MINCO / min-jerk / min-snap trajectory
 * solver.  Plain C: opaque handle, POD arrays, no C++ or torch types cross this line.
 *
 * What each entry point replaces in the reference (KumarRobotics/AllocNet, paths relative to
 * the reference root) is cited per function.  `minco.hpp` itself is NOT part of the reference
 * tree; the MINCO entry points follow the upstream GCOPTER method names
 * the north star asks for (setConditions / setParameters / getEnergy / getCoeffs /
 * getEnergyPartialGradBy{Coeffs,Times} / propogateGrad).
 *
 * Conventions (the reference's own):
 *   - s      : order, 3 = min-jerk (degree 5), 4 = min-snap (degree 7); 2 = min-acc also works.
 *   - D      : 2*s coefficients per axis per piece, HIGHEST POWER FIRST
 *              (src/planner/include/gcopter/trajectory.hpp:75-133).
 *   - coeffs : piece-major, then axis x,y,z, then the D coefficients
 *              (src/planner/include/planner/learning_planner.hpp:212,227).
 *   - head/tail : 3 x c, row = axis, columns p,v,a[,j] (src/planner/src/learning_planning.cpp:150-151);
 *              c = number of boundary derivatives fixed per end: 3 = reference convention
 *              (qp_solver.hpp:37,152-158; for snap the end jerk is then free -> natural
 *              condition p''''=0), c = s = classic MINCO convention.
 *   - wps    : interior waypoints, (N-1) x 3 (waypoint-major, like GCOPTER's 3 x (N-1)
 *              column-major inPs).
 *   - energy : int (p^(s))^2 dt summed over axes (MINCO getEnergy convention, no 1/2);
 *              the reference's Trajectory::getTrajCost convention (1/2, m_34=1400) is
 *              available through anet_traj_cost*.
 *
 * Two families of entry points:
 *   *_dev : pointers are DEVICE pointers in the batch-minor layout: value f of trajectory b
 *           lives at ptr[f*ld + b] (f = the flattened per-trajectory index in the order given
 *           above, ld >= batch).  Asynchronous on `stream` (a hipStream_t, NULL = default).
 *   plain : pointers are HOST pointers, trajectory-major (each trajectory's values contiguous,
 *           exactly the reference's flattening).  Synchronous.
 *
 * All functions return ANET_OK (0) or a negative error code; anet_last_error() gives text.
 * One context per host thread per device; a context is not re-entrant: in particular ONE L-BFGS call in flight per
 * context (its completion flag lives in the context), whatever the streams (same as the
 * reference's QPSolver, qp_solver.hpp:43-45).
 */
#ifndef ALLOCNET_AMD_H
#define ALLOCNET_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANET_ABI_VERSION 2 /* 2: QP default method = interior point, QP max-iter status -2 (OSQP), FIRI ok = 2, new entry points */

enum {
  ANET_OK = 0,
  ANET_ERR_INVALID = -1,     /* bad argument (order, piece count, batch, NULL pointer ...) */
  ANET_ERR_HIP = -2,         /* a HIP runtime call failed; text in anet_last_error()       */
  ANET_ERR_UNSUPPORTED = -3, /* valid request this build has no kernel for                 */
  ANET_ERR_NOMEM = -4,
  ANET_ERR_NODEVICE = -5     /* no usable gfx950 device: the product path has NO CPU fallback */
};

#define ANET_MAX_PIECES 16   /* register-resident kernels are instantiated for N <= 16      */
#define ANET_MAX_POLY_ROWS 50 /* learning_planner.hpp:40 (eigen_stacked_hpolys 4*50)        */

typedef struct anet_ctx anet_ctx;

int anet_abi_version(void);
int anet_device_count(void);
int anet_create(int device, anet_ctx **out);
void anet_destroy(anet_ctx *ctx);
const char *anet_last_error(const anet_ctx *ctx);
/* Compute units of the context's device (hipDeviceAttributeMultiprocessorCount, read once by anet_create: 256 on an
 * MI355X in SPX mode, 32 per logical device in CPX).  Every launch-shape threshold of the library -- lane per trajectory or
 * per (trajectory, axis), one launch or three per cost + gradient evaluation, workgroups per CU of the QP, one or two
 * launches of the batched optimisers -- is a number of rounds of workgroups per compute unit and scales with it.           */
int anet_compute_units(const anet_ctx *ctx);
/* hipStream_t the plain (host) entry points run on. */
void *anet_stream(anet_ctx *ctx);
int anet_synchronize(anet_ctx *ctx);

/* ---- device buffers for callers that do not link the HIP runtime themselves ---------------- */
int anet_dev_alloc(anet_ctx *ctx, size_t n_doubles, double **out);
void anet_dev_free(double *p);
int anet_dev_upload(anet_ctx *ctx, double *dst_dev, const double *src_host, size_t n_doubles);   /* synchronous */
int anet_dev_download(anet_ctx *ctx, double *dst_host, const double *src_dev, size_t n_doubles); /* synchronous */

/* Recommended row stride for `batch` trajectories in the batch-minor layout: a multiple of 64 that
 * is >= batch and NOT a multiple of 4 KiB worth of doubles.  A power-of-two row stride puts the same
 * column of every field on the same HBM channel/bank; measured on MI355X the 8-segment solve runs
 * 59 % of the HBM roofline at ld = 2^20 and 63-65 % at ld = 2^20 + 576.      */
int64_t anet_recommended_ld(int64_t batch);

/* ---- layout helpers: trajectory-major host/device <-> batch-minor device ---------------- */
/* dst[f*ld + b] = src[b*nfield + f]  (both device pointers). */
int anet_to_batch_minor_dev(anet_ctx *ctx, int64_t batch, int64_t nfield, int64_t ld,
                            const double *src, double *dst, void *stream);
/* dst[b*nfield + f] = src[f*ld + b]. */
int anet_to_traj_major_dev(anet_ctx *ctx, int64_t batch, int64_t nfield, int64_t ld,
                           const double *src, double *dst, void *stream);

/* ---- MINCO coefficient solve + energy --------------------------------------------------- */
/* Replaces (north star; upstream GCOPTER minco.hpp, absent from the reference tree):
 *   MINCO_S{2,3,4}NU::setConditions(head,tail,N) + setParameters(inPs,ts) + getCoeffs +
 *   getEnergy, batched.  Fixed waypoints and durations; minimises int (p^(s))^2.
 * coeffs may be NULL (energy only); energy may be NULL.                                      */
int anet_minco_solve_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                         const double *head,  /* [3*c][ld]        */
                         const double *tail,  /* [3*c][ld]        */
                         const double *wps,   /* [(N-1)*3][ld]    (ignored when N == 1) */
                         const double *T,     /* [N][ld]          */
                         double *coeffs,      /* [N*3*2s][ld]     */
                         double *energy,      /* [batch]          */
                         void *stream);
/* Trajectories whose durations spread widely (max T / min T > min_spread; <= 1 selects all) solved again by the classic
 * formulation -- one 2sN x 2sN banded collocation system, LU with partial pivoting -- and their coeffs / energy
 * overwritten; the others are left as they are.  The fast kernel solves a reduced system whose conditioning is the
 * square of this one's: accurate to 1e-8 up to a spread of 100, 5e-4 at 10^3 (snap).  The host entry point
 * anet_minco_solve applies this by itself above a spread of 50; device callers call it when their durations can spread
 * (about 10^3 times slower per trajectory that is redone).                                                    */
int anet_minco_solve_wide_spread_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                                     const double *head, const double *tail, const double *wps, const double *T,
                                     double min_spread, double *coeffs, double *energy, void *stream);
/* flags[b] (device int32 [batch]) = 1 where the durations of trajectory b spread over more than min_spread (max T >
 * min_spread * min T; min_spread <= 0 selects the library's own threshold of 50), 0 elsewhere: which trajectories the
 * call above redoes, and which results of anet_lbfgs_minco[_dev] had their returned coefficients re-solved that way. */
int anet_minco_spread_flags_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, const double *T /* [N][ld] */,
                                double min_spread, int32_t *flags, void *stream);

/* Time-allocation sampling (north star: "batch of candidate trajectories / time-allocation samples"): MANY candidate
 * duration vectors for FEW problems in ONE launch.  A sampler does not have 1024 different problems -- the literal
 * BASELINE configs[1] batch, launch-bound at 2 MB per launch -- it has one problem (boundary states, waypoints) and K
 * candidate duration vectors.  Sample b (0 <= b < problems * samples_per_problem) belongs to problem b / samples_per_problem;
 * head / tail / wps are per PROBLEM (batch-minor with row stride ldp >= problems), T per SAMPLE (row stride ld); the only
 * output is cost[b] = int (p^(s))^2 + rho * sum T (rho = 0: the energy of MINCO_S*NU::getEnergy), 8 (N + 1) bytes of
 * traffic per sample instead of the 1920 of a full solve.  No counterpart in the reference (it solves one trajectory per
 * call, learning_planner.hpp:196); upstream's use is a loop over setParameters / getEnergy.
 * ACCURACY ENVELOPE: the costs come from the reduced (block-tridiagonal) system only -- there is no pivoted re-solve
 * here as anet_minco_solve_wide_spread_dev / anet_lbfgs_minco apply above a spread of 50.  Relative error of the energy:
 * <= 1e-8 while max T / min T of a sample stays below ~100, degrading beyond it (order 1e-4 at 10^3 for snap).  A sampler
 * that draws wider spreads should flag those samples with anet_minco_spread_flags_dev (same T layout) and re-evaluate
 * them with anet_minco_solve_wide_spread_dev.                                                                        */
int anet_minco_sample_costs_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t problems, int64_t samples_per_problem,
                                int64_t ld, int64_t ldp, const double *head /* [3c][ldp] */, const double *tail,
                                const double *wps /* [(N-1)*3][ldp] */, const double *T /* [N][ld] */, double rho,
                                double *cost /* [problems * samples_per_problem] */, void *stream);
/* Host variant for ONE problem: head / tail [3][c], wps [N-1][3], T [samples][N] (trajectory-major), cost [samples]. */
int anet_minco_sample_costs(anet_ctx *ctx, int s, int c, int n_pieces, int64_t samples, const double *head,
                            const double *tail, const double *wps, const double *T, double rho, double *cost);
int anet_minco_solve(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch,
                     const double *head,  /* [batch][3][c]     */
                     const double *tail,  /* [batch][3][c]     */
                     const double *wps,   /* [batch][N-1][3]   */
                     const double *T,     /* [batch][N]        */
                     double *coeffs,      /* [batch][N][3][2s] */
                     double *energy);     /* [batch]           */

/* ---- Trajectory<D> evaluation --------------------------------------------------------- */
/* Replaces Trajectory<D>::getPos/getVel/getAcc/getJer (gcopter/trajectory.hpp:516-538) =
 * locatePieceIdx (:496-514, including its clamp to the last piece for t beyond the total
 * duration) + Piece<D>::getPos/getVel/getAcc/getJer (:75-133), and network/utils/trajectory.py
 * get_pos/get_vel/get_acc (:47-98), batched: nq query times per trajectory.
 * deriv: 0 position, 1 velocity, 2 acceleration, 3 jerk.                                      */
int anet_traj_eval_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld,
                       const double *coeffs, /* [N*3*2s][ld] */
                       const double *T,      /* [N][ld]      */
                       int nq, const double *tq, /* [nq][ld] absolute times from trajectory start */
                       int deriv, double *out,   /* [nq*3][ld]  (query-major, then axis) */
                       void *stream);
int anet_traj_eval(anet_ctx *ctx, int s, int n_pieces, int64_t batch,
                   const double *coeffs, /* [batch][N][3][2s] */
                   const double *T,      /* [batch][N]        */
                   int nq, const double *tq, /* [batch][nq]   */
                   int deriv, double *out);  /* [batch][nq][3] */

/* Replaces Trajectory<D>::getTrajCost(order) (gcopter/trajectory.hpp:354-427):
 * sum over pieces and axes of 1/2 z' Q_s(T) z on the s highest coefficients.  m34 is the (3,4)
 * entry constant of the snap block: 1400.0 reproduces the reference (qp_solver.hpp:212,
 * trajectory.hpp:385, min_traj_opt.py:493), 1440.0 is the true integral.  Ignored for s != 4. */
int anet_traj_cost_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld,
                       const double *coeffs, const double *T, double m34, double *cost /* [batch] */,
                       void *stream);
int anet_traj_cost(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs,
                   const double *T, double m34, double *cost);
/* d(getTrajCost)/dT_i with the coefficients held fixed: 1/2 z_i' (dQ_s/dT)(T_i) z_i summed over axes.
 * This is the time-allocation gradient the reference's training actually back-propagates: in
 * OsqpLayer the QP solution is a detached leaf (network/utils/learning/layers.py:121,222), so the loss
 * 1/2 z'Q(T)z / path_length (:143-147, :245) reaches the segment times only through Q(T); the KKT hook
 * (:136-141, :238-243) rewrites the gradient of that leaf and never reaches the network.
 * gradT: [N][ld] (dev) / [batch][N] (host).                                                        */
int anet_traj_cost_grad_T_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld,
                              const double *coeffs, const double *T, double m34, double *gradT, void *stream);
int anet_traj_cost_grad_T(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs,
                          const double *T, double m34, double *gradT);

/* Replaces Piece<D>::getMaxVelRate / getMaxAccRate (gcopter/trajectory.hpp:177-273; root isolation in
 * gcopter/root_finder.hpp) batched: the maximum of ||v|| (which = 1) or ||a|| (which = 2) over every piece.
 * Trajectory<D>::getMaxVelRate/getMaxAccRate (:576-604) is the maximum over the pieces, and
 * checkMaxVelRate/checkMaxAccRate(bound) (:275-314, 606-630) is "max < bound" (both ends and interior).
 * rate: [N][ld] (dev) / [batch][N] (host).                                                          */
int anet_traj_max_rate_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld,
                           const double *coeffs, const double *T, int which, double *rate, void *stream);
int anet_traj_max_rate(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs,
                       const double *T, int which, double *rate);

/* Exact margin of every piece against linear rows a.x <= b (no counterpart in the reference, whose solvers hold these rows at
 * sample points only): for deriv d in {0, 1, 2}
 *     margin[i] = max over the non-padding rows r of piece i, max over t in [0, T_i], of  a_r . p_i^(d)(t) - b_r
 * positive: the deepest excursion out of the polytope; negative: the clearance kept; -inf: the piece has no row; NaN: a NaN or
 * infinite coefficient, duration or row field of that piece.  With d = 0 and corridor rows this is the corridor margin; with
 * d = 1, 2 and the six rows +-e_axis, b = MaxVelBox / MaxAccBox it is the margin of the box rows of QPSolver::solve
 * (planner/qp_solver.hpp:244-296).  rows: [N*M*4][ld] in the layout of `hpolys` below (dev) / [batch][N][M][4] (host), all-zero
 * rows are padding, 1 <= M = poly_rows <= ANET_MAX_POLY_ROWS.  margin, t: double [N][ld] (dev) / [batch][N] (host); row: int32, the
 * same shapes.  row (a maximising row, -1 without one) and t (its local time in [0, T_i], 0 without one) may be NULL; they are
 * diagnostics: a_row . p^(d)(t) - b_row reproduces margin.  Accuracy: 32 eps (sum_ax |a_ax| sum_k |u_ax,k| + |b|), u the
 * coefficients of p^(d) in normalised time (csrc/corridor_margin_kernels.h). */
int anet_traj_row_margin_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                             int deriv, int poly_rows, const double *rows, double *margin, int32_t *row, double *t, void *stream);
int anet_traj_row_margin(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs, const double *T, int deriv,
                         int poly_rows, const double *rows, double *margin, int32_t *row, double *t);

/* Replaces Piece<D>::normalizePosCoeffMat / normalizeVelCoeffMat / normalizeAccCoeffMat (gcopter/trajectory.hpp:135-171) for a
 * batch of independent pieces: the coefficients of the position (deriv = 0), velocity (1) or acceleration (2) polynomial of each
 * piece in normalised time tau = t / duration, highest power first: column i = (falling factorial of its power) * coeffMat.col(i) *
 * duration^power.  coeffs [pieces][3][2s], T [pieces], out [pieces][3][2s - deriv]; HOST pointers (the _dev variant: device
 * pointers, the same piece-major layout, asynchronous on `stream`). */
int anet_piece_normalized_coeffs(anet_ctx *ctx, int s, int64_t pieces, const double *coeffs, const double *T, int deriv,
                                 double *out);
int anet_piece_normalized_coeffs_dev(anet_ctx *ctx, int s, int64_t pieces, const double *coeffs, const double *T, int deriv,
                                     double *out, void *stream);

/* ---- cost + analytic gradients ----------------------------------------------------------- */
/* Penalty functional on the reference's own inequality rows (QPSolver::solve step three,
 * planner/qp_solver.hpp:244-296; MinTrajOpt.fill_ineq, network/utils/min_traj_opt.py:535-613):
 * for piece i and sample j in [0,res) at t = j*T_i/res
 *     corridor rows   a_r . p(t) - b_r            (hPolys[i] rows, a.x <= b form)
 *     box rows        +-v_axis(t) - max_vel,  +-a_axis(t) - max_acc     (per axis)
 * the reference imposes them as hard constraints of a QP; here each row g enters the cost as
 *     J_pen = sum_i (T_i/res) sum_j sum_rows w_row * smoothedL1(smooth_mu, g)
 * with firi::smoothedL1 (gcopter/firi.hpp:60-84), the MINCO/GCOPTER penalty-functional form the
 * north star asks for.  Total cost: J = int (p^(s))^2 + rho*sum(T) + J_pen.                    */
typedef struct anet_penalty {
  double rho;        /* weight of sum(T)                                               */
  double w_corridor; /* weight of corridor rows                                        */
  double w_vel;      /* weight of velocity box rows                                    */
  double w_acc;      /* weight of acceleration box rows                                */
  double smooth_mu;  /* smoothedL1 mu, > 0                                             */
  double max_vel;    /* MaxVelBox (config/planner.yaml:17)                             */
  double max_acc;    /* MaxAccBox (config/planner.yaml:19)                             */
  int32_t res;       /* ConstRes, samples per piece (config/planner.yaml:21)           */
  int32_t poly_rows; /* M: rows per polytope in `hpolys`; all-zero rows are padding    */
} anet_penalty;

/* Partial gradients of  [with_energy] int (p^(s))^2  +  [pen != NULL] J_pen  with respect to the
 * coefficients and durations, the coefficients being treated as independent variables
 * (MINCO getEnergyPartialGradByCoeffs / getEnergyPartialGradByTimes + the penalty functional).
 * hpolys: [N*M*4][ld], row r of polytope i at fields (i*M + r)*4 + {0,1,2,3} = a_x,a_y,a_z,b;
 * may be NULL (box rows only).  piece_cost (may be NULL): per-piece J_pen share, [N][ld].      */
int anet_minco_partial_grads_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld,
                                 const double *coeffs, const double *T, const double *hpolys,
                                 const anet_penalty *pen, int with_energy,
                                 double *gdC,        /* [N*3*2s][ld] */
                                 double *gdT,        /* [N][ld]      */
                                 double *piece_cost, /* [N][ld]      */
                                 void *stream);

/* MINCO propogateGrad: total gradient of a scalar J(c(wps,T), T) w.r.t. the interior waypoints and
 * the durations from its partial gradients gdC, gdT; coeffs must be the MINCO coefficients for
 * (c, wps, T).  gradP: [(N-1)*3][ld] (waypoint-major, like wps), gradT: [N][ld].               */
int anet_minco_propagate_grad_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                                  const double *T, const double *coeffs, const double *gdC,
                                  const double *gdT, double *gradP, double *gradT, void *stream);

/* Whole objective in one call: solve -> partial gradients -> propagate.
 * work: device scratch of anet_minco_cost_grad_workspace(s, N, ld) doubles.
 * coeffs_out may be NULL.  cost: [batch].                                                     */
int64_t anet_minco_cost_grad_workspace(int s, int n_pieces, int64_t ld);
/* Kernel launches anet_minco_cost_grad_dev makes for this shape (order s, boundary count c) on this context's device: 1
 * (k_minco_cost_grad_fused: batches of up to three rounds of one workgroup per compute unit, orders 3 and 4, res <= 64 -- six /
 * eight rounds for 8-piece snap / 16-piece jerk with c = 3 at res = 20, whose phase 2 runs on the FP64 matrix instructions) or 3
 * (k_minco_solve -> k_piece_grad[_mx] -> k_minco_propagate); negative = error.  For callers that label a measurement with the
 * kernel that ran (bench.py).                                                                                                  */
int anet_minco_cost_grad_launches(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const anet_penalty *pen);
/* The launch shape anet_minco_partial_grads_dev picks for this shape on this context's device: 0 one lane per (trajectory,
 * piece) (k_piece_grad, large batches); 1 two lanes per pair; 2 two lanes and the samples over a workgroup's four waves (the small
 * batches); 3 k_piece_grad_mx -- four lanes per pair, the contractions with the basis table on the FP64 matrix instructions
 * (large batches, orders 3 and 4, res = 20: the penalty functional of qp_solver.hpp:244-296's rows at planner.yaml:21's sampling);
 * negative = error.  For callers that label a measurement with the kernel that ran (bench.py).                                */
int anet_minco_piece_grad_shape(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const anet_penalty *pen);
int anet_minco_cost_grad_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                             const double *head, const double *tail, const double *wps,
                             const double *T, const double *hpolys, const anet_penalty *pen,
                             double *work, double *cost, double *gradP, double *gradT,
                             double *coeffs_out, void *stream);
int anet_minco_cost_grad(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch,
                         const double *head, const double *tail, const double *wps, const double *T,
                         const double *hpolys, /* [batch][N][M][4] or NULL */
                         const anet_penalty *pen, double *cost, /* [batch] */
                         double *gradP,  /* [batch][N-1][3] */
                         double *gradT,  /* [batch][N]      */
                         double *coeffs_out /* [batch][N][3][2s] or NULL */);

/* ---- differential flatness: states, limits, penalty gradients ------------------------------ */
/* Replaces flatness::FlatnessMap (gcopter/flatness.hpp:37-260): reset's six parameters, forward (:54-134) from velocity,
 * acceleration, jerk, yaw and yaw rate to thrust, attitude quaternion (w, x, y, z) and body rate, and backward (:136-260), the
 * adjoint of that map.  With w = (1 + cp sqrt(|v|^2 + eps)) v,  zu = a + (dh/m) w + g e3,  z = zu / |zu|:
 *   thr = z . (m a + dv w + m g e3),  quat = tilt(z) * yaw(psi),  omg = body rate of (z, dz/dt, psi, dpsi).
 * The adjoint is derived from this forward and pinned by automatic differentiation and finite differences.
 * Singular only at z = -e3 (inverted thrust direction), as the reference.                                                   */
typedef struct anet_flat_params {
  double mass;       /* vehicle mass, > 0                       (reset: vehicle_mass)               */
  double grav;       /* gravitational acceleration              (gravitational_acceleration)        */
  double horiz_drag; /* dh                                      (horitonral_drag_coeff)             */
  double vert_drag;  /* dv                                      (vertical_drag_coeff)               */
  double paras_drag; /* cp                                      (parasitic_drag_coeff)              */
  double speed_eps;  /* eps under the square root of the speed, > 0 (speed_smooth_factor)           */
} anet_flat_params;

/* Pointwise, one element per lane.  vel, acc, jer: [3][ld]; psi, dpsi: [ld] or NULL (NULL = 0; both NULL: no trigonometry, the
 * call process() makes, learning_planning.cpp:243).  thr [ld], quat [4][ld] (w, x, y, z), omg [3][ld].                      */
int anet_flat_forward_dev(anet_ctx *ctx, const anet_flat_params *params, int64_t batch, int64_t ld, const double *vel,
                          const double *acc, const double *jer, const double *psi, const double *dpsi, double *thr, double *quat,
                          double *omg, void *stream);
/* Host variant: vel, acc, jer [batch][3]; psi, dpsi [batch] or NULL; thr [batch], quat [batch][4], omg [batch][3]. */
int anet_flat_forward(anet_ctx *ctx, const anet_flat_params *params, int64_t batch, const double *vel, const double *acc,
                      const double *jer, const double *psi, const double *dpsi, double *thr, double *quat, double *omg);
/* FlatnessMap::backward at the given inputs (stateless: the forward intermediates are recomputed).  Upstream gradients
 * thr_grad [ld], quat_grad [4][ld], omg_grad [3][ld]; pos_grad, vel_grad [3][ld] pass through additively (either may be NULL = 0).
 * Totals: vel_total, acc_total, jer_total [3][ld]; pos_total [3][ld], psi_total, dpsi_total [ld] may be NULL (not written).  */
int anet_flat_backward_dev(anet_ctx *ctx, const anet_flat_params *params, int64_t batch, int64_t ld, const double *vel,
                           const double *acc, const double *jer, const double *psi, const double *dpsi, const double *pos_grad,
                           const double *vel_grad, const double *thr_grad, const double *quat_grad, const double *omg_grad,
                           double *pos_total, double *vel_total, double *acc_total, double *jer_total, double *psi_total,
                           double *dpsi_total, void *stream);
/* Host variant, element-major as anet_flat_forward. */
int anet_flat_backward(anet_ctx *ctx, const anet_flat_params *params, int64_t batch, const double *vel, const double *acc,
                       const double *jer, const double *psi, const double *dpsi, const double *pos_grad, const double *vel_grad,
                       const double *thr_grad, const double *quat_grad, const double *omg_grad, double *pos_total,
                       double *vel_total, double *acc_total, double *jer_total, double *psi_total, double *dpsi_total);

/* Along trajectories (psi = dpsi = 0, as in the reference): the piece location of anet_traj_eval, then velocity, acceleration and
 * jerk at each query and the forward map.  Per query 11 fields: thr, q0..q3, omg0..2, speed = |v|, the tilt angle (acos(1 - 2 (q1^2 + q2^2)),
 * computed as 2 atan2(sqrt(q1^2 + q2^2), sqrt(q0^2 + q3^2)), which keeps small tilts), bdr = |omg| -- the last three and thr are what process() publishes (learning_planning.cpp:249-251).
 * out: [nq*11][ld] (dev, query-major then field) / [batch][nq][11] (host).                                                    */
#define ANET_FLAT_STATE_FIELDS 11
int anet_traj_flat_states_dev(anet_ctx *ctx, const anet_flat_params *params, int s, int n_pieces, int64_t batch, int64_t ld,
                              const double *coeffs, const double *T, int nq, const double *tq, double *out, void *stream);
int anet_traj_flat_states(anet_ctx *ctx, const anet_flat_params *params, int s, int n_pieces, int64_t batch, const double *coeffs,
                          const double *T, int nq, const double *tq, double *out);
/* Minimum thrust, maximum thrust, maximum tilt and maximum body-rate magnitude of each trajectory over the samples
 * t = j T_i / res, j = 0..res, of every piece (both ends included).  A SAMPLED check: the flat outputs are not polynomials in t, so
 * unlike anet_traj_max_rate nothing bounds them between the samples.  out: [4][ld] (dev) / [batch][4] (host).               */
int anet_traj_flat_extrema_dev(anet_ctx *ctx, const anet_flat_params *params, int s, int n_pieces, int64_t batch, int64_t ld,
                               const double *coeffs, const double *T, int res, double *out, void *stream);
int anet_traj_flat_extrema(anet_ctx *ctx, const anet_flat_params *params, int s, int n_pieces, int64_t batch, const double *coeffs,
                           const double *T, int res, double *out);

/* Thrust, tilt and body-rate limits as a penalty of the MINCO objective, with the quadrature and the smoothedL1 of J_pen:
 *   J_flat = sum_i (T_i/res) sum_{j<res} [ w_thrust (phi(thr - max_thrust) + phi(min_thrust - thr))
 *                                        + w_tilt phi(cos(max_tilt) - cos(tilt)) + w_bdr phi(|omg|^2 - max_bdr^2) ]
 * at t = j T_i / res with psi = dpsi = 0;  cos(tilt) = 1 - 2 (q1^2 + q2^2).                                                  */
typedef struct anet_flat_penalty {
  double w_thrust, w_tilt, w_bdr;
  double smooth_mu;  /* smoothedL1 mu, > 0 (in the units of each row: thrust, cosine, squared rate) */
  double min_thrust, max_thrust; /* min_thrust < max_thrust                                        */
  double max_tilt;   /* radians, in (0, pi)                                                        */
  double max_bdr;    /* body-rate magnitude                                                        */
  int32_t res;       /* samples per piece, >= 1                                                    */
} anet_flat_penalty;
/* Partial gradients of J_flat w.r.t. the coefficients and durations, in the layout of anet_minco_partial_grads_dev; orders 3 and
 * 4 (ANET_ERR_UNSUPPORTED otherwise).  accumulate = 0: gdC, gdT, piece_cost are written; != 0: J_flat's share is ADDED to them, so
 * that energy, corridor, box and flatness terms go through one anet_minco_propagate_grad_dev.  piece_cost may be NULL.       */
int anet_minco_flat_partial_grads_dev(anet_ctx *ctx, const anet_flat_params *params, const anet_flat_penalty *pen, int s,
                                      int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                                      int accumulate, double *gdC, double *gdT, double *piece_cost, void *stream);

/* ---- QP assembly (the reference's own formulation) ----------------------------------------- */
/* Replaces the assembly part of QPSolver::solve (planner/qp_solver.hpp:61-296: setOrder/zero_A_,
 * get_t_state, equality rows :139-177, objective :180-242, inequality rows :244-296) and its Python
 * twin MinTrajOpt.fill_eq_obj / fill_ineq (network/utils/min_traj_opt.py:300-697), batched.
 * Dense, trajectory-major outputs with the reference's shapes:
 *   n = 3*2s*N variables, m_e = 3*(6 + s*(N-1)) equalities, m_g = res*(sum_i rows_i + 12*N) inequalities
 *   Q [n][n], A [m_e][n], b [m_e], G [m_g][n], h [m_g]      (row-major, one set per trajectory)
 * row_order:  ANET_QP_ORDER_CPP    per piece, per sample: the polytope rows, then 12 box rows
 *                                  (qp_solver.hpp:258-294)
 *             ANET_QP_ORDER_PYTHON all corridor rows (G1,h1) first, then all box rows (G2,h2)
 *                                  (min_traj_opt.py:535-613; OsqpLayer stacks them, layers.py:66-70)
 * float_time != 0 reproduces the C++ planner's arithmetic: segment times arrive as float32 and the
 * time powers of the basis rows and of the cost block are formed in float (qp_solver.hpp:90-116 with
 * T = float, :183-236, :252-263); 0 = float64 throughout (the Python twin).
 * m34: (3,4) entry constant of the snap cost block, 1400.0 = reference, 1440.0 = true integral.
 * state: ini/fin PVA, [batch][2][3][3] = {ini,fin} x axis x (p,v,a) (learning_planning.cpp:150-151).
 * hpolys [batch][N][M][4] rows (a_x,a_y,a_z,b) meaning a.x <= b; rows[batch][N] = valid rows per
 * polytope (<= M).  All pointers are DEVICE pointers in the _dev variant.                        */
#define ANET_QP_ORDER_CPP 0
#define ANET_QP_ORDER_PYTHON 1
typedef struct anet_qp_dims { int64_t n, m_e, m_g; } anet_qp_dims;
/* Sizes for ONE trajectory given its polytope row counts (host array rows[N]). */
int anet_qp_dims_of(int s, int n_pieces, int res, const int32_t *rows, anet_qp_dims *out);
/* Every trajectory of a batch must have the same sum of polytope rows (so the dense outputs have one
 * shape); pad polytopes with all-zero rows (0.x <= 0, inert) to equalise, as the reference's own
 * tensor packing does (learning_planner.hpp:157-166, 50 x 4 x 5 zero-padded).                     */
int anet_qp_assemble_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M,
                         double max_vel, double max_acc, double m34, int float_time, int row_order,
                         const double *state, const double *T, const double *hpolys, const int32_t *rows,
                         double *Q, double *A, double *b, double *G, double *h, void *stream);
int anet_qp_assemble(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                     double max_acc, double m34, int float_time, int row_order, const double *state,
                     const double *T, const double *hpolys, const int32_t *rows, double *Q, double *A,
                     double *b, double *G, double *h);

/* ---- inequality-constrained QP solve (replaces OSQP) ------------------------------------- */
/* Replaces the solver part of QPSolver::solve (planner/qp_solver.hpp:299-358: OsqpEigen data/settings,
 * initSolver, solveProblem, getObjValue, getStatus, getSolution) and OsqpLayer's forward solve
 * (network/utils/learning/layers.py:66-81,167-181), batched: the SAME QP the reference assembles
 *      min 1/2 z'Qz   s.t.  A z = b,   G z <= h                      (anet_qp_assemble gives it densely)
 * OSQP itself is a third-party dependency absent from the reference tree: its iterates are not comparable, the
 * solution is (same convex problem) -- parity is checked through the KKT conditions.  Two methods:
 *   INTERIOR_POINT (default): the optimum to 1e-6 in 10-20 Newton steps.  On random corridor problems it returns
 *       `Solved` for every problem either method can solve (profiles/r02_qp_unsolved.json);
 *   ADMM: OSQP's own iteration (Stellato et al. 2020, Algorithm 1) with OSQP's default settings (below), its modified Ruiz
 *       equilibration (`scaling` = 10 passes on the reference's own matrices, cost scaling included), its stopping rule on the
 *       UNSCALED residuals and its rho estimate from the scaled ones.  At max_iter = 4000 it leaves 1-6 % of feasible 5- and
 *       8-piece snap problems unsolved (profiles/r05_qp_unsolved_admm.json), which QPSolver::solve's caller treats as a failed
 *       plan (qp_solver.hpp:334-352) -- hence not the default.  OSQP itself is not in the image: its iterates remain unpinned.
 * The solve never forms Q, A, G: see allocnet_amd/csrc/qp_ipm.h, qp_admm.h.                          */
typedef struct anet_qp_settings {
  double rho;        /* 0.1   OSQP default; equality rows use 1e3*rho like OSQP                 */
  double sigma;      /* 1e-6                                                                    */
  double alpha;      /* 1.6                                                                     */
  double eps_abs;    /* 1e-3  (the reference never changes it: qp_solver.hpp:301-302, layers.py:79) */
  double eps_rel;    /* 1e-3                                                                    */
  int32_t max_iter;  /* 4000                                                                    */
  int32_t check_termination; /* 25                                                              */
  int32_t adaptive_rho_interval; /* 100; 0 disables (OSQP picks its interval from wall-clock time) */
  int32_t scaled_termination;    /* 0: OSQP's rule -- residuals of the reference's own (unscaled) QP;
                                    1: residuals of the internally normalised QP (like OSQP's
                                    scaled_termination): ~2-3x fewer iterations, looser on stiff problems */
  int32_t method;                /* ANET_QP_METHOD_ADMM: OSQP's algorithm, settings above.
                                    ANET_QP_METHOD_INTERIOR_POINT (default): primal-dual interior point on the same QP in
                                    Hermite node coordinates (allocnet_amd/csrc/qp_ipm.h) -- the optimum to
                                    min(eps, 1e-6) in 10-20 Newton steps; uses only eps_abs/eps_rel and max_iter
                                    (capped at 200) of the fields above; infeasible problems are reported
                                    PRIMAL_INFEASIBLE when the iteration diverges, MAX_ITER_REACHED otherwise */
} anet_qp_settings;
#define ANET_QP_METHOD_ADMM 0
#define ANET_QP_METHOD_INTERIOR_POINT 1
/* Row form, a bit OR-ed into anet_qp_settings.method (anet_qp_solve, _dev, _time_grad, _ordered_dev, _vjp) or into row_order
 * (anet_qp_assemble[_dev]).  Without it the corridor and box rows are held at `res` samples per piece (the reference's form: nothing
 * is held between two samples).  With it they are held on Bernstein control values, so for EVERY t of every piece: res must be
 * k * 2s (k >= 1 Bernstein segments per piece; anything else is ANET_ERR_INVALID), and group j = q*2s + r takes the place of sample
 * j -- for derivative d = 0, 1, 2 the d-th derivative of the piece restricted to segment q = [q T/k, (q+1) T/k], its Bernstein control
 * values (degree 2s-1-d) degree-elevated d times to 2s values beta^d_r; the group carries the piece's M corridor rows on beta^0_r and
 * the 12 box rows +-beta^1_r[ax] <= max_vel, +-beta^2_r[ax] <= max_acc.  Row counts, row order (both ANET_QP_ORDER_*), workspace and
 * every shape are those of the sample form at the same res; Q, A, b are untouched.  A curve lies in the hull of its control values
 * and elevated values are convex combinations of them, so a solution satisfies every row for all t up to the primal residual, and
 * junctions lie in both neighbouring polytopes; the feasible set is smaller than the sample form's, and that of 2k contains that
 * of k.  Interior point only (with ADMM: ANET_ERR_UNSUPPORTED); assembled in double only (with float_time: ANET_ERR_UNSUPPORTED). */
#define ANET_QP_ROWS_CONTROL_POINTS 0x100
void anet_qp_default_settings(anet_qp_settings *s);
#define ANET_QP_SOLVED 1          /* OSQP_SOLVED                 */
#define ANET_QP_MAX_ITER_REACHED (-2) /* OSQP_MAX_ITER_REACHED; the reference treats anything but Solved as failure (qp_solver.hpp:346-350) */
#define ANET_QP_PRIMAL_INFEASIBLE (-3) /* OSQP_PRIMAL_INFEASIBLE: OSQP's certificate test on y(k+1)-y(k), eps_prim_inf 1e-4 */
#define ANET_QP_UNSOLVED (-10)    /* OSQP_UNSOLVED: a problem no workgroup took (a launch_order that skips it); obj = NaN, iters = 0 */
/* hpolys [batch][N][M][4] rows a.x <= b with all-zero rows as inert padding.
 * coeffs [batch][N][3][2s] (the flatten order callModel unpacks, learning_planner.hpp:212,227),
 * obj [batch] = 1/2 z'Qz (QPSolver::getObjCost), status/iters [batch], residuals [batch][2] (primal, dual;
 * may be NULL).  All HOST pointers; the _dev variant takes DEVICE pointers (same trajectory-major
 * layout) plus a device workspace of anet_qp_solve_workspace() doubles (the slacks and multipliers of every row, and for the
 * two-launch form of large batches the parked iterates and the order of the second launch: always ask, never compute it). */
int anet_qp_solve(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                  double max_acc, double m34, const double *state, const double *T, const double *hpolys,
                  const anet_qp_settings *settings, double *coeffs, double *obj, int32_t *status,
                  int32_t *iters, double *residuals);
int64_t anet_qp_solve_workspace(int s, int n_pieces, int64_t batch, int res, int M);
int anet_qp_solve_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                      double max_acc, double m34, const double *state, const double *T,
                      const double *hpolys, const anet_qp_settings *settings, double *work, double *coeffs,
                      double *obj, int32_t *status, int32_t *iters, double *residuals, void *stream);

/* The form of the interior-point kernel a batch of this shape takes on this context's device with the default settings (the
 * selection of anet_qp_solve* itself: allocnet_amd/csrc/api_qp.hip), as a bit set:
 *   form & ANET_QP_IPM_FORM_PER_CU_MASK   workgroups per compute unit the kernel's registers are bounded for: 1, 2 or 3
 *   form & ANET_QP_IPM_FORM_THROUGHPUT    the four-pass form of large batches; clear = the FUSE form (small batches, lone problems,
 *                                         problems whose LDS fills a compute unit; always 1 per compute unit)
 *   form & ANET_QP_IPM_FORM_TWO_LAUNCHES  every problem through a few Newton steps, then the unfinished ones resumed
 * with_launch_order != 0: as for anet_qp_solve_ordered_dev with an order (always one launch).  0 for an empty batch (nothing
 * is launched); negative = error: ANET_ERR_INVALID (bad shape), ANET_ERR_UNSUPPORTED (the problem does not fit the 160 KB LDS).
 * For tests and callers that label a measurement with the kernel that ran.                                                  */
#define ANET_QP_IPM_FORM_PER_CU_MASK 0x3
#define ANET_QP_IPM_FORM_THROUGHPUT 0x10
#define ANET_QP_IPM_FORM_TWO_LAUNCHES 0x20
int anet_qp_ipm_launch_form(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, int with_launch_order);

/* The same with a launch order for the interior-point method (one workgroup per problem, 512 resident at a time: a batch ends
 * with whichever long problem started late -- 27 % above its balanced figure for 4096 problems): launch_order
 * (device, int32 [batch], a permutation of 0..batch-1) is the problem each successive workgroup takes; longest first from the
 * iters[] of a previous solve of the same or a similar batch (anet_launch_order_from_steps_dev) -- the re-solve of a receding-
 * horizon planner or a sampler.  Results are bit-identical for any order; NULL = as given; the ADMM method ignores it.
 * Entries are not checked on the host (device memory): an entry outside [0, batch) is skipped and a problem no entry names
 * reports status ANET_QP_UNSOLVED, iters 0 and obj NaN (its coeffs are left untouched).  A REPEATED entry is undefined
 * behaviour for the problem it names: two workgroups then run on the same per-problem slack / multiplier state and write
 * the same coeffs / status concurrently (a race, not a redundant solve) -- the order must be a permutation.
 * No reference counterpart (QPSolver::solve takes one problem: qp_solver.hpp:119).                                        */
int anet_qp_solve_ordered_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                              double max_acc, double m34, const double *state, const double *T, const double *hpolys,
                              const anet_qp_settings *settings, const int32_t *launch_order, double *work, double *coeffs,
                              double *obj, int32_t *status, int32_t *iters, double *residuals, void *stream);

/* The same solve plus grad_T [batch][N] = d(obj)/dT_i, the derivative of the OPTIMAL cost 1/2 z*'Q z*
 * with respect to the segment durations -- the "time-allocation gradient" the reference's training loop
 * is after (network/layers.py:120-147 installs a -J^-1 grad KKT hook for it, a dense (n+m)^2 solve per
 * sample).  Because the loss IS the QP objective, no KKT solve is needed: by the
 * envelope theorem the derivative is dL/dT at the optimum, assembled inside the solve kernel (either method)
 * from the solution and its multipliers (allocnet_amd/csrc/qp_admm.h, qp_ipm.h).  Exact at the optimum of a problem with a
 * stable active set; its accuracy follows the solve tolerance.  Not what the reference's autograd
 * delivers today (its z is a detached leaf: that quantity is anet_traj_cost_grad_T) -- see DESIGN.md 8b. */
int anet_qp_solve_time_grad(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                            double max_acc, double m34, const double *state, const double *T,
                            const double *hpolys, const anet_qp_settings *settings, double *coeffs, double *obj,
                            int32_t *status, int32_t *iters, double *residuals, double *grad_T);
int anet_qp_solve_time_grad_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                                double max_acc, double m34, const double *state, const double *T,
                                const double *hpolys, const anet_qp_settings *settings, double *work,
                                double *coeffs, double *obj, int32_t *status, int32_t *iters, double *residuals,
                                double *grad_T, void *stream);

/* Backward pass through the QP (replaces the KKT hook of network/utils/learning/layers.py:129-141,
 * 230-243: grad <- -J^-1 grad with J = [[Q, G'diag(lambda), A'], [G, diag(Gz-h), 0], [A, 0, 0]], a dense (n+m)^2 solve
 * per sample whose result stops at the detached leaf z).  Solves the QP (interior-point method only) and returns,
 * for a caller-supplied gradient grad_z = d loss / d z* (layout of `coeffs`), grad_T [batch][N] = d loss / d T:
 * the adjoint is taken at the optimum with the method's own block-tridiagonal Newton matrix (Hermite coordinates:
 * the equality block is built in, the inequality rows enter through lambda / s) and contracted in closed form with
 * the dependence of the cost blocks, the continuity scalings, the pinned end states, the box bounds and the
 * coefficient scaling on the durations.  Any smooth loss of the optimal coefficients can be differentiated this way;
 * for loss = the QP objective it reproduces anet_qp_solve_time_grad (minus the explicit 1/2 z'(dQ/dT)z part, which
 * anet_traj_cost_grad_T gives).  settings as in anet_qp_solve (the tolerance is tightened to 1e-9).            */
int anet_qp_solve_vjp(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                      double max_acc, double m34, const double *state, const double *T, const double *hpolys,
                      const anet_qp_settings *settings, const double *grad_z /* [batch][N][3][2s] */, double *coeffs,
                      double *obj, int32_t *status, int32_t *iters, double *residuals, double *grad_T /* [batch][N] */);
int anet_qp_solve_vjp_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int res, int M, double max_vel,
                          double max_acc, double m34, const double *state, const double *T, const double *hpolys,
                          const anet_qp_settings *settings, const double *grad_z, double *work, double *coeffs,
                          double *obj, int32_t *status, int32_t *iters, double *residuals, double *grad_T,
                          void *stream);

/* ---- polytope depth: geo_utils::findInterior / geo_utils::overlap, sfc_gen::shortCut --------------------------- */
/* Replaces the 4-variable linear programme of geo_utils::findInterior and geo_utils::overlap
 * (src/planner/include/gcopter/geo_utils.hpp:43-85, solved there by sdlp::linprog<4>), batched: for each polytope
 * (rows h: h0 x + h1 y + h2 z + h3 <= 0, all-zero rows are padding up to max_rows)
 *     depth = max t  s.t.  n.x + t <= -h3  for every row,   n = h[0:3] / |h[0:3]| (normalise = 1, findInterior)
 *                                                            or h[0:3]            (normalise = 0, overlap)
 * and the point x that attains it (point may be NULL).  findInterior(hPoly) is depth > 0; overlap(hPoly0, hPoly1, eps) is
 * depth > eps of the two polytopes' rows stacked (sfc_gen::shortCut, sfc_gen.hpp:188-226, calls it with eps = 0.1);
 * depth = -inf for a polytope of padding rows only, +inf for an unbounded one (the reference's tests read both as false).
 * Exact: an active-set ascent, one lane per polytope, whose result is certified (feasible, multipliers >= 0) before it is
 * returned; what it cannot certify falls back to the enumeration of the vertices (allocnet_amd/csrc/firi_kernels.h;
 * C(rows, 4) candidates, hence max_rows <= 256: ANET_ERR_UNSUPPORTED beyond).
 * Bounded polytopes (corridors always carry their bounding box).                                                       */
int anet_polytope_depth(anet_ctx *ctx, int64_t batch, int max_rows, const double *hpoly /* [batch][max_rows][4] */,
                        int normalise, double *depth /* [batch] */, double *point /* [batch][3] or NULL */);
int anet_polytope_depth_dev(anet_ctx *ctx, int64_t batch, int max_rows, const double *hpoly, int normalise,
                            double *depth, double *point, void *stream);

/* geo_utils::enumerateVs (geo_utils.hpp:155-202, with filterVs :128-150), batched: the vertices of polytopes given by their
 * half-spaces, hpoly as for anet_polytope_depth (all-zero rows are padding), 1 <= max_rows <= 128 (two stacked FIRI outputs;
 * ANET_ERR_UNSUPPORTED beyond).  The rows are scaled to unit normals (n, d).  A triple i < j < k of them with
 * |det(n_i, n_j, n_k)| >= 1e-8 gives a candidate point; it is feasible when n.x + d <= epsilon for every row (epsilon: the
 * reference's parameter, 1e-6 there).  Feasible candidates are visited in ascending lexicographic order of (i, j, k) and one is
 * dropped when a vertex kept before it lies within max(epsilon, mag * DBL_EPSILON) of it in the max-norm (mag: the largest
 * absolute coordinate among the kept vertices and the candidate) -- filterVs's resolution as a distance, where the reference
 * rounds to a grid and compares cells (two points 1e-12 apart on both sides of a cell edge stay distinct there).  verts[b] holds
 * the kept vertices in that order, whatever the launch shape.
 * active (or NULL): per kept vertex the rows with |n.x + d| <= epsilon, bit r % 64 of word r / 64 for row r of hpoly[b].
 * status[b] (or NULL): ANET_POLYTOPE_OK; ANET_POLYTOPE_SKIPPED with count[b] = 0 when the polytope's depth
 * (anet_polytope_depth, normalised) is not a positive finite number -- empty, flat, padding only, or unbounded: where the
 * reference's two-argument overload returns false -- or when no triple gives a feasible point (a slab: an unbounded set of
 * finite depth; an unbounded polytope that HAS vertices is not detected, corridors carry their bounding box);
 * ANET_POLYTOPE_TRUNCATED when it has more vertices than max_vertices (>= 1): count[b] is the true number, the first
 * max_vertices are written -- or more than 256 distinct ones: count[b] = 256, a lower bound (252 = 2 * rows - 4 is the most a
 * polytope of 128 rows has; 2 * rows - 4 vertices suffice for every non-degenerate polytope).
 * The host call zero-fills the slots behind count[b]; the _dev call leaves them as they are, takes device pointers, runs
 * asynchronously on `stream` and keeps the depths in the context's workspace (calls on one context do not overlap).        */
#define ANET_POLYTOPE_OK 0
#define ANET_POLYTOPE_SKIPPED 1
#define ANET_POLYTOPE_TRUNCATED 2
int anet_polytope_vertices(anet_ctx *ctx, int64_t batch, int max_rows, const double *hpoly, double epsilon, int max_vertices,
                           double *verts /* [batch][max_vertices][3] */, int32_t *count /* [batch] */,
                           uint64_t *active /* [batch][max_vertices][2] or NULL */, int32_t *status /* [batch] or NULL */);
int anet_polytope_vertices_dev(anet_ctx *ctx, int64_t batch, int max_rows, const double *hpoly, double epsilon, int max_vertices,
                               double *verts, int32_t *count, uint64_t *active, int32_t *status, void *stream);

/* ---- batched L-BFGS ------------------------------------------------------------------------ */
/* lbfgs::lbfgs_parameter_t, same fields and defaults (gcopter/lbfgs.hpp:15-129). */
typedef struct anet_lbfgs_params {
  int32_t mem_size;       /* 8      */
  double g_epsilon;       /* 1e-5   */
  int32_t past;           /* 3      */
  double delta;           /* 1e-6   */
  int32_t max_iterations; /* 0 = until convergence */
  int32_t max_linesearch; /* 64     */
  double min_step;        /* 1e-20  */
  double max_step;        /* 1e+20  */
  double f_dec_coeff;     /* 1e-4   */
  double s_curv_coeff;    /* 0.9    */
  double cautious_factor; /* 1e-6   */
  double machine_prec;    /* 1e-16  */
} anet_lbfgs_params;
void anet_lbfgs_default_params(anet_lbfgs_params *p);
/* lbfgs_optimize's own parameter validation (lbfgs.hpp:449-495): 0 or the LBFGSERR_INVALID_* code. */
int anet_lbfgs_check_params(int n, const anet_lbfgs_params *p);
/* lbfgs::lbfgs_strerror (lbfgs.hpp:724-799). */
const char *anet_lbfgs_strerror(int code);

/* Per problem the control flow, line search (Lewis-Overton weak Wolfe), cautious update, stopping
 * tests and return codes are those of lbfgs::lbfgs_optimize / line_search_lewisoverton
 * (gcopter/lbfgs.hpp:276-384, 434-717); the batch advances one objective evaluation per step, each
 * problem in its own state.  status[b] is lbfgs_optimize's return value (0 convergence, 1 stop,
 * negative LBFGSERR_*), iters[b] its iteration counter k, evals[b] the number of objective
 * evaluations.  max_evals (> 0) bounds the evaluations per problem; problems still running then
 * report status ANET_LBFGS_RUNNING.                                                            */
#define ANET_LBFGS_RUNNING 2147483647

/* Objective = firi::costMVIE (gcopter/firi.hpp:86-157), the reference's only L-BFGS call site
 * (firi::maxVolInsEllipsoid, firi.hpp:207-227).  A: per problem the M x 3 matrix COLUMN-major, as the
 * reference packs optData (firi.hpp:186-200); x: 9 variables [p, sqrt-diag, off-diag], in/out.   */
int anet_lbfgs_mvie(anet_ctx *ctx, int64_t batch, int M, const double *A /* [batch][3*M] */,
                    double smooth_eps, double penalty_wt, double *x /* [batch][9] */,
                    double *f /* [batch] */, const anet_lbfgs_params *params, int max_evals,
                    int32_t *status, int32_t *iters, int32_t *evals);

/* lbfgs::lbfgs_optimize for an objective the CALLER evaluates on the device (lbfgs.hpp:434-440: x, f, proc_evaluate,
 * proc_stepbound, proc_progress, instance, param).  proc_evaluate (lbfgs.hpp:186-219) becomes a host function that ENQUEUES
 * the evaluation of the whole batch on `stream`: given x ([n][ld] device, batch-minor: variable i of problem b at x[i*ld + b])
 * it must leave f[b] and g[i*ld + b] for every problem b < batch (the values of problems that have stopped are ignored) and
 * return 0; anything else aborts the run with ANET_ERR_INVALID.  The call synchronises `stream` as it goes (completion polls) and at
 * its end: x, f, status, iters and evals are complete on return, on whatever stream the caller reads them.  It is called once per evaluation step of the batch (the
 * lockstep shape: every running problem consumes one evaluation per call; a completion flag is polled every eight steps, so
 * up to eight calls may follow the last problem's stop).  x is the start point in, the result out; f and g are the caller's
 * buffers the callback fills ([batch] and [n][ld]); on return f[b] is lbfgs_optimize's fx.  proc_stepbound: the one bound
 * with a use is built in -- bound_from < n keeps the variables i >= bound_from at or above bound_min within every line search
 * (lbfgs.hpp:557-565; bound_from >= n: none); proc_progress: anet_set_cancel_flag.  work: anet_lbfgs_workspace() doubles.  */
typedef int (*anet_lbfgs_evaluate_t)(void *instance, const double *x, double *f, double *g, int64_t batch, int64_t ld, int n,
                                     void *stream);
int64_t anet_lbfgs_workspace(int n, int64_t ld, const anet_lbfgs_params *params);
int anet_lbfgs_optimize_dev(anet_ctx *ctx, int n, int64_t batch, int64_t ld, double *x, double *f, double *g,
                            anet_lbfgs_evaluate_t proc_evaluate, void *instance, const anet_lbfgs_params *params,
                            int max_evals, int bound_from, double bound_min, double *work, int32_t *status,
                            int32_t *iters, int32_t *evals, void *stream);

/* lbfgs::lbfgs_optimize for an objective evaluated ON THE HOST, with the reference's three callbacks (lbfgs.hpp:186-246, called
 * as lbfgs.hpp:434-717 calls them): one problem, x [n] host memory (start point in, result out), *f = fx on return, *ret =
 * lbfgs_optimize's return value (LBFGS_CONVERGENCE / LBFGS_STOP / LBFGS_CANCELED / LBFGSERR_*, parameter errors included),
 * *iters = k, *evals = objective evaluations (iters / evals may be NULL).
 *   proc_evaluate (required): returns f(x) and fills g [n]                                    -- lbfgs_evaluate_t
 *   proc_stepbound (may be NULL): upper bound of the step along d from xp                    -- lbfgs_stepbound_t, lbfgs.hpp:557-565
 *   proc_progress (may be NULL): called after every successful line search with x, g, fx, step, k, ls;
 *                 a non-zero return ends the run with LBFGS_CANCELED                        -- lbfgs_progress_t, lbfgs.hpp:580-587
 * The optimiser's vectors and all its arithmetic (line-search bookkeeping, cautious update, two-loop recursion, stopping
 * tests) stay on the device -- the lockstep update kernel with a batch of one -- and the state machine parks where the
 * reference calls back: per evaluation x goes to the host and f, g come back; per line search xp and d go to the host and the
 * bound comes back.  There is no CPU optimiser in the library.  A PCIe round trip per evaluation: for objectives that can be
 * evaluated on the device use anet_lbfgs_optimize_dev.  The call returns ANET_OK when the run ended by lbfgs_optimize's own rules,
 * whatever *ret says. */
typedef double (*anet_lbfgs_host_evaluate_t)(void *instance, const double *x, double *g, int n);
typedef double (*anet_lbfgs_host_stepbound_t)(void *instance, const double *xp, const double *d, int n);
typedef int (*anet_lbfgs_host_progress_t)(void *instance, const double *x, const double *g, double fx, double step, int k,
                                          int ls, int n);
int anet_lbfgs_optimize_host(anet_ctx *ctx, int n, double *x, double *f, anet_lbfgs_host_evaluate_t proc_evaluate,
                             anet_lbfgs_host_stepbound_t proc_stepbound, anet_lbfgs_host_progress_t proc_progress,
                             void *instance, const anet_lbfgs_params *params, int32_t *ret, int32_t *iters, int32_t *evals);

/* Objective = the MINCO cost  int (p^(s))^2 + rho*sum(T) + J_pen  (anet_minco_cost_grad) over the
 * interior waypoints (opt_flags bit 0) and/or the durations (bit 1), the durations through the
 * smooth bijection T(tau) so the problem is unconstrained.  wps and T are in/out.
 * Accuracy: inside the loop the cost and its gradient come from the reduced (Hermite / block-tridiagonal) system, whose
 * error grows with the spread of the durations (1e-8 up to max T / min T = 100, 5e-4 on snap coefficients at 10^3:
 * DESIGN.md section 2) -- the optimiser is free to walk there when ANET_OPT_TIMES is set.  What is RETURNED does not
 * carry that envelope: coeffs_out of a problem whose optimised durations spread over more than 50 are re-solved by the
 * pivoted collocation solve (anet_minco_solve_wide_spread_dev); anet_minco_spread_flags_dev on the returned T tells
 * which problems those were.                                                                     */
#define ANET_OPT_WAYPOINTS 1
#define ANET_OPT_TIMES 2
/* Execution shape (same result up to rounding): by default problems that fit one wavefront (orders 3 and 4, at most
 * 64 variables, mem_size <= 8, past <= 64) run as ONE launch, one wave per problem, each until its
 * own stop (lbfgs.hpp:551-709 is one loop per problem); this bit forces the launch-per-evaluation kernels instead,
 * which advance the whole batch in lockstep (up to twice the throughput per evaluation step at batches of 10^5, so the
 * better shape for a small FIXED evaluation budget there; a run to convergence is faster in one launch at any batch).
 * Batches of >= 4096 problems with >= 36 variables take the wave-per-problem shape in TWO launches -- 1000 evaluations of
 * every problem, then the unfinished ones resumed longest-expected first -- with bit-identical results.   */
#define ANET_OPT_LOCKSTEP 4
int anet_lbfgs_minco(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head,
                     const double *tail, double *wps, double *T, const double *hpolys,
                     const anet_penalty *pen, const anet_lbfgs_params *params, int opt_flags,
                     int max_evals, double *cost, double *coeffs_out, int32_t *status, int32_t *iters,
                     int32_t *evals);
/* Device variant: batch-minor device arrays, workspace from anet_lbfgs_minco_workspace() doubles.
 * status/iters/evals are device int32 arrays [batch].  The one-launch shape only enqueues kernels on `stream` (no
 * host-side test for completion, no allocation: it can be captured into a hipGraph); the lockstep shape synchronises
 * the stream every few evaluations to test for completion.                                         */
int64_t anet_lbfgs_minco_workspace(int s, int n_pieces, int64_t ld, const anet_lbfgs_params *params);
int anet_lbfgs_minco_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                         const double *head, const double *tail, double *wps, double *T,
                         const double *hpolys, const anet_penalty *pen,
                         const anet_lbfgs_params *params, int opt_flags, int max_evals, double *work,
                         double *cost, double *coeffs_out, int32_t *status, int32_t *iters,
                         int32_t *evals, void *stream);
/* The same with a launch order for the one-launch shape: launch_order (device, int32 [batch], a permutation of
 * 0..batch-1, or NULL) names the problem each successive workgroup takes.  Results do not depend on it (problems are
 * independent); the run time does: a batch larger than the 2048 waves the device holds ends with whichever problem
 * started late and runs long, so handing over the problems longest-first shortens the run (4096 x 16-segment jerk:
 * 0.19 s as given, 0.12 s by the true evaluation counts, 0.14 s by the counts of a previous solve of a perturbed copy
 * of the batch -- the re-solve case of a sampler or a receding-horizon planner: feed evals[] of the last call,
 * sorted descending).  Entries are not checked beyond their range: an out-of-range entry is skipped and a problem no
 * entry names is left unsolved (ANET_LBFGS_RUNNING, zero counters); a REPEATED entry is undefined behaviour for the
 * problem it names (two waves race on its state) -- the order must be a permutation.  Ignored by the lockstep shape.  */
int anet_lbfgs_minco_ordered_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                                 const double *head, const double *tail, double *wps, double *T,
                                 const double *hpolys, const anet_penalty *pen,
                                 const anet_lbfgs_params *params, int opt_flags, int max_evals,
                                 const int32_t *launch_order, double *work, double *cost, double *coeffs_out,
                                 int32_t *status, int32_t *iters, int32_t *evals, void *stream);
/* The same with lbfgs_optimize's step bound (lbfgs.hpp:221-224 lbfgs_stepbound_t, applied as lbfgs.hpp:557-565:
 * step_max = min(proc_stepbound(xp, d), max_step); step = step < step_max ? step : step_max / 2; the line search then runs
 * with that step_max) -- a host callback cannot run inside the kernels, so the one bound with a use is built in: a MINIMUM
 * DURATION.  min_duration > 0 bounds every line search to the largest step along the search direction that keeps every
 * duration variable tau_i >= backward_T(min_duration), i.e. T_i >= min_duration: 1 / max_i(-d_i / (tau_i - tau_min)) over the
 * duration variables that move down.  min_duration = 0: no bound (identical to the calls above).  Both execution shapes
 * apply it (the one-launch kernel and, with ANET_OPT_LOCKSTEP or problems that do not fit a wave, the per-evaluation
 * update kernels).  Start durations below the minimum make the first bound 0 and the run end with
 * LBFGSERR_INVALIDPARAMETERS, as the reference's loop would.                                                          */
int anet_lbfgs_minco_bounded(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head,
                             const double *tail, double *wps, double *T, const double *hpolys,
                             const anet_penalty *pen, const anet_lbfgs_params *params, int opt_flags,
                             int max_evals, double min_duration, double *cost, double *coeffs_out, int32_t *status,
                             int32_t *iters, int32_t *evals);
int anet_lbfgs_minco_bounded_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld,
                                 const double *head, const double *tail, double *wps, double *T,
                                 const double *hpolys, const anet_penalty *pen, const anet_lbfgs_params *params,
                                 int opt_flags, int max_evals, double min_duration, const int32_t *launch_order, double *work,
                                 double *cost, double *coeffs_out, int32_t *status, int32_t *iters, int32_t *evals,
                                 void *stream);

/* lbfgs_optimize's progress callback (lbfgs.hpp:226-246 lbfgs_progress_t, called at lbfgs.hpp:580-587 after every
 * successful line search; a non-zero return ends the run with LBFGS_CANCELED) -- a host callback cannot run inside the
 * kernels, so its one effect is offered as a word the caller owns: `flag` (device-visible int32 -- device memory written from
 * another stream, or mapped pinned host memory; NULL: none) is read once per evaluation by every problem of the one-launch
 * MINCO L-BFGS calls (either execution shape) that follow on this context; while it is non-zero a problem stops after the iteration it is in, at
 * the point lbfgs.hpp:583 would, with status LBFGS_CANCELED (2), its iterate, cost and counters as they stand.  Problems
 * that stopped on their own keep their status.  Both shapes of the MINCO L-BFGS look at it (the lockstep update kernels
 * read it once per problem and evaluation); the MVIE objective does not.                                               */
int anet_set_cancel_flag(anet_ctx *ctx, const int32_t *flag);

/* launch_order for the call above from the evals[] of a previous solve of the same or a similar batch: longest first, in
 * buckets of 16 evaluations (device arrays; work: ANET_LAUNCH_ORDER_WORK_INTS int32 of scratch; asynchronous on `stream`). */
#define ANET_LAUNCH_ORDER_WORK_INTS 4096
int anet_launch_order_from_counts_dev(anet_ctx *ctx, int64_t batch, const int32_t *counts, int32_t *launch_order,
                                      int32_t *work, void *stream);
/* The same in buckets of ONE: for the Newton-step counts iters[] of anet_qp_solve_dev (-> anet_qp_solve_ordered_dev). */
int anet_launch_order_from_steps_dev(anet_ctx *ctx, int64_t batch, const int32_t *steps, int32_t *launch_order,
                                     int32_t *work, void *stream);

/* ---- corridor generation: batched FIRI ------------------------------------ */
/* firi::firi + firi::maxVolInsEllipsoid (gcopter/firi.hpp:159-416), the inner step of
 * sfc_gen::convexCover (gcopter/sfc_gen.hpp:116-186): for each corridor segment (a, b), obstacle points
 * pc and bounding half-spaces bd, alternate `iterations` times between the polytope that separates the
 * current ellipsoid from the obstacles and the maximum-volume ellipsoid inscribed in that polytope
 * (L-BFGS on costMVIE with the call-site parameters of firi.hpp:212-217).
 * bd [batch][n_bd][4] and hpoly [batch][max_rows][4] rows h: h0 x + h1 y + h2 z + h3 <= 0 (GCOPTER's raw
 * form; LearningPlanner normalises and negates it into a.x <= b, learning_planner.hpp:293-299);
 * pc [batch][max_points][3] with n_points[batch] valid points each; a, b [batch][3].
 * n_rows [batch] rows written per corridor (the rest of hpoly is zero);
 * ok [batch]: 1 = done, 2 = done, but an inner MVIE optimisation was cut off by mvie_max_evals (the corridor is still
 *            valid: every pass only shrinks towards the obstacles; the reference continues after a failed optimisation
 *            too, firi.hpp:229-232), 0 = a or b violates bd (firi returns false, firi.hpp:282-286),
 *            -1 = the polytope needs more than max_rows rows;   ellipsoid [batch][15] (optional) =
 * R row-major, p, r of the last inscribed ellipsoid.  All HOST pointers.
 * sdlp::linprog<4> and Eigen::JacobiSVD, third-party pieces of the reference, are replaced by exact
 * equivalents (allocnet_amd/csrc/firi_kernels.h).                                                   */
typedef struct anet_firi_params {
  int32_t iterations;     /* 4     firi.hpp:273 */
  double epsilon;         /* 1e-6  firi.hpp:274 */
  double smooth_eps;      /* 1e-2  firi.hpp:218 */
  double penalty_wt;      /* 1e3   firi.hpp:219 */
  int32_t mvie_max_evals; /* 20000 evaluation budget of one MVIE optimisation (the reference has none) */
} anet_firi_params;
void anet_firi_default_params(anet_firi_params *p);
int anet_firi(anet_ctx *ctx, int64_t batch, int n_bd, int max_points, int max_rows, const double *bd,
              const double *pc, const int32_t *n_points, const double *a, const double *b,
              const anet_firi_params *params, double *hpoly, int32_t *n_rows, int32_t *ok, double *ellipsoid);
/* The same with DEVICE pointers (same layouts; ok is required) and a device workspace of
 * anet_firi_workspace() doubles: corridor generation, the QP / MINCO solve and the evaluation chain on the
 * device without a PCIe round trip.  Asynchronous on `stream`.                                        */
int64_t anet_firi_workspace(int64_t batch, int max_points, int max_rows);
int anet_firi_dev(anet_ctx *ctx, int64_t batch, int n_bd, int max_points, int max_rows, const double *bd,
                  const double *pc, const int32_t *n_points, const double *a, const double *b,
                  const anet_firi_params *params, double *work, double *hpoly, int32_t *n_rows, int32_t *ok,
                  double *ellipsoid, void *stream);

/* The same with a pass count per corridor: iterations[b] (1 .. params->iterations; NULL: params->iterations for all) -- a
 * corridor keeps the polytope of its last pass and sits out the rest.  sfc_gen::convexCover (sfc_gen.hpp:163, 176) calls
 * firi::firi with 4 passes for a segment and with 1 for a gap polytope: with this entry point both kinds go in ONE batch.
 * The host variant rejects counts outside [1, params->iterations]; the device variant cannot look at them without a
 * synchronisation and clamps instead (below 1 -> one pass, above params->iterations -> params->iterations).
 * Consumers test ok >= 1: ok = 2 is a usable corridor whose inner MVIE optimisation ran into mvie_max_evals. */
int anet_firi_var(anet_ctx *ctx, int64_t batch, int n_bd, int max_points, int max_rows, const double *bd,
                  const double *pc, const int32_t *n_points, const double *a, const double *b,
                  const int32_t *iterations /* [batch] or NULL */, const anet_firi_params *params, double *hpoly,
                  int32_t *n_rows, int32_t *ok, double *ellipsoid);
int anet_firi_var_dev(anet_ctx *ctx, int64_t batch, int n_bd, int max_points, int max_rows, const double *bd,
                      const double *pc, const int32_t *n_points, const double *a, const double *b,
                      const int32_t *iterations, const anet_firi_params *params, double *work, double *hpoly,
                      int32_t *n_rows, int32_t *ok, double *ellipsoid, void *stream);

/* ---- voxel map: cloud occupancy, dilation, surface and the corridor's point selection ---------------- */
/* voxel_map::VoxelMap (gcopter/voxel_map.hpp, voxel_dilater.hpp) on a device byte grid: voxel (x, y, z) at
 * x + size[0] * (y + size[1] * z), values 0 Unoccupied, 1 Occupied, 2 Dilated; size[0] * size[1] * size[2] < 2^31.
 * Byte-identical voxels and bit-identical surface coordinates; the surface is in ASCENDING voxel index order (the
 * reference's is in breadth-first discovery order: the same set).  Device pointers, asynchronous on `stream`.      */
typedef struct anet_voxel_grid {
  int32_t size[3];
  double origin[3];
  double scale;
} anet_voxel_grid;
/* setOccupied for n records `stride` bytes apart, each starting with three float32 (f64 = 0, a PointCloud2 with
 * point_step = stride) or float64 (f64 = 1) coordinates: records with a non-finite coordinate are skipped
 * (mapCallBack), the index is ((pos - o) / scale) truncated toward zero, out-of-range points are dropped.           */
int anet_voxel_set_occupied_dev(anet_ctx *ctx, const anet_voxel_grid *grid, uint8_t *voxels, const void *records, int64_t n,
                                int64_t stride, int f64, void *stream);
/* setOccupied(Eigen::Vector3i id) for n index triples ids [n][3] (x, y, z): in-bounds voxels are set to 1, the rest dropped */
int anet_voxel_set_occupied_ids_dev(anet_ctx *ctx, const anet_voxel_grid *grid, uint8_t *voxels, const int32_t *ids, int64_t n,
                                    void *stream);
/* bytes of device workspace of anet_voxel_dilate_dev / anet_voxel_surface_dev (-1: bad grid) */
int64_t anet_voxel_workspace(const anet_voxel_grid *grid);
/* dilate(r): r synchronous 26-neighbour frontier rounds (round 1 grows from the voxels == 1, each later round from the
 * voxels the previous one added, only into voxels == 0; grown voxels become 2).  r <= 0 does nothing.  The last round's
 * front stays in `work` for anet_voxel_surface_dev until the next dilate on that workspace.                          */
int anet_voxel_dilate_dev(anet_ctx *ctx, const anet_voxel_grid *grid, uint8_t *voxels, int r, void *work, void *stream);
/* the surface (the voxels the last round of the last dilate added) as ascending linear ids: min(count, cap) written to
 * ids, the true count to *count (device int32).                                                                    */
int anet_voxel_surface_dev(anet_ctx *ctx, const anet_voxel_grid *grid, void *work, int64_t cap, int32_t *ids, int32_t *count,
                           void *stream);
/* getSurf: out [n][3] = id * stepScale + oc in the reference's offset form, the product and the sum each rounded.   */
int anet_voxel_surf_points_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const int32_t *ids, int64_t n, double *out,
                               void *stream);
/* query: out[i] = 1 when position i (pos [n][3]) is outside the map or in a voxel != 0, else 0                      */
int anet_voxel_query_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *voxels, const double *pos, int64_t n,
                         uint8_t *out, void *stream);
/* Exact first collision of every piece with the map (no counterpart in the reference, which has no trajectory-against-map test):
 *     t_hit[i] = inf { t in [0, T_i] : blocked(p_i(t)) },  blocked(p) <=> anet_voxel_query_dev answers 1 for p
 * (outside the map, or in a voxel != 0; cell = ((p - origin) / scale) truncated toward zero, so cell 0 spans -1 < q < 1), +inf
 * when the piece is free: the minimum over the pieces of (earlier durations + t_hit) is the trajectory's first collision.  Not
 * sampled: a curve that clips a voxel between two samples is found.  coeffs, T: the layouts of anet_traj_eval[_dev]; voxels: the
 * DEVICE byte grid in both forms; t_hit: double [N][ld] (dev) / [batch][N] (host); voxel (may be NULL): int32 of the same shape,
 * the linear index of the blocked voxel entered, ANET_HIT_FREE, ANET_HIT_OUTSIDE (the curve left the map) or ANET_HIT_INVALID.
 * A curve that starts blocked has t_hit = 0; a piece with T_i == 0 is the point p_i(0).  A NaN or infinite coefficient or
 * duration, or T_i < 0, gives t_hit = NaN and ANET_HIT_INVALID for that piece only.  ANET_HIT_INVALID with a FINITE t_hit: the
 * kernel's bounded search ran out; the piece is free before t_hit and undecided from there on (treat as a hit).  A bad grid
 * (non-finite fields, scale <= 0, sizes < 1) is ANET_ERR_INVALID.  Accuracy (csrc/voxel_hit_kernels.h):
 * |t_hit - t*| <= T_i 2^-32 + 32 eps (sum_k |u_k| + |q_plane|) / |dq/dtau| T_i on the crossed axis, u the coefficients of q in
 * normalised time; a voxel penetrated deeper than tol_pos is never missed, one farther than tol_pos away never reported.
 * The host form runs on the context's stream: the map must be complete (its stream synchronised) before the call. */
#define ANET_HIT_FREE (-1)
#define ANET_HIT_OUTSIDE (-2)
#define ANET_HIT_INVALID (-3)
int anet_traj_voxel_hit_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                            const anet_voxel_grid *grid, const uint8_t *voxels, double *t_hit, int32_t *voxel, void *stream);
int anet_traj_voxel_hit(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs, const double *T,
                        const anet_voxel_grid *grid, const uint8_t *voxels /* DEVICE: the map lives there */, double *t_hit,
                        int32_t *voxel);
/* convexCover's per-segment selection: for box k (bd [n_boxes][6][4], the layout of anet_firi's bd), the points p of
 * points [n_points][3] with max_r(bd[k][r][:3] . p + bd[k][r][3]) < 0, in their order, into out [n_boxes][max_points][3]
 * (rows past the count untouched); n_out[k] = the true count, which may exceed max_points.                           */
int64_t anet_voxel_gather_workspace(int64_t n_boxes, int64_t n_points);
int anet_voxel_gather_boxes_dev(anet_ctx *ctx, int64_t n_boxes, const double *bd, const double *points, int64_t n_points,
                                int64_t max_points, void *work, double *out, int32_t *n_out, void *stream);
/* Exact clearance of every piece to obstacle points (no counterpart in the reference): for piece i and the points q_j given for it
 *     clearance[i] = min over finite points j, min over t in [0, T_i], of || p_i(t) - q_j ||      (Euclidean, metres)
 * Not sampled: the minimum between two samples is found.  point[i] (may be NULL): a minimising point's index within its set, -1
 * when the set has no finite point; t[i] (may be NULL): the local time of the minimum, 0 without a point.  Both are diagnostics
 * specified by consistency, as row and t of anet_traj_row_margin are: || p_i(t) - q_point || reproduces clearance within the
 * bound; there is no tie-breaking rule.  A piece without a finite point has clearance +inf.  A point with a non-finite coordinate
 * is skipped, as setOccupied skips such records.  T_i == 0 is the point p_i(0).  A NaN or infinite coefficient or duration, or
 * T_i < 0, gives clearance NaN, point -1 and t 0 for that piece only; so does a product c_k T_i^k that is not finite (an
 * overflowing power of T_i also where c_k = 0).  Orders s = 2, 3, 4.
 * coeffs, T: the layouts of anet_traj_row_margin[_dev]; clearance, point, t: [N][ld] (dev) / [batch][N] (host).
 * points: [n_sets][max_points][3] doubles, on the DEVICE for the _dev form and on the HOST for the host form; counts: int32
 * [n_sets] (same side), or NULL = max_points each; a count is clamped to [0, max_points].  n_sets is 1 (one cloud shared by every
 * piece) or n_pieces (piece i uses set i: exactly the out / n_out pair of anet_voxel_gather_boxes_dev, whose counts may exceed
 * max_points; hence the clamp); anything else is ANET_ERR_INVALID.  max_points == 0 is valid (points may be NULL): every piece
 * gets +inf; max_points < 2^31.  batch == 0 returns ANET_OK after the argument checks.
 * Accuracy (csrc/clearance_kernels.h): |clearance - exact| <= 32 eps scale + location term, scale = sum_ax (sum_k |u_ax,k| +
 * |q_ax|), u the coefficients in normalised time; the location term is min(sqrt(2) E / sqrt(kappa), E^2 / (kappa d)) at an interior
 * minimum, E = 16 eps scale ||u'|| + 32 eps d sum_ax sum_k k |u_ax,k| + 2 eps kappa, kappa = g''/2 there, and 0 at an end.
 * The value is always an actual distance of the curve to a point of the set: never below the exact one by more than 32 eps scale. */
int anet_traj_clearance_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                            int n_sets, int64_t max_points, const double *points /* [n_sets][max_points][3], device */,
                            const int32_t *counts /* [n_sets] device, or NULL */, double *clearance, int32_t *point, double *t,
                            void *stream);
int anet_traj_clearance(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs, const double *T, int n_sets,
                        int64_t max_points, const double *points /* HOST */, const int32_t *counts /* HOST or NULL */,
                        double *clearance, int32_t *point, double *t);
/* Exact minimum separation between pairs of trajectories of one batch (no counterpart in the reference): for the pair (a, b)
 *     sep = min over the common intervals, min over t, of || p_a,i(t - K_i^a) - p_b,j(t - K_j^b) ||      (Euclidean, metres)
 * Knots are float64 by definition: K_0 = t0 (t0 == NULL: 0), K_(i+1) = K_i + T_i summed in piece order; piece i lives on global time
 * [K_i, K_(i+1)] and is evaluated at local time t - K_i; a piece with K_(i+1) == K_i occupies no time (T_i = 0: padding).  The window
 * is W = [max(K_0^a, K_0^b), min(K_N^a, K_N^b)]; the intervals are the maximal sub-intervals of W of positive length between
 * consecutive distinct knots of either trajectory, each closed and with its own two pieces at both ends (trajectories need not be
 * continuous).  Not sampled: the minimum between two samples is found.  Holding position before the start or after the end is
 * not a mode: prepend or append a constant piece.
 * t (may be NULL): the global time of a minimum; piece_a, piece_b (may be NULL): its pieces.  They are diagnostics specified by
 * consistency, as point and t of anet_traj_clearance are: the distance of the two named pieces at t reproduces sep within the
 * bound, and t lies in W and in both pieces' spans; there is no tie-breaking rule.  No interval (disjoint or merely touching
 * windows): sep +inf, t 0, pieces -1.  a == b is a valid pair with separation 0.  sep NaN, t 0, pieces -1, for that pair only: a
 * duration, t0 or knot of either trajectory that is not finite, a negative duration; a coefficient or a product c_k T_i^k that is
 * not finite in a piece that takes part in an interval (a piece that takes part in none is not read); on the _dev form a pair
 * index outside [0, batch), for which nothing is read.  The host form refuses such an index with ANET_ERR_INVALID.
 * cutoff >= 0 (INFINITY: off; NaN or negative: ANET_ERR_INVALID): every reported sep is an actual distance of the two curves at
 * the reported t, with or without a cutoff; it is within the full bound of the exact minimum whenever that minimum is below
 * cutoff; an interval whose certified lower bound is at least cutoff is left at its best sampled distance.
 * coeffs, T: the layouts of anet_traj_clearance[_dev]; t0: [batch]; pair_a, pair_b: int32 [n_pairs]; sep, t, piece_a, piece_b:
 * [n_pairs]; everything on the device for the _dev form and on the host for the host form.  n_pairs == 0 or batch == 0 returns
 * ANET_OK after the argument checks and touches nothing.  No workspace.  A pair list sorted by a reads fastest.
 * Accuracy (csrc/separation_kernels.h): |sep - exact| <= 64 eps scale + 4 eps |t| v + location term, scale the two pieces' sums of
 * |c_k T^k|, v a bound of the two speeds, |t| the largest modulus of the times involved; never below the exact minimum by more
 * than the first two terms. */
int anet_traj_separation_dev(anet_ctx *ctx, int s, int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                             const double *t0 /* [batch] or NULL */, int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                             double cutoff, double *sep, double *t, int32_t *piece_a, int32_t *piece_b, void *stream);
int anet_traj_separation(anet_ctx *ctx, int s, int n_pieces, int64_t batch, const double *coeffs, const double *T,
                         const double *t0 /* [batch] or NULL */, int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                         double cutoff, double *sep, double *t, int32_t *piece_a, int32_t *piece_b);

/* ---- trajectory avoidance as a penalty of the MINCO objective (no counterpart in the reference) -----------------------------
 * What anet_traj_separation finds, this term removes: B EGO trajectories are kept min_dist away from listed neighbours of an OTHER
 * set of Bo piecewise polynomials of the same order s -- other vehicles at a frozen iterate, moving obstacles.  The others are
 * constants of the objective; their buffers may be the ego buffers themselves (everything is read only).
 *   ego     coeffs [n_pieces*3*2s][ld], T [n_pieces][ld]: the layout of anet_minco_partial_grads_dev (column col holds the power
 *           k = 2s - 1 - col); t0 [batch] or NULL (= 0).
 *   others  o_coeffs [o_pieces*3*2s][o_ld], o_T [o_pieces][o_ld], o_t0 [o_batch] or NULL.  A piece with o_T = 0 is padding and is
 *           never located: others of different lengths share one buffer.
 *   lists   CSR: nbr_start int32 [batch + 1], nbr int32 [nbr_start[batch]], indices into the other set.  Ego b is penalised against
 *           nbr[nbr_start[b] .. nbr_start[b+1]), in that order; the kernel never adds or removes a neighbour (leaving b out of its
 *           own list when the sets alias is the caller's job).
 * Knots are float64 by definition, as for anet_traj_separation: K_0 = t0, K_(i+1) = K_i + T_i summed in piece order; the knots L_m
 * of an other likewise.  Sample j < res of ego piece i:
 *     sigma = (double)j / (double)res,  tau = sigma * T_i,  t = K_i + tau      one rounding each, nothing contracted into an FMA
 * The located piece of other o is the m with L_m <= t < L_(m+1) and L_(m+1) > L_m, evaluated at u = t - L_m.  t < L_0 or
 * t >= L_No: the other is not there and contributes exactly nothing (holding position is not a mode: prepend or append a constant
 * piece).
 *     r = p_b,i(tau) - p_o,m(u),   q = r_x^2 + r_y^2 + (r_z / z_scale)^2,   Phi = w smoothedL1_mu(min_dist^2 - q)
 *     J_avoid(b) = sum_i (T_i / res) sum_(j < res) sum_(o in nbr(b)) Phi        the left Riemann sum of J_pen and J_flat
 * Partial gradients with coefficients and durations independent, as anet_minco_partial_grads_dev; rt = (r_x, r_y, r_z / z_scale^2),
 * F = sum_o -2 w phi' rt,  G = sum_o (-2 w phi' rt) . v_o,m(u):
 *     dJ/dc[i][ax][k] = (T_i/res) sum_j F_ax tau^k
 *     dJ/dT_i         = (1/res) sum_j sum Phi + (T_i/res) sum_j sigma (F . v_b,i(tau) - G) + sum_(i' > i) S_i'
 *     S_i             = -(T_i/res) sum_j G      (a later knot moves every later sample in global time),    dJ/dt0_b = sum_i S_i
 * The indicator "o is there" and the piece switch of an other are differentiated almost everywhere: neither has a gradient.
 * gdC, gdT, piece_cost (may be NULL): the shapes of anet_minco_partial_grads_dev; gd_t0 [ld] (may be NULL).  accumulate = 0: they
 * are written; != 0: the kernel's complete share is added to the stored value with one unfused addition, bit for bit the sum of
 * the two separate results (anet_minco_flat_partial_grads_dev), gd_t0 included.  Lanes in [batch, ld) are never touched.
 * NaN in every output of ego b, and of b only: a duration, t0 or knot of b that is not finite, a duration of b <= 0; a neighbour
 * index outside [0, o_batch) (nothing is read for it); a duration or knot of a listed neighbour that is not finite, a negative
 * duration of one.  An ego with an empty list, or whose every term is inactive, gets exact zeros.
 * Deterministic: no atomics; the outputs of ego b have the same bits whether b is alone in the launch or one of many and whatever
 * ld and o_ld are; they may depend on the order of b's list.  No workspace.  Orders 2, 3, 4 (ANET_ERR_UNSUPPORTED otherwise);
 * ANET_ERR_INVALID: a NULL pointer other than t0, o_t0, piece_cost, gd_t0; ld < batch, o_ld < o_batch; piece counts outside
 * [1, ANET_MAX_PIECES]; a penalty outside the ranges below.  batch == 0 returns ANET_OK and touches nothing.                  */
typedef struct anet_avoid_penalty {
  double w;         /* weight, >= 0 */
  double smooth_mu; /* smoothedL1 mu in m^2, > 0 */
  double min_dist;  /* metres, > 0 */
  double z_scale;   /* > 0; 1 = sphere, > 1 = taller keep-out (downwash) */
  int32_t res;      /* samples per ego piece, >= 1 */
} anet_avoid_penalty;
int anet_minco_avoid_partial_grads_dev(anet_ctx *ctx, const anet_avoid_penalty *pen, int s, int n_pieces, int64_t batch, int64_t ld,
                                       const double *coeffs, const double *T, const double *t0 /* [batch] or NULL */, int o_pieces,
                                       int64_t o_batch, int64_t o_ld, const double *o_coeffs, const double *o_T,
                                       const double *o_t0 /* [o_batch] or NULL */, const int32_t *nbr_start, const int32_t *nbr,
                                       int accumulate, double *gdC, double *gdT, double *piece_cost /* may be NULL */,
                                       double *gd_t0 /* [ld], may be NULL */, void *stream);

/* ---- exact distance field of the voxel map, its query and its penalty of the MINCO objective (no counterpart in the reference) ----
 * The field: sd2 [n_voxels] int32 in the layout of the voxel bytes is the SIGNED SQUARED Euclidean distance in voxel units, an
 * exact integer.  blocked(v) <=> voxels[v] != 0, the predicate of anet_voxel_query_dev (dilated voxels count):
 *     free v      sd2[v] = + min over blocked u of |v - u|^2      (index coordinates)
 *     blocked v   sd2[v] = - min over free u of |v - u|^2
 * walls != 0: the voxels outside the map count as blocked too, as query answers 1 there, so the candidates of a free voxel include
 * min(x + 1, sx - x, y + 1, sy - y, z + 1, sz - z)^2; walls never count as free.  A minimum over an empty set gives
 * +ANET_DIST_NONE / -ANET_DIST_NONE; such a map is uniformly one sentinel, and with walls +ANET_DIST_NONE cannot occur.
 * Every axis <= 4096 voxels, so |sd2| <= 3 * 4096^2 < 2^31; a longer axis is ANET_ERR_UNSUPPORTED, a bad grid or a NULL pointer
 * ANET_ERR_INVALID.  Asynchronous on `stream`, deterministic, no atomics, no workspace: sd2 is the only memory written.        */
#define ANET_DIST_NONE INT32_MAX
int anet_voxel_distance_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *voxels, int walls, int32_t *sd2 /* [n_voxels] */,
                            void *stream);
/* The query: the centre value of voxel v is D(v) = scale * sgn(sd2[v]) * sqrt(|sd2[v]|) in double (+-inf for a sentinel), the centres
 * are oc + index * scale with oc = origin + 0.5 * scale.  Per axis
 *     u = (p - oc) / scale (a subtraction and an IEEE division, not contracted),  i0 = clamp(floor(u), 0, max(size - 2, 0)),
 *     f = clamp(u - i0, 0, 1),  i1 = min(i0 + 1, size - 1)
 * dist [n] is the trilinear interpolant of D at the eight corners; grad [n][3] (may be NULL) is the gradient of that interpolant
 * inside its cell divided by scale (an IEEE division; the interpolant's own sums may be fused), and 0 where f was clamped or size == 1.  BEYOND THE OUTERMOST CENTRES THE FIELD
 * THEREFORE CONTINUES AS A CONSTANT: a curve is kept inside the map by a corridor, or by `walls` with a clearance above one voxel.
 * Across a lattice plane the gradient jumps.  A sentinel corner (a uniform map): dist = +-inf, grad = 0.  A non-finite coordinate
 * gives NaN in dist and grad of that point only.  pos [n][3]; n == 0 returns ANET_OK.                                           */
int anet_voxel_distance_query_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const int32_t *sd2, const double *pos /* [n][3] */,
                                  int64_t n, double *dist /* [n] */, double *grad /* [n][3], may be NULL */, void *stream);
/* The penalty: what anet_traj_voxel_hit and getClearance find, this term removes.  Layouts, orders 2 / 3 / 4 and ANET_MAX_PIECES are
 * those of anet_minco_avoid_partial_grads_dev; the sum is the left Riemann sum of J_pen, J_flat and J_avoid.  Sample j < res of
 * piece i: sigma = (double)j / (double)res, tau = sigma * T_i, one rounding each.  With d and grad d from the query above at
 * p_i(tau):
 *     Phi = w smoothedL1_mu(clearance - d)
 *     J_obs(b)        = sum_i (T_i / res) sum_(j < res) Phi
 *     F               = -w phi' grad d
 *     dJ/dc[i][ax][k] = (T_i/res) sum_j F_ax tau^k
 *     dJ/dT_i         = (1/res) sum_j Phi + (T_i/res) sum_j sigma (F . v_i(tau))
 * There is no t0: the map does not move.  gdC, gdT, piece_cost (may be NULL): the shapes of anet_minco_partial_grads_dev.
 * accumulate = 0: they are written; != 0: the kernel's complete share is added to the stored value with one unfused addition, bit
 * for bit the sum of the two separate results.  Lanes in [batch, ld) are never touched.  No atomics, no workspace; the outputs of
 * trajectory b have the same bits alone or among many, and at any ld.  Exact zeros when every term is inactive, a map of
 * +ANET_DIST_NONE included.  All outputs of b, and only of b, are NaN when a duration of b is not finite or <= 0, a sample position
 * of b is not finite, or d = -inf (the all-blocked map).  Orders 2, 3, 4 (ANET_ERR_UNSUPPORTED otherwise); ANET_ERR_INVALID: a NULL
 * pointer other than piece_cost, ld < batch, a piece count outside [1, ANET_MAX_PIECES], a bad grid, a penalty outside the ranges
 * below.  batch == 0 returns ANET_OK and touches nothing.                                                                      */
typedef struct anet_obstacle_penalty {
  double w;         /* weight, >= 0 */
  double smooth_mu; /* smoothedL1 mu in m, > 0 */
  double clearance; /* the distance to keep in m, finite */
  int32_t res;      /* samples per piece, >= 1 */
} anet_obstacle_penalty;
int anet_minco_obstacle_partial_grads_dev(anet_ctx *ctx, const anet_obstacle_penalty *pen, int s, int n_pieces, int64_t batch,
                                          int64_t ld, const double *coeffs, const double *T, const anet_voxel_grid *grid,
                                          const int32_t *sd2, int accumulate, double *gdC, double *gdT,
                                          double *piece_cost /* may be NULL */, void *stream);

/* ---- stop within known space: speed coupled with the distance field, penalty and sampled check (no counterpart in the reference) ----
 * With the field of a map whose blocked set is occupied OR unknown (OccupancyMap::toVoxelMap(unknown = blocked)), d is the distance
 * to everything the vehicle has not seen to be free.  A vehicle that reacts for t_react and then brakes at a_brake comes to rest within
 * t_react |v| + v.v / (2 a_brake) of where it is; this term holds that ball, grown by `clearance`, inside free space, which none of
 * the corridor, obstacle and collision terms does: they bound where the vehicle is, not how fast it moves towards what it cannot see.
 * Sampling, layouts, orders, the sum and the accumulate contract are those of anet_minco_obstacle_partial_grads_dev: sample j < res
 * of piece i at sigma = (double)j / (double)res, tau = sigma * T_i, one rounding each; p, v, a the position, velocity and acceleration
 * of the piece at tau; d and grad d from anet_voxel_distance_query_dev's rule at p (the same cell rule, clamping and sentinels).
 *     s_eps = sqrt(v.v + eps^2)                            (eps = speed_eps)
 *     g     = t_react s_eps + (v.v) hb + clearance - d     (hb = 0.5 / a_brake, one IEEE division on the host)
 *     Phi   = w smoothedL1_mu(g)         phi' = smoothedL1_mu'(g)
 *     kappa = t_react / s_eps + 1 / a_brake
 *     F     = -w phi' grad d             G = w phi' kappa v
 *     J_stop(b)        = sum_i (T_i / res) sum_(j < res) Phi
 *     dJ/dc[i][ax][k]  = (T_i/res) sum_j ( F_ax tau^k + G_ax k tau^(k-1) )        (k: the power of tau this coefficient multiplies)
 *     dJ/dT_i          = (1/res) sum_j Phi + (T_i/res) sum_j sigma (F . v + G . a)
 * With t_react == 0 the terms in s_eps are absent from g and kappa (speed_eps may then be 0, and a sample at rest is no singular
 * point).  Three properties:
 *   - s_eps >= |v|, so g is never below the true excess: if every sample j < res of a piece is inactive (g <= 0), the margin of
 *     anet_traj_stop_margin_dev with the same pen is >= 0 at those samples.
 *   - v.v >= 0, so the term dominates the obstacle term of the same clearance, w and smooth_mu: a caller uses one or the other.
 *   - with a_brake = +inf and t_react = 0 it IS the obstacle term (hb = kappa = 0, G = 0).
 * gdC, gdT, piece_cost (may be NULL): the shapes of anet_minco_partial_grads_dev.  accumulate = 0: they are written; != 0: the
 * kernel's complete share is added to the stored value with one unfused addition, bit for bit the sum of the two separate results.
 * Lanes in [batch, ld) are never touched.  No atomics, no workspace; the outputs of trajectory b have the same bits alone or among
 * many, and at any ld.  Exact zeros when every sample is inactive, a map of +ANET_DIST_NONE included.  All outputs of b, and only of
 * b, are NaN when a duration of b is not finite or <= 0, a sample position, velocity or acceleration of b is not finite (v.v or
 * a.a not finite counts), or d = -inf (the all-blocked map).  Orders 2, 3, 4 (ANET_ERR_UNSUPPORTED otherwise); ANET_ERR_INVALID: a NULL pointer other than
 * piece_cost, ld < batch, a piece count outside [1, ANET_MAX_PIECES], a bad grid, a penalty outside the ranges below.  batch == 0
 * returns ANET_OK and touches nothing.                                                                                          */
typedef struct anet_stop_penalty {
  double w;          /* weight, >= 0, finite */
  double smooth_mu;  /* smoothedL1 mu in m, > 0 */
  double clearance;  /* m, finite: kept on top of the stop distance */
  double a_brake;    /* m/s^2, > 0; +inf allowed: no braking distance */
  double t_react;    /* s, >= 0, finite */
  double speed_eps;  /* m/s, >= 0, finite; > 0 required when t_react > 0 */
  int32_t res;       /* samples per piece, >= 1 */
} anet_stop_penalty;
int anet_minco_stop_partial_grads_dev(anet_ctx *ctx, const anet_stop_penalty *pen, int s, int n_pieces, int64_t batch, int64_t ld,
                                      const double *coeffs, const double *T, const anet_voxel_grid *grid, const int32_t *sd2,
                                      int accumulate, double *gdC, double *gdT, double *piece_cost /* may be NULL */, void *stream);
/* A SAMPLED check, as anet_traj_body_margin (the field is no polynomial in t: nothing bounds the value between the samples): per
 * piece the minimum over sigma = j / res, tau = sigma T_i, j = 0..res (both ends; the penalty's samples and the piece's end) of
 *     ((d(p) - clearance) - t_react |v|) - (v.v) hb,          |v| = sqrt(v.v) exactly: no eps
 * with nothing contracted.  margin >= 0: at every sample the vehicle can stop `clearance` short of the blocked set, by the ball
 * form (the direction of v is not used).  w, smooth_mu and speed_eps of `pen` are not read (speed_eps must still be >= 0, finite).  margin [N][ld]
 * (dev) / [batch][N] (host); t (local time), speed (|v|) and dist (d) at the minimiser, the first j on ties: the same shapes, each may
 * be NULL; they are diagnostics, specified by consistency as those of anet_traj_body_margin are: the expression above at the
 * piece's p(t), v(t) reproduces margin, and dist - clearance - t_react speed - speed^2 hb does.  A non-finite coefficient or
 * duration of a piece, or a duration <= 0, gives NaN in all four for that piece only.  A sentinel map gives margin = dist = +-inf.
 * The host form takes trajectory-major coeffs [batch][N][3][2s] and T [batch][N], staged as anet_traj_voxel_hit stages its own;
 * sd2 is a DEVICE pointer in both forms: the map lives there.  Errors as above (the optional outputs may be NULL).               */
int anet_traj_stop_margin_dev(anet_ctx *ctx, const anet_stop_penalty *pen, int s, int n_pieces, int64_t batch, int64_t ld,
                              const double *coeffs, const double *T, const anet_voxel_grid *grid, const int32_t *sd2, double *margin,
                              double *t, double *speed, double *dist, void *stream);
int anet_traj_stop_margin(anet_ctx *ctx, const anet_stop_penalty *pen, int s, int n_pieces, int64_t batch, const double *coeffs,
                          const double *T, const anet_voxel_grid *grid, const int32_t *sd2 /* DEVICE */, double *margin, double *t,
                          double *speed, double *dist);

/* ---- yaw trajectories: one-axis MINCO, field of view and yaw rate (no counterpart in the reference) ---------------------------
 * A quadrotor has four flat outputs; the heading psi is the fourth.  It is carried as a second, ONE-AXIS minimum-control polynomial
 * over the SAME pieces and durations as the position trajectory, with an order sy in {2, 3, 4} of its own.  psi is an unwrapped real
 * number in radians: nothing wraps it.  Yaw coefficients are [N * 2 sy][ld] (dev) / [batch][N][2 sy] (host), highest power first.
 *
 * anet_minco_solve_scalar[_dev]: anet_minco_solve[_dev] for one axis.  head, tail [c][ld], wps [N - 1][ld] (ignored at N = 1),
 * T [N][ld]; coeffs [N * 2s][ld] or NULL, energy [ld] or NULL (int (psi^(s))^2 dt).  Host: head, tail [batch][c]; wps [batch][N - 1];
 * T [batch][N]; coeffs [batch][N][2s]; energy [batch].  The arithmetic is that of one axis of anet_minco_solve_dev's lane-per-
 * trajectory kernel at ANET_MAX_PIECES pieces (no wide-spread redo in the host form).
 * anet_minco_propagate_grad_scalar_dev: anet_minco_propagate_grad_dev for one axis: gdC [N * 2s][ld], gradP [max(N - 1, 1)][ld],
 * gradT [N][ld].  gdT [N][ld] may be NULL (= zeros): the durations are shared with the position trajectory, so a joint objective
 * adds the direct dJ/dT once, on the position side, and takes only the adjoint's share from here.
 * Errors of both: those of anet_minco_solve_dev / anet_minco_propagate_grad_dev.                                                 */
int anet_minco_solve_scalar_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld, const double *head,
                                const double *tail, const double *wps, const double *T, double *coeffs /* may be NULL */,
                                double *energy /* may be NULL */, void *stream);
int anet_minco_solve_scalar(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head, const double *tail,
                            const double *wps, const double *T, double *coeffs, double *energy);
int anet_minco_propagate_grad_scalar_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld, const double *T,
                                         const double *coeffs, const double *gdC, const double *gdT /* may be NULL */, double *gradP,
                                         double *gradT, void *stream);
/* The yaw penalty.  Sampling, layouts, the sum and the accumulate contract are those of anet_minco_stop_partial_grads_dev: sample
 * j < res of piece i at sigma = (double)j / (double)res, tau = sigma * T_i, one rounding each.  h = (v_x, v_y) and (a_x, a_y) of the
 * position piece and psi, dpsi, ddpsi of the yaw piece at tau, by one Horner recurrence each; (sin psi, cos psi) from one sincos;
 * ca = cos(half_fov), computed once on the host:
 *     s_eps  = sqrt(h.h + eps^2)                                    (eps = speed_eps)
 *     g_look = ca s_eps - (h_x cos psi + h_y sin psi)   [m/s]       Phi_look = w_look smoothedL1_mu_look(g_look)
 *     g_rate = dpsi^2 - max_rate^2                      [(rad/s)^2] Phi_rate = w_rate smoothedL1_mu_rate(g_rate)
 *     G = w_look phi'_look (ca h / s_eps - (cos psi, sin psi))      (x and y only; the z rows receive nothing)
 *     A = w_look phi'_look (h_x sin psi - h_y cos psi)              R = w_rate phi'_rate 2 dpsi
 *     J_yaw(b)           = sum_i (T_i / res) sum_(j < res) (Phi_look + Phi_rate)  +  w_energy sum_i int_0^T_i (psi^(sy))^2 dt
 *     dJ/dc [i][ax][k]   = (T_i / res) sum_j G_ax k tau^(k-1)                              ax in {x, y}
 *     dJ/dcy[i][k]       = (T_i / res) sum_j (A tau^k + R k tau^(k-1))  +  the effort term's closed form
 *     dJ/dT_i            = (1/res) sum_j (Phi_look + Phi_rate) + (T_i/res) sum_j sigma (G . a_xy + A dpsi + R ddpsi)
 *                          + w_energy (psi^(sy)(T_i))^2
 * Two properties: s_eps >= |h| and ca >= 0, so g_look is never below the true excess ca |h| - h.u: a sample that is inactive in
 * the look term has its horizontal velocity inside the field of view (which is why half_fov > pi/2 is ANET_ERR_INVALID); and the
 * look term scales with speed: at rest any heading is free, up to the ca eps the smoothing leaves.
 * gdC [N*3*2s][ld], gdT [N][ld], piece_cost [N][ld] (may be NULL; the effort of a piece included) are shared with the position
 * terms: accumulate = 0 writes them (all of gdC, zeros in the z rows); != 0 adds the kernel's complete share to the stored value
 * with one unfused addition.  gdCy [N*2sy][ld] is always overwritten.  A weight of 0 skips its term (its mu, and speed_eps for
 * w_look, are then not read); all three 0 give exact zeros.  Lanes in [batch, ld) are never touched.  No atomics, no workspace; the
 * outputs of trajectory b have the same bits alone or among many, and at any ld.  All outputs of b, and only of b, are NaN when a
 * duration of b is not finite or <= 0, a position or yaw coefficient of b is not finite, or a sample value is not finite.
 * Orders s, sy outside 2..4: ANET_ERR_UNSUPPORTED.  ANET_ERR_INVALID: a NULL pointer other than piece_cost, ld < batch, a piece
 * count outside [1, ANET_MAX_PIECES], a penalty outside the ranges below.  batch == 0 returns ANET_OK and touches nothing.         */
typedef struct anet_yaw_penalty {
  double w_look, mu_look;    /* weight, >= 0, finite; smoothedL1 mu in m/s, > 0 when w_look > 0                 */
  double half_fov;           /* horizontal half field of view alpha in rad, 0 < alpha <= pi/2                  */
  double speed_eps;          /* smoothing of |v_xy| in m/s, > 0 when w_look > 0                                */
  double w_rate, mu_rate;    /* weight; mu in (rad/s)^2, > 0 when w_rate > 0                                   */
  double max_rate;           /* rad/s, > 0, +inf allowed                                                       */
  double w_energy;           /* weight of int (psi^(sy))^2 dt, >= 0; 0: the term is skipped                    */
  int32_t res;               /* samples per piece, >= 1                                                        */
} anet_yaw_penalty;
int anet_minco_yaw_partial_grads_dev(anet_ctx *ctx, const anet_yaw_penalty *pen, int s, int sy, int n_pieces, int64_t batch, int64_t ld,
                                     const double *coeffs, const double *ycoeffs, const double *T, int accumulate, double *gdC,
                                     double *gdCy, double *gdT, double *piece_cost /* may be NULL */, void *stream);
/* A SAMPLED check, as anet_traj_stop_margin (nothing bounds the angle between the samples): per piece, over sigma = j / res,
 * tau = sigma T_i, j = 0..res (the penalty's samples and the piece's end), among the samples with |h| >= v_min (m/s, >= 0, finite),
 *     margin = half_fov - |atan2(h x u, h . u)|,   u = (cos psi, sin psi),  h x u = h_x sin psi - h_y cos psi,  |h| exact, no eps
 * with nothing contracted: the first minimum over j, and its local time in t.  A piece with no such sample reports +inf and time
 * 0.  A sample at rest (|h| = 0, which counts only at v_min = 0) has no direction: its angle is 0.  rate: the largest |dpsi| over all
 * res + 1 samples.  margin, t, rate [N][ld] (dev) / [batch][N] (host); t and rate may be
 * NULL.  Only half_fov and res of `pen` are read.  A non-finite coefficient (position or yaw) or duration of a piece, or a
 * duration <= 0, gives NaN in all three for that piece only.  The host form takes trajectory-major coeffs [batch][N][3][2s],
 * ycoeffs [batch][N][2sy] and T [batch][N].  Errors as above.                                                                    */
int anet_traj_yaw_margin_dev(anet_ctx *ctx, const anet_yaw_penalty *pen, double v_min, int s, int sy, int n_pieces, int64_t batch,
                             int64_t ld, const double *coeffs, const double *ycoeffs, const double *T, double *margin, double *t,
                             double *rate, void *stream);
int anet_traj_yaw_margin(anet_ctx *ctx, const anet_yaw_penalty *pen, double v_min, int s, int sy, int n_pieces, int64_t batch,
                         const double *coeffs, const double *ycoeffs, const double *T, double *margin, double *t, double *rate);
/* anet_traj_flat_states[_dev] with the yaw: the same piece location and the same 11 fields per query, with psi, dpsi evaluated from
 * the yaw piece at the same local time and the flatness map taken with them (anet_flat_forward with psi, dpsi given).  A zero yaw
 * polynomial reproduces anet_traj_flat_states.                                                                                  */
int anet_traj_states_yaw_dev(anet_ctx *ctx, const anet_flat_params *params, int s, int sy, int n_pieces, int64_t batch, int64_t ld,
                                  const double *coeffs, const double *ycoeffs, const double *T, int nq, const double *tq, double *out,
                                  void *stream);
int anet_traj_states_yaw(anet_ctx *ctx, const anet_flat_params *params, int s, int sy, int n_pieces, int64_t batch,
                              const double *coeffs, const double *ycoeffs, const double *T, int nq, const double *tq, double *out);

/* ---- whole-body corridor terms: body vertices through the flatness attitude ----------------------------------------------
 * Every other corridor term holds a_r . p(t) <= h_r for the POINT p.  Here the vehicle is a body-fixed convex polytope with vertices
 * b_k, k < K = n_verts <= ANET_MAX_BODY_VERTS, in the body frame in metres, shared by the batch; its attitude is the one the
 * trajectory itself implies, q(t) = the quaternion of the flatness map (anet_flat_forward with psi = dpsi = 0, as every
 * trajectory-level flatness entry point has it) at v(t), a(t), and each vertex  p(t) + R(q(t)) b_k  is held inside the corridor (the
 * SE(3) constraint of upstream GCOPTER; no counterpart in the reference tree).  A flat vehicle can so roll to pass a slot narrower
 * than its span.  R(q), q = (w, v), is the homogeneous quadratic form
 *     R b = (w^2 - v.v) b + 2 (v.b) v + 2 w (v x b),
 * and for g = a . R(q) b:  dg/dw = 2 w (a.b) + 2 a.(v x b),  dg/dv = -2 (a.b) v + 2 (v.b) a + 2 (a.v) b + 2 w (b x a).  q(t) stays on
 * the unit sphere and the adjoint of the flatness map applies the exact Jacobian of q, so the radial part of the quaternion's
 * gradient is annihilated: any extension of R off the sphere gives the same composed gradient.  The penalty is
 *     J_body = sum_i (T_i/res) sum_(j < res) sum_r sum_k  w_body smoothedL1_mu( a_r . (p(t_j) + R(q(t_j)) b_k) - h_r ),  t_j = j T_i / res,
 * r over the rows of hpolys[i] in the layout of anet_minco_partial_grads_dev (all-zero rows are padding, M = poly_rows in
 * [1, ANET_MAX_POLY_ROWS]).  A sample of piece i is tested against polytope i ONLY: next to a junction, where the body already
 * reaches into the next polytope, this is conservative (the body is held inside the piece's own polytope), as upstream's SE(3)
 * penalty is.                                                                                                                   */
#define ANET_MAX_BODY_VERTS 16
typedef struct anet_body_penalty {
  double w_body;    /* weight                                                */
  double smooth_mu; /* smoothedL1 mu in m, > 0                               */
  int32_t res;      /* samples per piece, >= 1 (and within the basis table)  */
  int32_t poly_rows; /* M: rows per polytope in `hpolys`, [1, ANET_MAX_POLY_ROWS] */
  int32_t n_verts;  /* K, [1, ANET_MAX_BODY_VERTS]                           */
  int32_t pad;
  double verts[ANET_MAX_BODY_VERTS][3]; /* b_k, finite; entries behind n_verts are not read */
} anet_body_penalty;
/* Partial gradients of J_body w.r.t. the coefficients and durations; layouts and the accumulate contract are exactly those of
 * anet_minco_flat_partial_grads_dev: accumulate = 0: gdC, gdT, piece_cost (may be NULL) are written; != 0: the share is formed
 * completely and added with one unfused addition, bit for bit the sum of the two separate results.  Lanes in [batch, ld) are never
 * touched.  Where no term is active (the body far inside its corridor) cost and gradients are exactly 0; a non-finite coefficient,
 * duration or row field of a piece makes that piece's outputs NaN and no other's.  Orders 3 and 4
 * (ANET_ERR_UNSUPPORTED otherwise).  ANET_ERR_INVALID: n_verts outside [1, ANET_MAX_BODY_VERTS], res < 1 or above the basis table's
 * limit (4096), poly_rows outside [1, ANET_MAX_POLY_ROWS], a non-finite vertex,
 * smooth_mu <= 0, hpolys or another pointer except piece_cost NULL, ld < batch.  batch == 0 returns ANET_OK after the argument checks. */
int anet_minco_body_partial_grads_dev(anet_ctx *ctx, const anet_flat_params *params, const anet_body_penalty *pen, int s,
                                      int n_pieces, int64_t batch, int64_t ld, const double *coeffs, const double *T,
                                      const double *hpolys, int accumulate, double *gdC, double *gdT, double *piece_cost,
                                      void *stream);
/* A SAMPLED check, as anet_traj_flat_extrema (the attitude is no polynomial in t: nothing bounds the value between the samples):
 * per piece the maximum of  a_r . (p(t) + R(q(t)) b_k) - h_r  over t = j T_i / res, j = 0..res (both ends included), the non-padding
 * rows of hpolys[i] and the vertices; only w_body and smooth_mu of `pen` are not used.  margin [N][ld] (dev) / [batch][N] (host);
 * t (local time), row, vert (int32): the same shapes, each may be NULL; they are diagnostics, specified by consistency as row and
 * t of anet_traj_row_margin are: a_row . (p(t) + R(q(t)) b_vert) - h_row reproduces margin.  A piece with no row gives -inf (row,
 * vert -1, t 0); a non-finite coefficient, duration or row field of that piece gives NaN (the same), for that piece only.
 * hpolys: [N*M*4][ld] (dev) / [batch][N][M][4] (host).  Orders 2, 3, 4.                                                        */
int anet_traj_body_margin_dev(anet_ctx *ctx, const anet_flat_params *params, const anet_body_penalty *pen, int s, int n_pieces,
                              int64_t batch, int64_t ld, const double *coeffs, const double *T, const double *hpolys,
                              double *margin, double *t, int32_t *row, int32_t *vert, void *stream);
int anet_traj_body_margin(anet_ctx *ctx, const anet_flat_params *params, const anet_body_penalty *pen, int s, int n_pieces,
                          int64_t batch, const double *coeffs, const double *T, const double *hpolys, double *margin, double *t,
                          int32_t *row, int32_t *vert);

/* ---- front-end route on the voxel map: sfc_gen::planPath ----------------------------------------------------------------
 * A collision-free polyline from s to g and its length, by a shortest-path field on the grid, a walk back along it and a
 * line-of-sight shortcut; exact and deterministic (no time budget).  box = {lb[3], hb[3]} (host array), the planner's
 * [getOrigin(), getCorner()] by default.
 *   free voxel  byte 0 and its centre posI2D(id) = id * scale + (origin + 0.5 scale) inside [lb, hb]; a position is free
 *               when query(pos) == 0 and its voxel is free.
 *   graph       26 neighbours, weights 10 / 14 / 17 (face / edge / corner); a move by d is an edge only when every voxel
 *               cur + e, e_i in {0, d_i}, is free (no corner cutting).  The field is uint32 cost-to-come, UINT32_MAX
 *               unreached; grids with 17 * voxels >= 2^32 - 1 are refused (ANET_ERR_UNSUPPORTED).
 *   target      g when g is free and reached (EXACT), else the centre of the reached voxel nearest to g, least squared
 *               distance in double, ties to the lowest id (APPROXIMATE).  A start that is not free: INVALID_START, cost
 *               INFINITY, no points.
 *   walk        from the target voxel, the first neighbour in the order dz, dy, dx in {-1, 0, 1} with d[n] + w == d[cur]
 *               and an edge; waypoints s, the centres of the walk's voxels after the start's, the target (g when EXACT);
 *               s and g in one voxel give [s, g].
 *   shortcut    greedy from W_0: the next waypoint is the LARGEST k whose segment is visible (a 3-D DDA visits only free
 *               voxels; where crossings of several axes tie, the whole block of that step is checked).
 *   cost        the sum of the final segments' lengths, in path order.                                                   */
enum { ANET_PATH_EXACT = 0, ANET_PATH_APPROXIMATE = 1, ANET_PATH_INVALID_START = 2 };
/* bytes of device workspace for n_problems searches on `grid` (fields, walks, activity words); -1: bad or too large grid */
int64_t anet_voxel_path_workspace(const anet_voxel_grid *grid, int64_t n_problems);
/* the cost-to-come fields of the starts [n_problems][3] (device) into `work`, by rounds of tile relaxation; *rounds (host)
 * = the rounds that had an active tile.  SYNCHRONISES `stream` (it reads a device word every 8 rounds to stop).         */
int anet_voxel_path_field_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *voxels, const double box[6],
                              const double *starts, int64_t n_problems, void *work, int32_t *rounds, void *stream);
/* problem b's field [n_voxels] uint32 inside `work` (no device access)                                                 */
int anet_voxel_path_field_ptr(const anet_voxel_grid *grid, void *work, int64_t b, uint32_t **field);
/* target, walk, shortcut and cost for (starts[b], goals[b]) on the fields of the last anet_voxel_path_field_dev on `work`
 * (same grid, voxels, box and starts): paths [n_problems][max_points][3] get min(count, max_points) points, n_points[b]
 * the true count (call again with a larger max_points when it exceeds it; max_points = 0 writes no points), cost[b],
 * status[b] (ANET_PATH_*, or -1 when the fields do not belong to these starts).  Device outputs, asynchronous.          */
int anet_voxel_path_extract_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *voxels, const double box[6],
                                const double *starts, const double *goals, int64_t n_problems, void *work, int64_t max_points,
                                double *paths, int32_t *n_points, double *cost, int32_t *status, void *stream);

/* ---- the time-allocation network (network/utils/learning/minsnap_network_conv_lstm.py:37-88, 114-187) ---- */
/* Inference of the exported model the planner loads (LearningPlanner::loadModel / callModel), batched, all arithmetic in float32:
 *   state  (9, 2)     -> Conv1d(9->8, k 3, pad 1) -> ReLU -> MaxPool1d(2) -> Linear(8->6)
 *   hpolys (50, 4, L) -> Conv2d(50->16, 3x3, pad 1) -> ReLU -> MaxPool2d(2) -> MaxPool2d(2) -> Flatten -> Linear(->32)
 *   x = [6 | 32], the same at every step; h = c = 0; L steps of an LSTM cell (hidden 256, gates i, f, g, o);
 *   tf_k = w_t . h + b_t, stop_k = sigmoid(w_s . h + b_s); count = 1 + first k with stop_k > threshold (L if none);
 *   times = tf[:count], zero after.  The export stops at threshold 0.5, forward_batch at 0.42.
 * The handle owns the device copy of the weights (the recurrent matrices repacked into the order the kernels read) and a grow-only
 * workspace; it belongs to the context it was created on and is destroyed by its owner (before or after the context).
 * weights: ANET_TIMENET_TENSORS host pointers, float32, natural (state-dict) shapes, in this order:
 *   state_input_module.0.weight (8,9,3), .0.bias (8), .4.weight (6,8), .4.bias (6),
 *   hpoly_input_module.0.weight (16,50,3,3), .0.bias (16), .5.weight (32, 16 (L/4)), .5.bias (32),
 *   output_module.weight_ih_l0 (1024,38), weight_hh_l0 (1024,256), bias_ih_l0 (1024), bias_hh_l0 (1024),
 *   tfs_output_layer.weight (1,256), .bias (1), stop_token_output_layer.0.weight (1,256), .0.bias (1).
 * seq_len must be 5 or 10 and hidden 256 (ANET_ERR_UNSUPPORTED otherwise).                                                       */
#define ANET_TIMENET_TENSORS 16
typedef struct anet_timenet anet_timenet;
int anet_timenet_create(anet_ctx *ctx, int seq_len, int hidden, const float *const *weights, anet_timenet **out);
void anet_timenet_destroy(anet_timenet *net);
/* bytes of device memory the handle holds (weights, workspace, staging of the host entry point) */
int64_t anet_timenet_device_bytes(const anet_timenet *net);
/* flags of the forward calls */
#define ANET_TIMENET_KEEP_PADDING 1 /* do not skip zero rows / zero polytopes (the results are the same bits; kept for the test) */
#define ANET_TIMENET_FORM_SINGLE 2  /* one workgroup per problem, a thread per hidden unit, whatever the batch                   */
#define ANET_TIMENET_FORM_TILE 4    /* one workgroup per 32 problems on the f32 matrix instruction, whatever the batch           */
/* without a FORM flag: batches up to this take the single form, larger ones the tile form */
#define ANET_TIMENET_SINGLE_MAX 1024
/* state [batch][9][2], hpolys [batch][50][4][seq_len] float32 in the reference's layout (the tensors of callModel, stacked);
 * times [batch][seq_len], count [batch]; tf, stop [batch][seq_len] (all steps, whatever the count) or NULL.
 * _dev: device pointers, asynchronous on `stream`, no synchronisation, and no allocation after the first call at a batch size.
 * The two forms agree in count and within the tolerance of DESIGN.md 8g, not bit for bit.                                        */
int anet_timenet_forward_dev(anet_ctx *ctx, anet_timenet *net, int seq_len, int64_t batch, const float *state, const float *hpolys,
                             double threshold, int flags, float *times, float *tf, float *stop, int32_t *count, void *stream);
int anet_timenet_forward(anet_ctx *ctx, anet_timenet *net, int seq_len, int64_t batch, const float *state, const float *hpolys,
                         double threshold, int flags, float *times, float *tf, float *stop, int32_t *count);

/* ---- multi-GPU: all-gather of the per-trajectory costs over RCCL / xGMI --------------------------- */
/* Trajectories are independent, so a batch shards contiguously across GPUs (one process and one
 * context per GPU) with no collective inside a solve; the only exchange the path has is this
 * all-gather of costs (8 B per trajectory: latency-bound).  RCCL is loaded at run time (dlopen of
 * librccl.so, override with ANET_RCCL_PATH) so single-GPU users carry no dependency.
 * Usage: rank 0 calls anet_comm_unique_id and ships the 128 bytes to the other ranks by any side
 * channel (file, socket, MPI, a torch.distributed store), then every rank calls anet_comm_init.       */
#define ANET_COMM_ID_BYTES 128
int anet_comm_unique_id(anet_ctx *ctx, unsigned char id[ANET_COMM_ID_BYTES]);
int anet_comm_init(anet_ctx *ctx, int nranks, int rank, const unsigned char id[ANET_COMM_ID_BYTES]);
/* recv[r*count + i] = rank r's send[i]; device pointers; asynchronous on `stream`. */
int anet_comm_allgather_costs_dev(anet_ctx *ctx, const double *send, double *recv, int64_t count,
                                  void *stream);
int anet_comm_destroy(anet_ctx *ctx);

/* ---- corridor-constrained MINCO L-BFGS: waypoints as vertex weights of corridor overlaps ---------- */
/* Waypoint w (0 .. N-2) of a problem is a convex combination of the vertices v_0 .. v_{k-1} of overlap(polytope w, polytope
 * w + 1), padded with zero rows to max_verts = K: P_w = (sum_j xi_j^2 v_j) / S, S = sum_j xi_j^2, with K free variables xi per
 * waypoint (upstream GCOPTER's forwardP; allocnet_amd/csrc/sfc_param_kernels.h states the transform, its gradient, the norm
 * restriction w_norm max(S - 1, 0)^3 and the inverse once).  Every iterate of the optimiser over (xi, tau) so has its junctions
 * inside both polytopes they join.  Device arrays are batch-minor with the common row stride ld:
 *   xi [(N-1) K][ld], row w K + j;  verts [(N-1) K 3][ld], row (w K + j) 3 + a;  count, status [(N-1)][ld] int32;
 *   wps, grad_p [3 (N-1)][ld], row 3 w + a (what anet_minco_cost_grad_dev takes and returns);  norm [3 (N-1)][ld]: rows w hold
 *   1 / S, rows (N-1) + w the norm cost of waypoint w, rows 2 (N-1) + w its gradient factor 6 w_norm max(S - 1, 0)^2.
 * anet_sfc_overlap_vertices_dev: hpolys [N poly_rows 4][ld] as for anet_minco_cost_grad_dev (a.x <= b, zero rows padding),
 * 2 poly_rows <= 128; the (N-1) batch stacked pairs go through anet_polytope_vertices_dev (same epsilon, same order of the
 * vertices).  status: ANET_POLYTOPE_OK, _SKIPPED (no interior: count 0) or _TRUNCATED (more than max_verts vertices: the first
 * max_verts are kept -- still a convex subset of the overlap -- and count is clamped to max_verts).  Slots behind count are zero.
 * work: anet_sfc_overlap_workspace() doubles.
 * anet_sfc_forward_p_dev: xi -> wps, norm.  anet_sfc_backward_grad_p_dev: grad_xi_j = 2 xi_j ((v_j - P_w) . grad_p_w) / S + the
 * norm term, from the wps and norm rows the forward call left; cost ([ld] or NULL): the problem's norm costs are added to it.
 * anet_sfc_backward_p_dev: xi of unit norm per waypoint minimising |P_w(xi) - wps_w|^2 from the vertex mean (L-BFGS, mem_size 8,
 * g_epsilon 0, past 3, delta 1e-16, at most 200 evaluations) and residual [(N-1)][ld] = |P_w(xi) - wps_w|: positive for a point
 * outside the overlap, +inf (xi = 0) for a waypoint without vertices.  work: anet_sfc_backward_p_workspace() doubles.          */
int64_t anet_sfc_overlap_workspace(int n_pieces, int64_t batch, int poly_rows, int max_verts);
int anet_sfc_overlap_vertices_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int poly_rows, const double *hpolys,
                                  double epsilon, int max_verts, double *verts, int32_t *count, int32_t *status, double *work,
                                  void *stream);
int anet_sfc_forward_p_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int max_verts, const double *xi,
                           const double *verts, double w_norm, double *wps, double *norm, void *stream);
int anet_sfc_backward_grad_p_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int max_verts, const double *xi,
                                 const double *verts, const double *wps, const double *norm, const double *grad_p,
                                 double *grad_xi, double *cost, void *stream);
int64_t anet_sfc_backward_p_workspace(int n_pieces, int max_verts, int64_t ld);
int anet_sfc_backward_p_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int max_verts, const double *verts,
                            const int32_t *count, const double *wps, double *xi, double *residual, double *work, void *stream);

/* anet_lbfgs_minco_dev over x = (xi rows, tau rows), n = (N-1) max_verts + (N with ANET_OPT_TIMES): the lockstep shape
 * (ANET_OPT_LOCKSTEP is implied), each evaluation forward_p -> cost + gradient -> backward_grad_p.  xi and T are read and written
 * in place (start in, result out); wps_out [3 (N-1)][ld] receives P(xi) of the final iterate, coeffs_out (or NULL) its
 * coefficients.  count / overlap_status ([(N-1)][ld], the latter may be NULL) are anet_sfc_overlap_vertices_dev's.  A problem
 * with a waypoint of count < 2 or overlap status ANET_POLYTOPE_SKIPPED does not run: status ANET_SFC_NO_OVERLAP, zero counters,
 * cost NaN, xi and T untouched.  min_duration and the cancel word as for anet_lbfgs_minco_bounded_dev.  The cost includes the
 * norm restriction (0 while every S <= 1).  work: anet_sfc_workspace() doubles.                                                */
#define ANET_SFC_NO_OVERLAP (-2048)
int64_t anet_sfc_workspace(int s, int n_pieces, int max_verts, int64_t ld, const anet_lbfgs_params *params);
int anet_lbfgs_minco_sfc_dev(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, int64_t ld, const double *head,
                             const double *tail, double *xi, double *T, const double *verts, const int32_t *count,
                             const int32_t *overlap_status, int max_verts, const double *hpolys, const anet_penalty *pen,
                             const anet_lbfgs_params *params, int opt_flags, int max_evals, double min_duration, double w_norm,
                             double *work, double *cost, double *wps_out, double *coeffs_out, int32_t *status, int32_t *iters,
                             int32_t *evals, void *stream);
/* The host-staged form: hpolys [batch][N][poly_rows][4] (pen->poly_rows; pen is required), wps_start [batch][N-1][3] or NULL
 * (NULL: every waypoint starts at the mean of its overlap's vertices).  Enumerates the overlaps (epsilon), runs backward_p on
 * the start waypoints, then the optimisation.  Out: wps_out [batch][N-1][3], T in place, cost, coeffs_out [batch][N][3][2s] or
 * NULL, status / iters / evals, residual [batch][N-1] (backward_p's distances; 0 with wps_start NULL), overlap_status
 * [batch][N-1] and xi_out [batch][(N-1) max_verts] (each may be NULL).                                                          */
int anet_lbfgs_minco_sfc(anet_ctx *ctx, int s, int c, int n_pieces, int64_t batch, const double *head, const double *tail,
                         const double *wps_start, double *T, const double *hpolys, const anet_penalty *pen,
                         const anet_lbfgs_params *params, int opt_flags, int max_evals, double min_duration, double w_norm,
                         double epsilon, int max_verts, double *wps_out, double *cost, double *coeffs_out, int32_t *status,
                         int32_t *iters, int32_t *evals, double *residual, int32_t *overlap_status, double *xi_out);

/* ---- shortest route through a corridor: upstream GCOPTER's getShortestPath in the same variables ---------- */
/* P_0 = start and P_N = goal are fixed; P_w(xi), w = 1 .. N-1, is the transform above on the vertices of overlap(polytope w-1,
 * polytope w).  The objective (stated once in allocnet_amd/csrc/sfc_path_kernels.h, one launch per evaluation) is
 *   L(xi) = sum_{i=0}^{N-1} sqrt(|P_{i+1} - P_i|^2 + eps^2) + w_norm sum_w max(S_w - 1, 0)^3,      eps in metres,
 * summed per problem in a fixed order (legs ascending, then norm terms ascending).  anet_sfc_shortest_path_dev minimises it by the
 * lockstep L-BFGS over x = the xi rows, n = (N-1) max_verts.  start, goal [3][ld]; verts, count, overlap_status (may be NULL) are
 * anet_sfc_overlap_vertices_dev's; xi [(N-1) K][ld] in and out, from_mean != 0: xi is first set to the vertex mean
 * xi_j = 1 / sqrt(count).  params NULL: anet_lbfgs_default_params (mem_size 8, past 3, delta 1e-6, g_epsilon 1e-5); max_evals <= 0:
 * ANET_SFC_PATH_MAX_EVALS.  Out: wps_out [3 (N-1)][ld] = anet_sfc_forward_p_dev of the returned xi, length_out [ld] (or NULL) the
 * UNSMOOTHED length sum_i |P_{i+1} - P_i| of start, wps_out, goal, cost_out [ld] (or NULL) the objective, status / iters / evals
 * as for anet_lbfgs_minco_sfc_dev.  A problem with a waypoint of count < 2 or overlap status ANET_POLYTOPE_SKIPPED does not run:
 * status ANET_SFC_NO_OVERLAP, zero counters, length and cost NaN, xi untouched.  The cancel word is honoured.
 * work: anet_sfc_shortest_path_workspace() doubles -- the optimiser's state (x rows first, then the gradient rows), then the norm
 * rows of the final anet_sfc_forward_p_dev.                                                                                     */
#define ANET_SFC_PATH_MAX_EVALS 400
/* one evaluation alone: cost [ld] = L(xi), grad_xi [(N-1) K][ld] = dL/dxi (one launch of k_sfc_path_eval) */
int anet_sfc_path_cost_grad_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int max_verts, const double *start,
                                const double *goal, const double *xi, const double *verts, double eps, double w_norm, double *cost,
                                double *grad_xi, void *stream);
int64_t anet_sfc_shortest_path_workspace(int n_pieces, int max_verts, int64_t ld, const anet_lbfgs_params *params);
int anet_sfc_shortest_path_dev(anet_ctx *ctx, int n_pieces, int64_t batch, int64_t ld, int max_verts, const double *start,
                               const double *goal, const double *verts, const int32_t *count, const int32_t *overlap_status,
                               double *xi, int from_mean, double eps, double w_norm, const anet_lbfgs_params *params, int max_evals,
                               double *work, double *wps_out, double *length_out, double *cost_out, int32_t *status, int32_t *iters,
                               int32_t *evals, void *stream);
/* The host-staged form: hpolys [batch][N][poly_rows][4] (rows a.x <= b, zero rows padding), start, goal [batch][3].  Enumerates
 * the overlaps (epsilon, max_verts) and runs the route from the vertex mean on one staging buffer.  Out: wps_out [batch][N-1][3],
 * length_out [batch], status / iters / evals, overlap_status [batch][N-1] and xi_out [batch][(N-1) max_verts] (zeros for a
 * problem that did not run); each but wps_out may be NULL.                                                                       */
int anet_sfc_shortest_path(anet_ctx *ctx, int n_pieces, int64_t batch, int poly_rows, const double *hpolys, const double *start,
                           const double *goal, double epsilon, int max_verts, double eps, double w_norm,
                           const anet_lbfgs_params *params, int max_evals, double *wps_out, double *length_out, int32_t *status,
                           int32_t *iters, int32_t *evals, int32_t *overlap_status, double *xi_out);

/* ---- occupancy from sensor scans: a log-odds grid by ray carving, depth unprojection, first hit of a segment (no counterpart in the
 * reference, whose mapCallBack stamps a finished world cloud; csrc/occupancy_kernels.h) ------------------------------------------
 * The grid: logodds [n_voxels] int16 on the DEVICE in the voxel order of anet_voxel_grid.  ANET_OCC_UNKNOWN marks a voxel no ray
 * has crossed; every other value is a clamped integer log-odds in units the caller chooses (lo <= L <= hi).
 * THE WALK of a segment o -> q, shared by the scan and the ray query:
 *   cell(p)_c = floor((p_c - origin_c) / scale).  This is NOT the truncation of anet_voxel_set_occupied_dev / anet_voxel_query_dev:
 *   the two agree inside the map, but a point up to one voxel below the origin is OUTSIDE here (cell -1), inside cell 0 there.
 *   Per axis dir = q_c - o_c, step = sign(dir), bnd = (double)(cur_c + (step > 0)) * scale + origin_c, tmax = (bnd - o_c) / dir,
 *   tdel = scale / |dir| (both +inf for dir == 0).  While cur != end: tm = the least tmax over the axes with cur_c != end_c; every
 *   such axis with tmax <= tm + 1e-9 steps, all together, and tmax += tdel; the new cell is visited.  Where crossings tie only the
 *   diagonal cell is visited, not the other cells of the block (for carving the conservative side).  Visited: the start cell and
 *   each cell after a step, the last being the end cell.  Cells outside the map are walked through and not touched.  Every
 *   floating-point operation is rounded on its own (no fused multiply-add), so the cells are reproducible bit for bit.
 * No input makes a walk longer than 3 * (65536 + 1) steps: the range bounds below, and the refusals of the ray query, see to it. */
#define ANET_OCC_UNKNOWN (-32768)
typedef struct anet_occupancy_params {
  int32_t hit;      /* added to a voxel a return fell in, > 0                                        */
  int32_t miss;     /* added to a voxel a ray passed through, < 0                                    */
  int32_t lo, hi;   /* the clamps: -32767 <= lo < 0 < hi <= 32767                                    */
  double min_range; /* returns closer than this are dropped whole; finite, >= 0                      */
  double max_range; /* rays are cut here and then only carve; finite, > 0, max_range / scale <= 65536 */
} anet_occupancy_params;
/* bytes of the device workspace of a grid: one mark byte per voxel (rounded up), all zero between calls; -1: bad grid */
int64_t anet_occupancy_workspace(const anet_voxel_grid *grid);
/* every voxel ANET_OCC_UNKNOWN, every mark 0: call once before the first scan (it is what makes `work` valid) */
int anet_occupancy_reset_dev(anet_ctx *ctx, const anet_voxel_grid *grid, int16_t *logodds, void *work, void *stream);
/* One scan from ONE sensor origin (world frame).  records: those of anet_voxel_set_occupied_dev (n of them, `stride` bytes apart,
 * three float32 (f64 == 0) or float64 (f64 == 1) world coordinates first).  Per record p: a non-finite coordinate skips it;
 * d = p - o, len = sqrt(dx dx + dy dy + dz dz) summed left to right; len < min_range skips it; len > max_range TRUNCATES the ray to
 * q = o + d * (max_range / len), else q = p.  The walk o -> q marks every visited cell but the end MISS and the end cell HIT, or
 * MISS when the ray was truncated.  Then every marked voxel is updated ONCE, however many rays marked it, a hit mark winning
 * over any number of miss marks:  hit: L = min((L == UNKNOWN ? 0 : L) + hit, hi);  miss only: L = max((L == UNKNOWN ? 0 : L) + miss, lo)
 * in int32.  The marks are cleared again.  The result is a function of the SET of rays: permuting or duplicating records changes
 * nothing.  The update runs over the cells within ceil(max_range / scale) + 1 of the sensor's cell, cut to the map, not over the grid.
 * ANET_ERR_INVALID, with the grid untouched: a bad grid or params, a non-finite origin or one whose cell index reaches 2^30 in
 * magnitude on an axis, n < 0, a bad stride, a NULL or misaligned pointer.  Asynchronous on `stream`.                           */
int anet_occupancy_integrate_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const anet_occupancy_params *params, int16_t *logodds,
                                 const double origin[3], const void *records, int64_t n, int64_t stride, int f64, void *work,
                                 void *stream);
/* the same with the records in HOST memory (logodds and work stay on the DEVICE: the map lives there); returns when it is done */
int anet_occupancy_integrate(anet_ctx *ctx, const anet_voxel_grid *grid, const anet_occupancy_params *params, int16_t *logodds,
                             const double origin[3], const void *records, int64_t n, int64_t stride, int f64, void *work);
/* The hand-over to the byte grid: voxels[v] = 1 when L != UNKNOWN and L >= occ, 1 when L == UNKNOWN and unknown_blocked != 0, else 0.
 * Every byte is written; the bytes are the input of dilate, surface, path, distance and hit.                                    */
int anet_occupancy_to_voxels_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const int16_t *logodds, int32_t occ, int unknown_blocked,
                                 uint8_t *voxels, void *stream);
/* Depth image -> world points.  depth: DEVICE, row-major [height][width], float32 metres (u16 == 0) or uint16 (u16 == 1).  Kept
 * pixels: (u, v) with u, v in {0, step, 2 step, ...}, row-major, n = ceil(width / step) * ceil(height / step) of them.  K = {fx, fy,
 * cx, cy}, R [9] row-major and t [3] the camera-to-world pose (HOST).  Per pixel, every operation rounded on its own:
 *   z = depth * depth_scale;  x = (u - cx) / fx * z;  y = (v - cy) / fy * z;  world_r = (R[r][0] x + R[r][1] y) + R[r][2] z + t[r]
 * A pixel with z non-finite, z <= min_depth or z > max_depth gives a NaN row, which the integrate call skips.
 * points: DEVICE double [n][3], ready for anet_occupancy_integrate_dev (stride 24, f64 = 1).                                    */
int anet_depth_to_points_dev(anet_ctx *ctx, const void *depth, int u16, int width, int height, int step, double depth_scale,
                             const double K[4], const double R[9], const double t[3], double min_depth, double max_depth,
                             double *points, void *stream);
/* First hit along segments on the byte grid: origins, ends [n][3] DEVICE doubles.  voxel[i]: the linear index of the first visited
 * in-bounds cell with a byte != 0, by the walk above; t[i] (may be NULL): the parameter in [0, 1] at which that cell was entered --
 * 0 when the start cell is blocked, otherwise the tm of the step that entered it.  No blocked cell met: ANET_HIT_FREE and t = 1.
 * ANET_HIT_INVALID with t = NaN: a non-finite coordinate, a cell index of 2^30 or more in magnitude, a span of more than 65536
 * cells on an axis.  Cells OUTSIDE the map are passed through: they are NOT blocked here, unlike in anet_voxel_query_dev, so a
 * sensor outside the map sees into it and a segment wholly outside is ANET_HIT_FREE.                                            */
int anet_voxel_raycast_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *voxels, const double *origins, const double *ends,
                           int64_t n, int32_t *voxel, double *t, void *stream);

/* ---- exploration goals on the occupancy grid: frontier, connected components, view gain (csrc/frontier_kernels.h) ----------------
 * Everything below is integer, or the walk above: each result is a function of its inputs alone, bit for bit.
 * The frontier: mask[v] = 1 when logodds[v] != ANET_OCC_UNKNOWN, logodds[v] < occ (the threshold of anet_occupancy_to_voxels_dev, so
 * "free" means the same in both), v lies in the box of cells [box_lo, box_lo + box_ext) (both NULL: the whole map) and at least one
 * of the six face neighbours INSIDE the map is ANET_OCC_UNKNOWN; a neighbour outside the map is not unknown space.  Every byte of
 * mask [n_voxels] is written, 0 outside the box.  count_dev (DEVICE, may be NULL): the number of ones.  ANET_ERR_INVALID before
 * anything is written: a bad grid, a NULL pointer, one of box_lo / box_ext NULL, a box not inside the map (lo >= 0, ext >= 1,
 * lo + ext <= size).  Asynchronous on `stream`.                                                                                 */
int anet_occupancy_frontier_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const int16_t *logodds, int32_t occ, const int32_t box_lo[3],
                                const int32_t box_ext[3], uint8_t *mask, int64_t *count_dev, void *stream);
/* Connected components of a byte grid (any: a frontier mask, or the free bytes of a voxel map -- two voxels are mutually reachable
 * exactly when their labels are equal).  mask [n_voxels] DEVICE, a voxel is in the set when its byte != 0; connectivity 6 (faces) or
 * 26 (faces, edges, corners).  labels [n_voxels] int32 DEVICE: -1 where mask[v] == 0, otherwise the SMALLEST linear voxel index of
 * v's component -- a function of the mask alone.  Label equivalence with root chasing: tiles of 8 x 8 x 4 voxels are resolved in
 * LDS, the links across tile borders by atomic minima on root labels, then every label is set to its root; rounds of the last two
 * steps repeat until one links nothing (the word that says so is read once per two rounds; the loop is bounded by the voxel count).
 * rounds_host (HOST, may be NULL): the rounds that ran (a multiple of two: they are issued in pairs).  work: anet_voxel_components_workspace()
 * bytes, 8-byte aligned (-1: bad grid), shared with anet_voxel_component_stats_dev.  Returns when the labels are final.          */
int64_t anet_voxel_components_workspace(const anet_voxel_grid *grid);
int anet_voxel_label_components_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const uint8_t *mask, int connectivity, int32_t *labels,
                                    void *work, int32_t *rounds_host, void *stream);
/* The table of the components of `labels` (the output above), in ASCENDING order of root label (the roots are the voxels with
 * labels[v] == v): n_components_dev [1] the true number, even above max_components; for the first max_components of them root
 * [max], count [max] the voxels, sum_xyz [max][3] int64 the sums of the integer cell coordinates, bbox [max][6] the inclusive cell
 * box (lo x y z, hi x y z).  Voxels of later components are ignored.  All DEVICE; max_components == 0 counts only (the four
 * tables may then be NULL).  work: as above; a root's rank is left at its own index in it.  Asynchronous on `stream`.            */
int anet_voxel_component_stats_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const int32_t *labels, int32_t max_components,
                                   int32_t *n_components_dev, int32_t *root, int32_t *count, int64_t *sum_xyz, int32_t *bbox, void *work,
                                   void *stream);
/* View gain: gain[v] = the number of DISTINCT voxels in U_v, the unknown voxels a scan with the template `pts` from pose v would
 * cross.  Per template point p_s = pts[r] (sensor frame): the world point p_c = (R[c][0] x + R[c][1] y) + R[c][2] z + t[c], each
 * operation rounded on its own (anet_depth_to_points_dev's expression); the ray from o = t exactly as a scan forms it (a non-finite
 * point or one closer than min_range is skipped, one beyond max_range is cut to o + d * (max_range / len)); the walk above at the
 * scan's span limit.  Per visited cell: outside the map: continue; L != UNKNOWN and L >= occ: stop (an occupied cell blocks and is
 * not counted); L == UNKNOWN: the cell is in U_v; known free: continue.  The end cell is treated like any other.
 * A view with a non-finite entry in R or t gets -1, the other views are unaffected; a view in an occupied cell gets 0 by the rule.
 * gain is a function of the SET of template points, and on a map without an occupied voxel it equals the number of voxels
 * anet_occupancy_integrate_dev turns from UNKNOWN to known when given the same world points from the same origin.
 * view_R [V][9] row-major, view_t [V][3], pts [n_pts][3], gain [V]: all DEVICE.  work: one mark byte per cell of a view's sub-box
 * (the cells within ceil(max_range / scale) + 1 of the view's cell, cut to the map), a slot per view, all zero between calls like
 * the marks of anet_occupancy_workspace (a fresh buffer is zeroed by the caller once).  Views run in chunks of as many slots as
 * work_bytes holds -- one mark launch and one count-and-clear launch per chunk -- and the result does not depend on the chunking.
 * anet_occupancy_view_gain_workspace: the bytes for n_views in one chunk; _min: for one view; -1: bad grid or params.
 * ANET_ERR_INVALID: a bad grid or params, negative counts, a NULL pointer, work not 16-byte aligned, work_bytes below _min.      */
int64_t anet_occupancy_view_gain_workspace(const anet_voxel_grid *grid, const anet_occupancy_params *params, int32_t n_views);
int64_t anet_occupancy_view_gain_workspace_min(const anet_voxel_grid *grid, const anet_occupancy_params *params);
int anet_occupancy_view_gain_dev(anet_ctx *ctx, const anet_voxel_grid *grid, const anet_occupancy_params *params, const int16_t *logodds,
                                 int32_t occ, const double *view_R, const double *view_t, int32_t n_views, const double *pts,
                                 int32_t n_pts, int32_t *gain, void *work, int64_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ALLOCNET_AMD_H */
