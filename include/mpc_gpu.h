/*
 * mpc_gpu.h -- C ABI of libmpcgpu.so: batched real-time-iteration NMPC solve on AMD MI355X (gfx950).
 *
 * Drop-in boundary.  In the reference the hot path sits behind acados' ctypes objects
 * `AcadosOcpSolver` / `AcadosSimSolver`, used from src/simulation/robot_ocp_problem.py.  Each entry point
 * below names the reference call site(s) it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain C, no exceptions; every function returns 0 on success, a negative code on error
 *     (MPC_ERR_*), and mpc_last_error() returns a thread-local message for the last failure.
 *   - all arrays are float64, C-contiguous, batch-major:
 *       x0[B][5], goal[B][2], P[B][N+1][n_obst][2], obst[B][n_obst][4] = (x, y, vx, vy),
 *       X[B][N+1][5], U[B][N][2], u0[B][2], cost[B]; status/iters are int32[B].
 *     State is [x, y, psi, v, omega], control is [u_a, u_alpha] (src/models/robot_model.py:14-25).
 *   - per-instance solver status uses the acados codes the reference inspects
 *     (robot_ocp_problem.py:203): 0 ok, 2 QP not converged -- it hit qp_iter_max, or its polish ended with the step estimate still 100 polish_tol
 *     (mpc_config.polish_tol) -- and its step is still applied, 4 QP failure (no step).
 *   - functions without the _dev suffix take HOST pointers and copy; they synchronise before returning.
 *     _dev functions take DEVICE pointers, enqueue on `stream` (a hipStream_t passed as void*, NULL = the
 *     handle's own stream) and do not synchronise.
 *   - a handle is bound to one device and owns the warm-start iterate (X, U) for up to max_batch
 *     instances, as the acados solver object owns it in the reference.  Calls on one handle must be
 *     serialised by the caller; different handles may be used from different threads.
 *   - the library never falls back to a CPU path: without a usable HIP device mpc_create fails.
 */
#ifndef MPC_GPU_H
#define MPC_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_OK 0
#define MPC_ERR_ARG (-1)      /* bad argument / unsupported size */
#define MPC_ERR_HIP (-2)      /* HIP runtime error (message has the hipError string) */
#define MPC_ERR_NODEVICE (-3) /* no usable gfx950 device */

#define MPC_NX 5
#define MPC_NU 2

/* Version of this header's binary interface: bumped whenever `struct mpc_config` changes size or layout or an entry point changes its signature
 * (round 4: trailing field qp_fail_policy, +8 bytes; round 5, version 6: trailing fields polish_ratio, polish_tol, polish_step_frac, +24 bytes, mpc_abi_version itself;
 * round 6, version 7: trailing field polish_res_g, +8 bytes).  A host compares it with mpc_abi_version() of the library it loaded BEFORE it calls
 * mpc_default_config / mpc_create: a host built against an older struct would otherwise be written past its end.  (No reference counterpart: acados
 * regenerates and recompiles its C interface per problem.) */
#define MPC_ABI_VERSION 7

/* largest obstacle count a handle takes (mpc_create2; mpc_create keeps 1..10) */
#define MPC_MAX_OBST 32

/* Problem definition.  Defaults (mpc_default_config) are the reference's constants. */
typedef struct mpc_config {
    int32_t N;              /* N_SOLV                     src/models/world_specification.py:44   */
    int32_t n_obst;         /* N_OBST, 1..10 (mpc_create2: 1..32, beyond 10 with N <= 31)  world_specification.py:25 */
    double Tf;              /* TF                         world_specification.py:43              */
    double W[6];            /* diag W, y=[x,y,v,w,ua,ual] robot_ocp_problem.py:24-26,78-80       */
    double We[4];           /* diag W_e, y_e=[x,y,v,w]    robot_ocp_problem.py:27,83             */
    double lm;              /* levenberg_marquardt        robot_ocp_problem.py:128               */
    double bx_lo[4];        /* lbx on idx [0,1,3,4]       robot_ocp_problem.py:91-93             */
    double bx_hi[4];
    double bu_lo[2];        /* lbu / ubu                  robot_ocp_problem.py:95-97             */
    double bu_hi[2];
    double r_safe;          /* R_OBST+R_ROBOT+MARGIN      src/models/robot_model.py:62           */
    double slack_a;         /* 1e4                        robot_ocp_problem.py:146               */
    double slack_b;         /* 50                         robot_ocp_problem.py:146               */
    int32_t qp_iter_max;    /* QP_ITER                    robot_ocp_problem.py:131               */
    double qp_tol;          /* interior-point tolerance (linear residuals, complementarity)      */
    /* acados-semantics switches; defaults reproduce 2022-era acados           */
    int32_t cost_scale_dt;  /* stage cost x dt                                      default 1   */
    int32_t slack_scale_dt; /* slack penalties x dt for stages < N                  default 1   */
    int32_t lm_scaled;      /* LM term x dt for stages < N (pinned per seed) default 1 */
    int32_t bx_terminal;    /* path box also at stage N                              default 0   */
    int32_t soft_h;         /* obstacle rows softened (slack=True, :106)             default 1   */
    double arena[4];        /* X_MIN, X_MAX, Y_MIN, Y_MAX  world_specification.py:7-10           */
    int32_t bug_compat_predict; /* look-ahead uses vx = vy, src/utils/visualization.py:69  default 1 */
    double mu0;             /* interior-point cold start: lam = mu0 / t                          */
    double thr0;            /*                            t = max(rho, thr0)                     */
    int32_t qp_fail_policy; /* what a QP that does not converge does (robot_ocp_problem.py:131 qp_solver_iter_max, :203-205 status 4 -> set_initial_guess()):
                               0: the divergence tests are on -- mu > 1e8 mu0 ends the solve at once with status 4 (iterate untouched), and a solve that
                                  reaches qp_iter_max with mu > 1e4 mu0 (from iteration 20 on: above mu0) is a failure (4), not a slow solve (2);
                               1: "truncate" -- no divergence test: the interior point runs to qp_iter_max and its step is applied (status 2), as acados'
                                  SQP_RTI did with a HPIPM solve that returned MAX_ITER; NaN / overflow / step collapse stay status 4.
                               default: what the reference's recorded tables select                                    */
    double polish_ratio;    /* polish of the interior point (round 5): a solve that meets qp_tol takes up to 2 further iterations while (a) its last iteration reduced the largest
                               live complementarity product by less than 1 / polish_ratio (c_max(k) > polish_ratio c_max(k-1): not yet the superlinear end-game), or */
    double polish_tol;      /* (b) for any stage the estimate s r min(1, 10 r) of the remaining primal error exceeds polish_tol (s: max-norm of the stage's last step,
                               r = min(s / previous s, 1/2): a multiplier that collapsed to the floor on a weakly active row leaves the termination test blind but the
                               step long).  0 = that indicator off.  Defaults 1e-2 and 1e-6 (the stated parity tolerance): the solves that met the tolerance 1e-6 .. 2e-5
                               from the QP's exact solution (0.7 % of the first solves of BASELINE configs[4]'s problem) are gone at +0.5 % iterations (DESIGN.md
                               section 2).  (The qp_solver tolerances of robot_ocp_problem.py:126-132 are left at acados' defaults there.) */
    double polish_step_frac; /* floor of that estimate as a fraction of the step: est = max(s r min(1, 10 r), polish_step_frac s).  Default 0.01 from N = 30 on, else 0: at long
                               horizons the last Newton step leaves 1.5 .. 10 % of itself behind whatever contraction was observed (5 solves of 1.2e7 fuzz solves ended
                               1e-5 .. 2e-5 from the exact solution without it, none beyond 3e-7 with it; +0.4 .. 0.8 % iterations there, +3.8 % at N = 20 where nothing needs it) */
    double polish_res_g;    /* (c), round 6: the stationarity residual of the QP's Lagrangian -- HPIPM's res_g, which acados' default tolerances gate
                               (robot_ocp_problem.py:126-132 leaves them alone) -- above this value when the termination test holds asks for a polish iteration as well.
                               Formed once per solve by one open-loop adjoint sweep (input blocks B_i' pi_{i+1} + (H z + q - C' lam)_u; slack equations per row).
                               Default 1e-7: on BASELINE configs[4]'s problem the solves beyond 1e-7 from the QP's exact solution fall from 5 to 1 of 4000 and the worst
                               from 1.3e-6 to 2.4e-7 at +0.11 % iterations.  0 = off. */
} mpc_config;

typedef struct mpc_handle mpc_handle;

/* MPC_ABI_VERSION the library was built with */
int mpc_abi_version(void);

/* thread-local description of the last error returned on this thread */
const char *mpc_last_error(void);

/* number of visible HIP devices (0 when none); never initialises a context */
int mpc_device_count(void);

/* fill `cfg` with the reference's constants for a given horizon / obstacle count */
int mpc_default_config(mpc_config *cfg, int N, int n_obst, double Tf);

/* Replaces AcadosOcpSolver(...) / AcadosSimSolver(...) construction, robot_ocp_problem.py:135-136.
 * Allocates device buffers for up to max_batch instances on `device`; warm start is zero-initialised. */
int mpc_create(const mpc_config *cfg, int device, int max_batch, mpc_handle **out);
/* mpc_create for up to MPC_MAX_OBST obstacles: the same for n_obst 1..10; 11..32 need N <= 31 and run on the multi-wavefront solve kernel
 * (rti_wide_kernel: one instance per workgroup of 2 or 4 wavefronts).  MPC_ERR_ARG for n_obst outside [1, 32] or N > 31 with more than 10. */
int mpc_create2(const mpc_config *cfg, int device, int max_batch, mpc_handle **out);
int mpc_destroy(mpc_handle *h);

/* Device pointers of the handle-owned iterate (X[max_batch][N+1][5], U[max_batch][N][2]) and the handle's stream */
int mpc_iterate_ptrs(mpc_handle *h, double **d_X, double **d_U, void **stream);

/* ocp_solver.set(i,'x',..)/set(i,'u',..) for all stages, robot_ocp_problem.py:254-258,305-306 */
int mpc_set_warmstart(mpc_handle *h, int batch, const double *X, const double *U);
/* ocp_solver.get(i,'x') / get(i,'u') for all stages, robot_ocp_problem.py:198,232,240 */
int mpc_get_traj(mpc_handle *h, int batch, double *X, double *U);
/* set_initial_guess(): reset(), X[i] = [x0_x, x0_y, x0_psi, 0, 0], U = 0, robot_ocp_problem.py:286-306 */
int mpc_reset_guess(mpc_handle *h, int batch, const double *x0);
/* set_initial_guess() as the commented block robot_ocp_problem.py:293-300 computes it -- the variant that recorded the two `interpolate_init`
 * tables of src/simulation/test_data (20221031_225145, _225445): stage i starts at (x0_x, x0_y + i/N (goal_y - x0_y), arctan2(goal_y - x0_y, 0), 0, 0),
 * U = 0; the reference's slips (`x0[0] - x0[0]`, `subgoal[0] - subgoal[0]`) included, bit for bit numpy's arithmetic. */
int mpc_reset_guess_interp(mpc_handle *h, int batch, const double *x0, const double *goal);
/* warm-start shift, robot_ocp_problem.py:253-258 */
int mpc_shift(mpc_handle *h, int batch);

/* The solve core, robot_ocp_problem.py:186-198: parameterize_model (P), parameterize_slack (from x0, goal),
 * lbx_0 = ubx_0 = x0, ocp_solver.solve(), u* = get(0,'u').  One SQP_RTI iteration per instance on the
 * handle-owned iterate.  u0/cost/status/iters may be NULL.  cost = NLP objective at the new iterate. */
int mpc_solve(mpc_handle *h, int batch, const double *x0, const double *P, const double *goal,
              double *u0, double *cost, int32_t *status, int32_t *iters);
/* Same with the obstacle look-ahead fused: obst[B][n_obst][4] -> P on device
 * (Obstacle.predict_trajectory, src/utils/visualization.py:62-79 + parameterize_model, :154-166) */
int mpc_solve_obst(mpc_handle *h, int batch, const double *x0, const double *obst, const double *goal,
                   double *u0, double *cost, int32_t *status, int32_t *iters);

/* parameterize_slack(), robot_ocp_problem.py:145-152: the reference uploads zl_i = Zl_i = alpha_i * ones(n_obst) for every stage i
 * before every solve (cost_set(i,'zl'|'Zl')).  By default the solve kernel evaluates that schedule itself from (x0, goal, slack_a,
 * slack_b); a caller who changes parameterize_slack passes the weights here instead: alpha[batch][N+1] (host; copied) applies to all
 * following solves of the first `batch` instances until it is replaced; alpha = NULL returns to the built-in schedule.  Weights must be
 * finite and >= 0 (0 = the row is vacuous, as at the reference's terminal stage).  slack_scale_dt still multiplies stages < N.
 * _dev: a device array [max_batch][N+1] used in place (not copied; NULL = built-in). */
int mpc_set_slack_schedule(mpc_handle *h, int batch, const double *alpha);
int mpc_set_slack_schedule_dev(mpc_handle *h, const double *d_alpha);

/* Per-stage reference (acados cost_set(stage, 'yref', v) / cost_set(N, 'yref_e', v), robot_ocp_problem.py:284): yref[batch][T][6] in y order
 * (x, y, v, omega, u_a, u_alpha), optional row offsets offset[batch] (int32, NULL = 0).  Stage i < N of instance b tracks row
 * min(offset[b] + i, T - 1), the terminal stage columns 0..3 of row min(offset[b] + N, T - 1): the gradient is cs W (y - yref_i) and the
 * reported cost is the LS cost against it.  Everything else (slack schedule, interpolated guess, goal-reached test, distances) still reads
 * the per-call goal.  Host arrays, copied; applies to every following solve (mpc_solve, mpc_solve_obst, mpc_solve_dev,
 * mpc_closed_loop_step_dev, mpc_linearize_dev) of the first `batch` instances until it is replaced; yref = NULL returns to the goal-derived
 * reference.  MPC_ERR_ARG for non-finite entries, T < 1, batch outside [1, max_batch] and negative offsets.
 * _dev: device arrays d_yref[max_batch][T][6] and d_offset[max_batch] (or NULL), used in place and not validated.
 * A solve with a reference runs the stage-split mapping for N <= 31 (also where the goal path would pack several instances into a wavefront),
 * one instance per wavefront on compact stage blocks beyond (or with mpc_set_lanes_per_stage(1)), and the multi-wavefront kernel for more than
 * 10 obstacles; with mpc_set_matrix_cores(1), mpc_set_row_parallel(0), mpc_set_block_riccati(1) or lanes per instance 16, 21 or 32 it
 * returns MPC_ERR_ARG. */
int mpc_set_reference(mpc_handle *h, int batch, int T, const double *yref, const int32_t *offset);
int mpc_set_reference_dev(mpc_handle *h, int T, const double *d_yref, int32_t *d_offset);

/* Per-instance cost weights and per-obstacle radii: W[batch][6] and We[batch][4] in the order of mpc_config.W / .We, r_safe[batch][n_obst] and
 * r_hit[batch][n_obst].  Any pointer may be NULL: that group keeps the handle's mpc_config value; all four NULL switch the feature off and the handle
 * runs the kernels it ran before.  Instance b then solves with its own weights (gradient, Hessian diagonal, reported cost, stationarity residual,
 * q of mpc_linearize_dev), obstacle row j of every stage of instance b reads h = |p - o_j|^2 - r_safe[b][j]^2 (hval of mpc_linearize_dev, the penalty
 * in the reported cost), and the episode bookkeeping of mpc_closed_loop_step_dev (margin, hit flag) uses r_hit[b][j] for obstacle j in place of its
 * constant 1.2.  With r_safe given and r_hit NULL, r_hit[b][j] = r_safe[b][j] - (cfg.r_safe - 1.2): the handle's margin between the two radii is kept.
 * The Levenberg-Marquardt term, cost_scale_dt / lm_scaled, bounds, slack schedule and tolerances stay per handle.
 * Host arrays, validated (finite, weights >= 0, radii > 0, batch in [1, max_batch]; MPC_ERR_ARG otherwise) and copied; applies to every following
 * solve (mpc_solve, mpc_solve_obst, mpc_solve_dev, mpc_closed_loop_step_dev, mpc_linearize_dev) of the first `batch` instances until replaced.
 * Works together with mpc_set_reference, with explicit P, with the in-kernel look-ahead and with every flag of the fused step.
 * _dev: device arrays of max_batch rows, used in place and not validated: the values they hold when a solve is launched are the ones it uses (a small
 * kernel in front of each solve, on the solve's stream, forms the derived constants with the host's rounding).
 * The mappings are those of a per-stage reference: the stage-split kernel for N <= 31 at every batch size, one instance per wavefront on compact
 * stage blocks beyond, the multi-wavefront kernel for more than 10 obstacles; with mpc_set_matrix_cores(1), mpc_set_row_parallel(0),
 * mpc_set_block_riccati(1) or lanes per instance 16, 21 or 32 a solve returns MPC_ERR_ARG while the feature is on. */
int mpc_set_instance_params(mpc_handle *h, int batch, const double *W, const double *We, const double *r_safe, const double *r_hit);
int mpc_set_instance_params_dev(mpc_handle *h, const double *d_W, const double *d_We, const double *d_r_safe, const double *d_r_hit);

/* Per-instance obstacle masks: bit j of mask[b] set means obstacle j exists for instance b; one batch then holds problems with different obstacle sets
 * (sweeps over the obstacle count, obstacles that enter and leave an instance's view).  NULL switches the feature off and the handle runs the kernels
 * it ran before.  An absent obstacle has no row at any stage: no inequality pairs, no entries in the item count behind mu, no part in the cold start,
 * the complementarity and polish tests or the slack equations of the stationarity residual, no penalty term in the reported cost -- the solve is the
 * one of a handle built for the present obstacles only.  Its entries in P / obst may hold anything, NaN and Inf included: they reach no output and
 * not the non-finite-input test (status 4).  A word of 0 is valid: that instance solves the problem without obstacle rows.
 * Host words, validated (batch in [1, max_batch], no bit at or above n_obst; MPC_ERR_ARG otherwise) and copied; applies to every following solve
 * (mpc_solve, mpc_solve_obst, mpc_solve_dev, mpc_closed_loop_step_dev) of the first `batch` instances until replaced.
 * _dev: max_batch device words, used in place and not validated (bits at and above n_obst are ignored): a solve reads them when it is launched, so
 * a caller may rewrite them on the device between steps with no host call.
 * mpc_closed_loop_step_dev: every obstacle still moves and still consumes its noise pair (the noise stream and a later re-activation stay consistent);
 * absent obstacles do not enter the margin or the hit flag unless MPC_STEP_MARGIN_ALL is given ("not sensed, but it is there": the solve sees the
 * masked set, the bookkeeping every obstacle).
 * Works together with mpc_set_reference, mpc_set_instance_params, explicit P, the in-kernel look-ahead and every flag of the fused step; thr0 and all
 * other mpc_config fields stay per handle.  mpc_linearize_dev is NOT masked: hval / dh are geometry and keep reporting every obstacle.
 * Mappings and refusals are those of mpc_set_instance_params (above), always on the run-time-row-count kernels (also when n_obst fills the row capacity). */
int mpc_set_obstacle_mask(mpc_handle *h, int batch, const uint32_t *mask);
int mpc_set_obstacle_mask_dev(mpc_handle *h, const uint32_t *d_mask);

/* Per-instance box bounds: bx_lo[batch][4] and bx_hi[batch][4] in the order of mpc_config.bx_lo / .bx_hi (x, y, v, omega), bu_lo[batch][2] and
 * bu_hi[batch][2] (u_a, u_alpha); one batch then holds robots with different actuator and speed limits.  Any pointer may be NULL: that group keeps the
 * handle's mpc_config value for every instance; all four NULL switch the feature off and the handle runs the kernels it ran before.  Instance b then
 * solves with its own boxes at every place a solve reads one (the input box of stages 0 .. N-1, the state box of stages 1 .. N-1 and, with bx_terminal,
 * N).  bx_terminal, arena and every other mpc_config field stay per handle; x0 is not boxed, so an instance whose x0 lies outside its own box gets the
 * status the usual rules give.  The plant step, the bookkeeping of the fused step, the reported cost and mpc_linearize_dev read no bound.
 * Host arrays, validated (batch in [1, max_batch], every entry finite, lo < hi in every component -- against the handle's value where only one side is
 * given; MPC_ERR_ARG with the field's name otherwise, and nothing is switched on) and copied; applies to every following solve (mpc_solve,
 * mpc_solve_obst, mpc_solve_dev, mpc_closed_loop_step_dev) of the first `batch` instances until replaced; a solve of more instances is refused.
 * _dev: one packed device table d_bounds[max_batch][12], a row being bu_lo[2], bu_hi[2], bx_lo[4], bx_hi[4], used in place and not validated: a solve
 * reads the values when it is launched (no kernel runs in front of it), so a caller may rewrite them on the device between steps with no host call.
 * NULL switches the feature off.
 * Works together with mpc_set_reference, mpc_set_instance_params, mpc_set_obstacle_mask, explicit P, the in-kernel look-ahead and every flag of the
 * fused step.  Mappings and refusals are those of mpc_set_obstacle_mask (above), on the run-time-row-count kernels; switching the bounds off returns
 * the handle to the kernels and results it had. */
int mpc_set_instance_bounds(mpc_handle *h, int batch, const double *bx_lo, const double *bx_hi, const double *bu_lo, const double *bu_hi);
int mpc_set_instance_bounds_dev(mpc_handle *h, const double *d_bounds);

/* Several SQP iterations per solve launch: acados' nlp_solver_type = 'SQP' with nlp_solver_max_iter = max_iter in place of the 'SQP_RTI' the reference
 * configures (robot_ocp_problem.py:126-132), with the plain full step of the real-time iteration (no globalisation).  max_iter = 1 switches the feature
 * off: the handle runs the kernels and gives the results it had.  max_iter in 2 .. MPC_MAX_SQP_ITER switches it on for every following mpc_solve,
 * mpc_solve_obst, mpc_solve_dev and mpc_closed_loop_step_dev.  MPC_ERR_ARG (naming the field) for max_iter outside 1 .. MPC_MAX_SQP_ITER and for a
 * step_tol that is NaN or negative; +inf is valid.
 * One launch then runs, per instance b and for k = 1, 2, ..., one RTI iteration (linearise, QP, interior point from its cold start, full step) on b's
 * current iterate.  The inputs are those of the launch and the same for every k: x0, P or the look-ahead computed once, goal, slack schedule, reference,
 * instance parameters, mask, bounds.  The loop of instance b ends behind iteration k when its status is 4, or k == max_iter, or the step it applied has
 * max-norm <= step_tol (over every entry of dX, stages 0 .. N, and dU; unscaled, in double, the step itself).  Reported: status = that of the last
 * iteration run; iters = the sum of the interior-point iterations of all iterations run (the iters accumulator gets the same sum, the status accumulator
 * one word for the final status); cost and u* = U[0] at the final iterate; sqp_iters[b] = k.  The rest of the fused step -- reset on fail, plant,
 * obstacles, bookkeeping, shift, MPC_STEP_ADVANCE_REF -- happens once, behind the loop, on the final status.  A status 4 at iteration k leaves the iterate
 * of iteration k - 1.  In short: the result is that of the same sequence of single-iteration launches stopped by the same rule.  An idle instance
 * (episode over) runs nothing and its sqp_iters word is not written; mpc_debug_trace records the last iteration run -- every iteration writes its rows from row 0, `iters` is the sum over the
 * iterations and not the number of valid rows, and rows behind the last iteration's own may be left from an earlier, longer one: trace single
 * iterations (max_iter = 2, step_tol = +inf) where the rows of one are to be read; mpc_linearize_dev is unaffected.
 * Runs on feature-level kernels of their own (the instantiations of mpc_set_instance_bounds with one more flag): features that are not set read the
 * handle's own values; mappings and refusals are those of mpc_set_instance_bounds (above).
 * mpc_set_sqp_iters_out_dev: int32[max_batch] device words that receive k per instance at every following solve, NULL = off. */
#define MPC_MAX_SQP_ITER 100   /* acados' default nlp_solver_max_iter */
int mpc_set_sqp(mpc_handle *h, int max_iter, double step_tol);
int mpc_set_sqp_iters_out_dev(mpc_handle *h, int32_t *d_sqp_iters);

/* Plant integrator, ocp_integrator.set/solve/get, robot_ocp_problem.py:207-212 (same IRK as the OCP) */
int mpc_plant_step(mpc_handle *h, int batch, const double *x, const double *u, double *x_next);
/* Obstacle look-ahead only: obst[B][n_obst][4] -> P[B][N+1][n_obst][2] (visualization.py:62-79) */
int mpc_predict(mpc_handle *h, int batch, const double *obst, double *P);

/* ---- device-pointer (asynchronous) variants: inputs already resident in HBM ---- */
int mpc_solve_dev(mpc_handle *h, int batch, const double *d_x0, const double *d_P, const double *d_goal,
                  double *d_X, double *d_U, double *d_u0, double *d_cost, int32_t *d_status, int32_t *d_iters,
                  void *stream);
int mpc_predict_dev(mpc_handle *h, int batch, const double *d_obst, double *d_P, void *stream);

/* One whole control step of RobotOcpProblem.step (robot_ocp_problem.py:184-260) in ONE kernel launch, batched:
 *   look-ahead of the obstacles (visualization.py:62-79) -> RTI solve (:186-198) -> u* -> optional set_initial_guess on
 *   status 4 (:203-205) -> plant step, x0 updated in place (:207-212) -> obstacle motion with optional noise, obst updated
 *   in place (:217-218) -> margin / arena / goal bookkeeping (:213-250) -> warm-start shift (:253-258).
 * flags: OR of MPC_STEP_*.  d_noise: [B][n_obst][2] standard normals or NULL.  Metrics buffers (MPC_STEP_METRICS):
 * min_margin[B] (initialise to +inf), ep_flags int32[B] (bit0 goal reached -> the instance idles from then on, bit1 left the
 * arena, bit2 min_margin <= 0), ep_steps int32[B] (the reference's iteration counter i). */
#define MPC_STEP_SHIFT 1
#define MPC_STEP_PLANT 2
#define MPC_STEP_OBSTACLES 4
#define MPC_STEP_RESET_ON_FAIL 8
#define MPC_STEP_ALIAS_BUG 16
#define MPC_STEP_METRICS 32
#define MPC_STEP_INTERP_GUESS 64   /* with MPC_STEP_RESET_ON_FAIL: the reset writes the straight-line guess of mpc_reset_guess_interp */
#define MPC_STEP_ADVANCE_REF 128   /* behind the step, offset[b] += 1 of the per-stage reference for every instance that stepped (idle ones do not); needs offsets */
#define MPC_STEP_MARGIN_ALL 256    /* with an obstacle mask: margin and hit flag count every obstacle, absent ones included (without a mask they all count anyway) */
int mpc_closed_loop_step_dev(mpc_handle *h, int batch, double *d_x0, double *d_obst, const double *d_goal, double *d_X, double *d_U,
                             double *d_u0, double *d_cost, int32_t *d_status, int32_t *d_iters, const double *d_noise,
                             double randomness, double vmax, int flags, double *d_min_margin, int32_t *d_ep_flags,
                             int32_t *d_ep_steps, void *stream);
int mpc_shift_dev(mpc_handle *h, int batch, double *d_X, double *d_U, void *stream);
int mpc_reset_guess_dev(mpc_handle *h, int batch, const double *d_x0, double *d_X, double *d_U, void *stream);
int mpc_reset_guess_interp_dev(mpc_handle *h, int batch, const double *d_x0, const double *d_goal, double *d_X, double *d_U, void *stream);
/* MULTI-START: K initial guesses per scenario, the best kept on the device.  The problem is non-convex -- an obstacle on the line from robot to goal
 * splits the solutions into "pass left" and "pass right", and an RTI / SQP iteration stays in the family its guess sits in (the reference starts every
 * solve from ONE guess, robot_ocp_problem.py:286-306, and shifts it, :253-258) -- so a caller spends some of the batch on several guesses per scenario.
 * Layout: `groups` scenarios of K members; member k of group g is instance g K + k of the ordinary arrays, and every member of a group is given the
 * same x0, obstacles and goal.  The solve between the two calls is the ordinary launch (mpc_solve_dev, mpc_closed_loop_step_dev) on groups * K
 * instances: neither call changes what a solve launches.  Both: MPC_ERR_ARG (with a message, nothing launched) for a null handle or a null mandatory
 * pointer, K outside 1 .. 64, groups < 0 or groups * K > max_batch; groups = 0 does nothing.
 *
 * mpc_seed_guesses_dev writes the iterate of member k of every group from the group's x0 (d_x0[groups][5]) and goal (d_goal[groups][2]) and the
 * lateral offset a = d_offsets[k] in metres (d_offsets[K]).  With d = goal - x0[0:2], L = |d|, t = d / L, n = (-t_y, t_x), s_i = i / N, for i = 0 .. N:
 *   X[i][0:2] = x0[0:2] + s_i d + a sin(pi s_i) n                                  (the straight line bent sideways by a half sine)
 *   X[i][2]   = x0_psi + wrap(atan2(tau_y, tau_x) - x0_psi),  tau = d + a pi cos(pi s_i) n the path tangent, wrap(e) = e - 2 pi rint(e / 2 pi)
 *   X[i][3:5] = 0 for i >= 1;  X[0] = x0 (all five entries);  U = 0.
 * L < 1e-9: the member gets the plain guess of mpc_reset_guess_dev.  keep_first != 0: member 0 of every group is not touched (the closed loop's
 * shifted warm start).  Non-finite inputs propagate into the iterate; the solve then reports status 4, as for any non-finite warm start.
 *
 * mpc_select_best_dev reads d_cost[groups * K] and d_status[groups * K] of a solve and decides per group:
 *   - member k is ELIGIBLE when its status is 0 or 2 and its cost is finite;
 *   - the winner is the eligible member of least cost, ties to the lowest k (a cross-lane butterfly with a lexicographic compare: no atomics, no
 *     dependence on the order workgroups run in, the same answer every time);
 *   - with incumbent_margin = m > 0 (0 <= m < 1; outside: MPC_ERR_ARG) an eligible member 0 stays the winner unless the challenger's cost is
 *     < (1 - m) cost[0] -- hysteresis against changing sides every control step;
 *   - no eligible member: winner = -1, best_cost = +inf, best_u0 = (0, 0), nothing is copied.
 * Outputs: d_winner[groups] (int32, mandatory), d_best_cost[groups], d_best_u0[groups][2] (each may be NULL).  best_u0 is row winner of d_u0
 * [groups * K][2], the u* array of the solve, bit for bit; with d_u0 NULL it is U[0] of the winner's row of d_U.
 * flags: MPC_SELECT_BROADCAST copies the winner's rows of d_X and d_U into every other member of its group (read once, written K - 1 times, never
 * onto itself), so that a following mpc_shift_dev leaves every member on the winner's shifted iterate; without it d_X / d_U may be NULL (unless
 * best_u0 is to come from d_U) and are not written.  Unknown flags: MPC_ERR_ARG. */
#define MPC_SELECT_BROADCAST 1
int mpc_seed_guesses_dev(mpc_handle *h, int groups, int K, const double *d_x0, const double *d_goal, const double *d_offsets, int keep_first,
                         double *d_X, double *d_U, void *stream);
int mpc_select_best_dev(mpc_handle *h, int groups, int K, const double *d_cost, const int32_t *d_status, double incumbent_margin, int flags,
                        double *d_X, double *d_U, int32_t *d_winner, double *d_best_cost, double *d_best_u0, const double *d_u0, void *stream);
/* MULTI-START, THE GROUP CONTROL STEP: everything a closed-loop control step of `groups` scenarios does BEHIND its solve launch, in one launch, episode
 * bookkeeping included.  The solve in front of it is the ordinary launch over groups * K instances (member k of group g = instance g K + k); with
 * select-by-rollout, mpc_predict_dev and mpc_rollout_merit_dev stand between the two.  Per group g whose ep_flags[g] bit 0 is clear, in this order:
 *   1. SELECT by exactly the rule of mpc_select_best_dev on d_key[groups * K] (the reported cost, or the rollout merit), d_status and incumbent_margin:
 *      out->winner[g], out->best_key[g], out->best_u0[g] = row winner of d_u0[groups * K][2] bit for bit, (0, 0) without a winner;
 *   2. PLANT: d_x[g] <- F(d_x[g], best_u0[g]) in place (d_x[groups][5]; F the integrator of mpc_plant_step_dev);
 *   3. OBSTACLES: d_obst[g] advanced in place (d_obst[groups][n_obst][4]) with mpc_obstacle_step_dev's arithmetic: d_noise[groups][n_obst][2] standard
 *      normals or NULL, randomness, vmax; any obstacle count a handle can have (1 .. 32);
 *   4. BOOKKEEPING, the rule of mpc_closed_loop_step_dev's MPC_STEP_METRICS on the NEW state and the MOVED obstacles: margin = min over the obstacles of
 *      |x[0:2] - o[0:2]| - r_hit, r_hit = 1.2 or row g K of the per-instance table (mpc_set_instance_params); an obstacle absent under the mask of row g K
 *      (mpc_set_obstacle_mask) does not count unless MPC_GROUP_MARGIN_ALL is given; min_margin[g] = min(min_margin[g], margin); ep_flags[g] bit 1 = outside
 *      the arena, bit 2 = min_margin <= 0, bit 0 = within 0.15 of d_goal[g] -- otherwise ep_steps[g] += 1; out->lost[g] += 1 when no member was eligible,
 *      out->switched[g] += 1 when winner > 0;
 *   5. NEXT ITERATES: member 0 <- the winner's iterate shifted (mpc_shift_dev's rule: X[N] kept, U[N - 1] = 0); members 1 .. K - 1 <- the guess of
 *      mpc_seed_guesses_dev for d_offsets[k] around the NEW d_x[g] and d_goal[g]; a group without a winner applied u = 0 and has member 0 seeded too, with
 *      d_offsets[0].  There is no broadcast: the launch writes no word that it overwrites.  (With mpc_set_guess_geometry on, members 1 .. K - 1 take
 *      the amplitudes of its rule on the new state and the moved obstacles, d_offsets being the base family: GUESS FAMILY FROM GEOMETRY below);
 *   6. MEMBER INPUTS of the next solve: the new x[g], obst[g] and goal[g] into rows g K .. g K + K - 1 of out->member_x [groups * K][5], out->member_obst
 *      [groups * K][n_obst][4], out->member_goal [groups * K][2], and out->member_flags[g K + k] = ep_flags[g] & 1.
 * A group whose bit 0 is set on entry is IDLE: the launch reads its flag and writes none of its words.  It is not solved either when the solve launch is
 * mpc_closed_loop_step_dev with flags = MPC_STEP_METRICS alone on out->member_flags and two scratch arrays of groups * K words (margin, steps): that launch
 * idles the members whose flag is set and moves nothing; what it writes into the scratch words and member_flags of a running member is ignored, the group
 * arrays are the record and this call rewrites member_flags.
 * out: device pointers only, copied by the call; winner, min_margin (preset to +inf), ep_flags and ep_steps are mandatory, every other field may be NULL
 * and is then not written.  The member arrays must not overlap the group arrays.  MPC_ERR_ARG (with a message, nothing launched): a null handle or null
 * mandatory pointer (d_key, d_status, d_u0, d_x, d_obst, d_goal, d_offsets, d_X, d_U, out), K outside 1 .. 64, groups < 0 or groups * K > max_batch,
 * incumbent_margin outside [0, 1), unknown flags, a per-instance feature that covers fewer than groups * K instances.  groups = 0 does nothing. */
#define MPC_GROUP_MARGIN_ALL 1
typedef struct mpc_group_step_out {
    int32_t *winner;                                           /* [groups] */
    double *best_key, *best_u0;                                /* [groups], [groups][2] */
    double *min_margin;                                        /* [groups] */
    int32_t *ep_flags, *ep_steps;                              /* [groups] */
    int32_t *lost, *switched;                                  /* [groups] */
    double *member_x, *member_obst, *member_goal;              /* [groups * K] rows */
    int32_t *member_flags;                                     /* [groups * K] */
} mpc_group_step_out;
int mpc_group_step_dev(mpc_handle *h, int groups, int K, const double *d_key, const int32_t *d_status, const double *d_u0, double incumbent_margin,
                       int flags, double *d_x, double *d_obst, const double *d_goal, const double *d_offsets, const double *d_noise, double randomness,
                       double vmax, double *d_X, double *d_U, const mpc_group_step_out *out, void *stream);
/* MULTI-START, GUESS FAMILY FROM GEOMETRY: the lateral amplitudes of members 1 .. K - 1 chosen per group from the obstacles that are in the way, so that
 * the members are the group's pass-left / pass-right candidates instead of one fixed family (no reference counterpart; docs/PROBLEM.md section 4).
 * mpc_set_guess_geometry(h, mode, clearance, a_max, lead): mode 0 = off (the default of every handle; the other arguments are then checked and ignored),
 * 1 = the rule below.  MPC_ERR_ARG: a null handle, any other mode, a NaN, negative or infinite clearance or lead, a_max that is not finite and > 0.
 * THE RULE for one group with state x, goal, obstacle rows o_j = (x, y, vx, vy), j < n_obst, and base family offsets[K]: d = goal - x[0:2], L = |d|,
 * t = d / L, n = (-t_y, t_x) as in mpc_seed_guesses_dev.  Per obstacle: q_j = o_j[0:2] + lead o_j[2:4] (no wall reflection), e_j = q_j - x[0:2],
 * al_j = e_j . t, c_j = e_j . n, s_j = al_j / L, R_j = r_j + clearance with r_j = row g K of the per-instance r_safe table (mpc_set_instance_params) or the
 * handle's r_safe.  Obstacle j BLOCKS when it is present under the obstacle mask of row g K (mpc_set_obstacle_mask), 0 < s_j < 1 and |c_j| < R_j, both
 * strict -- a non-finite value makes the tests false.  A blocking obstacle offers, with w_j = sin(pi s_j), left_j = (c_j + R_j) / w_j and right_j =
 * (c_j - R_j) / w_j, each clamped to [-a_max, a_max]: the family's path is displaced by a sin(pi s) at fraction s, so these put it R_j beside q_j.
 * The blocking obstacles are ordered by al_j ascending, ties to the lower j.  Member 0 keeps offsets[0]; member k >= 1 takes, of the blocking obstacle
 * of rank (k - 1) / 2, `left` when k is odd and `right` when k is even; where the order has no such obstacle the member keeps offsets[k].  L < 1e-9:
 * every member keeps its base offset.  The iterate is mpc_seed_guesses_dev's for that amplitude.
 * While the mode is on, mpc_group_step_dev (point 5, on the NEW state and the MOVED obstacles) and mpc_group_refill_dev (start, on the start row and the
 * obstacles just drawn) form the amplitudes of the members they seed by this rule, d_offsets[K] being the base family; with the mode off both launch
 * the kernels they launched before the mode existed.  Member 0 of a group with a winner is the shifted winner, of a group without one offsets[0], as before.
 * mpc_seed_guesses_geom_dev is mpc_seed_guesses_dev with the rule applied per group: d_obst[groups][n_obst][4] are the groups' obstacle rows, and
 * d_offsets_out[groups][K] (may be NULL) receives the amplitude of every member (member 0: offsets[0], under keep_first too).  MPC_ERR_ARG as
 * mpc_seed_guesses_dev, and when the mode is off or a per-instance feature covers fewer than groups * K instances. */
int mpc_set_guess_geometry(mpc_handle *h, int mode, double clearance, double a_max, double lead);
int mpc_seed_guesses_geom_dev(mpc_handle *h, int groups, int K, const double *d_x0, const double *d_obst, const double *d_goal, const double *d_offsets,
                              int keep_first, double *d_X, double *d_U, double *d_offsets_out, void *stream);
/* ROLLOUT MERIT: score a plan by simulating its inputs.  The cost a solve reports is the NLP objective at the iterate (X + dX, U + dU), whose states follow
 * the linearisation about the guess, not the plant; one RTI iteration from a poor guess that pair is far from dynamically consistent, and its cost cannot be
 * compared with that of a converged one.  This call rolls U out from x0 -- X^r_0 = x0, X^r_{i+1} = F(X^r_i, U_i), F the integrator of mpc_plant_step_dev
 * (robot_model.py:39-43) -- and reports, per instance b (nothing in the reference stands behind merit, margin, boxviol or Xr; the defect is what acados'
 * get_residuals()[1], res_eq, measures on the iterate):
 *   d_merit[b]    the NLP objective (LS cost + exact penalty alpha_i ss (v + v^2 / 2), v = max(0, -h)) at (X^r, U), with everything the cost of the solve
 *                 launched at this moment would use for instance b: the slack schedule (built-in from (x0, goal), or mpc_set_slack_schedule's), the per-stage
 *                 reference at its current offset, per-instance W / We / r_safe, the obstacle mask;
 *   d_defect[b]   max(|X_0 - x0|_inf, max_i |X_{i+1} - F(X_i, U_i)|_inf) of the GIVEN iterate d_X (needs d_X; d_X is read for nothing else);
 *   d_margin[b]   min over i = 1 .. N and the present obstacles j of |X^r_i[0:2] - P_ij| - r_hit_j, r_hit the fused step's (1.2, or the per-instance table);
 *                 +inf when no obstacle is present;
 *   d_boxviol[b]  the largest violation (>= 0) of the instance's state boxes (mpc_config's, or mpc_set_instance_bounds') by X^r: x, y, v, omega at stages
 *                 1 .. N - 1, and N under bx_terminal;
 *   d_Xr[b]       X^r itself, [N + 1][5].
 * Instance b takes x0[5], P[N + 1][n_obst][2] and goal[2] from row b / members of d_x0, d_P, d_goal (members = 1: one row per instance; members = K: a
 * multi-start group shares one row, so P is predicted once per scenario), and U[N][2], X[N + 1][5] and every per-instance table from row b.  Every output
 * pointer may be NULL, not all of them; an output that is not asked for is not written.  MPC_ERR_ARG (with a message, nothing launched): batch < 1 or
 * > max_batch, members < 1, no output, d_defect without d_X, a null mandatory pointer or handle, and a per-instance feature that covers fewer instances than
 * batch.  Non-finite inputs propagate into the instance's own merit (mpc_select_best_dev treats such a member as not eligible) and touch no other
 * instance's words.  The rollout is three levels of prefix sums over the horizon (the plant is a chain of integrators), summed in a fixed order: the same
 * bits every launch, and the serial chain of mpc_plant_step_dev to rounding (a sum of <= 62 terms in another order). */
int mpc_rollout_merit_dev(mpc_handle *h, int batch, int members, const double *d_x0, const double *d_P, const double *d_goal, const double *d_X,
                          const double *d_U, double *d_merit, double *d_defect, double *d_margin, double *d_boxviol, double *d_Xr, void *stream);
int mpc_plant_step_dev(mpc_handle *h, int batch, const double *d_x, const double *d_u, double *d_xnext, void *stream);
/* Obstacle.step() ground-truth motion (visualization.py:20-33); d_noise[B*n_obst][2] standard normals or NULL */
int mpc_obstacle_step_dev(mpc_handle *h, int count, double *d_obst, const double *d_noise,
                          double randomness, double vmax, void *stream);
/* The reference's NOISE stream on the device (experiments.py:33-36, visualization.py:28-33): instance s carries numpy's legacy generator after
 * np.random.seed(seed0 + s) and the scenario generator's uniform draws (mpc_generate_scenarios_dev produces those values; here they are consumed), and
 * mpc_noise_draw_dev writes one control step's np.random.normal(size=2) per obstacle -- d_noise[count][n_obst][2], the array mpc_closed_loop_step_dev
 * takes -- and advances the state.  d_state: count * mpc_noise_state_words() uint32.  d_ep_flags (optional): instances whose episode is over (bit 0)
 * draw nothing, like the reference's loop that has left.  Bit for bit numpy's stream except for the last bit of ~1 draw in 10^4 (glibc's log is not
 * correctly rounded there; the device evaluates it in double-double arithmetic).  No host upload: 13000 episodes x 400 steps of normals are 416 MB. */
int mpc_noise_state_words(void);
int mpc_noise_init_dev(mpc_handle *h, int count, int scenario, unsigned seed0, uint32_t *d_state, void *stream);
int mpc_noise_draw_dev(mpc_handle *h, int count, uint32_t *d_state, double *d_noise, const int32_t *d_ep_flags, void *stream);
/* SEED SWEEPS: on-device episode refill.  experiments.py:20-36 runs seed after seed, each until the goal is reached (robot_ocp_problem.py:247-250) or
 * max_iter control steps are spent.  A sweep streams seed indices 0 .. seed_count-1 (numpy seeds seed_first + k) through a fixed number of slots: call
 * this once per control step IN FRONT OF mpc_closed_loop_step_dev, on the same stream, with the slot arrays that call takes.  One call:
 *   - a slot is FINISHED when ep_flags bit 0 is set or ep_steps >= max_steps;
 *   - a finished slot with slot_seed >= 0 parks the raw words of its result under its seed index: d_res_f[seed][6] = min_margin, x0[5] and
 *     d_res_i[seed][2] = ep_flags, ep_steps (table columns such as dist_to_goal are the host's to form);
 *   - the seed indices not started yet go to the finished slots in ASCENDING SLOT ORDER (lowest finished slot, lowest remaining index): no atomics, no
 *     dependence on the order workgroups run in, so the seed-to-slot schedule is a function of the episode lengths alone;
 *   - a finished slot that gets no index (sweep exhausted) has slot_seed = -1 and ep_flags bit 0 set: the fused step and the noise draw skip it;
 *   - a slot that gets index k is initialised as instance k of a scenario run: generator seeded with seed_first + k (d_state, the layout of
 *     mpc_noise_init_dev), the scenario's uniform draws taken from it in the reference's order as the slot's obstacle states (the values of
 *     mpc_generate_scenarios_dev; behind them the state is mpc_noise_init_dev's), x0 = the start row (v = omega = 0 with MPC_REFILL_ALIAS_BUG), the
 *     goal row, X / U = the initial guess of mpc_reset_guess_dev (MPC_REFILL_INTERP_GUESS: of mpc_reset_guess_interp_dev), min_margin = +inf,
 *     ep_flags = ep_steps = 0, slot_seed = k;
 *   - MPC_REFILL_DRAW_NOISE: behind that, one control step's normals for every slot that runs, as mpc_noise_draw_dev writes them into d_noise;
 *   - d_cursor[0] = seed indices handed out so far, d_cursor[1] = slots that run after this call (poll it; 0 = the sweep is over and every row parked).
 * d_start [rows][5], d_goal_rows [rows][2]: rows = 1 (per_seed 0) or seed_count (per_seed 1, row k for index k).  box: as mpc_generate_scenarios_dev.
 * First call of a sweep: slot_seed = -1, ep_flags = 1, cursor = {0, 0} -- every slot is then filled by the same code.  Two launches (a one-workgroup
 * scan that decides, a grid over the slots that applies); the decision is handed over in words of the handle, so consecutive calls on one handle
 * belong on one stream.  MPC_ERR_ARG (with a message, nothing launched): slots outside [1, max_batch], seed_count < 0, max_steps < 1, scenario outside
 * 0 .. 2, unknown flags, per_seed outside {0, 1}, a null array (d_noise may be null without MPC_REFILL_DRAW_NOISE). */
#define MPC_REFILL_ALIAS_BUG 1
#define MPC_REFILL_INTERP_GUESS 2
#define MPC_REFILL_DRAW_NOISE 4
int mpc_episode_refill_dev(mpc_handle *h, int slots, int scenario, unsigned seed_first, int seed_count, int max_steps, int flags, const double *box,
                           const double *d_start, const double *d_goal_rows, int per_seed, double *d_x0, double *d_obst, double *d_goal, double *d_X,
                           double *d_U, double *d_min_margin, int32_t *d_ep_flags, int32_t *d_ep_steps, uint32_t *d_state, double *d_noise,
                           int32_t *d_slot_seed, int32_t *d_cursor, double *d_res_f, int32_t *d_res_i, void *stream);
/* SEED SWEEPS, PER SEED: feature tables, a status log and a ring of seeded episodes.  All three are additive, off until set, and change neither the
 * prototype nor the meaning of mpc_episode_refill_dev: a handle on which none of the calls below was made launches exactly what it launched before.
 *
 * PER-SEED TABLES (mpc_set_refill_tables_dev).  The per-instance features -- cost weights and radii (mpc_set_instance_params_dev), obstacle masks
 * (mpc_set_obstacle_mask_dev), box bounds (mpc_set_instance_bounds_dev) -- read PER-SLOT device arrays in place when a solve is launched.  A sweep varies
 * them PER SEED: give the per-seed source (row k = seed index k) and the per-slot destination (row s = slot s: the very array registered with the _dev
 * setter), and the refill's apply launch copies row k of every source that is given into row s of its destination when seed index k starts in slot s.
 *   sources, each optional (NULL):  W[seed_count][6], We[seed_count][4], r_safe[seed_count][n_obst], r_hit[seed_count][n_obst], mask[seed_count] (uint32),
 *                                   bounds[seed_count][12] (the packed row of mpc_set_instance_bounds_dev: bu_lo[2], bu_hi[2], bx_lo[4], bx_hi[4]);
 *   destinations:                   slot_W[slots][6], ... slot_bounds[slots][12] -- a source without its destination is MPC_ERR_ARG, naming the field.
 * Slots that are kept or drained are not touched, so PRESET the destinations with valid values (the handle's own): a slot that never gets a seed is
 * still solved by the fused step.  Nothing is validated on the device: the sources hold what the host setters would accept (finite, weights >= 0,
 * radii > 0, lo < hi, no mask bit at or above n_obst).
 *
 * STATUS LOG.  log[slots][4] (int32: n2, n4, first_bad, seen) and res_log[seed_count][3], both or neither.  The apply launch resets
 * log[s] = {0, 0, -1, 0} when a seed starts in slot s and parks log[s][0..2] under the slot's old seed index beside its result row; behind every fused
 * step, on the same stream, mpc_episode_status_log_dev counts (one thread per slot): with now = ep_steps[s] + (ep_flags[s] & 1), if now > seen the slot
 * solved at episode step `seen` -- status 2 counts into n2, status 4 into n4, first_bad = seen if the status is nonzero and first_bad is still -1 --
 * and seen = now.  res_log[k] is then {solves of seed k that ended with status 2, with status 4, its first control step with a status != 0 or -1}.
 *
 * Every word the apply launch writes still belongs to its own slot or its own seed.  mpc_set_refill_tables_dev(h, NULL) switches tables and log off.
 * The struct holds device pointers only and is copied by the call.
 *
 * RING OF SEEDED EPISODES (mpc_episode_ring_dev, mpc_episode_ring_fill_dev), opt-in.  Seeding numpy's generator is ~2000 dependent integer steps that
 * one thread runs for every slot that starts a seed; the ring takes them out of the refill: it is seeded many entries at a time, every few control
 * steps, and a slot that starts a seed copies an entry.  Entries are VALIDATED BY TAGS; the ring is a cache and never a condition of correctness.
 *   attach: d_ring_state[capacity][mpc_noise_state_words()], d_ring_obst[capacity][n_obst][4], d_ring_tag[capacity] (preset to -1 by the caller),
 *     d_seed_src (int32[seed_count], or NULL).  capacity 0 detaches.  The arrays are the caller's and are used in place.
 *   fill: ONE launch, one thread per entry e, in front of the refill on the same stream.  With handed = d_cursor[0], thread e owns the one index k in
 *     [handed, handed + capacity) with k % capacity == e; if k < seed_count and tag[e] != k it seeds seed_first + k into ring_state[e], takes the
 *     scenario's draws into ring_obst[e] -- the refill's own sequence, so the state is mpc_noise_init_dev's -- and writes tag[e] = k LAST.  An entry is
 *     overwritten only by k + capacity, which is owned only once k has been handed out.  Call it every few control steps, not every step.
 *   apply with a ring attached: a slot that starts k copies state and obstacle row of entry k % capacity when its tag is k, and seeds in place, as
 *     without a ring, otherwise.  d_seed_src[k] = 1 (ring) or 0 (seeded in place).
 *   refusal: the handle remembers scenario, seed_first, seed_count and box of the last fill; while a ring is attached, a refill whose values differ is
 *     MPC_ERR_ARG and launches nothing (an entry seeded for another sweep would carry a matching tag).  Attaching forgets them.
 * No atomics, no spinning, no grid-wide synchronisation; no thread reads a word that another thread of the same launch writes. */
typedef struct mpc_refill_tables {
    const double *W, *We, *r_safe, *r_hit;                     /* per-seed sources */
    const uint32_t *mask;
    const double *bounds;
    double *slot_W, *slot_We, *slot_r_safe, *slot_r_hit;       /* per-slot destinations */
    uint32_t *slot_mask;
    double *slot_bounds;
    int32_t *log;                                              /* [slots][4] */
    int32_t *res_log;                                          /* [seed_count][3] */
} mpc_refill_tables;
int mpc_set_refill_tables_dev(mpc_handle *h, const mpc_refill_tables *t);
int mpc_episode_status_log_dev(mpc_handle *h, int slots, const int32_t *d_status, const int32_t *d_ep_flags, const int32_t *d_ep_steps, int32_t *d_log,
                               void *stream);
int mpc_episode_ring_dev(mpc_handle *h, int capacity, uint32_t *d_ring_state, double *d_ring_obst, int32_t *d_ring_tag, int32_t *d_seed_src);
int mpc_episode_ring_fill_dev(mpc_handle *h, int scenario, unsigned seed_first, int seed_count, const double *box, const int32_t *d_cursor, void *stream);
/* SEED SWEEPS, PER-SEED TRAJECTORIES (mpc_episode_trace_set_dev, mpc_episode_trace_dev), opt-in and additive like the calls above: a handle on which
 * neither was made launches exactly what it launched before.  What the reference keeps per experiment for its visualisation -- simX, the obstacle
 * trajectories, the predicted horizons (robot_ocp_problem.py:42-49, 234-241, 270-276) -- is recorded ON THE DEVICE for the seed indices that ask for it,
 * whatever slot and control step they run at.  seed_row[k] >= 0 names the row of seed index k in the arrays below, -1 = not traced; the NON-NEGATIVE
 * ENTRIES MUST BE DISTINCT AND BELOW rows -- that is the host's to guarantee, nothing on the device checks distinctness (an entry >= rows is not traced).
 * Rows hold max_steps control steps: give the refill's max_steps.  The struct holds device pointers only and is copied by the call; the arrays are the
 * caller's and are used in place.  mpc_episode_trace_set_dev(h, 0, 0, NULL) (NULL, or rows == 0) detaches.
 *
 * PROTOCOL of one control step, everything on one stream, in this order:
 *   1. mpc_episode_ring_fill_dev (if a ring is attached)   2. mpc_episode_refill_dev   3. mpc_episode_trace_dev, MPC_TRACE_START
 *   4. mpc_closed_loop_step_dev WITH a d_u0 array          5. mpc_episode_status_log_dev (if on)   6. mpc_episode_trace_dev, MPC_TRACE_STEP
 * Two phases, because the refill overwrites a finished slot before anything behind it could read the slot's last step: the last step of an episode is
 * recorded behind the fused step that made it (STEP), the state a seed starts from behind the refill that wrote it (START).
 * In both, for slot s: k = slot_seed[s], now = ep_steps[s] + (ep_flags[s] & 1) (the status log's "episode steps solved"), r = seed_row[k].
 *   START: if k >= 0 and k != slot_state[s].seed, seed k has just started here: slot_state[s] = {k, 0}; if r >= 0, x[r][0] = x0[s], obst[r][0] = obst[s],
 *     len[r] = 0.  If r >= 0 but now != 0 the caller skipped a START call: len[r] = -1 and nothing else is written (the seed is then never recorded: a
 *     protocol error is visible instead of a wrong row 0).
 *   STEP: acts only if k >= 0, k == slot_state[s].seed and now > seen; the slot then solved at episode step `seen`.  If r >= 0 and now <= max_steps:
 *     x[r][now] = x0[s], obst[r][now] = obst[s], u[r][seen] = u0[s], status[r][seen], iters[r][seen], pred[r][seen] = X[s] if pred is given (the RAW
 *     iterate as the fused step left it, i.e. shifted: stage j of the solve sits at X[j - 1], stage N is kept), len[r] = now.  Then seen = now.
 *   Slots that are drained (slot_seed = -1), idle or untraced write nothing but `seen`.
 * One wavefront per slot, 256-thread workgroups; the lanes stride over the doubles of a row, lane 0 writes len and slot_state last.  No atomics, no
 * spinning, no grid-wide synchronisation, bounded loops; every word written belongs to the slot or to the seed's own row; no thread reads a word that
 * another wavefront of the same launch writes.
 * MPC_ERR_ARG (with a message naming the field, nothing launched): rows < 0, max_steps < 1, a null required pointer (pred alone is optional); phase
 * outside {0, 1}, slots outside [1, max_batch], no trace attached, d_u0 / d_status / d_iters null in phase STEP (d_X too while pred is attached; START
 * reads none of the four). */
typedef struct mpc_episode_trace {
    const int32_t *seed_row;   /* [seed_count]: row of seed index k in the arrays below, or -1 = not traced */
    int32_t *slot_state;       /* [slots][2] = {seed index being traced, seen}; the caller presets {-1, 0} */
    int32_t *len;              /* [rows]  control steps recorded for the row (preset 0); -1 = protocol error */
    double *x;                 /* [rows][max_steps + 1][5]          plant state; row 0 = the state the seed started from */
    double *obst;              /* [rows][max_steps + 1][n_obst][4]  obstacle states, likewise */
    double *u;                 /* [rows][max_steps][2]              u* applied at the step */
    int32_t *status;           /* [rows][max_steps]                 the solve's status */
    int32_t *iters;            /* [rows][max_steps]                 its interior-point iterations */
    double *pred;              /* [rows][max_steps][N + 1][5] or NULL: the iterate X as the fused step left it */
} mpc_episode_trace;
int mpc_episode_trace_set_dev(mpc_handle *h, int rows, int max_steps, const mpc_episode_trace *t);
#define MPC_TRACE_START 0
#define MPC_TRACE_STEP 1
int mpc_episode_trace_dev(mpc_handle *h, int slots, int phase, const int32_t *d_slot_seed, const double *d_x0, const double *d_obst, const double *d_X,
                          const double *d_u0, const int32_t *d_status, const int32_t *d_iters, const int32_t *d_ep_flags, const int32_t *d_ep_steps,
                          void *stream);
/* SEED SWEEPS OF MULTI-START GROUPS: the refill for groups.  A sweep of groups streams seed indices 0 .. seed_count-1 through a fixed number of GROUP slots
 * -- a slot is a group of K members, member k of group g = instance g K + k, the layout of mpc_group_step_dev -- and a group whose episode has ended
 * starts the next seed on the device.  Call this once per control step IN FRONT OF the member solve, on the solve's stream, with the arrays the solve and
 * mpc_group_step_dev take.  The rule is mpc_episode_refill_dev's (experiments.py:20-36: seed after seed, each until its goal is reached or max_steps
 * control steps are spent), per group:
 *   DECIDE: mpc_episode_refill_dev's deciding launch, unchanged, on the group words a->ep_flags[groups] and a->ep_steps[groups].  A group is FINISHED when
 *     its bit 0 is set or ep_steps >= max_steps; the seed indices not started yet go to the finished groups in ASCENDING GROUP ORDER; no atomics.
 *     a->cursor[0] = seed indices handed out so far, a->cursor[1] = groups that run after this call (poll it; 0 = the sweep is over, every row parked).
 *   APPLY, one wavefront per group, by what the decision handed the group:
 *     - KEEP (not finished): none of the group's or its members' words is written;
 *     - PARK (every finished group with slot_seed[g] >= 0): a->res_f[seed][6] = min_margin, x[5] and a->res_i[seed][4] = ep_flags, ep_steps, lost, switched;
 *     - DRAIN (finished, no seed left): slot_seed[g] = -1, ep_flags[g] |= 1, member_flags[g K .. g K + K - 1] = 1 -- the member solve idles them -- and
 *       nothing else;
 *     - START seed index k: the generator seeded with seed_first + k into a->state[g] (the layout and the state of mpc_noise_init_dev) and the scenario's
 *       uniform draws taken from it into a->obst[g] (the values of mpc_generate_scenarios_dev); x[g] = the start row AS GIVEN (there is no alias switch);
 *       goal[g] = the goal row; min_margin = +inf, ep_flags = ep_steps = lost = switched = 0, slot_seed = k; members 0 .. K - 1 of a->X and a->U = the guess
 *       family of mpc_seed_guesses_dev (keep_first = 0) for d_offsets around x[g] and goal[g]; x[g], obst[g], goal[g] into the K member rows of
 *       a->member_x, a->member_obst, a->member_goal; member_flags = 0.  The selection's outputs (winner, best_key, best_u0) are not this call's.
 *       (With mpc_set_guess_geometry on, members 1 .. K - 1 take the amplitudes of its rule on the start row and the obstacles just drawn, with row g K
 *       of the handle's r_safe table and obstacle mask and that solve's coverage refusals; d_offsets is the base family.)
 * A wavefront reads every word it parks before it stores anything, and writes only words of its own group, its own members or its own seed.  No noise is
 * drawn: mpc_noise_draw_dev on a->state with the group flags follows, as in a batch of groups.
 * d_start [rows][5], d_goal_rows [rows][2]: rows = 1 (per_seed 0) or seed_count (per_seed 1, row k for index k).  box: as mpc_generate_scenarios_dev.
 * First call of a sweep: slot_seed = -1, ep_flags = 1, member_flags = 1, cursor = {0, 0} -- every group is then filled by the same code.  Two launches; the
 * decision is handed over in words of the handle, so consecutive calls on one handle belong on one stream.
 * NOT OFFERED for groups, and refused rather than ignored: a handle with per-seed tables or a status log (mpc_set_refill_tables_dev), a ring
 * (mpc_episode_ring_dev), a trace (mpc_episode_trace_set_dev) or a per-group record (mpc_group_record_set_dev) attached.
 * MPC_ERR_ARG (with a message, nothing launched): a null handle or a null pointer (every argument and every field of `a` is mandatory), K outside 1 .. 64,
 * groups < 1 or groups * K > max_batch, seed_count < 0, max_steps < 1, scenario outside 0 .. 2, per_seed outside {0, 1}.
 * a: device pointers only, copied by the call. */
typedef struct mpc_group_refill_arrays {
    double *x, *obst, *goal;                                   /* [groups][5], [groups][n_obst][4], [groups][2] */
    double *X, *U;                                             /* [groups * K][N + 1][5], [groups * K][N][2] */
    double *min_margin;                                        /* [groups] */
    int32_t *ep_flags, *ep_steps, *lost, *switched;            /* [groups] */
    uint32_t *state;                                           /* [groups][mpc_noise_state_words()] */
    int32_t *slot_seed, *cursor;                               /* [groups], [2] */
    double *res_f;                                             /* [seed_count][6] */
    int32_t *res_i;                                            /* [seed_count][4] */
    double *member_x, *member_obst, *member_goal;              /* [groups * K] rows */
    int32_t *member_flags;                                     /* [groups * K] */
} mpc_group_refill_arrays;
int mpc_group_refill_dev(mpc_handle *h, int groups, int K, int scenario, unsigned seed_first, int seed_count, int max_steps, const double *box,
                         const double *d_start, const double *d_goal_rows, int per_seed, const double *d_offsets, const mpc_group_refill_arrays *a,
                         void *stream);
/* MULTI-START EPISODES, THE PER-GROUP RECORD (mpc_group_record_set_dev, mpc_group_record_dev), opt-in and additive like the trace above: a handle on which
 * neither was made launches exactly what it launched before.  What mpc_episode_trace keeps per seed -- simX, the obstacle trajectories, the applied inputs
 * (robot_ocp_problem.py:42-49, 234-241, 270-276) -- and, per control step, what the group chose among: the K candidates' keys, status words, iterations,
 * first inputs and (optionally) solved plans, with the winner and its key.  It is recorded ON THE DEVICE and only for the groups that ask for it, because
 * mpc_group_step_dev selects the winner and overwrites the evidence in one launch (member 0 becomes the shifted winner, members 1 .. K - 1 are reseeded,
 * d_x and d_obst move in place): the candidates of a step exist on the device only between the member solve and the group step.
 * group_row[g] >= 0 names the row of group g in the arrays below, -1 = not recorded; the NON-NEGATIVE ENTRIES MUST BE DISTINCT AND BELOW rows -- that is
 * the host's to guarantee, nothing on the device checks distinctness (an entry >= rows is not recorded).  Rows hold max_steps = T control steps.  The struct
 * holds device pointers only and is copied by the call; the arrays are the caller's and are used in place.  mpc_group_record_set_dev(h, 0, 0, 0, NULL)
 * (NULL, or rows == 0) detaches.
 *
 * PROTOCOL of one control step, everything on one stream, in this order:
 *   1. the member solve   2. with the rollout merit as key: mpc_predict_dev, mpc_rollout_merit_dev   3. mpc_group_record_dev, MPC_GROUP_RECORD_SOLVED
 *   4. mpc_group_step_dev WITH out->best_key and out->best_u0   5. mpc_group_record_dev, MPC_GROUP_RECORD_STEPPED
 * with the d_x, d_obst, d_X, d_key, d_status, d_u0 and `out` of call 4 and the d_iters of the solve.  Two phases, because call 4 reads the candidates and
 * overwrites them: what the group chose among is recorded in front of it (SOLVED), what it chose and where that left it behind it (STEPPED).
 * For group g with r = group_row[g] >= 0:
 *   SOLVED acts when bit 0 of out->ep_flags[g] is clear and t = out->ep_steps[g] < T: x[r][t] = d_x[g], obst[r][t] = d_obst[g] (the states the solve started
 *     from), cand_key[r][t][k] = d_key[g K + k], cand_status, cand_iters, cand_u0 likewise, and with cand_X, cand_X[r][t][k] = d_X[g K + k]: the SOLVED
 *     iterate, stage j at row j, before the group step shifts or reseeds it.  Nothing else is written.
 *   STEPPED: with now = ep_steps[g] + (ep_flags[g] & 1) (the status log's "episode steps solved"), acts when now > len[r] and now <= T; the group then solved
 *     at step t = len[r]: winner[r][t] = out->winner[g] (-1: no member was eligible), best_key[r][t] = out->best_key[g], u[r][t] = out->best_u0[g],
 *     x[r][now] = d_x[g], obst[r][now] = d_obst[g], and len[r] = now, written last.  A group that was idle on entry to the step has now == len[r]: nothing.
 * One wavefront per group, four groups per workgroup; every lane loads the group's words first, the lanes then stride over the doubles of a row (the
 * K (N + 1) 5 doubles of a group's iterates are contiguous on both sides).  No atomics, no LDS, no spinning, no grid-wide synchronisation, loops bounded
 * by ceil(K (N + 1) 5 / 64); every word written belongs to the group's own row; no thread reads a word that another wavefront of the same launch writes
 * (len[r] is read and written by the group's own wavefront only); no input is written.
 * While a record is attached, mpc_group_refill_dev is refused (MPC_ERR_ARG, "not offered for groups"): a sweep moves seeds between groups, and this record
 * is keyed by group.
 * MPC_ERR_ARG (with a message naming the field, nothing launched): a null handle, rows < 0, max_steps < 1, K outside 1 .. 64, a null mandatory field
 * (cand_X alone is optional); phase outside {0, 1}, groups < 1 or groups * K > max_batch, K differing from the attached K, no record attached, a null pointer
 * argument, a null out->winner / ep_flags / ep_steps, and out->best_key or out->best_u0 null in phase STEPPED. */
typedef struct mpc_group_record {
    const int32_t *group_row;  /* [groups]: row of group g in the arrays below, or -1 = not recorded */
    int32_t *len;              /* [rows]  control steps recorded for the row (preset 0) */
    double *x;                 /* [rows][max_steps + 1][5]          plant state; row t = the state the solve of step t started from */
    double *obst;              /* [rows][max_steps + 1][n_obst][4]  obstacle states, likewise */
    double *u;                 /* [rows][max_steps][2]              the input applied at the step: the winner's u0, (0, 0) without a winner */
    int32_t *winner;           /* [rows][max_steps]                 the member selected, -1 = none was eligible */
    double *best_key;          /* [rows][max_steps]                 its key (+inf without a winner) */
    double *cand_key;          /* [rows][max_steps][K]              what the selection compared: the reported cost, or the rollout merit */
    int32_t *cand_status;      /* [rows][max_steps][K]              the members' solve status */
    int32_t *cand_iters;       /* [rows][max_steps][K]              their interior-point iterations */
    double *cand_u0;           /* [rows][max_steps][K][2]           their first inputs */
    double *cand_X;            /* [rows][max_steps][K][N + 1][5] or NULL: their solved iterates (NULL: the plans are not kept) */
} mpc_group_record;
int mpc_group_record_set_dev(mpc_handle *h, int rows, int max_steps, int K, const mpc_group_record *r);
#define MPC_GROUP_RECORD_SOLVED 0
#define MPC_GROUP_RECORD_STEPPED 1
int mpc_group_record_dev(mpc_handle *h, int groups, int K, int phase, const double *d_x, const double *d_obst, const double *d_X, const double *d_key,
                         const int32_t *d_status, const int32_t *d_iters, const double *d_u0, const mpc_group_step_out *out, void *stream);
/* MULTI-GPU: one process per GPU, every rank solves its own contiguous slice of the scenarios (the reference's 13 000 closed
 * loops, experiments.py:20-36, are independent), and the only exchange is an all-gather of the per-instance costs -- RCCL over xGMI, called directly
 * from this library (librccl.so.1 is loaded on first use; there is no link-time dependency and no other transport).  A C host does:
 *   rank 0: mpc_comm_unique_id(id), ships the 128 bytes to the other ranks by whatever means it has (a file, a socket, MPI);
 *   every rank: mpc_comm_init(h, rank, world, id)  [collective];  per round: mpc_allgather_cost_dev(h, count, d_cost, d_all, stream)  [collective,
 *   d_all[world][count], rank-major, equal counts on all ranks; enqueued on `stream` (NULL: the handle's), so it overlaps whatever runs on other streams];
 *   mpc_comm_destroy(h) (mpc_destroy does it too).  mpc_allgather_cost is the host-pointer form (stages through the handle's stream and waits). */
#define MPC_COMM_ID_BYTES 128
int mpc_comm_unique_id(unsigned char *id /* MPC_COMM_ID_BYTES */);
int mpc_comm_init(mpc_handle *h, int rank, int world, const unsigned char *id /* MPC_COMM_ID_BYTES */);
int mpc_comm_world(const mpc_handle *h);      /* ranks of the handle's communicator, 0 without one */
/* file name of the RCCL library the exchange is bound to (dladdr of its ncclAllGather): a process that has PyTorch's ROCm wheel loaded gets the wheel's
 * bundled librccl (same soname, already mapped), any other host /opt/rocm's -- measurement records name which one ran */
int mpc_comm_library_path(char *buf, int len);
int mpc_allgather_cost_dev(mpc_handle *h, int count, const double *d_cost, double *d_cost_all, void *stream);
int mpc_allgather_cost(mpc_handle *h, int count, const double *cost, double *cost_all);
int mpc_comm_destroy(mpc_handle *h);
/* generate_random_moving_obstacles (src/utils/obstacle_generator.py:8-28) for the seeds seed0 .. seed0+count-1: instance s gets
 * bit for bit what the reference draws after np.random.seed(seed0 + s) (numpy legacy MT19937 stream, reference draw order).
 * scenario: 0 RANDOM, 1 CENTER, 2 EDGE (:10-18).  box = {X_MIN_OBST, X_MAX_OBST, Y_MIN_OBST, Y_MAX_OBST, V_MAX_OBST, edge (7)}
 * (src/models/world_specification.py:25-40).  obst[count][n_obst][4] = (x, y, vx, vy). */
int mpc_generate_scenarios_dev(mpc_handle *h, int count, int scenario, unsigned seed0, const double *box, double *d_obst, void *stream);
int mpc_generate_scenarios(mpc_handle *h, int count, int scenario, unsigned seed0, const double *box, double *obst);
/* Linearisation products of the current iterate, for parity tests of the linearise stage:
 * A[B][N][5][5], Bm[B][N][5][2], b[B][N][5], q[B][N+1][7] (order u,x), hval[B][N+1][n_obst], dh[B][N+1][n_obst][2] */
int mpc_linearize_dev(mpc_handle *h, int batch, const double *d_x0, const double *d_P, const double *d_goal,
                      const double *d_X, const double *d_U,
                      double *d_A, double *d_B, double *d_b, double *d_q, double *d_hval, double *d_dh, void *stream);

/* The stationarity sweep of the polish (mpc_config.polish_res_g) on its own, for parity tests of that stage: the open-loop adjoint of a given per-stage gradient
 * g[B][N+1][7] (order u, x) over the linearisation of the iterate (X, U), in the lane layout of a solve kernel -- lanes_per_stage = 1 with lanes_per_instance 16, 21,
 * 32 or 64 (N + 1 lanes must fit), or lanes_per_stage 2 (N <= 31) / 3 (N <= 20) with one instance per wavefront.  ru[B][N] = max-norm of the input block
 * g_u,i + B_i' pi_{i+1} per stage, pi_i = g_x,i + A_i' pi_{i+1}.  (No reference counterpart: HPIPM forms res_g inside acados, robot_ocp_problem.py:126-132,195.) */
int mpc_debug_adjoint_dev(mpc_handle *h, int batch, int lanes_per_instance, int lanes_per_stage, const double *d_X, const double *d_U, const double *d_g,
                          double *d_ru, void *stream);

/* ---- measurement: HIP events around solve-kernel launches on the launch stream ----
 * on = 0: off; on = k > 0: events around every k-th launch (k = 1: every launch).  A pair of event records between two back-to-back
 * launches costs the stream ~7 us (measured, scripts/gap_probe.py), so a throughput run samples (bench.py: every 7th launch). */
int mpc_profile_enable(mpc_handle *h, int on);
/* synchronises; returns the summed duration and the number of solve-kernel launches since the last call */
int mpc_profile_read(mpc_handle *h, double *sum_ms, int *launches);

/* Optional device accumulators int32[max_batch] (NULL = off): every solve launch adds each instance's interior-point
 * iteration count to iters_acc and (status == 4) + 65536 * (status == 2) to status_acc, so a benchmark loop needs no
 * extra kernels to report mean iterations, QP failures and iteration-cap hits. */
int mpc_set_accumulators(mpc_handle *h, int32_t *d_iters_acc, int32_t *d_status_acc);

/* Debug aid for parity work: when enabled, every solve records (mu, sigma, alpha, cmax) of each interior-point
 * iteration into a device buffer [max_batch][qp_iter_max][4]; host_out (may be NULL) receives the first `batch` rows
 * (instance b's iterations at [b], whatever the launch order; batch outside [1, max_batch] with a host_out: MPC_ERR_ARG).
 * Rows at and behind an instance's iteration count keep what they held (zero from enabling on).
 * The call waits for the handle's stream only: a caller who solved on another stream synchronises that stream first. */
int mpc_debug_trace(mpc_handle *h, int enable, int batch, double *host_out);

/* lanes per instance (64, 32, 16 or 8) the dispatcher picked for `batch`; 0 = automatic (default) */
int mpc_set_lanes_per_instance(mpc_handle *h, int lanes);
int mpc_get_lanes_per_instance(mpc_handle *h, int batch);
/* 1: for batches <= 1024 (one instance per wavefront) the Riccati factorisation runs on the matrix cores (v_mfma_f64_16x16x4,
 * homogeneous 8x8 stage blocks).  0 (default).  Measured on MI355X it is slower than both vector-ALU variants (FP64 MFMA rate =
 * FP64 vector rate, 116-cycle dependent MFMA links, 75 % tile padding) and less accurate on ill-conditioned stages; it is kept
 * as evidence, see DESIGN.md section 4.  No reference counterpart (tuning / test hook). */
int mpc_set_matrix_cores(mpc_handle *h, int on);
/* Riccati factorisation sweep of the interior point (same arithmetic specification, different lane mapping).
 * 1 (default): row-parallel -- the 8 columns of a stage's homogeneous blocks sit in 8 lanes of a 16-lane DPP row and the
 * products run as v_fmac_f64_dpp row_newbcast chains (~135 instead of ~330 wave instructions per stage); the forward and
 * adjoint vector recursions run the same way on the closed-loop matrix.
 * 0: one-lane systolic sweeps (no LDS), the independent implementation the default is tested against.
 * No reference counterpart (tuning / test hook). */
int mpc_set_row_parallel(mpc_handle *h, int on);
/* Block-2 (partially condensed) stage recursions, default OFF (opt-in: measured 5 % slower than one stage per step at C2): where the mapping has them (the stage-split kernel on dense blocks, even horizons, all of
 * the kernel's obstacle rows in use) the Riccati factorisation and the three vector recursions of an interior-point iteration run over PAIRS of stages
 * (state x_2m, inputs (u_2m, u_2m+1); x_2m+1 eliminated) -- half the sequential steps at ~0.75x the instructions.  What HPIPM's PARTIAL_CONDENSING
 * (robot_ocp_problem.py:126) does on the CPU.  0: one stage per step (the default, and the form the block form is tested against).  Same interior point, same QP solution. */
int mpc_set_block_riccati(mpc_handle *h, int on);
/* Lanes per horizon stage.  0 (default): automatic -- a batch of at most eight instances per SIMD of the device (8192 on
 * MI355X) runs one instance per wavefront with the inequality rows of every stage dealt out to 3 (N <= 20) or 2 (N <= 31)
 * neighbouring lanes, which shortens the instruction stream such a latency-bound wavefront is limited by (and lets every
 * instance stop at its own iteration); larger batches keep one lane per stage and pack 64/G instances into a wavefront
 * (measured crossover between 8192 and 16384 instances).  1: always one lane per stage.  2 / 3: the split mapping whenever
 * the horizon fits (any batch).  Setting lanes per INSTANCE, matrix cores or the systolic sweep implies 1.
 * Same arithmetic specification either way.  No reference counterpart (tuning / test hook). */
int mpc_set_lanes_per_stage(mpc_handle *h, int lanes);
int mpc_get_lanes_per_stage(mpc_handle *h, int batch);
/* Instance scheduling (default on).  Where several instances share a wavefront (one lane per stage: 2, 3 or 4 of them) the wavefront runs
 * until its slowest instance has converged; iteration counts are heavy-tailed (C3: mean 6.6, mean of the per-wavefront maximum 9.4 with
 * three per wavefront) but strongly correlated between consecutive control steps of an instance.  The library therefore deals the instances
 * to wavefronts in the order of their iteration counts in this handle's previous launch of the same batch size (a stable counting sort on
 * the device behind every launch; 7.4 instead of 9.4).  Which instances share a wavefront has no effect on their results beyond the
 * rounding of the wavefront sums with three instances per wavefront (bit-identical with two or four).  No reference counterpart.
 * mpc_get_instance_order: the permutation in effect for the next launch of `batch` instances (returns 1) or 0 when it is the natural order. */
int mpc_set_instance_scheduling(mpc_handle *h, int on);
int mpc_get_instance_order(mpc_handle *h, int batch, int32_t *order);
/* name of the solve kernel instantiation a batch of this size runs (as rocprofv3 prints it, without the namespace), for measurement
 * records: "rti_split_kernel<row capacity, lanes per stage, two wavefronts per SIMD, masked, block-2 recursions>" or "rti_solve_kernel<row capacity, lanes per
 * instance, sweeps, masked>" or, beyond 10 obstacles, "rti_wide_kernel<row capacity, lanes per stage, masked>" (row capacity: 3, 5, 10, 20 or 32 obstacle row pairs per stage, the smallest that holds n_obst; masked: n_obst is below it;
 * sweeps: 0 systolic, 1 matrix cores, 2 row-parallel on dense LDS blocks, 3 row-parallel on compact LDS blocks).  lookahead: whether the
 * obstacle look-ahead runs inside the kernel (mpc_closed_loop_step_dev) -- it enters the LDS budget that selects the block layout. */
int mpc_get_kernel_name(mpc_handle *h, int batch, int lookahead, char *buf, int len);
/* Wavefronts per SIMD of the stage-split mapping.  0 (default): automatic -- two (256 registers per lane, compact LDS blocks: 14.7 KB per
 * wavefront at N = 20, eight wavefronts per CU) only for 3-obstacle problems in batches of more than four instances per SIMD of the device,
 * where a second resident wavefront fills the LDS and dependent-issue stalls of the first; one (all 512 registers, dense LDS blocks)
 * otherwise -- with 5 or 10 obstacle row pairs the 256-register build spills and loses at every batch, and a problem that uses fewer rows than
 * its kernel's capacity always runs one.  1 / 2: forced (ignored for such partial-row problems).  The one-lane-per-stage mapping always runs one
 * wavefront per SIMD.  Same arithmetic specification either way.  No reference counterpart (tuning / test hook). */
int mpc_set_waves_per_simd(mpc_handle *h, int waves);
int mpc_get_waves_per_simd(mpc_handle *h, int batch);

#ifdef __cplusplus
}
#endif
#endif /* MPC_GPU_H */
