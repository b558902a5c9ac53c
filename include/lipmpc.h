/* lipmpc.h — C ABI of the MI355X-native batched LIP-MPC / LDCBF step solver.
 *
 * The reference (salvatore373/Humanoid-Navigation-using-MPC-LDCBF) is pure Python and has no
 * FFI of its own; the boundary this library replaces is, per MPC step and per robot,
 *
 *   HumanoidMPC._precompute_theta_omega_naive      HumanoidNavigation/MPC/HumanoidMpc.py:137-160
 *   HumanoidMPC._get_list_c_and_eta                HumanoidNavigation/MPC/HumanoidMpc.py:296-319
 *     -> ObstaclesUtils.get_closest_point_and_normal_vector_from_obs
 *                                                  HumanoidNavigation/Utils/ObstaclesUtils.py:60-109
 *   HumanoidMPC._add_lcbf_constraint (+ CustomLCBF delta)
 *                                                  HumanoidMpc.py:263-294, HumanoidMPCCustomLCBF.py:30-31
 *   the constraint/cost definition                 HumanoidMpc.py:221-249, 321-333
 *   self.optim_prob.solve()  (CasADi Opti + IPOPT) HumanoidMpc.py:97-100, 417-418
 *   kth_solution.value(U_mpc[:,0]) / state advance HumanoidMpc.py:432-447
 *
 * batched over B independent (state, goal, obstacle-set) instances.  All pointers passed to
 * lipmpc_plan_step_batch / lipmpc_advance_batch are DEVICE pointers (HIP, the handle's
 * device); the caller owns every buffer; calls are asynchronous on `hip_stream` and results
 * are valid after that stream is synchronised.  No function throws; return 0 = ok, <0 = error
 * (lipmpc_strerror).  A handle is not thread-safe: one handle per (device, stream).
 */
#ifndef LIPMPC_H
#define LIPMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIPMPC_ABI_VERSION 5   /* 2: + lipmpc_plan_step_batch_c_eta, LIPMPC_STATUS_SENSOR_OVERFLOW; 3: + lipmpc_lidar_c_eta_batch;
                                * 4: lipmpc_plan_step_batch_c_eta takes the producer's overflow flags;
                                * 5: `active` is the primal tight set of the returned point (LIPMPC_TIGHT_TOL), the finish's
                                *    working set moves to the new optional output `working`, diag is [B,8],
                                *    + lipmpc_set_workspace / lipmpc_workspace_bytes;
                                *    backward-compatible additions since: + lipmpc_set_warm_start / lipmpc_warm_words;
                                *    + lipmpc_rrt_default_params / lipmpc_rrt_workspace_bytes / lipmpc_rrt_plan_batch;
                                *    + lipmpc_neighbour_workspace_bytes / lipmpc_neighbour_c_eta_batch;
                                *    + lipmpc_map_update_batch; + lipmpc_rrt_plan_grid_batch, LIPMPC_RRT_OUTSIDE_GRID;
                                *    + lipmpc_grid_field_batch / lipmpc_grid_path_batch;
                                *    + lipmpc_grid_frontier_field_batch / lipmpc_grid_frontier_path_batch;
                                *    + lipmpc_lidar_c_eta_split_batch / lipmpc_lidar_grid_c_eta_split_batch;
                                *    + lipmpc_fleet_recover_update_batch; + lipmpc_grid_frontier_assign_batch;
                                *    + lipmpc_grid_tiled_info / lipmpc_grid_tiled_workspace_bytes /
                                *      lipmpc_grid_field_tiled_batch / lipmpc_grid_frontier_field_tiled_batch /
                                *      lipmpc_grid_path_tiled_batch / lipmpc_grid_frontier_path_tiled_batch,
                                *      LIPMPC_RRT_FIELD_UNSETTLED;
                                *    + lipmpc_grid_clearance_cost_batch / lipmpc_grid_field_weighted_batch /
                                *      lipmpc_grid_frontier_field_weighted_batch / lipmpc_grid_path_weighted_batch /
                                *      lipmpc_grid_frontier_path_weighted_batch, LIPMPC_COST_MAX;
                                *    + lipmpc_grid_path_wave_batch / lipmpc_grid_frontier_path_wave_batch /
                                *      lipmpc_grid_frontier_utility_path_wave_batch;
                                *    + lipmpc_scan_match_batch */
/* An instrumented development build (tools/build_variant.sh: phase counters in `diag`, other buffer contracts) reports
 * LIPMPC_ABI_VERSION + LIPMPC_VARIANT_BASE from lipmpc_version(), so that a loader which checks the version refuses it. */
#define LIPMPC_VARIANT_BASE 1000

/* `active` bit i: canonical row i is in the problem and TIGHT at the returned point, slack_i(q) = h_i - g_i.q <=
 * LIPMPC_TIGHT_TOL.  The minimiser of the strictly convex step QP is unique, so this set is unique too -- unlike the set
 * of rows with a positive multiplier (`working`), which is not at a degenerate vertex (linearly dependent tight rows). */
#define LIPMPC_TIGHT_TOL 1e-7
#define LIPMPC_DIAG_WORDS 8

/* per-problem status written to status[b] */
#define LIPMPC_STATUS_SOLVED       0  /* exact optimum, KKT-certified active set */
#define LIPMPC_STATUS_MAX_ITER     1  /* interior-point iteration cap reached */
#define LIPMPC_STATUS_INFEASIBLE   2  /* no feasible step (incl. a violated constant k=0 LDCBF row);
                                         the reference raises inside solve() here (HumanoidMpc.py:419-429) */
#define LIPMPC_STATUS_DEGENERATE   3  /* x == c or zero-length edge: reference yields NaN (ObstaclesUtils.py:81,104) */
#define LIPMPC_STATUS_UNCERTIFIED  4  /* interior-point tolerance met, active-set finish not certified */
#define LIPMPC_STATUS_SENSOR_OVERFLOW 5 /* the sample's inferred obstacles did not fit the slots (overflow[b] != 0): the step is not
                                         solved (lipmpc_plan_step_batch_c_eta with overflow flags, lipmpc_sense_plan_step_batch)
                                         and the robot is stopped (lipmpc_fleet_update_batch) rather than planned against a
                                         truncated obstacle list -- the reference constrains against every inferred obstacle,
                                         HumanoidMPCUnknownEnvironment.py:55-64 */

/* flags */
#define LIPMPC_FLAG_INTERIOR 1  /* skip the active-set finish: return the strictly interior
                                   interior-point iterate (what IPOPT hands the reference's loop) */

#define LIPMPC_FLAG_WARM_START 2 /* every MPC step of a robot's closed loop starts from the previous step's interior-point
                                   result shifted by one stage (positions; multipliers clipped to [3, 100]) instead of
                                   "stand still", z = 30 -- the reference seeds its next solve with the shifted prediction,
                                   HumanoidMpc.py:450-455.  Same optimum, fewer iterations (-15..-30 %).
                                   lipmpc_rollout_batch: within the launch.  The step entry points (lipmpc_plan_step_batch,
                                   _c_eta, lipmpc_sense_plan_step_batch): through the warm-start records of
                                   lipmpc_set_warm_start; without records every step starts cold (with every row kept).
                                   Not for more than 14 obstacle slots or N = 1 (the rollout ignores the flag there,
                                   lipmpc_set_warm_start refuses); records also not for N > 8 with more than 4 slots. */
#define LIPMPC_FLAG_NO_PRESOLVE 4 /* keep every LDCBF row in the solve.  By default (exact mode, cold start) the rows that the
                                   leg-reach rows make redundant -- obstacle j at stage k with eta_j.(p_0 - c_j) - delta >
                                   k * (largest CoM step the reach rows allow) + 1e-3: never active, never violated -- are
                                   dropped before the solve and replaced, in the interior-point phase only, by copies of one
                                   direction-free ballast row (oracle/lipmpc_oracle.py: presolve_ldcbf).  Same feasible set,
                                   same minimiser, same active set; only the interior iterates differ, which is why
                                   LIPMPC_FLAG_INTERIOR and LIPMPC_FLAG_WARM_START imply this flag. */

/* error codes */
#define LIPMPC_OK            0
#define LIPMPC_E_ARG        -1
#define LIPMPC_E_UNSUPPORTED -2
#define LIPMPC_E_HIP        -3
#define LIPMPC_E_NOMEM      -4

typedef struct lipmpc_params {
  int32_t N;            /* horizon, 1..16                         (N_horizon, HumanoidMpc.py:50) */
  int32_t n_obs_max;    /* obstacle slots per problem, 0..50 */
  int32_t v_max;        /* vertex slots per obstacle ring, 3..32 */
  int32_t max_iter;     /* interior-point iteration cap */
  int32_t flags;        /* LIPMPC_FLAG_* */
  int32_t finish_rounds; /* cap on the rounds of the certified active-set finish (tail-latency control:
                           a problem that needs more ends UNCERTIFIED with the interior-point answer); 0 = default (8 for N <= 8, else 16) */
  double dt;            /* DELTA_T            config.yml:2  */
  double g;             /* GRAVITY_CONST      config.yml:3  */
  double h_com;         /* COM_HEIGHT         config.yml:4  */
  double alpha;         /* ALPHA              config.yml:5  */
  double l_max[2];      /* L_MAX_X, L_MAX_Y   config.yml:6-7 */
  double l_min[2];      /* L_MIN_X, L_MIN_Y   config.yml:8-9 */
  double v_min[2];      /* V_MIN              config.yml:10 */
  double v_max_xy[2];   /* V_MAX              config.yml:11 */
  double omega_max;     /* 0.156*pi           HumanoidMpc.py:21 */
  double ell;           /* 0.05               HumanoidMpc.py:200 */
  double sampling_time; /* theta update step  HumanoidMpc.py:159 */
  double tol;           /* interior-point stop (exact path): max|r_p| <= tol and mu <= tol */
  double tol_interior;  /* the same for LIPMPC_FLAG_INTERIOR: sets how far inside its constraints the returned iterate
                           stays (the reference's IPOPT stops at 1e-5); too tight and a closed loop lands on LDCBF
                           boundaries where the next eta = (x-c)/|x-c| is 0/0 */
  double k0_tol;        /* tolerated violation of the constant k=0 LDCBF rows (IPOPT constr_viol_tol, HumanoidMpc.py:99) */
} lipmpc_params;

typedef struct lipmpc_handle lipmpc_handle;

/* fills *p with the reference's config.yml values, N=3, n_obs_max=0, v_max=5, tol=1e-11, tol_interior=1e-9 */
int lipmpc_default_params(lipmpc_params* p);

int lipmpc_create(const lipmpc_params* p, int device, lipmpc_handle** out);
void lipmpc_destroy(lipmpc_handle* h);

/* number of inequality rows in canonical order reach(4N) | manoeuvr(N) | vel(4N) | LDCBF((N+1)*n_obs_max)
 * (insertion order of HumanoidMpc.py:230-249, 284-292) and of 64-bit words of the active mask */
int64_t lipmpc_num_rows(const lipmpc_params* p);
int64_t lipmpc_active_words(const lipmpc_params* p);

/* One MPC step for B problems.
 *  state      [B,5]  (p_x, v_x, p_y, v_y, theta)            X_pred[:,k]      HumanoidMpc.py:396-397
 *  goal       [B,2]                                          self.goal        HumanoidMpc.py:83
 *  first_foot [B]    s_v of the current stance, +1 right / -1 left            HumanoidMpc.py:104-108,403
 *  delta      [B] or NULL (=0)  LDCBF safety margin          HumanoidMPCCustomLCBF.py:30-31
 *  obs_xy     [B,n_obs_max,v_max,2]  CCW rings hull.points[hull.vertices], padded
 *  obs_nv     [B,n_obs_max]          vertices used per ring, 0 = slot empty
 * outputs
 *  U      [B,N,2]    footsteps U_mpc            X [B,N+1,4] predicted states X_mpc
 *  theta  [B,N+1]    omega [B,N]                obj [B] objective incl. the constant k=0 term
 *  status [B]  iters [B]
 *  active  [B,lipmpc_active_words]  bit i = canonical row i is tight at the returned point (slack <= LIPMPC_TIGHT_TOL): the
 *          active set of the optimum in the textbook sense, unique because the optimum is; all zero unless status is SOLVED
 *          or UNCERTIFIED (there: the tight rows of the interior-point iterate handed out)
 *  working [B,lipmpc_active_words] or NULL: the working set the certified finish ended on = the rows that carry a positive
 *          multiplier in its KKT certificate (a subset of `active` up to LIPMPC_TIGHT_TOL; at a degenerate vertex one of
 *          several valid choices); UNCERTIFIED: the interior-point estimate z_i > 1e5 s_i
 *  c_eta  [B,n_obs_max,4] (c_x,c_y,eta_x,eta_y) or NULL
 *  bounds [B,4] or NULL: per-problem (V_MAX_x, V_MAX_y, ALPHA, OMEGA_MAX) replacing the handle's values —
 *         the knobs the reference's bounds_tuning sweep mutates in `conf` (bounds_tuning.py:17-26)
 *  A handle with warm-start records (lipmpc_set_warm_start) starts each problem from its record and writes the record back.
 *  diag   [B,LIPMPC_DIAG_WORDS] or NULL: 0 active-set rounds used, 1 final equality residual of the finish,
 *         2 identification margin min_i |log(z_i/(1e5 s_i))| of the interior-point phase, 3 certificate margin =
 *         min(smallest multiplier on the working set, smallest slack outside it): ~0 flags a weakly determined WORKING set,
 *         4 tightness margin min_i |slack_i - LIPMPC_TIGHT_TOL| over the rows of the problem: how far the nearest row is
 *         from changing sides in `active` (a perturbation of the answer below it leaves `active` unchanged), 5-7 reserved (0)
 */
int lipmpc_plan_step_batch(lipmpc_handle* h, int64_t B,
                           const double* state, const double* goal, const int8_t* first_foot,
                           const double* delta, const double* obs_xy, const int32_t* obs_nv,
                           double* U, double* X, double* theta, double* omega, double* obj,
                           int32_t* status, int32_t* iters, uint64_t* active, uint64_t* working, double* c_eta,
                           double* diag, const double* bounds, void* hip_stream);

/* Optional launch order for the step solves of a handle.  A wave lasts as long as the slowest of its problems and a launch
 * of more problems than the GPU holds at once (4096 at N <= 8) runs in rounds, so WHICH problems share a wave and which start
 * first matters: with a schedule every lipmpc_plan_step_batch / _c_eta launch of at most `capacity` problems leaves there each
 * problem's cost (interior-point iterations + finish rounds) and (one small extra kernel) the order -- costliest first,
 * like with like -- in which the next launch of the same batch size places them (+12 % throughput at 32768 problems when
 * consecutive launches see the same or slowly moving problems, as the samples of a closed loop do).  A pure scheduling
 * hint: outputs stay indexed by problem, every order gives the same results, a buffer holding no order for this B means
 * index order.  `schedule`: device buffer of lipmpc_schedule_words(capacity) int32, zeroed once by the caller, owned by the
 * caller and alive until it is unset (NULL) or the handle destroyed; launches on it must be stream-ordered. */
int lipmpc_set_schedule(lipmpc_handle* h, int32_t* schedule, int64_t capacity);
int64_t lipmpc_schedule_words(int64_t B);

/* Optional WARM-START RECORDS for the step entry points (lipmpc_plan_step_batch, _c_eta, lipmpc_sense_plan_step_batch): the
 * seeding of HumanoidMpc.py:448-455 for loops driven from the host.  Record of problem b = lipmpc_warm_words(p) doubles at
 * record + b * lipmpc_warm_words(p):
 *   word 0        1.0 = the rest holds a step result; anything else = no result, start cold (a zeroed record starts cold)
 *   1 .. 2N       q of the interior-point phase: footstep positions, stage-major (x_0, y_0, x_1, y_1, ...)
 *   2N+1 ..       z of the interior-point phase in canonical row order (lipmpc_num_rows); rows not in the problem are 0,
 *                 the constant k = 0 LDCBF rows included
 * Every step launch of the handle reads problem b's record: word 0 = 1.0 starts the solve from it shifted by one stage (stage
 * k takes stage k+1's positions and multipliers, the last stage extrapolates; multipliers clipped to [3, 100]), otherwise
 * cold.  After the solve it writes this step's UNSHIFTED interior-point result back (exact mode: the iterate before the
 * active-set finish), word 0 = 1.0 if the status is SOLVED or UNCERTIFIED, else 0.0 -- a failed step makes the next one
 * cold.  Records are indexed by problem, so a schedule (lipmpc_set_schedule) may be set too.  Every row is kept in a warm
 * solve, which is why the handle must carry LIPMPC_FLAG_WARM_START (else LIPMPC_E_ARG).  LIPMPC_E_UNSUPPORTED for N = 1, for
 * more than 14 obstacle slots, and for N > 8 with more than 4 obstacle slots.  While records are set, a launch of more than `capacity` problems returns LIPMPC_E_ARG.
 * `record`: device buffer of capacity * lipmpc_warm_words(p) doubles, zeroed once by the caller, owned by the caller and
 * alive until unset (NULL or capacity 0) or the handle destroyed; launches that share it must be stream-ordered. */
int lipmpc_set_warm_start(lipmpc_handle* h, double* record, int64_t capacity);
int64_t lipmpc_warm_words(const lipmpc_params* p);     /* 1 + 2N + lipmpc_num_rows(p) */

/* Optional workspace for the SPLIT LAUNCH of a handle's step solves.  For 32-lane problems (N > 8) in the exact mode the
 * step kernel holds the solver bodies of 1, 2, 7 and the handle's LDCBF row slots per lane next to each other and a wave
 * picks the smallest that fits its problems after the presolve -- one register allocation for all of them, which spills
 * (304 B of scratch per lane at N = 16 / 50 obstacles).  With a workspace the step runs as: one classification pass (the
 * front end alone: which body each problem needs), a one-workgroup stable counting sort into one index list per body, and ONE
 * KERNEL PER BODY over its list, the kernels side by side on streams the handle owns (fork / join by events on the caller's
 * stream, so the call stays asynchronous and stream-ordered, and can be captured in a graph).  Against the single-kernel
 * launch the results have the same optimum and the same tight set; a status may differ only between SOLVED and UNCERTIFIED
 * (a problem may run in another solver body, whose sums run in another order: last-bit differences).  For a given batch
 * the split launch is deterministic from run to run; problems of one class share waves.  Ignored (single kernel) for
 * N <= 8, for the flags that keep every row, and for batches larger than the workspace was sized for.  While it is set,
 * the order of lipmpc_set_schedule is not applied (the costs are still left).
 * `workspace`: device buffer of lipmpc_workspace_bytes(h, capacity) bytes, contents arbitrary, owned by the caller, alive
 * until unset (NULL) or the handle is destroyed.  The workspace is shared by every launch made while it is registered: step
 * launches on one workspace must be stream-ordered.  Once the handle's side streams exist (the first workspace makes them:
 * not during a graph capture) this call only swaps a pointer, so a caller may register another workspace right before each
 * launch -- one per stream, one per captured launch -- and launches on different workspaces may then overlap (the side
 * streams and events they share only order them).  A graph keeps the pointer it was captured with. */
int64_t lipmpc_workspace_bytes(const lipmpc_handle* h, int64_t capacity);
int lipmpc_set_workspace(lipmpc_handle* h, void* workspace, int64_t capacity);

/* The same step with the LDCBF half-spaces GIVEN instead of derived from obstacle rings: the reference's subclass
 * hooks HumanoidMPC._get_list_c_and_eta(x_k, y_k) -> (list_c, list_eta) (HumanoidMpc.py:296-319; overridden by
 * HumanoidMPCUnknownEnvironment.py:30-68) and _compute_single_lcbf(x, eta, c) (HumanoidMpc.py:252-261; overridden by
 * HumanoidMPCCustomLCBF.py:30-31) as data.  Row j of every stage k is  eta_j . (p_k - c_j) - delta >= 0  with
 *  c_eta_in [B,n_obs_max,4] (c_x, c_y, eta_x, eta_y); eta need not be a unit vector; eta = (0,0) marks an empty slot,
 *  a NaN in eta marks degenerate geometry met by whoever produced the row (status DEGENERATE, as the ring front end gives).
 *  overflow [B] int32 or NULL: the producer's "obstacles were dropped" flags (lipmpc_lidar_c_eta_batch: the scan's clusters
 *  did not fit the obstacle slots).  A flagged problem is NOT solved against its truncated list -- the reference constrains
 *  against every inferred obstacle (HumanoidMPCUnknownEnvironment.py:55-64) -- it gets status SENSOR_OVERFLOW and NaN
 *  outputs, so lipmpc_advance_batch and every other consumer of `status` leave the robot where it is.
 * Nothing of the geometry front end runs; the constant k = 0 row is still checked against k0_tol.
 * Outputs as lipmpc_plan_step_batch (without c_eta). */
int lipmpc_plan_step_batch_c_eta(lipmpc_handle* h, int64_t B,
                                 const double* state, const double* goal, const int8_t* first_foot,
                                 const double* delta, const double* c_eta_in, const int32_t* overflow,
                                 double* U, double* X, double* theta, double* omega, double* obj,
                                 int32_t* status, int32_t* iters, uint64_t* active, uint64_t* working, double* diag,
                                 const double* bounds, void* hip_stream);

/* Closed-loop state advance (HumanoidMpc.py:432-447): for problems with status SOLVED/UNCERTIFIED
 * state <- (A_l x + B_l U[b,0], theta[b,1]), first_foot <- -first_foot; others are left untouched.
 * In place on state/first_foot. */
int lipmpc_advance_batch(lipmpc_handle* h, int64_t B, double* state, int8_t* first_foot,
                         const double* U, const double* theta, const int32_t* status,
                         void* hip_stream);

/* One sample of a host-driven closed loop for a fleet (the bookkeeping of HumanoidMpc.py:392, 419-447 around a solve
 * that was just enqueued on the same stream), per robot b:
 *   walking[b] &= last_obj[b] >= stop_obj        (stop rule of this sample, from the previous objective, :392)
 *   if walking: last_status[b] = overflow[b] ? SENSOR_OVERFLOW : status[b];  walking[b] &= last_status in {SOLVED, UNCERTIFIED}   (:419-429)
 *   if still walking: last_obj = obj; state <- (A_l x + B_l U[b,0], theta[b,1]); first_foot <- -first_foot (:432-447);
 *                     n_steps[b] += 1; n_overflow[b] += overflow[b] (if given)
 *   U_pred[b, k, :] = (U[b,0,:], omega[b,0]);  X_pred[b, k+1, :] = state[b]   with k = *sample (read on the device)
 * and one thread advances *sample by one, so that a captured graph can be replayed sample after sample.
 * walking [B] int8 (1 = walking), sample [1] int32, X_pred [B,k_max+1,5], U_pred [B,k_max,3]; samples >= k_max are ignored. */
int lipmpc_fleet_update_batch(lipmpc_handle* h, int64_t B, int32_t k_max, double stop_obj,
                              double* state, int8_t* first_foot, int8_t* walking, double* last_obj,
                              int32_t* n_steps, int32_t* last_status, int32_t* n_overflow, int32_t* sample,
                              double* X_pred, double* U_pred,
                              const double* U, const double* theta, const double* omega, const double* obj,
                              const int32_t* status, const int32_t* overflow, void* hip_stream);

/* lipmpc_fleet_update_batch WITH RECOVERY (backward-compatible addition): a failed solve need not end the robot's run.  A robot
 * whose solve failed takes one CAPTURE STEP -- the foot goes on the instantaneous capture point cp = p + v / beta,
 * beta = sqrt(g / h_com) -- and tries the solve again on the next sample.  Why that step: cp is a fixed point of the LIP step
 * (cp+ = cp), the velocity falls by v+ = (ch - sh) v = e^(-beta dt) v, and the CoM moves on the straight segment from p towards
 * cp without passing it.  The sample's LDCBF rows are half-planes that hold p, so the whole motion respects row j if and only
 * if cp does: one dot product per row decides exactly whether the manoeuvre is safe against everything the sample sensed.
 * One lane per robot, *sample read on the device and advanced by the call, no allocation and no host synchronisation (the call
 * can be captured in a graph); every refusal is decided on the host before anything is enqueued.
 *  every argument of lipmpc_fleet_update_batch, and
 *  goal           [B,2]  the goal the sample's solve was given
 *  c_eta          [B,n_obs_max,4] or NULL (no rows): the rows the sample's solve was given (c_x, c_y, eta_x, eta_y), neighbour rows
 *                 included; n_obs_max is the handle's; eta = (0,0) marks an empty slot
 *  delta          [B] or NULL (= 0)
 *  max_recover    >= 0: the most consecutive recovery samples a robot may take; 0 = lipmpc_fleet_update_batch
 *  recover_run    [B] int32, in/out: consecutive recovery samples so far
 *  n_recover      [B] int32, in/out: recovery samples in all
 *  recover_margin [B] double, out
 * PER ROBOT the rule of lipmpc_fleet_update_batch word for word -- stop rule, overflow, last_status, counters, the U_pred / X_pred
 * rows -- except where walking would become 0 because of the status:
 *   solved (SOLVED, UNCERTIFIED): as there, and recover_run = 0 (left as it is with max_recover = 0).
 *   otherwise the safety test is EVALUATED if the robot is walking after the stop rule, the status (SENSOR_OVERFLOW where
 *     overflow[b] != 0) is INFEASIBLE or MAX_ITER, recover_run < max_recover and the four LIP state words (p_x, v_x, p_y, v_y)
 *     are finite.  DEGENERATE (NaN rows) and SENSOR_OVERFLOW (the truncated rows cannot vouch for anything) never recover.
 *   THE SAFETY TEST, IEEE double, no contraction, evaluated as written: cp = (p_x + v_x / beta, p_y + v_y / beta);
 *     margin = min over the slots j with eta_j != (0,0) of (eta_jx * (cp_x - c_jx) + eta_jy * (cp_y - c_jy)) - delta,
 *     +inf with no such slot or a NULL c_eta, -inf if the margin of any such slot is NaN (a NaN in a used row fails the test: an
 *     evaluated margin is never NaN).  It passes iff margin >= 0.
 *   recover_margin[b] = that margin if the test was evaluated, NaN otherwise (written for every robot on every sample < k_max).
 *   RECOVER, if the test was evaluated and passed: omega_r = min(max(atan2(g_y - p_y, g_x - p_x) - theta, -omega_max), omega_max)
 *     (the step's own heading rule at k = 0, no wrapping, HumanoidMpc.py:137-160: the recovery turns the way the next solve
 *     will; omega_max is the handle's); state <- (A_l x + B_l cp, theta + omega_r * sampling_time); first_foot <- -first_foot;
 *     recover_run += 1; n_recover += 1; walking stays 1; last_obj and n_steps (solved samples) are unchanged; last_status keeps
 *     the failed status until a later solve succeeds; the U_pred row is (cp_x, cp_y, omega_r), the X_pred row the new state.
 *     The failed solve's U / theta / omega / obj are not read for that robot.
 *   in every other case: as lipmpc_fleet_update_batch, final (recover_run and n_recover are left as they are).
 * With max_recover = 0 every buffer of lipmpc_fleet_update_batch is left exactly as that call leaves it; the counters are
 * unchanged and recover_margin is NaN.
 * WARM START: nothing to do here.  A step that ends INFEASIBLE or MAX_ITER has already written word 0 = 0.0 into the robot's
 * warm-start record (lipmpc_set_warm_start), so the solve after a recovery sample starts cold; this call does not touch records.
 * Refusals (LIPMPC_E_ARG): max_recover < 0, a null goal / recover_run / n_recover / recover_margin, and whatever
 * lipmpc_fleet_update_batch refuses.  B = 0 enqueues nothing.  Restated in numpy by tests/recover_oracle.py. */
int lipmpc_fleet_recover_update_batch(lipmpc_handle* h, int64_t B, int32_t k_max, double stop_obj,
                                      double* state, int8_t* first_foot, int8_t* walking, double* last_obj,
                                      int32_t* n_steps, int32_t* last_status, int32_t* n_overflow, int32_t* sample,
                                      double* X_pred, double* U_pred,
                                      const double* U, const double* theta, const double* omega, const double* obj,
                                      const int32_t* status, const int32_t* overflow,
                                      const double* goal, const double* c_eta, const double* delta, int32_t max_recover,
                                      int32_t* recover_run, int32_t* n_recover, double* recover_margin, void* hip_stream);

/* Closed loop on the device: HumanoidMPC.run_simulation (HumanoidMpc.py:345-459) for B robots, one group of
 * lanes per robot for the whole run, no host round trip.  Per sample k < k_max: stop when the previous
 * step's objective < stop_obj (0.05 in the reference, :392); on MPC samples (k % mpc_step == 0,
 * mpc_step = max(1, int(DELTA_T / sampling_time)), :74-75) solve the step and advance x+ = A x + B u_0
 * (:441-442), on the others only the heading moves (:443-447); a failed solve ends that robot's run
 * (:419-429).  Uses the handle's flags (LIPMPC_FLAG_INTERIOR = advance with the interior iterate).
 *  state0 [B,5], goal [B,2], first_foot [B], delta [B] or NULL, obs_xy/obs_nv as in lipmpc_plan_step_batch
 * outputs
 *  X_pred  [B,k_max+1,5]  (p_x,v_x,p_y,v_y,theta) per sample; rows 0..n_steps[b] are valid
 *  U_pred  [B,k_max,3]    (f_x,f_y,omega) per sample;        rows 0..n_steps[b]-1 are valid
 *  n_steps [B] samples completed, last_status [B] status of the last solve, total_iters [B] sum of IPM iterations
 */
int lipmpc_rollout_batch(lipmpc_handle* h, int64_t B, int32_t k_max, int32_t mpc_step, double stop_obj,
                         const double* state0, const double* goal, const int8_t* first_foot, const double* delta,
                         const double* obs_xy, const int32_t* obs_nv, double* X_pred, double* U_pred,
                         int32_t* n_steps, int32_t* last_status, int32_t* total_iters, const double* bounds,
                         void* hip_stream);

/* Unknown-environment front end (BASELINE config 5): what HumanoidMPCUnknownEnvironment._get_list_c_and_eta does
 * before the closest-point step (HumanoidMPCUnknownEnvironment.py:30-55): range_finder() =
 * compute_lidar_readings -> Gaussian noise -> DBSCAN(eps, min_samples) -> convex hull per cluster
 * (RangeFinder/range_finder_wth_polygons_dbscan.py:26-63, 100-126, 157-180).  One wavefront per robot; the rings
 * come out in the layout lipmpc_plan_step_batch takes as obs_xy / obs_nv.
 *  state      [B,5]  only (p_x, p_y) are read
 *  env_xy     [n_env,v_env,2] if env_shared else [B,n_env,v_env,2]; env_nv likewise: the TRUE map as vertex rings
 *             in the order the reference iterates them (`ch.points`, HumanoidMPCUnknownEnvironment.py:46); n_env <= 65535
 *  ray_table  [resolution,2] (cos, sin) of angle_i = i * 2 pi / resolution, computed on the host (bit-identical
 *             directions to the reference's math.cos / math.sin); resolution <= 384
 *  noise      [B,resolution,2] added to valid readings, or NULL.  The reference draws N(0, 0.01) from numpy's
 *             global, unseeded generator (:162-172); here the caller supplies the (seeded) sample.
 * outputs
 *  obs_xy [B,n_obs_max,v_max,2], obs_nv [B,n_obs_max]: CCW rings of the inferred obstacles, cluster order
 *  n_inferred [B]; overflow [B] = 1 if clusters/vertices did not fit (n_obs_max, v_max), if more than 384 true
 *  obstacles were within range of the robot, or if an env_nv entry exceeded v_env (the surplus is dropped, never read),
 *  or if a ring of more than 152 edges was within range of the robot: such a ring is skipped as a whole -- the readings,
 *  labels and rings are those of the map without it -- and the scan is flagged.  "Within range" is the conservative test the
 *  scan lists its obstacles by: the ring's bounding circle (round the mean of its vertices) comes within lidar_range.  Of
 *  more than 384 obstacles within range the first 384 in list order are scanned.
 *  hits [B,resolution,2] (NaN = no reading) or NULL; labels [B,resolution] (-2 no reading, -1 noise, k cluster) or NULL
 */
int lipmpc_lidar_sense_batch(int device, int64_t B, int32_t resolution, int32_t n_env, int32_t v_env,
                             int32_t env_shared, double lidar_range, double eps, int32_t min_samples,
                             int32_t n_obs_max, int32_t v_max, const double* state, const double* env_xy,
                             const int32_t* env_nv, const double* ray_table, const double* noise,
                             double* obs_xy, int32_t* obs_nv, int32_t* n_inferred, int32_t* overflow,
                             double* hits, int32_t* labels, void* hip_stream);

/* Unknown-environment CONSTRAINT ASSEMBLY in one launch (BASELINE config 5: "LiDAR point cloud -> convex-hull obstacle
 * rebuild fused into the constraint-assembly kernel"): everything HumanoidMPCUnknownEnvironment._get_list_c_and_eta does
 * (HumanoidMPCUnknownEnvironment.py:30-68) -- range_finder() as in lipmpc_lidar_sense_batch, then for every inferred
 * hull the closest point c and the unit normal eta at the robot's CoM with the inside flip (:54-62 ->
 * ObstaclesUtils.py:60-109) -- with the hulls never leaving LDS.  The (c, eta) rows are the LDCBF half-spaces
 * lipmpc_plan_step_batch_c_eta solves against; they are bit-identical to what lipmpc_plan_step_batch derives from the
 * rings lipmpc_lidar_sense_batch writes.
 *  inputs as lipmpc_lidar_sense_batch
 *  c_eta [B,n_obs_max,4] (c_x, c_y, eta_x, eta_y) per inferred obstacle, cluster order; empty slots all zero;
 *        eta = NaN where the geometry is degenerate (CoM on the hull boundary, zero-length hull edge)
 *  n_inferred [B], overflow [B] as lipmpc_lidar_sense_batch
 *  obs_xy / obs_nv: the rings as well, or both NULL;  hits, labels: or NULL
 *  schedule: NULL (the robots are scanned in index order), or a device buffer of lipmpc_lidar_schedule_words(B) int32, contents
 *        arbitrary: scratch for the LAUNCH ORDER of this call.  A scan's length grows with its reading count, a whole batch of
 *        4096 robots is resident at once (16 waves per compute unit), and the launch lasts as long as its most loaded SIMD.  With
 *        the buffer the call first ranks its robots -- one small kernel estimates every robot's reading count (all rays for a
 *        robot inside an obstacle, else from the bounding circles of the obstacles in range), a one-workgroup counting sort
 *        turns the estimates into launch positions that give every SIMD a heavy robot with light ones -- and then starts
 *        the scans in that order (both included in the call: ~11 us per 4096 robots).  Nothing carries over
 *        from one call to the next; every order gives the same results; calls sharing a buffer must be stream-ordered. */
int lipmpc_lidar_c_eta_batch(int device, int64_t B, int32_t resolution, int32_t n_env, int32_t v_env,
                             int32_t env_shared, double lidar_range, double eps, int32_t min_samples,
                             int32_t n_obs_max, int32_t v_max, const double* state, const double* env_xy,
                             const int32_t* env_nv, const double* ray_table, const double* noise,
                             double* c_eta, int32_t* n_inferred, int32_t* overflow, double* obs_xy,
                             int32_t* obs_nv, double* hits, int32_t* labels, int32_t* schedule, void* hip_stream);
int64_t lipmpc_lidar_schedule_words(int64_t B);

/* One MPC step of the unknown-environment variant in ONE call (what HumanoidMPCUnknownEnvironment does per step,
 * HumanoidMPCUnknownEnvironment.py:30-68 + HumanoidMpc.py:387-418): lipmpc_lidar_c_eta_batch (scan, clusters, hulls,
 * closest point / normal: one launch, n_obs_max / v_max from the handle) followed on the same stream by
 * lipmpc_plan_step_batch_c_eta against those half-spaces and the scan's overflow flags (a robot whose scan overflowed gets
 * status SENSOR_OVERFLOW, not a plan).  c_eta [B,n_obs_max,4] is the hand-over buffer (and an output);
 * schedule as in lipmpc_lidar_c_eta_batch or NULL; every other argument as in the two functions. */
int lipmpc_sense_plan_step_batch(lipmpc_handle* h, int64_t B, int32_t resolution, int32_t n_env, int32_t v_env,
                                 int32_t env_shared, double lidar_range, double eps, int32_t min_samples,
                                 const double* state, const double* goal, const int8_t* first_foot, const double* delta,
                                 const double* env_xy, const int32_t* env_nv, const double* ray_table, const double* noise,
                                 double* c_eta, int32_t* n_inferred, int32_t* overflow, int32_t* schedule,
                                 double* U, double* X, double* theta, double* omega, double* obj, int32_t* status,
                                 int32_t* iters, uint64_t* active, uint64_t* working, double* diag, const double* bounds,
                                 void* hip_stream);

/* The unknown-environment front end on an OCCUPANCY GRID (backward-compatible addition): lipmpc_lidar_c_eta_batch with the true
 * map given as cells instead of vertex rings.  Only the ray casting differs; the readings then go through the same clustering,
 * hulls and constraint assembly in the same launch, and every output means what it means there.  (One convex hull per cluster
 * over-covers a concave wall, and the hull of a room's walls holds the robot standing in the room: such a robot gets a flipped
 * half-space and no feasible step.  lipmpc_lidar_grid_c_eta_split_batch cuts the clusters into sectors first.)
 *  occ    uint8, [W,H] if grid_shared else [B,W,H], DEVICE: cell (i, j) at occ[i * H + j], solid if nonzero
 *  origin (ox, oy), cell (dx, dy): two doubles each, HOST pointers read during the call; dx, dy > 0.  Cell (i, j) is the
 *         rectangle [ox + i dx, ox + (i+1) dx) x [oy + j dy, oy + (j+1) dy); everything outside the grid is free (a robot
 *         outside the grid sees into it)
 *  the rest as lipmpc_lidar_c_eta_batch; the robots are scanned in index order (no schedule).
 * THE SCAN, in IEEE double, no contraction, division and square root correctly rounded, every expression evaluated as written:
 *  - robot cell: ci = floor((x0 - ox) / dx), cj = floor((y0 - oy) / dy).  Unless |ci|, |cj| < 2^30 (NaN included) the robot
 *    has no reading.  If (ci, cj) is a solid cell of the grid NO SCAN IS MADE: n_inferred = 0, no reading, overflow = 1
 *    (lipmpc_sense_grid_plan_step_batch then gives LIPMPC_STATUS_SENSOR_OVERFLOW and NaN outputs: the scan is unusable).
 *  - ray i, as the polygon scan: e = (x0 + range * cos_i, y0 + range * sin_i), d = (e_x - x0, e_y - y0), points x0 + t d.
 *  - boundary crossings: with inv_x = 1 / d_x, the crossing of the x boundary of index a is t = ((ox + a * dx) - x0) * inv_x
 *    (a converted to double; y likewise with oy, dy, y0, inv_y).  The ray starts in (ci, cj) with t_x the crossing of
 *    a = ci + 1 if d_x > 0, of a = ci if d_x < 0, and +inf if d_x = 0; t_y likewise.
 *  - step: if t_x <= t_y (a tie goes to x) then t = t_x, ci += sign(d_x), t_x = the crossing of the next boundary that way
 *    (a = ci + 1 if d_x > 0 else ci, with the new ci); else the same in y.  The ray is now in cell (ci, cj), entered at t.
 *  - stop, without a reading: unless t <= 1 (NaN included), or when the cell is more than floor(range / dx) + 2 columns or
 *    floor(range / dy) + 2 rows from the robot's cell (no reading can lie there).
 *  - hit: the first solid cell of the grid so entered ends the ray.  Its reading q lies ON the boundary that was crossed:
 *    entered in x through the boundary of index a, q = (ox + a * dx, y0 + t * d_y); entered in y, q = (x0 + t * d_x,
 *    oy + a * dy) -- readings on one face of a wall are exactly collinear, as the polygon scan's are on an axis-parallel
 *    edge.  It is kept only if sqrt((q_x - x0)^2 + (q_y - y0)^2) < range, strictly, as in the polygon scan.  Noise is added
 *    to kept readings.
 * Reproduced bit for bit in numpy by tests/grid_lidar_oracle.py.
 * The window of cells a ray can reach, (2 floor(range / dx) + 5) x (2 floor(range / dy) + 5), is staged per robot as a
 * bitmap in the kernel's LDS: a (range, cell) pair whose window exceeds 49152 cells is refused with LIPMPC_E_UNSUPPORTED
 * before anything is enqueued.  Other refusals (LIPMPC_E_ARG): resolution outside 1..384, W or H < 1, a cell size that is
 * not positive and finite, a range that is negative or not finite, a null origin / cell / c_eta. */
int lipmpc_lidar_grid_c_eta_batch(int device, int64_t B, int32_t resolution, int32_t W, int32_t H, int32_t grid_shared,
                                  const double* origin, const double* cell, double lidar_range, double eps,
                                  int32_t min_samples, int32_t n_obs_max, int32_t v_max, const double* state,
                                  const uint8_t* occ, const double* ray_table, const double* noise, double* c_eta,
                                  int32_t* n_inferred, int32_t* overflow, double* obs_xy, int32_t* obs_nv, double* hits,
                                  int32_t* labels, void* hip_stream);

/* CLUSTERS SPLIT INTO SECTORS (backward-compatible addition): lipmpc_lidar_c_eta_batch / lipmpc_lidar_grid_c_eta_batch with a stage
 * between clustering and hulls, in the same launch, that cuts every cluster into PIECES of at most split_rays consecutive rays.
 * Every piece gets its own hull and its own (c, eta) row; wherever the two parents say "cluster" about hulls, slots and
 * overflow, these say "piece".  Why: the walls of a room the robot stands in are ONE cluster whose hull contains the robot.
 * For split_rays <= resolution / 2 the rays of a piece lie in an open half-plane through the robot, so the robot is an extreme
 * point of the cone that holds the piece's noise-free readings and cannot lie in their hull.
 *  split_rays  0: off -- every output bit-identical to the parent entry point's (which IS this call with 0 and NULL).
 *              < 0 or > resolution / 2: LIPMPC_E_ARG.
 *  pieces      [B,resolution] int32 or NULL: -2 no reading, -1 noise, else the number of the reading's piece in the order below,
 *              counted before any piece is dropped (with split_rays = 0 every cluster is one piece: the cluster's label).
 *  the rest as the parent entry point.
 * THE RULE, in integers, R = resolution.  For one cluster take the rays of its readings in ascending order, r_1 < ... < r_n
 * (DBSCAN noise belongs to no cluster and to no piece; border readings belong to their cluster):
 *  - gaps: g_t = (r_t - r_{t-1}) mod R with r_0 = r_n; for n = 1 the gap is R.
 *  - anchor: a = the r_t with the largest g_t, the smallest such r_t on a tie (a cluster holding every ray anchors at ray 0).
 *  - offsets: o_t = (r_t - a) mod R;  extent: E = max o_t + 1;  piece count: n_p = ceil(E / split_rays).
 *  - piece of reading t: p_t = floor(o_t * n_p / E) -- balanced pieces, each within split_rays consecutive rays; a cluster
 *    with E <= split_rays stays whole.
 * Pieces are numbered cluster by cluster (clusters in label order) and inside a cluster by ascending p.  Each piece then goes
 * through the hull and the constraint assembly as a cluster does: a piece with fewer than 3 extreme points takes no slot, the
 * others fill the slots in piece order, and overflow = 1 if more than 64 pieces exist (the kernel stages 64; then, as with more
 * than 64 clusters, nothing but the flag is defined about slots and `pieces`) or if the pieces do not fit n_obs_max / v_max.
 * Reproduced bit for bit in numpy by tests/lidar_split_oracle.py.
 * There is no split twin of the lipmpc_sense_*plan_step_batch calls: issue the scan and lipmpc_plan_step_batch_c_eta. */
int lipmpc_lidar_c_eta_split_batch(int device, int64_t B, int32_t resolution, int32_t n_env, int32_t v_env,
                                   int32_t env_shared, double lidar_range, double eps, int32_t min_samples,
                                   int32_t n_obs_max, int32_t v_max, const double* state, const double* env_xy,
                                   const int32_t* env_nv, const double* ray_table, const double* noise,
                                   double* c_eta, int32_t* n_inferred, int32_t* overflow, double* obs_xy,
                                   int32_t* obs_nv, double* hits, int32_t* labels, int32_t* schedule,
                                   int32_t split_rays, int32_t* pieces, void* hip_stream);
int lipmpc_lidar_grid_c_eta_split_batch(int device, int64_t B, int32_t resolution, int32_t W, int32_t H, int32_t grid_shared,
                                        const double* origin, const double* cell, double lidar_range, double eps,
                                        int32_t min_samples, int32_t n_obs_max, int32_t v_max, const double* state,
                                        const uint8_t* occ, const double* ray_table, const double* noise, double* c_eta,
                                        int32_t* n_inferred, int32_t* overflow, double* obs_xy, int32_t* obs_nv, double* hits,
                                        int32_t* labels, int32_t split_rays, int32_t* pieces, void* hip_stream);

/* lipmpc_sense_plan_step_batch on an occupancy grid: lipmpc_lidar_grid_c_eta_batch (n_obs_max / v_max from the handle), then on
 * the same stream lipmpc_plan_step_batch_c_eta against those half-spaces and the scan's overflow flags -- a robot whose
 * clusters did not fit, or that stands in a solid cell, gets LIPMPC_STATUS_SENSOR_OVERFLOW and NaN outputs. */
int lipmpc_sense_grid_plan_step_batch(lipmpc_handle* h, int64_t B, int32_t resolution, int32_t W, int32_t H, int32_t grid_shared,
                                      const double* origin, const double* cell, double lidar_range, double eps,
                                      int32_t min_samples, const double* state, const double* goal, const int8_t* first_foot,
                                      const double* delta, const uint8_t* occ, const double* ray_table, const double* noise,
                                      double* c_eta, int32_t* n_inferred, int32_t* overflow,
                                      double* U, double* X, double* theta, double* omega, double* obj, int32_t* status,
                                      int32_t* iters, uint64_t* active, uint64_t* working, double* diag, const double* bounds,
                                      void* hip_stream);

/* SCAN INTEGRATION (backward-compatible addition): one call adds one scan per robot to an occupancy-EVIDENCE grid -- the memory
 * between the scans and lipmpc_rrt_plan_grid_batch.  Asynchronous on hip_stream; no allocation and no host synchronisation, so
 * the call can be captured in a graph.
 *  W, H, grid_shared, origin, cell: the grid's geometry exactly as lipmpc_lidar_grid_c_eta_batch takes it (the same cell
 *             rectangles, the same i * H + j layout; origin / cell HOST pointers).  It need not be the geometry of the map scanned.
 *  state      [B,5]  only (p_x, p_y) = p0 are read
 *  hits       [B,resolution,2] as the scans write them: a NaN coordinate = the ray has no reading
 *  ray_table  [resolution,2] as the scans take it; lidar_range as the scan's
 *  mask       [B] int32 or NULL: a robot with mask == 0 is skipped (a fleet passes `walking`)
 *  w_hit, w_miss  integer weights, each 1..32767;  depth >= 0, finite (a caller's default: half the smaller cell size)
 *  evidence   int32, [W,H] if grid_shared else [B,W,H], updated IN PLACE
 * THE UPDATE, in IEEE double, no contraction, division and square root correctly rounded, every expression evaluated as written:
 *  - robot cell (ci, cj) as the grid scan's: floor((x0 - ox) / dx), floor((y0 - oy) / dy).  A robot with mask == 0, or unless
 *    |ci|, |cj| < 2^30 (a NaN or infinite position included), contributes nothing.
 *  - window: nx = floor((lidar_range + depth) / dx) + 2 columns, ny likewise rows: only cells (i, j) with |i - ci| <= nx and
 *    |j - cj| <= ny are updated.
 *  - ray i WITH a reading q: d = (q_x - x0, q_y - y0), L = sqrt(d_x * d_x + d_y * d_y), s = depth / L, the END POINT
 *    e = (q_x + s * d_x, q_y + s * d_y).  If L == 0 or L, e_x or e_y is not finite the ray contributes nothing.  The HIT CELL is
 *    (floor((e_x - ox) / dx), floor((e_y - oy) / dy)); a hit cell outside the window is dropped (the ray still marches).
 *    Why depth: a grid scan's reading lies exactly ON the face of the solid cell, so for a ray travelling toward -x or -y the
 *    floor of the reading itself names the free neighbour; the overshoot puts the hit inside the wall.
 *  - ray i WITHOUT a reading: e = (x0 + lidar_range * cos_i, y0 + lidar_range * sin_i), as the scan forms it; no hit cell.
 *  - the march from p0 to e, by the rules of the grid scan above with r = (e_x - x0, e_y - y0) in the place of its d: crossings
 *    recomputed from the boundary's index, x on a tie, the ray then in the next cell of that axis, entered at t.  The robot's own
 *    cell is visited first.  The ray stops, the cell just entered NOT visited: unless t <= 1 (NaN included); when that cell is
 *    outside the window; when it is the hit cell.  Every visited cell that is not the ray's hit cell is PASSED by the ray.
 *  - ONE UPDATE PER CELL, ROBOT AND CALL: a cell of the window that is the hit cell of any ray of the scan gets + w_hit; a cell
 *    otherwise passed by any ray gets - w_miss (hit wins over passed).  Cells outside the grid are ignored.  Plain int32
 *    addition, NO SATURATION: the sum wraps beyond int32 (no sooner than after 65536 updates of one cell at the largest weight).
 *  - shared map: all robots add into the one grid with integer atomics.  Integer addition commutes, so the result does not
 *    depend on the launch order or on how the atomics fell: two calls from the same inputs give identical bits, and the shared
 *    map is the sum of the per-robot maps.
 * Reproduced integer for integer in numpy by tests/map_oracle.py.
 * The window, (2 nx + 1) x (2 ny + 1) cells, is kept per robot as two bitmaps (passed, hit) in the kernel's LDS: a (range + depth,
 * cell) pair whose window exceeds 49152 cells (2 x 6 KiB) is refused with LIPMPC_E_UNSUPPORTED before anything is enqueued.
 * Other refusals (LIPMPC_E_ARG): resolution outside 1..384, W or H < 1, a cell size that is not positive and finite, a range
 * or a depth that is negative or not finite, a weight outside 1..32767, a null state / hits / ray_table / evidence / origin / cell. */
int lipmpc_map_update_batch(int device, int64_t B, int32_t resolution, int32_t W, int32_t H, int32_t grid_shared,
                            const double* origin, const double* cell, double lidar_range, double depth, int32_t w_hit,
                            int32_t w_miss, const double* state, const double* hits, const double* ray_table,
                            const int32_t* mask, int32_t* evidence, void* hip_stream);

/* CORRELATIVE SCAN MATCHING (backward-compatible addition): lipmpc_scan_match_batch -- where a robot is ON THE MAP IT BUILDS.  Per
 * robot a window of candidate poses (whole-cell shifts (a, b) of the believed position and a table of yaws) is scored by the
 * evidence under the scan's hit cells, and the best candidate is returned (Olson 2009, over whole cells).  The evidence is only
 * read.  Asynchronous on hip_stream; no allocation and no host synchronisation, so the call can be captured in a graph.
 *  resolution, W, H, grid_shared, origin, cell, lidar_range, depth: as lipmpc_map_update_batch takes them
 *  n_x, n_y   0..16: the search half-widths in cells;  n_yaw 0..16: the yaw half-width, T = 2 n_yaw + 1 yaws
 *  rot_table  [T,2] doubles on the device: (cos, sin) of (k - n_yaw) * yaw_step as the caller evaluated them (numpy); may be NULL
 *             only when n_yaw == 0; entry n_yaw is never read (it stands for (1, 0))
 *  clamp      1..127;  min_score any int32;  min_gain >= 0
 *  state      [B,5]  the BELIEVED pose; only (p_x, p_y) = p0 are read
 *  hits       [B,resolution,2] the readings as placed at that pose, a NaN coordinate = no reading
 *  mask       [B] int32 or NULL: a robot with mask == 0 gets zeros in every output and nothing else of it is read
 *  evidence   int32, [W,H] if grid_shared else [B,W,H], READ ONLY (plain reads: order the call before an update by the stream)
 * THE RULE, in IEEE double, no contraction, division and square root correctly rounded, every expression evaluated as written:
 *  - robot cell c0 = (ci, cj), the window half-widths (mx, my) and, for reading r, the END POINT e_r with its validity tests:
 *    exactly lipmpc_map_update_batch's (mx, my are its nx, ny).  A robot without a cell gets zeros in every output.
 *  - yaw index k = n_yaw: the rotated end point is e_r itself, NO ARITHMETIC -- the zero candidate scores exactly the cells the
 *    update would raise.  Any other k, with (c, s) = rot_table[k] and (rx, ry) = (e_x - x0, e_y - y0):
 *    x = x0 + (c * rx - s * ry), y = y0 + (s * rx + c * ry).
 *  - its cell (i, j): fi' = floor((x - ox) / dx), fj' = floor((y - oy) / dy).  The pair (r, k) is USED if r has a valid end point
 *    and |fi' - ci| <= mx and |fj' - cj| <= my, the differences taken in double as the update takes them (so an index too large
 *    for an int, an infinity or a NaN is simply not used); then i = ci + (fi' - ci), j likewise.
 *  - V(i, j) = min(max(evidence(i, j), -clamp), clamp) inside the map, 0 outside.
 *  - score(k, a, b) = sum over the used (r, k) of V(i + a, j + b), |a| <= n_x, |b| <= n_y: every reading counts, also two in a cell.
 *  - THE BEST candidate minimises (-score, a * a + b * b, |k - n_yaw|, k, (a + n_x) * (2 n_y + 1) + (b + n_y)) lexicographically:
 *    integers and a total order, so the result does not depend on thread order; an empty map returns the zero candidate.
 *  - it is ACCEPTED if score_best >= min_score and score_best - score_zero >= min_gain (score_zero: k = n_yaw, a = b = 0);
 *    otherwise the zero candidate is returned.
 * OUTPUTS, all written for every robot:
 *  offset_cells [B,2] int32 (a, b);  yaw_index [B] int32 k - n_yaw;  offset [B,2] double (a * dx, b * dy), one product each
 *  score      [B,2] int32: the best candidate's BEFORE the acceptance test, and the zero candidate's
 *  n_used     [B] int32: the used pairs at k = n_yaw;  matched [B] int8: accepted and not the zero candidate
 * Reproduced bit for bit in numpy by tests/scan_match_oracle.py.
 * The update's window grown by (n_x, n_y), (2 (mx + n_x) + 1) x (2 (my + n_y) + 1) cells, is kept as one signed byte per cell in
 * the kernel's LDS: more than 49152 cells are refused with LIPMPC_E_UNSUPPORTED before anything is enqueued.  Other refusals
 * (LIPMPC_E_ARG): what lipmpc_map_update_batch refuses of the shared arguments, n_x, n_y or n_yaw outside 0..16, clamp outside
 * 1..127, min_gain < 0, n_yaw > 0 with a null rot_table, a null state / hits / evidence / output / origin / cell.  B == 0
 * enqueues nothing. */
int lipmpc_scan_match_batch(int device, int64_t B, int32_t resolution, int32_t W, int32_t H, int32_t grid_shared,
                            const double* origin, const double* cell, double lidar_range, double depth, int32_t n_x, int32_t n_y,
                            int32_t n_yaw, const double* rot_table, int32_t clamp, int32_t min_score, int32_t min_gain,
                            const double* state, const double* hits, const int32_t* mask, const int32_t* evidence,
                            int32_t* offset_cells, int32_t* yaw_index, double* offset, int32_t* score, int32_t* n_used,
                            int8_t* matched, void* hip_stream);

/* RRT* SUB-GOAL PLANNER (backward-compatible addition): the global planner of HumanoidMPCWithRRT
 * (HumanoidMPCVariants/HumanoidMPCWithRRT.py:21-135) for B independent problems, one workgroup per problem.  Per problem b:
 *  - bounds: min / max over {start_x, goal_x, every ring vertex x} -/+ margin, the same for y (the reference's origin is
 *    `start`, NULL = (0, 0) as there); H = ceil(W * ((max_y - min_y) / (max_x - min_x))), W = width.
 *    world -> cell: rint(((x - min_x) / (max_x - min_x)) * W) (half to even, as np.round), H for y; cell -> world:
 *    min_x + ((i * (max_x - min_x)) / W).  The grid is (W+1) x (H+1) cells, cell index i * (H+1) + j.
 *  - occupancy: cell (i, j) is occupied if for some ring xmin <= i < xmax and ymin <= j < ymax over its ROUNDED vertices and
 *    (i, j) lies in the closed convex hull of those rounded vertices (exact integer orientation tests).
 *  - d2: exact squared Euclidean distance to the nearest occupied cell (0 on occupied cells); C = exp(-sqrt(d2)).
 *  - draw k = 0, 1, ... of seed s: z = splitmix64 finaliser of (s + (k+1) * 0x9E3779B97F4A7C15), cell ((z >> 32) * ncells)
 *    >> 32; a draw on an occupied, the start or the goal cell is skipped and is not a sample; at most 64 * n_samples draws.
 *  - RRT* per sample x: v_near = nearest vertex (integer |p_v - x|^2, lowest index on ties); the sample is dropped (it still
 *    counts) if that distance is 0 or the segment v_near -> x is blocked.  Near set = {v : |p_v - x|^2 <= r_rewire^2} +
 *    v_near.  Parent = argmin over near vertices with a free segment of cost(v) + C[x] * sqrt(|p_v - x|^2) (lowest index on
 *    ties).  Rewire, against the costs before this sample: every near u != parent with a free segment and
 *    cost(x) + C[u] * len(x, u) < cost(u) takes x as parent; then the costs of x's subtree are recomputed top-down,
 *    cost(v) = cost(parent(v)) + C[v] * len(parent(v), v).
 *  - segment a -> b: endpoints in lexicographic order, m = max(|dx|, |dy|), cells a + floor((2 k d + m) / (2 m)), k = 0..m;
 *    free if none is occupied.
 *  - goal: its parent is the argmin of cost(v) + C[goal] * len over vertices within r_rewire with a free segment.
 *  - output: the tree path without the root, ending with the goal CELL, in world coordinates.
 * A problem's result depends only on its own inputs and seed.  Reproduced in numpy by tests/rrt_oracle.py. */
#define LIPMPC_RRT_FOUND            0
#define LIPMPC_RRT_NO_PATH          1  /* no vertex within r_rewire of the goal has a free segment to it */
#define LIPMPC_RRT_START_OCCUPIED   2
#define LIPMPC_RRT_GOAL_OCCUPIED    3
#define LIPMPC_RRT_GRID_TOO_LARGE   4  /* (W+1)(H+1) > max_cells or H+1 > 4096 */
#define LIPMPC_RRT_NO_OBSTACLE_GRID 5  /* no occupied cell: the distance transform is not defined */
#define LIPMPC_RRT_PATH_OVERFLOW    6  /* the path has more than S_max sub-goals (path_cost is still written) */
#define LIPMPC_RRT_OUTSIDE_GRID     7  /* lipmpc_rrt_plan_grid_batch only: the start or the goal rounds to a cell outside the given grid */
#define LIPMPC_RRT_FIELD_UNSETTLED  8  /* the tiled path calls only: the robot's field has settled == 0 (more rounds are needed) */

typedef struct lipmpc_rrt_params {
  int32_t width;        /* W, grid cells across x minus one: 1..4095           (width_grid_size, :102) */
  int32_t n_samples;    /* RRT* samples                                          (n=1500, :127) */
  int32_t r_rewire;     /* near radius in cells, 1..8192                          (r_rewire=80, :127) */
  int32_t max_cells;    /* cap on (W+1)(H+1): the tree kernel keeps the occupancy bitmap of this many cells in LDS */
  double margin;        /* world margin around start, goal and obstacles          (3, :46-49) */
} lipmpc_rrt_params;

/* fills *p with 250, 1500, 80, 2^17 cells (16 KiB of bitmap, about 57 KiB of LDS per problem with the tree), 3.0 */
int lipmpc_rrt_default_params(lipmpc_rrt_params* p);
/* device workspace for B problems (contents arbitrary); < 0 if the parameters are invalid or the tree and bitmap do not
 * fit the 160 KiB of LDS: 28 (n_samples + 1) + max_cells / 8 + 256 bytes */
int64_t lipmpc_rrt_workspace_bytes(const lipmpc_rrt_params* p, int64_t B);
/* All pointers are DEVICE pointers; asynchronous on hip_stream.
 *  obs_xy [B,n_obs_max,v_max,2], obs_nv [B,n_obs_max]: as lipmpc_plan_step_batch (any ring of >= 1 vertex is an obstacle,
 *         v_max <= 64); start [B,2] or NULL (= origin); goal [B,2]; seed [B] uint64
 * outputs
 *  sub_goals [B,S_max,2]: rows 0..n_sub[b]-1 written (FOUND only), the rest untouched; n_sub [B] (0 unless FOUND);
 *  status [B] LIPMPC_RRT_*; path_cost [B] cost of the goal (NaN unless FOUND / PATH_OVERFLOW)
 *  grid_dims [B,2] (W+1, H+1) or NULL
 *  occ_d2 [B,max_cells] int32 or NULL: d2 of cell i*(H+1)+j for the first (W+1)(H+1) cells (0 = occupied; -1 everywhere on a
 *         NO_OBSTACLE_GRID problem; untouched if GRID_TOO_LARGE)
 *  cost_grid [B,max_cells] or NULL: C likewise (NaN on a NO_OBSTACLE_GRID problem)
 *  tree [B,n_samples+2,4] or NULL: row 0 (vertex count V, goal's parent or -1, draws used, samples), row 1+v
 *         (cell i, cell j, parent or -1, cost) for v < V; 0 for a problem whose status is decided before the tree. */
int lipmpc_rrt_plan_batch(int device, const lipmpc_rrt_params* p, int64_t B, const double* obs_xy, const int32_t* obs_nv,
                          int32_t n_obs_max, int32_t v_max, const double* start, const double* goal, const uint64_t* seed,
                          void* workspace, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                          int32_t* grid_dims, int32_t* occ_d2, double* cost_grid, double* tree, int32_t S_max,
                          void* hip_stream);

/* The planner on a GIVEN occupancy grid (backward-compatible addition): lipmpc_rrt_plan_batch with the occupancy taken from
 * `occ` instead of rasterised rings -- a GridMap, e.g. the thresholded evidence of lipmpc_map_update_batch.
 *  W, H, grid_shared, origin, cell, occ: the grid as lipmpc_lidar_grid_c_eta_batch takes it (occ uint8 DEVICE, [W,H] if
 *         grid_shared else [B,W,H], cell (i, j) at occ[i * H + j], occupied if nonzero; origin / cell HOST pointers); W, H >= 2
 *  the planner's grid of problem b is the W x H cell CENTRES: min = origin + cell / 2, max = origin + (W - 1/2) * cell per
 *         axis, W_p = W - 1, H_p = H - 1 -- the inverse of the placement GridMap.from_planner gives a planner grid -- and
 *         world <-> cell are the maps of lipmpc_rrt_plan_batch with those bounds; cell index i * H + j; grid_dims = (W, H)
 *  p->width and p->margin are ignored (and not checked)
 *  status: LIPMPC_RRT_GRID_TOO_LARGE if W * H > max_cells or H > 4096 or W > 4096; else LIPMPC_RRT_OUTSIDE_GRID if the rounded
 *         cell of the start or the goal is not a cell of the grid (a NaN coordinate included); both are decided before the
 *         distance transform (occ_d2 / cost_grid untouched); then as lipmpc_rrt_plan_batch
 * Distance transform, sampler, tree and outputs, the workspace and every other status: exactly lipmpc_rrt_plan_batch's (the
 * same kernels).  LIPMPC_E_ARG: W or H < 2, a cell size that is not positive and finite, an origin that is not finite, a null
 * origin / cell / occ, and what lipmpc_rrt_plan_batch refuses.  Restated in numpy by tests/rrt_grid_oracle.py. */
int lipmpc_rrt_plan_grid_batch(int device, const lipmpc_rrt_params* p, int64_t B, int32_t W, int32_t H, int32_t grid_shared,
                               const double* origin, const double* cell, const uint8_t* occ, const double* start,
                               const double* goal, const uint64_t* seed, void* workspace, double* sub_goals, int32_t* n_sub,
                               int32_t* status, double* path_cost, int32_t* grid_dims, int32_t* occ_d2, double* cost_grid,
                               double* tree, int32_t S_max, void* hip_stream);

/* GRID FIELD PLANNER (backward-compatible addition): a COMPLETE, DETERMINISTIC global planner on an occupancy grid.  A
 * cost-to-go field from a goal cell (lipmpc_grid_field_batch) and, down that field, sub-goals for any number of robots
 * (lipmpc_grid_path_batch).  A path that exists is found, it is a shortest one in the metric below, there is no seed, and one
 * field serves every robot that shares the map and the goal.  Both calls: all pointers DEVICE pointers but origin / cell (HOST);
 * asynchronous on hip_stream; no allocation and no host synchronisation, so they can be captured in a graph; every refusal is a
 * return code decided on the host before anything is enqueued.
 *
 * lipmpc_grid_field_batch: F fields, one workgroup per field.
 *  W, H, grid_shared, origin, cell, occ: the grid as lipmpc_rrt_plan_grid_batch takes it (occ uint8, [W,H] if grid_shared else
 *         [F,W,H], cell (i, j) at occ[i * H + j]; the cell rectangles of lipmpc_lidar_grid_c_eta_batch); W, H >= 2
 *  goal   [F,2];  r_inflate  0..16, in cells (e.g. the body radius over the cell size, rounded up)
 *  field  [F,W,H] uint32, layout i * H + j;  field_status [F] int32
 * THE FIELD of one goal:
 *  - solid(c) <=> occ[c] != 0.  blocked(i, j) <=> some solid cell (i', j') OF THE GRID has (i - i')^2 + (j - j')^2 <= r_inflate^2.
 *    There are no cells outside the grid: nothing outside blocks, and no move leaves the grid.
 *  - goal cell: (floor((g_x - ox) / dx), floor((g_y - oy) / dy)), the grid scan's robot-cell rule, in IEEE double.
 *  - field_status: LIPMPC_FIELD_OK; LIPMPC_FIELD_GOAL_OUTSIDE if the goal cell is outside the grid (a NaN coordinate included);
 *    else LIPMPC_FIELD_GOAL_BLOCKED if it is blocked.  On a non-zero status the whole field is 0xFFFFFFFF (INF).
 *  - moves go between unblocked cells, 8-connected; an axial step costs 5, a diagonal step 7.  A diagonal (di, dj) from (i, j)
 *    is allowed only if (i + di, j) and (i, j + dj) are both unblocked (no corner is cut).
 *  - field[c] = the least total cost from c to the goal cell; INF if there is no path or c is blocked.
 *  The metric counts CELLS: on a grid with dx != dy lengths are in cells, not in metres.
 *  The least cost is unique, so the field does not depend on the order in which the kernel relaxes its cells: two calls give
 *  identical bits.  The field is kept in LDS, sized to the map, when 4 W H bytes beside the blocked bitmap (W H / 8 bytes) fit the
 *  160 KiB of a workgroup (up to about 39,700 cells; a 92 x 80 map takes 30 KiB); a larger map is relaxed in `field` itself.
 * LIPMPC_E_UNSUPPORTED: W * H > 2^17, W > 4096 or H > 4096 (the RRT planner's caps).  LIPMPC_E_ARG: F < 0, W or H < 2, a cell
 *  size that is not positive and finite, an origin that is not finite, r_inflate outside 0..16, a null origin / cell / occ / goal /
 *  field / field_status.  F = 0 enqueues nothing and returns 0. */
#define LIPMPC_FIELD_OK            0
#define LIPMPC_FIELD_GOAL_OUTSIDE  1
#define LIPMPC_FIELD_GOAL_BLOCKED  2
#define LIPMPC_FIELD_INF           0xFFFFFFFFu
int lipmpc_grid_field_batch(int device, int64_t F, int32_t W, int32_t H, int32_t grid_shared, const double* origin,
                            const double* cell, const uint8_t* occ, const double* goal, int32_t r_inflate, uint32_t* field,
                            int32_t* field_status, void* hip_stream);

/* lipmpc_grid_path_batch: B robots, one lane per robot, each down a field of lipmpc_grid_field_batch.
 *  F      1 or B: robot b uses field f = (F == 1 ? 0 : b) -- with F = 1 every robot descends the one field
 *  W, H, origin, cell, occ, grid_shared, goal [F,2], r_inflate: what the field call was given (occ [W,H] if grid_shared else [F,W,H])
 *  field [F,W,H], field_status [F]: its outputs;  start [B,2]
 *  max_seg  >= 5, in field units: the spacing cap of the sub-goals (a value no field reaches, e.g. 2^31 - 1: no cap)
 *  sub_goals [B,S_max,2], n_sub [B], status [B] (LIPMPC_RRT_*: everything downstream of the RRT planner reads them unchanged),
 *  path_cost [B]
 * PER ROBOT, passable(c) <=> field[c] != INF:
 *  - status, the first that applies: field_status[f] is GOAL_OUTSIDE -> LIPMPC_RRT_OUTSIDE_GRID; is GOAL_BLOCKED ->
 *    LIPMPC_RRT_GOAL_OCCUPIED; the start cell (floor rule) is outside the grid -> LIPMPC_RRT_OUTSIDE_GRID; the start cell is
 *    solid -> LIPMPC_RRT_START_OCCUPIED.
 *  - SNAP: if the start cell is not passable (a robot walks closer to walls than r_inflate), the start becomes the cell with a
 *    finite field within Chebyshev distance r_inflate + 1 of it that has the least (d^2, field, index), d^2 = di^2 + dj^2,
 *    index = i * H + j; LIPMPC_RRT_NO_PATH if there is none.
 *  - DESCENT: from cell c the next cell is the first neighbour n in the order (-1,-1), (-1,0), (-1,1), (0,-1), (0,1), (1,-1),
 *    (1,0), (1,1) with field[n] + cost == field[c], a diagonal only past two passable side cells; it ends where the field is 0.
 *    The path is c_0 (the start after the snap), c_1, ..., c_L (the goal cell).
 *  - SUB-GOALS BY STRING PULLING: the anchor a is c_0.  Walking k = 1, 2, ...: when LOS(a, c_k) fails, or the path cost since the
 *    anchor, field[a] - field[c_k], reaches max_seg, the centre of c_{k-1} is emitted -- of c_k if c_{k-1} is the anchor itself
 *    -- the emitted cell becomes the anchor and the walk goes on from the cell after it.  LOS is the RRT planner's segment rule:
 *    endpoints in lexicographic order, m = max(|di|, |dj|), cells a + floor((2 k d + m) / (2 m)), k = 0..m, every one passable.
 *    A cell centre is (ox + (i + 0.5) * dx, oy + (j + 0.5) * dy), evaluated as written in double, no contraction.
 *    The goal cell's centre is never emitted: the LAST sub-goal is the given goal[f], bit for bit (a caller recognises the
 *    arrival at its final goal by equality).
 *  - outputs: LIPMPC_RRT_FOUND with n_sub >= 1 rows written, rows from n_sub on untouched; more than S_max sub-goals ->
 *    LIPMPC_RRT_PATH_OVERFLOW, nothing written; n_sub = 0 unless FOUND; path_cost = field[start cell after the snap] / 5.0, the
 *    path's length in cells (NaN unless FOUND / PATH_OVERFLOW).  A `field` that is no cost-to-go field of this map (no neighbour
 *    satisfies the descent) ends LIPMPC_RRT_NO_PATH.
 * Restated in numpy by tests/field_oracle.py (Dijkstra); the device's outputs equal it bit for bit.
 * LIPMPC_E_UNSUPPORTED as the field call.  LIPMPC_E_ARG: what the field call refuses, B < 0, F neither 1 nor B, max_seg < 5,
 *  S_max < 1, a null pointer.  B = 0 enqueues nothing and returns 0. */
int lipmpc_grid_path_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin, const double* cell,
                           const uint8_t* occ, int32_t grid_shared, const uint32_t* field, const int32_t* field_status,
                           const double* goal, const double* start, int32_t r_inflate, int32_t max_seg, int32_t S_max,
                           double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, void* hip_stream);

/* FRONTIER EXPLORER (backward-compatible addition): where to walk when nobody hands over a goal -- nearest-frontier exploration
 * (Yamauchi 1997) on the evidence grid of lipmpc_map_update_batch.  A FRONTIER cell is a cell a robot can stand in that touches
 * cells nobody has decided yet; lipmpc_grid_frontier_field_batch finds them and relaxes the cost-to-go to the NEAREST one, and
 * lipmpc_grid_frontier_path_batch sends any number of robots down that field.  On a shared map one field serves every robot.
 * Everything compared is an integer, as in the grid field planner.  Both calls: all pointers DEVICE pointers but origin / cell
 * (HOST); asynchronous on hip_stream; no allocation and no host synchronisation, so they can be captured in a graph; every
 * refusal is a return code decided on the host before anything is enqueued.
 *
 * lipmpc_grid_frontier_field_batch: F maps, one workgroup per map.
 *  evidence   [F,W,H] int32, layout i * H + j, as lipmpc_map_update_batch leaves it (a shared map: F = 1)
 *  t_free, t_occ  1..2^30 (a mapper's w_miss and w_hit);  r_inflate 0..16, in cells;  min_unknown 1..8
 *  frontier   [F,W,H] uint8 or NULL;  field [F,W,H] uint32;  n_frontier [F] int32
 * THE FIELD of one map, e = evidence[c]:
 *  - solid(c) <=> e >= t_occ;  free(c) <=> e <= -t_free;  unknown(c) <=> neither.  Exact for every int32 value, INT32_MIN and
 *    INT32_MAX included (two plain comparisons; with both thresholds >= 1 no cell is solid and free).
 *  - blocked(i, j) <=> !free(i, j), or some solid cell (i', j') OF THE GRID has (i - i')^2 + (j - j')^2 <= r_inflate^2: the
 *    inflation of lipmpc_grid_field_batch, applied to solid cells only.  Unknown cells are impassable but not inflated.
 *  - frontier(c) <=> !blocked(c) and at least min_unknown of the cell's 8 neighbours INSIDE THE GRID are unknown.  Nothing
 *    outside the grid counts: the grid's edge is no frontier.
 *  - moves, the costs 5 / 7 and the no-corner-cut rule: lipmpc_grid_field_batch's, between unblocked cells.
 *  - field[c] = the least total cost from c to ANY frontier cell: 0 on frontier cells, LIPMPC_FIELD_INF on blocked cells and on
 *    cells from which no frontier can be reached.
 *  - n_frontier[f] = the number of frontier cells.  With 0 the whole field is INF: nothing left to explore, not an error.
 *  - frontier, if given: 1 on frontier cells, 0 elsewhere.
 *  The least cost is unique for several sources as for one, so two calls give identical bits; n_frontier is an integer sum.
 *  The field is kept in LDS, sized to the map, when 4 W H bytes beside three bitmaps (solid, unknown, blocked) fit the 160 KiB of
 *  a workgroup: 4 (3 (2 ceil(W H / 64) + 2) + 2 + W H) + 256 <= 163840, up to about 37,300 cells; a larger map is relaxed in
 *  `field`.
 * LIPMPC_E_ARG: F < 0, W or H < 2, t_free or t_occ outside 1..2^30, r_inflate outside 0..16, min_unknown outside 1..8, a null
 *  evidence / field / n_frontier (whatever F).  Then LIPMPC_E_UNSUPPORTED: W * H > 2^17, W > 4096 or H > 4096.  Then F = 0
 *  enqueues nothing and returns 0. */
int lipmpc_grid_frontier_field_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence, int32_t t_free,
                                     int32_t t_occ, int32_t r_inflate, int32_t min_unknown, uint8_t* frontier, uint32_t* field,
                                     int32_t* n_frontier, void* hip_stream);

/* lipmpc_grid_frontier_path_batch: B robots, one lane per robot, each to the nearest frontier of its map.
 *  F      1 or B: robot b uses map and field f = (F == 1 ? 0 : b)
 *  W, H, evidence [F,W,H], t_occ, r_inflate: what the field call was given;  origin, cell: the grid's placement, as
 *         lipmpc_grid_path_batch takes it;  field [F,W,H], n_frontier [F]: the field call's outputs;  start [B,2]
 *  max_seg, S_max, sub_goals [B,S_max,2], n_sub [B], status [B] (LIPMPC_RRT_*), path_cost [B]: lipmpc_grid_path_batch's
 *  target_cell [B] int32
 * PER ROBOT this is lipmpc_grid_path_batch, passable(c) <=> field[c] != INF, with these differences and no others:
 *  - status, the first that applies: the start cell (floor rule) is outside the grid (a NaN coordinate included) ->
 *    LIPMPC_RRT_OUTSIDE_GRID; evidence[start cell] >= t_occ -> LIPMPC_RRT_START_OCCUPIED; n_frontier[f] == 0, or the snap finds
 *    no finite cell -> LIPMPC_RRT_NO_PATH.
 *  - the descent ends at the first cell c_L whose field is 0: a frontier cell.
 *  - the LAST sub-goal is the CENTRE of c_L, (ox + (i + 0.5) * dx, oy + (j + 0.5) * dy) as written, no contraction.  A start
 *    that is itself a frontier cell gives n_sub = 1, its own centre.
 *  - target_cell[b] = the index i * H + j of c_L; -1 unless the status is FOUND or PATH_OVERFLOW.
 *  The snap's window and key, the descent's order, the string pulling, max_seg, S_max, path_cost = field[start cell after the
 *  snap] / 5.0 (NaN unless FOUND / PATH_OVERFLOW), n_sub = 0 unless FOUND and "rows from n_sub on untouched" are word for word
 *  lipmpc_grid_path_batch's.
 * Restated in numpy by tests/frontier_oracle.py (multi-source Dijkstra); the device's outputs equal it bit for bit.
 * LIPMPC_E_ARG: B < 0, F neither 1 nor B, max_seg < 5, S_max < 1, t_occ outside 1..2^30, W or H < 2, a cell size that is not
 *  positive and finite, an origin that is not finite, r_inflate outside 0..16, a null pointer.  LIPMPC_E_UNSUPPORTED as the field
 *  call.  B = 0 enqueues nothing and returns 0. */
int lipmpc_grid_frontier_path_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                    const double* cell, const int32_t* evidence, int32_t t_occ, const uint32_t* field,
                                    const int32_t* n_frontier, const double* start, int32_t r_inflate, int32_t max_seg,
                                    int32_t S_max, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                    int32_t* target_cell, void* hip_stream);

/* lipmpc_grid_frontier_assign_batch (backward-compatible addition): COORDINATED exploration.  The path call sends every robot
 * to ITS nearest frontier cell, so robots side by side pick the same one.  This call runs after it on ONE shared map and lets
 * the robots claim frontier targets apart: the classic greedy rule (Burgard et al. 2005) with the utility discount taken as
 * "within r_claim cells of a claimed target = already taken", stated in integers.  One workgroup does the whole call.
 *  B robots, one map (F = 1);  W, H, origin, cell, r_inflate, max_seg, S_max, start [B,2]: what the path call was given
 *  frontier [W,H] uint8, field [W,H] uint32: the outputs of lipmpc_grid_frontier_field_batch (F = 1); both are only read
 *  may_claim [B] int8 or NULL (= every robot may);  r_claim 0..4096, in cells;  max_claims 0..4096
 *  work [W,H] uint32: scratch, contents arbitrary on entry and on return; it overlaps nothing else
 *  sub_goals, n_sub, status, path_cost, target_cell: the outputs of lipmpc_grid_frontier_path_batch (F = 1) for the same map and
 *    start -- read, and rewritten for the robots that claim
 *  claim_round [B] int32, n_claims [1] int32: written whole
 * THE RULE:
 *  - passable(c) <=> the given field[c] != LIPMPC_FIELD_INF.  Moves go between passable cells at the costs 5 / 7 with the
 *    no-corner-cut rule of lipmpc_grid_field_batch.  For every cell that any subset of the frontier can reach this IS "unblocked"
 *    of the frontier field call: a cell that is unblocked and INF there reaches no frontier cell at all.
 *  - S_0 = the (passable) cells with frontier[c] != 0.  U_0 = the robots b with may_claim[b] != 0 and status[b] FOUND or
 *    PATH_OVERFLOW.
 *  - round k = 0, 1, ... runs while k < max_claims, U_k is not empty and S_k is not empty:
 *      field_k = the least cost to any cell of S_k, relaxed by the call itself (round 0 included; the given field is read for
 *        passability only).
 *      every b in U_k: s_b = its start cell (floor rule) if field_k is finite there, else the SNAP of lipmpc_grid_path_batch in
 *        field_k (window r_inflate + 1, key (d^2, field, index)); cost_b = field_k[s_b].  A robot with no such cell is no
 *        candidate in this round.  With no candidate the rounds end.
 *      the winner is the candidate with the least (cost_b, b).  Its rows are written by the path rule of
 *        lipmpc_grid_frontier_path_batch on field_k -- descent order, string pulling, max_seg, S_max, the last sub-goal the
 *        centre of c_L, as written, no contraction: status (FOUND, or PATH_OVERFLOW with nothing written to sub_goals), n_sub,
 *        sub_goals rows below n_sub (rows from n_sub on untouched), path_cost = field_k[s_b] / 5.0, target_cell = c_L, and
 *        claim_round[b] = k.
 *      S_{k+1} = S_k without the cells (i, j) with (i - i_t)^2 + (j - j_t)^2 <= r_claim^2, t = c_L (the disc clipped to the
 *        grid); U_{k+1} = U_k without the winner.  A PATH_OVERFLOW winner claims like any other.
 *  - every other robot keeps every output the path call gave it and gets claim_round = -1: robots that are not eligible, and
 *    robots still in U when the rounds end -- FOLLOWERS, who keep their plain nearest-frontier plan and so share a target.
 *  - n_claims[0] = the number of rounds that had a winner.
 *  Hence: max_claims = 0 writes only claim_round = -1 and n_claims = 0; the round-0 winner's rows equal what the path call
 *  wrote; the targets of two winners are more than r_claim apart; the winners' costs do not decrease from round to round.  The
 *  outputs are a function of the inputs alone -- every comparison is an integer with a total order -- so two calls give
 *  identical bits.  There is no memory between calls: a replan may hand a robot another target.
 *  COST: the rounds are sequential, one relaxation of the whole map per claim.  field_k is kept in LDS when 4 W H bytes beside two
 *  bitmaps (impassable, sources) and 22 words fit the 160 KiB of a workgroup: 4 (2 (2 ceil(W H / 64) + 2) + 22 + W H) + 256 <=
 *  163840, up to about 38,400 cells; a larger map is relaxed in `work`.
 * Restated in numpy by tests/assign_oracle.py (multi-source Dijkstra per round); the device's outputs equal it bit for bit.
 * All pointers DEVICE pointers but origin / cell (HOST); asynchronous on hip_stream; no allocation and no host synchronisation,
 * so the call can be captured in a graph; every refusal is decided on the host before anything is enqueued.
 * LIPMPC_E_ARG: B outside 0..2^31-1, W or H < 2, a cell size that is not positive and finite, an origin that is not finite,
 *  r_inflate outside 0..16, r_claim outside 0..4096, max_claims outside 0..4096, max_seg < 5, S_max < 1, any null pointer but
 *  may_claim.  Then LIPMPC_E_UNSUPPORTED: W * H > 2^17, W > 4096 or H > 4096.  Then B = 0 enqueues nothing and returns 0. */
int lipmpc_grid_frontier_assign_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                      const uint8_t* frontier, const uint32_t* field, const double* start, const int8_t* may_claim,
                                      int32_t r_inflate, int32_t r_claim, int32_t max_claims, int32_t max_seg, int32_t S_max,
                                      uint32_t* work, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                      int32_t* target_cell, int32_t* claim_round, int32_t* n_claims, void* hip_stream);

/* lipmpc_grid_frontier_assign_keep_batch (backward-compatible addition): CLAIM HYSTERESIS.  lipmpc_grid_frontier_assign_batch
 * with a KEEP PHASE ahead of its greedy rounds: a robot that had a target at the last replan keeps what is left of it while it
 * is still a source, still reachable and not much farther than the robot's nearest frontier.  One workgroup does the whole call.
 * The arguments, S, U, passability and the path rule are lipmpc_grid_frontier_assign_batch's, plus:
 *  prev_target [B] int32: a cell index i * H + j of this same W x H grid; a value outside 0..W*H-1 means "none"
 *  r_keep 0..64, in cells;  keep_ratio16 16..1024, in sixteenths;  keep_slack 0..4096, in cells
 *  kept [B] int8, n_kept [1] int32: written whole
 * THE RULE:
 *  - a SLOT is one relaxation of the whole map.  A call makes at most max_claims slots, keep attempts and greedy rounds counted
 *    together.  k counts the slots that had a winner: claim_round still runs 0, 1, ... in the order won, and n_claims is the
 *    number of winners, the kept ones included.
 *  - keep phase: the robots b of U_0 whose start lies on the grid and whose prev_target is a cell, in ascending index, while
 *    slots are left:
 *      ANCHOR a_b = the cell of the current S within (i - i_p)^2 + (j - j_p)^2 <= r_keep^2 of the previous target p with the
 *        least (d^2, cell index).  None: b is skipped and no slot is spent.  (The frontier recedes as the robot approaches:
 *        r_keep is how far it may recede and still be the same target.)
 *      one slot is spent.  keepfield = the least cost to {a_b} alone: the same relaxation, costs, no-corner-cut rule and
 *        passability as a greedy round's field.
 *      ENTRY s_b = the start cell if keepfield is finite there, else the snap in keepfield, as in a greedy round.  None: b is
 *        not kept and stays in U.
 *      near_b = the given field at the robot's entry into the GIVEN field (its start cell if finite there, else the snap
 *        there; none: b is not kept).  b keeps its target iff, in 64 bits,
 *            16 * keepfield[s_b] <= keep_ratio16 * near_b + 80 * keep_slack
 *        (costs are in fifths of a cell).  Otherwise b stays in U for the greedy rounds.
 *      on success the rows are written by the winner's path rule on keepfield (PATH_OVERFLOW included), target_cell = a_b,
 *        claim_round[b] = k, kept[b] = 1; S loses the r_claim disc round a_b and U loses b.
 *  - greedy phase: lipmpc_grid_frontier_assign_batch's rounds on what is left of S, U and the slots.
 *  - every other robot gets kept[b] = 0.  n_kept[0] = the number of kept robots.
 *  Hence: with every prev_target "none" all outputs but kept / n_kept equal lipmpc_grid_frontier_assign_batch's bit for bit;
 *  the targets of two winners, kept or claimed, are more than r_claim apart (an anchor is taken from the current S);
 *  keep_ratio16 = 16 with keep_slack = 0 keeps only a target that is as near as the nearest frontier; a failed keep attempt
 *  changes nothing but that it spends a slot; two calls give identical bits.  The test compares with the NEAREST frontier, not
 *  with what the greedy rounds would have handed the robot.
 *  COST: one relaxation per slot, and per keep candidate a search of the clipped (2 r_keep + 1)^2 window.  The slot's field is
 *  kept in LDS when 4 (2 (2 ceil(W H / 64) + 2) + 34 + W H) + 256 <= 163840 (34 words: the 22 of the assign kernels, three
 *  more pointers, four scalars and the entry cell for the lane that walks, the count of U); a larger map is relaxed in `work`.
 * Restated in numpy by tests/assign_keep_oracle.py; the device's outputs equal it bit for bit.
 * All pointers DEVICE pointers but origin / cell (HOST); asynchronous on hip_stream; no allocation and no host synchronisation,
 * so the call can be captured in a graph; every refusal is decided on the host before anything is enqueued.
 * LIPMPC_E_ARG: what lipmpc_grid_frontier_assign_batch refuses as such, r_keep outside 0..64, keep_ratio16 outside 16..1024,
 *  keep_slack outside 0..4096, a null prev_target, kept or n_kept.  Then LIPMPC_E_UNSUPPORTED and B = 0 as there. */
int lipmpc_grid_frontier_assign_keep_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                           const uint8_t* frontier, const uint32_t* field, const double* start,
                                           const int8_t* may_claim, const int32_t* prev_target, int32_t r_inflate, int32_t r_claim,
                                           int32_t r_keep, int32_t keep_ratio16, int32_t keep_slack, int32_t max_claims,
                                           int32_t max_seg, int32_t S_max, uint32_t* work, double* sub_goals, int32_t* n_sub,
                                           int32_t* status, double* path_cost, int32_t* target_cell, int32_t* claim_round,
                                           int32_t* n_claims, int8_t* kept, int32_t* n_kept, void* hip_stream);

/* INFORMED EXPLORER (backward-compatible addition): send explorers where they will see most.  The frontier path call sends a
 * robot to its NEAREST frontier cell, whatever that cell would reveal: a cell behind a wall stub is worth as much as one that
 * faces an open unknown half-plane.  These three calls add the expected-visibility utility of frontier exploration (Gonzalez-
 * Banos and Latombe 2002; Burgard et al. 2005): lipmpc_grid_frontier_gain_batch counts the unknown cells a robot standing on a
 * frontier cell would see, lipmpc_grid_frontier_utility_field_batch relaxes a cost-to-go field whose sources start ahead by
 * what they reveal -- so ONE field per shared map still serves every robot -- and lipmpc_grid_frontier_utility_path_batch sends
 * any number of robots down it.  Everything compared is an integer.  All three calls: all pointers DEVICE pointers but origin /
 * cell (HOST); asynchronous on hip_stream; no allocation and no host synchronisation, so they can be captured in a graph; every
 * refusal is a return code decided on the host before anything is enqueued -- LIPMPC_E_ARG first, then LIPMPC_E_UNSUPPORTED
 * (W * H > 2^17, W > 4096 or H > 4096), then F = 0 / B = 0 enqueues nothing and returns 0.
 *
 * lipmpc_grid_frontier_gain_batch: F maps; a wave per frontier cell, a lane per ray.
 *  evidence [F,W,H] int32, t_free, t_occ 1..2^30: what lipmpc_grid_frontier_field_batch was given
 *  frontier [F,W,H] uint8: its output (not optional here);  r_view 1..64, in cells: how far a robot sees
 *  gain     [F,W,H] int32, written whole
 * THE GAIN of one map, solid / free / unknown as in the frontier field call, r = r_view:
 *  - gain[c] = 0 where frontier[c] == 0.  The call does not re-derive the frontier: it takes the given bytes.
 *  - for a frontier cell s = (i, j) the END CELLS are the 8 r offsets (di, dj) with max(|di|, |dj|) == r.
 *  - the RAY to an end cell visits, for k = 1, 2, ..., r, the offset (a, b) = (floor((2 k di + r) / (2 r)),
 *    floor((2 k dj + r) / (2 r))), the floor toward minus infinity: the planners' LOS expression walked outward from s, with no
 *    lexicographic swap.
 *  - the ray ENDS before the first k at which a^2 + b^2 > r^2, or (i + a, j + b) is outside the grid, or that cell is solid.
 *    Unknown and free cells do not stop a ray (an unknown cell is no partial occluder).
 *  - gain[s] = the number of DISTINCT unknown cells visited by any of the 8 r rays.
 *  The count is the size of a set: it depends on neither ray order nor lane order, so two calls give identical bits.  On an
 *  all-unknown map the fan reaches every cell of the disc: gain = (cells with a^2 + b^2 <= r^2) - 1, 12852 at r = 64.
 *  Work follows the number of frontier cells, not W H r^2: a workgroup takes 2048 cells of a map, compacts their frontier cells
 *  and hands them to its 16 waves.  LDS: the map's solid and unknown bitmaps (2 x 16 KiB at 2^17 cells), the list of 2048 cells,
 *  and per wave a window of (2 r + 1)^2 bits (2.1 KiB at r = 64) that the rays OR into and whose popcount is the gain.
 * LIPMPC_E_ARG: F < 0, W or H < 2, t_free or t_occ outside 1..2^30, r_view outside 1..64, a null evidence / frontier / gain
 *  (whatever F). */
int lipmpc_grid_frontier_gain_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence, int32_t t_free,
                                    int32_t t_occ, const uint8_t* frontier, int32_t r_view, int32_t* gain, void* hip_stream);

/* lipmpc_grid_frontier_utility_field_batch: F maps, one workgroup per map: cost-to-go with a head start for cells that reveal more.
 *  frontier [F,W,H] uint8, field [F,W,H] uint32: the outputs of lipmpc_grid_frontier_field_batch; both are only read
 *  gain     [F,W,H] int32: lipmpc_grid_frontier_gain_batch's output -- or any int32 array: values are clamped to 0..g_cap
 *  w_gain 0..65535;  g_cap 1..16384;  min_gain 0..16384
 *  ufield   [F,W,H] uint32 (it overlaps nothing else);  n_sources [F] int32
 * THE RULE:
 *  - passable(c) <=> field[c] != LIPMPC_FIELD_INF: `field` is read for passability only, the argument
 *    lipmpc_grid_frontier_assign_batch makes.  Moves go between passable cells at the costs 5 / 7 with the no-corner-cut rule.
 *  - source(c) <=> frontier[c] != 0 && passable(c) && gain[c] >= min_gain (gain[c] as stored).
 *  - seed(c) = (w_gain * (g_cap - min(max(gain[c], 0), g_cap))) >> 4: sixteenths of a cost unit per cell that c reveals less
 *    than g_cap; at most 2^26.
 *  - ufield[c] = the least, over sources s, of seed(s) + the cost from c to s; INF on impassable cells and on cells that reach
 *    no source.  Finite values stay below 7 * 2^17 + 2^26: no addition wraps.
 *  - n_sources[f] = the number of sources.  With 0 the whole ufield is INF.
 *  Hence: w_gain = 0 and min_gain = 0 give ufield == field, bit for bit.  With g_cap well below the disc's cell count every
 *  cell that reveals at least g_cap has seed 0, and robots go to the NEAREST GOOD-ENOUGH frontier cell instead of all to the
 *  single best one; min_gain > 0 prunes slivers, and when nothing worth seeing is left n_sources is 0.  A source may be
 *  DOMINATED (ufield[c] < seed(c)): a better cell is near enough that nobody stops here.
 *  The relaxation of lipmpc_grid_field_batch converges from any seeds by monotone minimum, and the least sum is unique: two
 *  calls give identical bits.  ufield is kept in LDS, sized to the map, when 4 W H bytes beside one bitmap (impassable) and the
 *  count's word pair fit the 160 KiB of a workgroup: 4 ((2 ceil(W H / 64) + 2) + 2 + W H) + 256 <= 163840, up to about 39,600
 *  cells; a larger map is relaxed in `ufield` itself.
 * Restated in numpy by tests/gain_oracle.py (seeded multi-source Dijkstra); the device's outputs equal it bit for bit.
 * LIPMPC_E_ARG: F < 0, W or H < 2, w_gain outside 0..65535, g_cap outside 1..16384, min_gain outside 0..16384, a null pointer
 *  (whatever F). */
int lipmpc_grid_frontier_utility_field_batch(int device, int64_t F, int32_t W, int32_t H, const uint8_t* frontier,
                                             const uint32_t* field, const int32_t* gain, int32_t w_gain, int32_t g_cap,
                                             int32_t min_gain, uint32_t* ufield, int32_t* n_sources, void* hip_stream);

/* lipmpc_grid_frontier_utility_path_batch: B robots, one lane per robot, each down the utility field of its map.
 *  B, F, W, H, origin, cell, evidence, t_occ, start, r_inflate, max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell:
 *         lipmpc_grid_frontier_path_batch's
 *  frontier, gain, ufield [F,W,H], n_sources [F], w_gain, g_cap, min_gain: what the utility field call was given and wrote
 *  target_gain [B] int32
 * PER ROBOT this is lipmpc_grid_frontier_path_batch with ufield in the place of field, with these differences and no others:
 *  - n_sources[f] == 0 ends LIPMPC_RRT_NO_PATH, in the place of n_frontier[f] == 0.
 *  - terminal(c) <=> source(c) && ufield[c] == seed(c): a source that nothing dominates.
 *  - the descent ends at the FIRST terminal cell c_L.  The terminal test is made before a descending neighbour is looked for,
 *    so a source whose seed ties a route through it is where the robot stops.  A start cell that is terminal after the snap
 *    gives n_sub = 1, its own centre.  A non-terminal cell with no descending neighbour ends LIPMPC_RRT_NO_PATH: the input is
 *    no utility field of this map.
 *  - path_cost = (ufield[s] - ufield[c_L]) / 5.0, s the start cell after the snap: the walk's length in cells.
 *  - target_gain[b] = gain[c_L] as stored; -1 unless the status is FOUND or PATH_OVERFLOW.
 *  The snap's window and key, the descent's order, the string pulling, max_seg on ufield[a] - ufield[c_k], S_max, "rows from
 *  n_sub on untouched", the centre expression without contraction and target_cell are lipmpc_grid_frontier_path_batch's.
 *  With w_gain = 0 and min_gain = 0 every output equals that call's, bit for bit.
 * Restated in numpy by tests/gain_oracle.py; the device's outputs equal it bit for bit.
 * LIPMPC_E_ARG: what lipmpc_grid_frontier_path_batch refuses, the three gain parameters out of range, any null pointer
 *  (whatever B). */
int lipmpc_grid_frontier_utility_path_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                            const double* cell, const int32_t* evidence, int32_t t_occ, const uint8_t* frontier,
                                            const int32_t* gain, const uint32_t* ufield, const int32_t* n_sources, int32_t w_gain,
                                            int32_t g_cap, int32_t min_gain, const double* start, int32_t r_inflate, int32_t max_seg,
                                            int32_t S_max, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                            int32_t* target_cell, int32_t* target_gain, void* hip_stream);

/* lipmpc_grid_frontier_assign_utility_batch (backward-compatible addition): GAIN-SEEDED CLAIMS.  The claim rounds of
 * lipmpc_grid_frontier_assign_batch seed every round's field with 0, so a robot wins a sliver behind a wall stub as readily as a
 * cell that faces an open unknown half-plane; the utility path call knows what a cell reveals, but its one shared field herds
 * robots that stand together.  This call joins the two: the rounds are the assign call's, each round's field is seeded as the
 * utility field is, and the winner's walk ends as the utility path's does.  The discount stays the r_claim disc: no gain is
 * recomputed after a claim.  One workgroup does the whole call.
 * The arguments are lipmpc_grid_frontier_assign_batch's in their order, and ahead of hip_stream:
 *  gain [W,H] int32: lipmpc_grid_frontier_gain_batch's output (F = 1) -- or any int32 array; only read
 *  w_gain 0..65535;  g_cap 1..16384;  min_gain 0..16384
 *  target_gain [B] int32: read, and rewritten for the robots that claim
 *  sub_goals, n_sub, status, path_cost, target_cell, target_gain: the outputs of lipmpc_grid_frontier_utility_path_batch (F = 1)
 *    for the same map, gain parameters and start
 * THE RULE:
 *  - passable(c) <=> the given field[c] != LIPMPC_FIELD_INF, as in the assign call: `field` is read for passability only.
 *  - S_0 = the utility field's sources: frontier[c] != 0 && passable(c) && gain[c] >= min_gain (gain[c] as stored).
 *  - seed(c) = (w_gain * (g_cap - min(max(gain[c], 0), g_cap))) >> 4, the utility field's.
 *  - U_0 as in the assign call: may_claim[b] != 0 and status[b] FOUND or PATH_OVERFLOW.
 *  - round k = 0, 1, ... runs while k < max_claims, U_k is not empty and S_k is not empty:
 *      ufield_k[c] = the least, over s in S_k, of seed(s) + the cost from c to s, relaxed by the call itself, round 0 included.
 *      every b in U_k: s_b = its start cell if ufield_k is finite there, else the snap in ufield_k (window r_inflate + 1, key
 *        (d^2, field, index)); cost_b = ufield_k[s_b].  With no candidate the rounds end.
 *      the winner is the candidate with the least (cost_b, b).  Its rows are written by the path rule of
 *        lipmpc_grid_frontier_utility_path_batch on ufield_k with terminal(c) <=> c in S_k && ufield_k[c] == seed(c); the
 *        terminal test is made before a descending neighbour is looked for; descent order, string pulling, max_seg, S_max and
 *        the centre expression are unchanged.  A PATH_OVERFLOW winner writes nothing to sub_goals and claims like any other.
 *      for the winner: path_cost = (ufield_k[s_b] - ufield_k[c_L]) / 5.0, target_cell = c_L, target_gain = gain[c_L] as
 *        stored, claim_round = k.
 *      S_{k+1} = S_k without the r_claim disc round c_L (clipped to the grid); U_{k+1} = U_k without the winner.
 *  - every other robot keeps every output the utility path call gave it and gets claim_round = -1.
 *  - n_claims[0] = the number of rounds that had a winner.
 *  Hence: with w_gain = 0 and min_gain = 0 every output the two calls share equals lipmpc_grid_frontier_assign_batch's, bit for
 *  bit, whatever gain holds at or above 0 (a negative stored gain is no source at any min_gain); max_claims = 0 writes only claim_round = -1 and n_claims = 0; the round-0 winner's rows equal what
 *  the utility path call wrote for it; the targets of two winners are more than r_claim apart; the winning cost_b does not
 *  decrease from round to round (S only shrinks, so no ufield_k value falls); a min_gain that leaves no source gives
 *  n_claims = 0; two calls give identical bits.  There is no memory between calls and no hysteresis for these claims
 *  in this call: lipmpc_grid_frontier_assign_keep_utility_batch, below, is the keep phase on these sources and seeds.
 *  COST: the assign call's -- one relaxation of the whole map per claim, sequential.  ufield_k is kept in LDS when it fits
 *  beside two bitmaps (impassable, S_k) and 34 words (the assign kernels' 22, three more pointers -- gain, target_gain,
 *  n_claims -- and six scalars: w_gain, g_cap, max_seg, S_max, r_claim, max_claims):
 *  4 (2 (2 ceil(W H / 64) + 2) + 34 + W H) + 256 <= 163840; a larger map is relaxed in `work`.
 *  gain stays in global memory and is read at source cells only.
 * Restated in numpy by tests/assign_utility_oracle.py; the device's outputs equal it bit for bit.
 * All pointers DEVICE pointers but origin / cell (HOST); asynchronous on hip_stream; no allocation and no host synchronisation,
 * so the call can be captured in a graph; every refusal is decided on the host before anything is enqueued.
 * LIPMPC_E_ARG: what lipmpc_grid_frontier_assign_batch refuses as such, w_gain outside 0..65535, g_cap outside 1..16384,
 *  min_gain outside 0..16384, any null pointer but may_claim.  Then LIPMPC_E_UNSUPPORTED (W * H > 2^17, W > 4096 or H > 4096).
 *  Then B = 0 enqueues nothing and returns 0. */
int lipmpc_grid_frontier_assign_utility_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                              const uint8_t* frontier, const uint32_t* field, const double* start,
                                              const int8_t* may_claim, int32_t r_inflate, int32_t r_claim, int32_t max_claims,
                                              int32_t max_seg, int32_t S_max, uint32_t* work, double* sub_goals, int32_t* n_sub,
                                              int32_t* status, double* path_cost, int32_t* target_cell, int32_t* claim_round,
                                              int32_t* n_claims, const int32_t* gain, int32_t w_gain, int32_t g_cap, int32_t min_gain,
                                              int32_t* target_gain, void* hip_stream);

/* lipmpc_grid_frontier_assign_keep_utility_batch (backward-compatible addition): CLAIM HYSTERESIS FOR THE GAIN-SEEDED CLAIMS.
 * lipmpc_grid_frontier_assign_keep_batch's rule on lipmpc_grid_frontier_assign_utility_batch's sources, seeds and fields: the far,
 * high-gain targets that the gain-seeded claims hand out jump between replans, and a robot that had one keeps what is left of
 * it while it is still a source and, as a utility, not much worse than the best the robot could have.  One workgroup does the
 * whole call.
 * The arguments are lipmpc_grid_frontier_assign_keep_batch's in their order, and ahead of hip_stream:
 *  gain [W,H] int32: lipmpc_grid_frontier_gain_batch's output (F = 1) -- or any int32 array; only read
 *  ufield [W,H] uint32: lipmpc_grid_frontier_utility_field_batch's output (F = 1) for the same map and gain parameters; only read
 *  w_gain 0..65535;  g_cap 1..16384;  min_gain 0..16384
 *  target_gain [B] int32: read, and rewritten for the robots that keep or claim
 *  sub_goals, n_sub, status, path_cost, target_cell, target_gain: the outputs of lipmpc_grid_frontier_utility_path_batch (F = 1)
 *    for the same map, gain parameters and start, as for lipmpc_grid_frontier_assign_utility_batch
 * THE RULE:
 *  - passable(c), S_0 (frontier[c] != 0 && passable(c) && gain[c] >= min_gain, gain as stored), seed(c) and U_0 are exactly
 *    lipmpc_grid_frontier_assign_utility_batch's.  Slots, k, claim_round, n_claims, kept and n_kept are exactly
 *    lipmpc_grid_frontier_assign_keep_batch's.
 *  - keep phase: the candidates and their order are the keep call's.
 *      ANCHOR a_b = the cell of the current S within r_keep of the previous target with the least (d^2, cell index): the keep
 *        call's key, unchanged, on this call's S.  None: b is skipped and no slot is spent.
 *      one slot is spent.  keepfield[c] = seed(a_b) + the cost from c to a_b: a single source that starts at its seed.
 *      ENTRY s_b as in a round (the start cell if keepfield is finite there, else the snap in keepfield).  None: b is not kept.
 *      near_b = the given ufield at the robot's entry into the GIVEN ufield (its start cell if finite there, else the snap
 *        there; none: b is not kept).  b keeps its target iff, in 64 bits,
 *            16 * keepfield[s_b] <= keep_ratio16 * near_b + 80 * keep_slack
 *        Both sides are utilities, so a target whose gain has fallen pays for it through its seed.
 *      on success the rows are written by the utility winner's path rule on keepfield with terminal(c) <=> c == a_b;
 *        path_cost = (keepfield[s_b] - keepfield[a_b]) / 5.0, target_cell = a_b, target_gain = gain[a_b] as stored,
 *        claim_round[b] = k, kept[b] = 1; S loses the r_claim disc round a_b and U loses b.
 *      a failed attempt spends its slot and changes nothing else.
 *  - greedy phase: lipmpc_grid_frontier_assign_utility_batch's rounds on what is left of S, U and the slots.
 *  Hence: with every prev_target "none" every output the calls share equals lipmpc_grid_frontier_assign_utility_batch's, bit for
 *  bit (kept and n_kept are 0); with w_gain = 0, min_gain = 0 and stored gains >= 0 (then ufield == field) every output equals
 *  lipmpc_grid_frontier_assign_keep_batch's, bit for bit, kept and n_kept included; the targets of two winners, kept or
 *  claimed, are more than r_claim apart; two calls give identical bits.  No addition wraps: a seed is below 2^26 and a finite cost
 *  below 7 * 2^24, and 16 (2^26 + 7 * 2^24) and 1024 (2^26 + 7 * 2^24) fit 64 bits with room to spare.
 *  COST: the keep call's -- one relaxation per slot.  The slot's field is kept in LDS when it fits beside two bitmaps
 *  (impassable, S) and 48 words (the keep kernels' 34 with ufield in the given field's place, four more pointers -- gain,
 *  target_gain, n_claims, n_kept, a word pair each -- and six more scalars -- w_gain, g_cap, r_claim, r_keep, r_inflate,
 *  max_claims):
 *  4 (2 (2 ceil(W H / 64) + 2) + 48 + W H) + 256 <= 163840; a larger map is relaxed in `work`.
 *  gain stays in global memory and is read at source cells only.
 * Restated in numpy by tests/assign_keep_utility_oracle.py; the device's outputs equal it bit for bit.
 * All pointers DEVICE pointers but origin / cell (HOST); asynchronous on hip_stream; no allocation and no host synchronisation,
 * so the call can be captured in a graph; every refusal is decided on the host before anything is enqueued.
 * LIPMPC_E_ARG: what lipmpc_grid_frontier_assign_keep_batch and lipmpc_grid_frontier_assign_utility_batch refuse as such, a
 *  null gain, ufield or target_gain.  Then LIPMPC_E_UNSUPPORTED and B = 0 as there. */
int lipmpc_grid_frontier_assign_keep_utility_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                                   const uint8_t* frontier, const uint32_t* field, const double* start,
                                                   const int8_t* may_claim, const int32_t* prev_target, int32_t r_inflate,
                                                   int32_t r_claim, int32_t r_keep, int32_t keep_ratio16, int32_t keep_slack,
                                                   int32_t max_claims, int32_t max_seg, int32_t S_max, uint32_t* work, double* sub_goals,
                                                   int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell,
                                                   int32_t* claim_round, int32_t* n_claims, int8_t* kept, int32_t* n_kept,
                                                   const int32_t* gain, const uint32_t* ufield, int32_t w_gain, int32_t g_cap,
                                                   int32_t min_gain, int32_t* target_gain, void* hip_stream);

/* TILED FIELDS (backward-compatible addition): the two cost-to-go fields above on LARGE maps, relaxed by many workgroups.  The
 * four calls above keep their cap of 2^17 cells and their one workgroup per field; the calls here take any map with
 * W * H <= 2^24 and W, H <= 4096 (a finite field value stays below 7 * 2^24; a WEIGHTED one, SOFT CLEARANCE below, below
 * (7 + LIPMPC_COST_MAX) * 2^24 = 255 * 2^24 < 2^32 - 1), and compute THE SAME FIELD, bit for bit: the
 * least cost is unique.  The map is cut into tiles of tile_w x tile_h cells (along i and along j; lipmpc_grid_tiled_info).  The
 * calls' set-up kernels (bitmaps, the blocked bitmap by the disc test, seeds, tile flags, n_frontier, statuses) run one
 * workgroup per 256 cells; then a call enqueues ROUNDS.  One round is one kernel launch with one workgroup per (field, tile): a
 * tile that is not marked active returns at once; an active tile stages its field words and blocked bits with a one-cell halo in
 * LDS, relaxes its cells to the local fixed point with the halo held, writes back the cells that fell and marks the
 * neighbouring tiles behind every part of its rim on which a cell fell active for the next round.  Workgroups are ordered by
 * the kernel boundaries on hip_stream and by nothing else: there is no cooperative launch, no grid barrier and no loop in which
 * one workgroup waits for another.  The device cannot end the rounds early, so the CALLER sets the budget: max_rounds rounds are
 * enqueued, and settled[f] tells whether they were enough.
 *
 * lipmpc_grid_tiled_info: *tile_w = the tile's cells along i, *tile_h = along j, *max_cells = 2^24.  Host only.  LIPMPC_E_ARG:
 *  a null pointer.
 * lipmpc_grid_tiled_workspace_bytes: the bytes of `work` for F fields on a W x H map; non-decreasing in F, in W and in H.  Host
 *  only.  LIPMPC_E_ARG (as a negative value): F < 0, W or H < 2; LIPMPC_E_UNSUPPORTED: a shape the field calls refuse.
 *
 * lipmpc_grid_field_tiled_batch: lipmpc_grid_field_batch's arguments, contract and outputs, and
 *  work, work_bytes  a device buffer of at least lipmpc_grid_tiled_workspace_bytes(F, W, H) bytes
 *  max_rounds  1..65536: the rounds this call enqueues
 *  resume      0: a COLD call -- it initialises everything it reads: the previous contents of work, field, field_status and
 *              settled are arbitrary.  1: work and field are as the previous call WITH THE SAME ARGUMENTS left them (same
 *              buffers, F, W, H, map, goal, r_inflate; stream-ordered after it); max_rounds more rounds are enqueued.
 *              field_status is written by a cold call only.
 *  settled     [F] int32: 1 <=> no tile of field f is marked active after the call's last round
 * WHAT HOLDS AFTER A CALL:
 *  - settled[f] == 1: field f is lipmpc_grid_field_batch's, bit for bit, and field_status[f] is that call's.  A resume on a
 *    settled field changes no bit of it.
 *  - settled[f] == 0: every finite word of field f is the cost of a real path from that cell to the goal cell, so >= the final
 *    value, and it IS the final value wherever the round guarantee says so.  Blocked cells hold INF.
 *  - THE ROUND GUARANTEE: after R rounds in total (the cold call's and every resume's), a cell holds its final value if some
 *    least-cost path from it to a source (the goal cell; a frontier cell) changes tile at most R - 1 times.  On an open W x H
 *    map ceil(W / tile_w) + ceil(H / tile_h) rounds therefore settle every cell's VALUE; settled itself may take a round more,
 *    in which nothing falls.
 *  - A diagonal move is judged on the blocked state of its two side cells (the contract's rule), never on whether their field
 *    words are finite yet: that is what makes the guarantee exact.
 *  - Two cold calls give identical bits in field, field_status and settled; with settled == 0 the FIELD's bits may differ
 *    between two runs (a halo word read in the round in which its owner lowers it may be the old or the new one), its settled
 *    cells, as guaranteed above, do not.
 * No allocation, no host synchronisation, capturable in a graph; every refusal is decided on the host before anything is
 * enqueued.  LIPMPC_E_ARG: what lipmpc_grid_field_batch refuses as such, a null occ / goal / field / field_status / work /
 *  settled (whatever F), max_rounds outside 1..65536, resume neither 0 nor 1.  Then LIPMPC_E_UNSUPPORTED: W * H > 2^24, W > 4096,
 *  H > 4096, or F * (W * H + 64) > 2^31 (the threads of one launch).  Then LIPMPC_E_ARG: work_bytes below
 *  lipmpc_grid_tiled_workspace_bytes(F, W, H).  Then F = 0 enqueues nothing and returns 0.
 *
 * lipmpc_grid_frontier_field_tiled_batch: the same over lipmpc_grid_frontier_field_batch's arguments, contract and outputs
 *  (frontier, field, n_frontier; frontier and n_frontier are written by a cold call only).  A map with n_frontier == 0 is settled
 *  before the first round.  Refusals as above, with lipmpc_grid_frontier_field_batch's LIPMPC_E_ARG cases.
 *
 * lipmpc_grid_path_tiled_batch, lipmpc_grid_frontier_path_tiled_batch: lipmpc_grid_path_batch and
 *  lipmpc_grid_frontier_path_batch word for word, with the cap above instead of theirs, and one more input:
 *  settled [F] int32, the field call's output.  A robot whose field has settled[f] == 0 gets LIPMPC_RRT_FIELD_UNSETTLED BEFORE
 *  any other rule, with n_sub = 0, path_cost = NaN, target_cell = -1 (the frontier call) and nothing else written: no path is
 *  walked down a field that may still change.  LIPMPC_E_ARG and B = 0 as those calls, a null settled included;
 *  LIPMPC_E_UNSUPPORTED as the tiled field calls. */
int lipmpc_grid_tiled_info(int32_t* tile_w, int32_t* tile_h, int64_t* max_cells);
int64_t lipmpc_grid_tiled_workspace_bytes(int64_t F, int32_t W, int32_t H);
int lipmpc_grid_field_tiled_batch(int device, int64_t F, int32_t W, int32_t H, int32_t grid_shared, const double* origin,
                                  const double* cell, const uint8_t* occ, const double* goal, int32_t r_inflate, uint32_t* field,
                                  int32_t* field_status, void* work, int64_t work_bytes, int32_t max_rounds, int32_t resume,
                                  int32_t* settled, void* hip_stream);
int lipmpc_grid_frontier_field_tiled_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence, int32_t t_free,
                                           int32_t t_occ, int32_t r_inflate, int32_t min_unknown, uint8_t* frontier,
                                           uint32_t* field, int32_t* n_frontier, void* work, int64_t work_bytes,
                                           int32_t max_rounds, int32_t resume, int32_t* settled, void* hip_stream);
int lipmpc_grid_path_tiled_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin, const double* cell,
                                 const uint8_t* occ, int32_t grid_shared, const uint32_t* field, const int32_t* field_status,
                                 const int32_t* settled, const double* goal, const double* start, int32_t r_inflate,
                                 int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub, int32_t* status,
                                 double* path_cost, void* hip_stream);
int lipmpc_grid_frontier_path_tiled_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                          const double* cell, const int32_t* evidence, int32_t t_occ, const uint32_t* field,
                                          const int32_t* n_frontier, const int32_t* settled, const double* start,
                                          int32_t r_inflate, int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub,
                                          int32_t* status, double* path_cost, int32_t* target_cell, void* hip_stream);

/* SOFT CLEARANCE (backward-compatible addition): a per-cell traversal cost that decays with the distance to the nearest solid cell,
 * and the two tiled fields and their paths in the metric that charges it.  r_inflate forbids cells; the cost layer prices them: a
 * path keeps clear of walls where there is room and still passes a door that is one cell wide.  Everything is an integer.
 *
 * lipmpc_grid_clearance_cost_batch: the layer of M maps.  Exactly one of
 *  occ       [M, W*H] uint8, solid = byte != 0, and
 *  evidence  [M, W*H] int32, solid = e >= t_occ (t_occ 1..2^30, read with evidence only)
 *  is non-null.  r_clear 1..31 (cells; a disc row is then at most 63 consecutive bits, one 64-bit window), w_clear
 *  0..LIPMPC_COST_MAX.  With d2(c) the least (i - si)^2 + (j - sj)^2 over the solid cells (si, sj) INSIDE the grid (the map's edge is
 *  not solid, as for r_inflate):
 *  cost      [M, W*H] uint8 (output): 0 if d2 > r_clear^2 (or the map has no solid cell), else
 *            (w_clear * (r_clear^2 - d2)) / r_clear^2 in integer division -- w_clear on a solid cell itself.
 *  Unknown cells of an evidence grid are no sources of cost, for the reason they are not inflated: it would eat the frontier.
 *  One workgroup per (map, tile); no workspace, no allocation, no host synchronisation, capturable.  LIPMPC_E_ARG: M < 0, W or
 *  H < 2, r_clear or w_clear outside their ranges, both or neither of occ / evidence, a null cost, t_occ outside 1..2^30 with
 *  evidence.  Then LIPMPC_E_UNSUPPORTED: the tiled caps, with M for F.  Then M = 0 enqueues nothing and returns 0.
 *
 * lipmpc_grid_field_weighted_batch, lipmpc_grid_frontier_field_weighted_batch: lipmpc_grid_field_tiled_batch's and
 *  lipmpc_grid_frontier_field_tiled_batch's arguments, refusals, workspace, rounds, resume and settled, word for word, plus
 *  cost      uint8 [grid_shared ? 1 : F, W*H] (the goal field), [F, W*H] (the frontier field): ANY byte layer, not only the one
 *            above.  A byte above LIPMPC_COST_MAX is read as LIPMPC_COST_MAX; nothing scans the layer on the host.  Null:
 *            LIPMPC_E_ARG.  A resume reads the same layer.
 *  THE CONTRACT: with k(c) = min(cost[c], LIPMPC_COST_MAX), the field is the unique fixed point of
 *      f(c) = k(c) + min over legal moves c -> n of (f(n) + step),   f = 0 on the sources,
 *  moves, steps (5 / 7), the blocked rule and the no-corner-cut rule being the tiled calls': a cell pays its own cost when it is
 *  LEFT, a source pays nothing.  settled[f] == 1: the field is that fixed point, bit for bit -- weighted Dijkstra's.  Before that
 *  every finite word is the cost of a real path, and THE ROUND GUARANTEE holds with "least-cost" in the weighted metric.  A finite
 *  value stays below (7 + LIPMPC_COST_MAX) * 2^24 = 255 * 2^24 < 2^32 - 1 = LIPMPC_FIELD_INF on the largest map: no addition
 *  wraps (the unweighted fields stay below 7 * 2^24).  With an all-zero layer the output is the tiled calls', bit for bit.
 *
 * lipmpc_grid_path_weighted_batch, lipmpc_grid_frontier_path_weighted_batch: the tiled path calls' arguments, status rules (the
 *  settled rule first), snap and refusals, plus the same `cost` (null with B > 0: LIPMPC_E_ARG).
 *  THE DESCENT takes the first neighbour n in the contract's order with a legal move and f(n) + step + k(c) == f(c).
 *  STRING PULLING keeps two sums: pen = the sum of k over the descended cells from the anchor (inclusive) to the current cell
 *  (exclusive); seg_pen(a, cur) = the sum of k over the cells the segment rule visits between the two, minus k(cur).  A sub-goal
 *  is set where the line of sight breaks, where seg_pen(a, cur) > pen (the straight segment would pay more penalty than the
 *  descended path did), or where the length since the anchor WITH PENALTIES EXCLUDED, (f(a) - f(cur)) - pen, reaches max_seg -- so
 *  max_seg counts steps only and 0x7FFFFFFF still means "no cap" although weighted values may exceed it.  Re-anchoring at the
 *  previous cell sets pen = k(prev), at the current cell pen = 0; the segment between two adjacent cells always passes.
 *  path_cost = f(s) / 5.0, PENALTIES INCLUDED: it is the weighted cost, not the length in cells.  The last sub-goal and
 *  target_cell are the tiled calls'.  With an all-zero layer every output is the tiled path calls', bit for bit. */
#define LIPMPC_COST_MAX 248
int lipmpc_grid_clearance_cost_batch(int device, int64_t M, int32_t W, int32_t H, const uint8_t* occ, const int32_t* evidence,
                                     int32_t t_occ, int32_t r_clear, int32_t w_clear, uint8_t* cost, void* hip_stream);
int lipmpc_grid_field_weighted_batch(int device, int64_t F, int32_t W, int32_t H, int32_t grid_shared, const double* origin,
                                     const double* cell, const uint8_t* occ, const uint8_t* cost, const double* goal,
                                     int32_t r_inflate, uint32_t* field, int32_t* field_status, void* work, int64_t work_bytes,
                                     int32_t max_rounds, int32_t resume, int32_t* settled, void* hip_stream);
int lipmpc_grid_frontier_field_weighted_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence,
                                              const uint8_t* cost, int32_t t_free, int32_t t_occ, int32_t r_inflate,
                                              int32_t min_unknown, uint8_t* frontier, uint32_t* field, int32_t* n_frontier,
                                              void* work, int64_t work_bytes, int32_t max_rounds, int32_t resume, int32_t* settled,
                                              void* hip_stream);
int lipmpc_grid_path_weighted_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin, const double* cell,
                                    const uint8_t* occ, int32_t grid_shared, const uint8_t* cost, const uint32_t* field,
                                    const int32_t* field_status, const int32_t* settled, const double* goal, const double* start,
                                    int32_t r_inflate, int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub,
                                    int32_t* status, double* path_cost, void* hip_stream);
int lipmpc_grid_frontier_path_weighted_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                             const double* cell, const int32_t* evidence, const uint8_t* cost, int32_t t_occ,
                                             const uint32_t* field, const int32_t* n_frontier, const int32_t* settled,
                                             const double* start, int32_t r_inflate, int32_t max_seg, int32_t S_max,
                                             double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                             int32_t* target_cell, void* hip_stream);

/* TILED EXPLORERS (backward-compatible addition): the informed and the coordinated explorer on LARGE maps.  The three informed
 * calls and the claim call above keep their cap of 2^17 cells and their one workgroup per map; the calls here take what the tiled
 * field calls take -- W, H <= 4096, W * H <= 2^24, F * (W * H + 64) <= 2^31 (the claim call: F = 1) -- and compute THE SAME
 * OUTPUTS, bit for bit.  All of them: device pointers but origin / cell (HOST); asynchronous on hip_stream; no allocation and no
 * host synchronisation, so they can be captured in a graph; every refusal is decided on the host before anything is enqueued, in
 * this order: LIPMPC_E_ARG, then the caps as LIPMPC_E_UNSUPPORTED, then a work_bytes that is too small as LIPMPC_E_ARG, then
 * F = 0 / B = 0 enqueues nothing and returns 0.
 *
 * lipmpc_grid_frontier_gain_tiled_batch: lipmpc_grid_frontier_gain_batch's arguments, contract and output, word for word, with
 *  the caps above.  No workspace and no rounds: the gain is local.  One workgroup per (map, tile of tile_w x tile_h cells): a tile
 *  whose frontier bytes hold no frontier cell writes its zeros and returns, so the work still follows the frontier; any other
 *  classifies the evidence of the tile grown by r_view on every side -- at most (tile_w + 128) x (tile_h + 128) = 160 x 192 cells
 *  -- into solid and unknown bits in LDS (a cell outside the grid ends a ray, as there), compacts the tile's frontier cells and
 *  runs that call's wave-per-cell, lane-per-ray march with the same quotient / remainder stepping and the same window popcount.
 *  LDS, bounded by r_view and no longer by the map, with g = (tile_w + 2 r)(tile_h + 2 r):
 *    4 (2 (2 ceil(g / 64) + 2) + 2 + tile_w tile_h + 16 * 2 ceil((2 r + 1)^2 / 64)) bytes, all dynamic: 49,304 at r = 64, 8,920 at r = 1.
 *  lipmpc_grid_frontier_gain_tiled_lds_bytes(r_view): that figure as the host passes it at launch.  Host only.  LIPMPC_E_ARG (as a
 *  negative value): r_view outside 1..64.
 *
 * lipmpc_grid_frontier_utility_field_tiled_batch: the utility field by rounds.
 *  F, W, H, evidence, t_free, t_occ, r_inflate: what the frontier field call was given
 *  frontier, gain, w_gain, g_cap, min_gain, ufield, n_sources: lipmpc_grid_frontier_utility_field_batch's
 *  work, work_bytes, max_rounds, resume, settled: lipmpc_grid_field_tiled_batch's; `work` is a workspace of this call's OWN
 *  (not the frontier field call's, which a resume of that call still reads), of lipmpc_grid_tiled_workspace_bytes(F, W, H) bytes
 *  A cold call builds the solid, unknown and blocked bitmaps from the evidence as the tiled frontier field call does, then
 *   source(c) <=> frontier[c] != 0 && !blocked(c) && gain[c] >= min_gain;  ufield = seed(c) on sources and INF elsewhere;
 *   n_sources by integer atomics; then max_rounds rounds and settled.  n_sources is written by a cold call only.  A map with
 *   n_sources == 0 is settled before the first round, its ufield all INF.
 *  PASSABLE HERE IS "UNBLOCKED", where the one-workgroup call reads field != INF.  The two agree on everything that matters: a
 *   frontier cell is always finite in the nearest-frontier field, so the sources are the same; an unblocked cell that is INF
 *   there reaches no frontier cell, hence no source, and is INF in either utility field; a diagonal's side cell is an axial
 *   neighbour of the diagonal's target, so judging diagonals on blocked bits allows the same moves among cells that reach a
 *   source.  So a settled ufield equals lipmpc_grid_frontier_utility_field_batch's, bit for bit -- and the call does not need the
 *   nearest-frontier field to be settled, or to exist.
 *  resume, settled, the round guarantee (with "a source" for "the goal cell", costs counted from the source's seed) and "two cold
 *   calls give identical bits" are lipmpc_grid_frontier_field_tiled_batch's.  Finite values stay below 7 * 2^24 + 2^26.
 *  LIPMPC_E_ARG: F < 0, W or H < 2, t_free or t_occ outside 1..2^30, r_inflate outside 0..16, the three gain parameters out of
 *   range, a null evidence / frontier / gain / ufield / n_sources / work / settled (whatever F), max_rounds outside 1..65536,
 *   resume neither 0 nor 1.
 *
 * lipmpc_grid_frontier_utility_path_tiled_batch: lipmpc_grid_frontier_utility_path_batch word for word, with the caps above and
 *  one more input, settled [F] int32, the utility field call's output.  settled[f] == 0 gives LIPMPC_RRT_FIELD_UNSETTLED BEFORE
 *  any other rule, with n_sub = 0, path_cost = NaN, target_cell = -1, target_gain = -1 and nothing else written.
 *
 * lipmpc_grid_frontier_assign_tiled_batch: lipmpc_grid_frontier_assign_batch's rule, word for word -- "passable <=> the given
 *  field[c] != INF" and the given frontier bytes included -- with every round's field relaxed by tiled rounds.
 *  B .. S_max, sub_goals .. n_claims: that call's
 *  settled [1] int32: of the given nearest-frontier field (the tiled frontier field call's output)
 *  work, work_bytes: at least lipmpc_grid_frontier_assign_tiled_workspace_bytes(W, H) bytes, 8-byte aligned (else LIPMPC_E_ARG).  It holds the
 *   impassable and the source bitmap, field_k [W * H], two tile-flag arrays, the 64-bit key, the target word, a `stopped` word
 *   and four more control words.
 *  max_rounds 1..65536: the budget of EACH claim round;  claims_settled [1] int32
 *  The host enqueues a fixed sequence that the device cannot shorten: two set-up kernels (bitmaps by ballots and the control
 *  words; the robots' -2 - start cell encoding of U_0), then for k = 0 .. max_claims - 1 the claim seed (one workgroup per tile:
 *  field_k = 0 on what is left of the sources and INF elsewhere, the tile's flag of the first round = a source among its cells or
 *  in its halo, its other flag 0), max_rounds rounds with F = 1 and the impassable bitmap, the settle kernel, the pick (over
 *  robots: the least (cost << 32 | b) by a wave reduction and a 64-bit atomicMin) and the claim (one workgroup: one lane walks the
 *  winner's path and writes its rows and claim_round, then all threads clear the disc from the source bitmap, both flag arrays
 *  and the key), and a last kernel that turns the robots still in U into followers and writes n_claims and claims_settled.  The
 *  rounds are over when no source is left, there is no candidate, U is used up, settled[0] == 0, or this round's field is not
 *  settled after max_rounds rounds; the kernel that finds that sets `stopped`, and every later kernel of the call returns on
 *  reading it -- a seed kernel that sets no flag leaves the round launches idle, one word read per workgroup.
 *  THE COST, whatever the fleet needs: max_claims * (max_rounds + 4) + 3 launches.
 *  - claims_settled[0] == 1 <=> the rounds ended by the rule (max_claims reached included); then every output equals
 *    lipmpc_grid_frontier_assign_batch's, bit for bit.
 *  - claims_settled[0] == 0 <=> settled[0] == 0 (then n_claims = 0) or some round's field did not settle within max_rounds: the
 *    claims made so far are exactly the rule's first n_claims rounds, and everyone else keeps the nearest-frontier plan.  A
 *    repeat of the WHOLE call with a larger budget on the same buffers reproduces those rounds and goes on: the rounds are a
 *    deterministic function of the inputs, and a winner's overwritten status stays FOUND or PATH_OVERFLOW, which keeps it in U_0.
 *    (The call restores nobody's rows: after a call that made MORE claims, a robot that claims no longer keeps that call's rows, not
 *    the path call's.  Repeat with the same or a larger budget, or run the path call first.)
 *  LIPMPC_E_ARG: what lipmpc_grid_frontier_assign_batch refuses as such, a null settled / claims_settled, max_rounds outside
 *   1..65536, max_claims * max_rounds > 2^20 (the launches of one call), a work that is not 8-byte aligned.
 * lipmpc_grid_frontier_assign_tiled_workspace_bytes: non-decreasing in W and in H.  Host only.  LIPMPC_E_ARG (as a negative
 *  value): W or H < 2; LIPMPC_E_UNSUPPORTED: a shape the call refuses. */
int64_t lipmpc_grid_frontier_gain_tiled_lds_bytes(int32_t r_view);
int lipmpc_grid_frontier_gain_tiled_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence, int32_t t_free,
                                          int32_t t_occ, const uint8_t* frontier, int32_t r_view, int32_t* gain, void* hip_stream);
int lipmpc_grid_frontier_utility_field_tiled_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence,
                                                   int32_t t_free, int32_t t_occ, int32_t r_inflate, const uint8_t* frontier,
                                                   const int32_t* gain, int32_t w_gain, int32_t g_cap, int32_t min_gain,
                                                   uint32_t* ufield, int32_t* n_sources, void* work, int64_t work_bytes,
                                                   int32_t max_rounds, int32_t resume, int32_t* settled, void* hip_stream);
int lipmpc_grid_frontier_utility_path_tiled_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                                  const double* cell, const int32_t* evidence, int32_t t_occ, const uint8_t* frontier,
                                                  const int32_t* gain, const uint32_t* ufield, const int32_t* n_sources,
                                                  const int32_t* settled, int32_t w_gain, int32_t g_cap, int32_t min_gain,
                                                  const double* start, int32_t r_inflate, int32_t max_seg, int32_t S_max,
                                                  double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                                  int32_t* target_cell, int32_t* target_gain, void* hip_stream);
int64_t lipmpc_grid_frontier_assign_tiled_workspace_bytes(int32_t W, int32_t H);
int lipmpc_grid_frontier_assign_tiled_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                            const uint8_t* frontier, const uint32_t* field, const int32_t* settled, const double* start,
                                            const int8_t* may_claim, int32_t r_inflate, int32_t r_claim, int32_t max_claims,
                                            int32_t max_seg, int32_t S_max, void* work, int64_t work_bytes, int32_t max_rounds,
                                            double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell,
                                            int32_t* claim_round, int32_t* n_claims, int32_t* claims_settled, void* hip_stream);

/* lipmpc_grid_frontier_assign_keep_tiled_batch (backward-compatible addition): CLAIM HYSTERESIS on large maps --
 * lipmpc_grid_frontier_assign_keep_batch's rule, word for word, with every slot's field relaxed by tiled rounds.
 *  The arguments of lipmpc_grid_frontier_assign_tiled_batch plus prev_target, r_keep, keep_ratio16, keep_slack, kept and n_kept
 *  as lipmpc_grid_frontier_assign_keep_batch takes them.  work: at least
 *  lipmpc_grid_frontier_assign_keep_tiled_workspace_bytes(W, H) bytes, 8-byte aligned: the tiled claim call's layout with eight
 *  more control words (the slot's mode, robot and anchor, the keep cursor, the keep count).
 *  The host enqueues a fixed sequence: the two set-up kernels, then for every slot 0 .. max_claims - 1 the MODE kernel (one
 *  workgroup: from the cursor on, the next robot of U with a previous target whose anchor exists in what is left of the sources --
 *  candidates without one are passed over and spend nothing; none left: this and every later slot is a greedy round), the seed
 *  (a keep slot seeds the anchor alone), max_rounds rounds and the settle kernel, the pick (a keep slot considers its robot
 *  alone) and the take (a keeper has to pass the test; on success its rows, kept, the disc; a keep slot without an entry cell or
 *  with a failed test ends without a winner and the call goes on), then the last kernel.  k is a control word that counts the
 *  winners: the host's slot index is not the claim index.  A slot whose field does not settle within max_rounds stops the call.
 *  THE COST, whatever the fleet needs: max_claims * (max_rounds + 5) + 3 launches; max_claims * max_rounds <= 2^20 as before.
 *  - claims_settled[0] == 1: every output equals lipmpc_grid_frontier_assign_keep_batch's, bit for bit.
 *  - claims_settled[0] == 0: settled[0] == 0 (then n_claims = n_kept = 0) or some slot's field did not settle: the keeps and
 *    claims made so far are exactly the rule's first n_claims winners, and everyone else keeps the nearest-frontier plan.  A
 *    repeat of the whole call with a larger budget reproduces them and goes on (what
 *    lipmpc_grid_frontier_assign_tiled_batch says about rows applies).
 *  LIPMPC_E_ARG: what lipmpc_grid_frontier_assign_tiled_batch and lipmpc_grid_frontier_assign_keep_batch refuse as such.
 * lipmpc_grid_frontier_assign_keep_tiled_workspace_bytes: as lipmpc_grid_frontier_assign_tiled_workspace_bytes. */
int64_t lipmpc_grid_frontier_assign_keep_tiled_workspace_bytes(int32_t W, int32_t H);
int lipmpc_grid_frontier_assign_keep_tiled_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                                 const uint8_t* frontier, const uint32_t* field, const int32_t* settled,
                                                 const double* start, const int8_t* may_claim, const int32_t* prev_target,
                                                 int32_t r_inflate, int32_t r_claim, int32_t r_keep, int32_t keep_ratio16,
                                                 int32_t keep_slack, int32_t max_claims, int32_t max_seg, int32_t S_max, void* work,
                                                 int64_t work_bytes, int32_t max_rounds, double* sub_goals, int32_t* n_sub,
                                                 int32_t* status, double* path_cost, int32_t* target_cell, int32_t* claim_round,
                                                 int32_t* n_claims, int8_t* kept, int32_t* n_kept, int32_t* claims_settled,
                                                 void* hip_stream);

/* lipmpc_grid_frontier_assign_utility_tiled_batch (backward-compatible addition): GAIN-SEEDED CLAIMS on large maps --
 * lipmpc_grid_frontier_assign_utility_batch's rule, word for word, with every round's field relaxed by tiled rounds.
 *  The arguments of lipmpc_grid_frontier_assign_tiled_batch in their order and, ahead of hip_stream, gain [W,H], w_gain, g_cap,
 *  min_gain and target_gain [B] as lipmpc_grid_frontier_assign_utility_batch takes them.  sub_goals .. target_cell and
 *  target_gain: the outputs of lipmpc_grid_frontier_utility_path_tiled_batch (F = 1).  settled, passability ("the given field[c]
 *  != INF"), work and its layout, max_rounds and claims_settled are the tiled claim call's; work: at least
 *  lipmpc_grid_frontier_assign_utility_tiled_workspace_bytes(W, H) bytes, 8-byte aligned.
 *  The host enqueues lipmpc_grid_frontier_assign_tiled_batch's sequence with three kernels of this call's own in it: the set-up
 *  (a source needs gain >= min_gain), the claim seed (a source starts at seed(c), not at 0; gain is read at source cells only)
 *  and the claim (the walk ends by terminal(c) <=> c in S_k && ufield_k[c] == seed(c); path_cost, target_gain).  The robots'
 *  set-up, the rounds, the settle kernel, the pick and the last kernel are that call's, launched as they are.
 *  THE COST, whatever the fleet needs: max_claims * (max_rounds + 4) + 3 launches; max_claims * max_rounds <= 2^20.
 *  - claims_settled[0] == 1: every output equals lipmpc_grid_frontier_assign_utility_batch's, bit for bit.
 *  - claims_settled[0] == 0: settled[0] == 0 (then n_claims = 0) or some round's field did not settle within max_rounds: the
 *    claims made so far are exactly the rule's first n_claims rounds, and everyone else keeps the utility plan.  A repeat of the
 *    whole call with a larger budget reproduces them and goes on (what lipmpc_grid_frontier_assign_tiled_batch says about rows
 *    applies).
 *  LIPMPC_E_ARG: what lipmpc_grid_frontier_assign_tiled_batch refuses as such, the three gain parameters out of range, a null
 *   gain or target_gain.  Then LIPMPC_E_UNSUPPORTED (W * H > 2^24, W > 4096 or H > 4096), then LIPMPC_E_ARG for a work_bytes
 *   below the size call's, then B = 0 returns 0, as there.
 * lipmpc_grid_frontier_assign_utility_tiled_workspace_bytes: as lipmpc_grid_frontier_assign_tiled_workspace_bytes. */
int64_t lipmpc_grid_frontier_assign_utility_tiled_workspace_bytes(int32_t W, int32_t H);
int lipmpc_grid_frontier_assign_utility_tiled_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                                    const uint8_t* frontier, const uint32_t* field, const int32_t* settled,
                                                    const double* start, const int8_t* may_claim, int32_t r_inflate, int32_t r_claim,
                                                    int32_t max_claims, int32_t max_seg, int32_t S_max, void* work, int64_t work_bytes,
                                                    int32_t max_rounds, double* sub_goals, int32_t* n_sub, int32_t* status,
                                                    double* path_cost, int32_t* target_cell, int32_t* claim_round, int32_t* n_claims,
                                                    int32_t* claims_settled, const int32_t* gain, int32_t w_gain, int32_t g_cap,
                                                    int32_t min_gain, int32_t* target_gain, void* hip_stream);

/* lipmpc_grid_frontier_assign_keep_utility_tiled_batch (backward-compatible addition): CLAIM HYSTERESIS FOR THE GAIN-SEEDED
 * CLAIMS on large maps -- lipmpc_grid_frontier_assign_keep_utility_batch's rule, word for word, with every slot's field relaxed by
 * tiled rounds.
 *  The arguments of lipmpc_grid_frontier_assign_keep_tiled_batch in their order and, ahead of hip_stream, gain [W,H], ufield
 *  [W,H], usettled [1] int32 (the `settled` word of the lipmpc_grid_frontier_utility_field_tiled_batch call that made ufield),
 *  w_gain, g_cap, min_gain and target_gain [B] as lipmpc_grid_frontier_assign_keep_utility_batch takes them.  sub_goals ..
 *  target_cell and target_gain: the outputs of lipmpc_grid_frontier_utility_path_tiled_batch (F = 1).  work: at least
 *  lipmpc_grid_frontier_assign_keep_utility_tiled_workspace_bytes(W, H) bytes, 8-byte aligned: the tiled keep call's layout.
 *  The host enqueues lipmpc_grid_frontier_assign_keep_tiled_batch's fixed sequence with three kernels of this call's own in it:
 *  the set-up (a source needs gain >= min_gain), the seed (a keep slot seeds the anchor alone at seed(a), a greedy slot what is
 *  left of S at its seeds) and the take (the utility terminal test -- c == a in a keep slot --, the keep test against ufield,
 *  path_cost and target_gain).  The mode, the robots' set-up, the rounds, the settle kernel, the pick and the last kernel are
 *  that call's, launched as they are.
 *  THE COST, whatever the fleet needs: max_claims * (max_rounds + 5) + 3 launches; max_claims * max_rounds <= 2^20.
 *  - claims_settled[0] == 1: every output equals lipmpc_grid_frontier_assign_keep_utility_batch's, bit for bit.
 *  - settled[0] == 0 or usettled[0] == 0: n_claims = n_kept = 0 and claims_settled[0] = 0.
 *  - a slot whose field does not settle within max_rounds stops the call with claims_settled[0] = 0: the keeps and claims made
 *    so far are exactly the rule's first n_claims winners, and everyone else keeps the utility plan.  A repeat of the whole call
 *    with a larger budget reproduces them and goes on (what lipmpc_grid_frontier_assign_tiled_batch says about rows applies).
 *  LIPMPC_E_ARG: what lipmpc_grid_frontier_assign_keep_tiled_batch refuses as such, the three gain parameters out of range, a
 *   null gain, ufield, usettled or target_gain.  Then LIPMPC_E_UNSUPPORTED (W * H > 2^24, W > 4096 or H > 4096), then
 *   LIPMPC_E_ARG for a work_bytes below the size call's, then B = 0 returns 0, as there.
 * lipmpc_grid_frontier_assign_keep_utility_tiled_workspace_bytes: as lipmpc_grid_frontier_assign_keep_tiled_workspace_bytes. */
int64_t lipmpc_grid_frontier_assign_keep_utility_tiled_workspace_bytes(int32_t W, int32_t H);
int lipmpc_grid_frontier_assign_keep_utility_tiled_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin,
                                                         const double* cell, const uint8_t* frontier, const uint32_t* field,
                                                         const int32_t* settled, const double* start, const int8_t* may_claim,
                                                         const int32_t* prev_target, int32_t r_inflate, int32_t r_claim,
                                                         int32_t r_keep, int32_t keep_ratio16, int32_t keep_slack, int32_t max_claims,
                                                         int32_t max_seg, int32_t S_max, void* work, int64_t work_bytes,
                                                         int32_t max_rounds, double* sub_goals, int32_t* n_sub, int32_t* status,
                                                         double* path_cost, int32_t* target_cell, int32_t* claim_round,
                                                         int32_t* n_claims, int8_t* kept, int32_t* n_kept, int32_t* claims_settled,
                                                         const int32_t* gain, const uint32_t* ufield, const int32_t* usettled,
                                                         int32_t w_gain, int32_t g_cap, int32_t min_gain, int32_t* target_gain,
                                                         void* hip_stream);

/* WAVE-PER-ROBOT PATH CALLS (backward-compatible addition): the path calls above with one wavefront (64 lanes) walking each
 * robot's path where those walk it in one lane -- the sight tests 64 cells at a time, a descent step in one round of loads.  Every
 * output is the named call's, bit for bit; only the time differs.  Three calls take the place of eight by way of NULLABLE inputs:
 *  lipmpc_grid_path_wave_batch: the arguments of lipmpc_grid_path_weighted_batch.
 *    cost null, settled null:  the contract of lipmpc_grid_path_batch (`field` from lipmpc_grid_field_batch)
 *    cost null, settled given: the contract of lipmpc_grid_path_tiled_batch
 *    cost given, settled given: the contract of lipmpc_grid_path_weighted_batch
 *    cost given, settled null: LIPMPC_E_ARG (a weighted field has the word)
 *  lipmpc_grid_frontier_path_wave_batch: the arguments of lipmpc_grid_frontier_path_weighted_batch, the same three forms --
 *    lipmpc_grid_frontier_path_batch, lipmpc_grid_frontier_path_tiled_batch, lipmpc_grid_frontier_path_weighted_batch -- and the
 *    same refusal.
 *  lipmpc_grid_frontier_utility_path_wave_batch: the arguments of lipmpc_grid_frontier_utility_path_tiled_batch.
 *    settled null: the contract of lipmpc_grid_frontier_utility_path_batch; given: of lipmpc_grid_frontier_utility_path_tiled_batch.
 *  REFUSALS, all decided on the host before anything is enqueued, in this order in every form: LIPMPC_E_ARG for what the tiled path
 *  calls refuse as such about scalars and the placement (max_seg < 5, S_max < 1, F not in {1, B}, origin / cell, t_occ, w_gain,
 *  g_cap, min_gain) and for cost without settled; then the TILED caps -- W, H <= 4096, W * H <= 2^24, F * (W * H + 64) <= 2^31:
 *  LIPMPC_E_UNSUPPORTED -- also in the forms that equal a one-workgroup call, whose cap of 2^17 cells belongs to the field's LDS (a
 *  path call needs none sized to the map); then B == 0 returns LIPMPC_OK; then a null pointer other than the nullable ones is
 *  LIPMPC_E_ARG.
 *  A `field` that is no cost-to-go field of the map (stale, constant, another map's) ends as in the one-lane calls: the descent
 *  takes strictly falling words only, so every walk ends within W * H steps.
 *  What stays one lane per robot: the winner's walk inside the claim calls (lipmpc_grid_frontier_assign_*_batch) and the RRT* planner. */
int lipmpc_grid_path_wave_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin, const double* cell,
                                const uint8_t* occ, int32_t grid_shared, const uint8_t* cost, const uint32_t* field,
                                const int32_t* field_status, const int32_t* settled, const double* goal, const double* start,
                                int32_t r_inflate, int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub, int32_t* status,
                                double* path_cost, void* hip_stream);
int lipmpc_grid_frontier_path_wave_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                         const double* cell, const int32_t* evidence, const uint8_t* cost, int32_t t_occ,
                                         const uint32_t* field, const int32_t* n_frontier, const int32_t* settled, const double* start,
                                         int32_t r_inflate, int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub,
                                         int32_t* status, double* path_cost, int32_t* target_cell, void* hip_stream);
int lipmpc_grid_frontier_utility_path_wave_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                                 const double* cell, const int32_t* evidence, int32_t t_occ, const uint8_t* frontier,
                                                 const int32_t* gain, const uint32_t* ufield, const int32_t* n_sources,
                                                 const int32_t* settled, int32_t w_gain, int32_t g_cap, int32_t min_gain,
                                                 const double* start, int32_t r_inflate, int32_t max_seg, int32_t S_max,
                                                 double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                                 int32_t* target_cell, int32_t* target_gain, void* hip_stream);

/* CLAIMS FROM PER-ROBOT FIELDS (backward-compatible addition): lipmpc_grid_frontier_assign_robot_fields_batch.  The claim calls
 * above relax the whole map once per claim.  The claims are a greedy over (robot, frontier cell) pairs whose costs come from ONE
 * single-source field per robot; those B fields are independent, so this call relaxes them together in max_rounds rounds of THE
 * TILED FIELD, after which every claim round and the whole keep phase are reductions over words already in memory.
 *  The arguments of lipmpc_grid_frontier_assign_keep_tiled_batch in their order, with `resume` (0 / 1) after max_rounds:
 *  frontier, field, settled: the tiled nearest-frontier field call's outputs on ONE shared map; start, may_claim, r_inflate,
 *  r_claim, max_claims, max_seg, S_max, r_keep, keep_ratio16, keep_slack as there, in the same ranges (the three keep parameters
 *  are range-checked even where they are not used).  prev_target [B] int32 or NULL: NULL = no keep phase; then kept and n_kept
 *  may be NULL too (given, they are written: 0).  work: at least lipmpc_grid_frontier_assign_robot_fields_workspace_bytes(B, W, H)
 *  bytes, 8-byte aligned; it holds the B fields, 4 B W H bytes, and stays below twice that from 16 x 16 cells on.  All pointers
 *  are DEVICE pointers except origin / cell; asynchronous on hip_stream, no allocation, no host synchronisation, capturable.
 *  On entry sub_goals, n_sub, status, path_cost and target_cell hold the nearest-frontier path call's outputs for the same starts.
 * THE RULE.  passable(c) <=> the given field[c] != LIPMPC_FIELD_INF; moves, the costs 5 / 7 and the no-corner-cut rule are
 *  lipmpc_grid_field_batch's.
 *  U_0 = the robots with may_claim != 0 (NULL: everybody) whose status is FOUND or PATH_OVERFLOW.
 *  ENTRY e_b of a robot of U_0: its start cell (the floor rule) if passable, else the SNAP in the GIVEN field: window
 *   r_inflate + 1, key (d^2, field, index).  It exists: the path call found it.  (lipmpc_grid_frontier_assign_batch snaps again
 *   in every round's field; this rule enters the map once.  The two differ only for a robot whose start cell is impassable.)
 *  D_b(c) = the least cost from e_b to c, LIPMPC_FIELD_INF if there is none; the move rules are symmetric, so this is also the
 *   cost from c to e_b.
 *  S_0 = the passable cells with frontier != 0.  k counts the WINNERS, kept ones included, and max_claims caps them: there are
 *   no relaxation slots to spend here, so -- unlike lipmpc_grid_frontier_assign_keep_batch -- a failed keep attempt costs nothing.
 *  KEEP PHASE (prev_target not NULL): the robots of U_0 whose prev_target is a cell of the grid, in ascending index while
 *   k < max_claims.  The ANCHOR a_b = the cell of the current S within r_keep of the previous target with the least (d^2, cell);
 *   none: the robot is passed over.  The robot is KEPT iff D_b(a_b) is finite and, in 64 bits,
 *       16 * D_b(a_b) <= keep_ratio16 * field[e_b] + 80 * keep_slack.
 *   A keeper gets the target a_b, claim_round = k, kept = 1; S loses the r_claim disc round a_b, U loses b, k grows by one.
 *  GREEDY ROUNDS, while k < max_claims and U and S are not empty: cost_b = min over c in S of D_b(c); a robot without a finite
 *   cost is no candidate; no candidate: the rounds end.  The winner is the candidate with the least (cost_b, b); its TARGET t is
 *   the cell of S with the least (D_b(c), c).  S loses the disc round t, U loses the winner, claim_round = k, k grows by one.
 *  ROWS of a winner or keeper b with target t.  The chain: c_0 = t; from c the next cell is the first neighbour n in the
 *   descent's order with D_b(n) + step == D_b(c), a diagonal only past two passable side cells; the chain ends at c_L = e_b.  The
 *   MARKED cells are the string pulling of lipmpc_grid_path_batch along that chain, word for word: the line of sight is judged
 *   on passability, the cost since the anchor a is D_b(a) - D_b(c_k), and the last chain cell -- the robot's own -- is never
 *   marked.  The sub-goals are the centres of the marked cells IN REVERSE ORDER (nearest the robot first), then the centre of t;
 *   a centre is ox + (i + 0.5) * dx as written, no contraction.  n_sub = marks + 1; more than S_max: status PATH_OVERFLOW,
 *   n_sub = 0 and nothing written to sub_goals -- the robot still claims.  Else status FOUND.  path_cost = D_b(t) / 5.0,
 *   target_cell = t; rows from n_sub on are untouched.  (The chain exists whenever claims_settled is 1: D_b(t) is finite.  Were a
 *   descent ever to break off, the robot would still claim and be reported as PATH_OVERFLOW with nothing written.)
 *  Everybody else keeps every output of the path call and gets claim_round = -1 and kept = 0 (a FOLLOWER).  n_claims[0] = k,
 *   n_kept[0] = the keepers among them.
 *  claims_settled[0] == 1 <=> settled[0] == 1 and every robot's field is settled after this call's rounds.  Otherwise NO row
 *   of any robot is rewritten: claim_round = -1 and kept = 0 for everybody, n_claims = n_kept = 0.  resume = 1 (same arguments,
 *   same buffers, stream-ordered after the call before) enqueues max_rounds more rounds on the fields in `work` and runs the
 *   claims again; a cold call (resume = 0) initialises everything it reads in `work`.
 *  HENCE: two winners' targets are more than r_claim apart; the greedy winners' costs do not decrease; a winner's target is a
 *   nearest live source of that winner; the round-0 greedy winner and its cost are lipmpc_grid_frontier_assign_batch's when every
 *   start cell of U_0 is passable (min over b of min over c of D_b(c) = min over b of field_0 at b's cell); the winners are
 *   those of the plain greedy over all (robot, cell) pairs by (cost, robot, cell) in which a pair leaves with its robot or with
 *   a cell in a winner's disc; with prev_target NULL or all "none" the outputs other than kept / n_kept are equal; every
 *   comparison is on integers with a total order, so two calls give identical bits.  Reproduced in numpy by
 *   tests/robot_fields_oracle.py.
 * THE COST.  The host enqueues a fixed sequence of max_rounds + 8 launches, whatever max_claims is: the set-up over cells, the
 *  robots' entries, the fill of the B fields, max_rounds rounds with F = B and one blocked bitmap, their settle kernel, the
 *  all-settled word, the claim kernel (ONE workgroup: the keep phase and every greedy round in a loop), the walks (a wavefront
 *  per winner, all winners at once) and the finish.  A resumed call leaves out the first three: max_rounds + 5.  A robot outside
 *  U_0 seeds nothing: its tiles stay idle at one word read per workgroup and round.
 * THE LIMITS.  Memory and the threads of a round launch grow with B: B * (W * H + 64) <= 2^31.  There are no gain seeds and no
 *  clearance layer.  The device still cannot end the rounds early: max_rounds launches are enqueued whatever the map needs.  The
 *  claim kernel is ONE workgroup that takes the robots of U one after another (a barrier pair and a scan of the source bitmap per
 *  robot at the start, and again per round for every robot whose best source was just claimed): its time grows with the robots
 *  that claim times the map's bitmap, and with thousands of claiming robots it is the sequential part that remains -- the caps
 *  (B up to 2^31 / (W H + 64), max_claims up to 4096) bound memory and threads, not that time.
 * LIPMPC_E_ARG: B outside 0..2^31-1, W or H < 2, a bad placement, r_inflate, r_claim, max_claims, max_seg, S_max, r_keep,
 *  keep_ratio16 or keep_slack out of their ranges, max_rounds outside 1..65536, resume not 0 / 1, a null pointer other than
 *  may_claim, prev_target and -- with prev_target NULL -- kept and n_kept, a `work` that is not 8-byte aligned.  Then
 *  LIPMPC_E_UNSUPPORTED: W or H > 4096, W * H > 2^24, B * (W * H + 64) > 2^31.  Then LIPMPC_E_ARG: work_bytes too small.  Then
 *  B = 0: nothing is enqueued.  Every refusal is decided on the host before anything is enqueued.
 * lipmpc_grid_frontier_assign_robot_fields_workspace_bytes: the bytes of `work`, monotone in B, W and H; LIPMPC_E_ARG or
 *  LIPMPC_E_UNSUPPORTED (negative) as above. */
int64_t lipmpc_grid_frontier_assign_robot_fields_workspace_bytes(int64_t B, int32_t W, int32_t H);
int lipmpc_grid_frontier_assign_robot_fields_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                                   const uint8_t* frontier, const uint32_t* field, const int32_t* settled,
                                                   const double* start, const int8_t* may_claim, const int32_t* prev_target,
                                                   int32_t r_inflate, int32_t r_claim, int32_t r_keep, int32_t keep_ratio16,
                                                   int32_t keep_slack, int32_t max_claims, int32_t max_seg, int32_t S_max, void* work,
                                                   int64_t work_bytes, int32_t max_rounds, int32_t resume, double* sub_goals,
                                                   int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell,
                                                   int32_t* claim_round, int32_t* n_claims, int8_t* kept, int32_t* n_kept,
                                                   int32_t* claims_settled, void* hip_stream);

/* FRONTIER REGIONS (backward-compatible addition): lipmpc_grid_frontier_regions_batch.  The frontier calls above mark frontier
 * CELLS; Yamauchi's frontiers are REGIONS, connected groups of frontier cells with a size and a centre.  This call labels the
 * regions of a given mask, sizes them and tables the ones that are large enough.  `size` has the layout and dtype of the gain
 * call's `gain` on purpose: every call that takes `gain` takes it, with min_gain acting as the minimum size, and `rep` can stand
 * where those calls take `frontier`.
 *  frontier [F,W,H] uint8, layout i * H + j: any non-zero byte is a frontier cell.  min_size 1..2^24.  R_max 0..2^20: the rows of
 *  the table per map.  work: at least lipmpc_grid_frontier_regions_workspace_bytes(F, W, H, R_max) bytes, 8-byte aligned, contents
 *  arbitrary on entry; calls that share one must be stream-ordered.  All pointers are DEVICE pointers; asynchronous on hip_stream,
 *  no allocation, no host synchronisation, capturable.
 * THE RULE, per map f.
 *  A REGION is a maximal 8-connected set of frontier cells; plain 8-connectivity: a diagonal pair is connected whatever lies
 *   beside it.
 *  label [F,W,H] int32: -1 off the frontier, else the least flat index of the cell's region (the region's ROOT).
 *  size  [F,W,H] int32: 0 off the frontier, else the number of cells of the cell's region.  Neither depends on min_size or R_max.
 *  A region is KEPT iff its size >= min_size.  The kept regions are RANKED by root, ascending.
 *  n_regions [F,3] int32: (all regions, kept regions, kept regions beyond R_max = max(kept - R_max, 0)).
 *  table [F,R_max,5] int32 or NULL if R_max == 0: row r < min(kept, R_max) is (root, size, centroid_cell, rep_cell, 0); the rows
 *   from there on are untouched.  centroid_cell = ci * H + cj with ci = (2 * sum of i + n) / (2 n), cj likewise with j: integer
 *   division of non-negative 64-bit values (the sum of i over a region reaches 2^36), n = size.  rep_cell, the REPRESENTATIVE, is
 *   the region's own cell with the least key ((i - ci)^2 + (j - cj)^2, flat index): a frontier cell even where the centroid is
 *   none, as for a ring.
 *  rep [F,W,H] uint8 or NULL: 1 on the rep_cell of every tabled region, 0 elsewhere; written whole.
 *  Everything is an integer and every reduction is an integer add or a min over totally ordered keys: two calls give identical
 *  bits.  Reproduced in numpy by tests/regions_oracle.py.
 * THE COST.  The host enqueues a fixed sequence of 9 launches, whatever the mask holds and whatever its size (R_max == 0, no
 *  table: the first 6 of them): the tiles' components in LDS (a lock-free union-find on the 32 x 64 tiles of the tiled field, the
 *  parent words in `label`), the unions across tile borders, the flatten with the roots' cell counts, the kept roots per 2048
 *  consecutive cells, their scan, the ranks with the first two table columns and every cell's size, the sums, the keys, the table.
 *  No kernel spins, waits for another thread's store or uses a grid-wide barrier; every loop is bounded by a size.
 * THE WORKSPACE is 4 bytes per cell (the root's rank), 32 bytes per table row and 8 bytes per 2048 cells, + 64: at most
 *  8 * F * W * H + 64 * F * R_max + 65536 bytes, monotone in every argument.  Statistics are kept per table row, not per cell.
 * LIPMPC_E_ARG: F < 0, W or H < 2, min_size outside 1..2^24, R_max outside 0..2^20, a null frontier, work, label, size or
 *  n_regions, a null table with R_max > 0, a `work` that is not 8-byte aligned or -- for a supported shape: the size of `work` is
 *  not defined for any other -- is too small.  Then LIPMPC_E_UNSUPPORTED: W or H > 4096, F * W * H > 2^31, whatever work_bytes
 *  is.  Then F = 0: nothing is enqueued.  Every refusal is decided on the host before anything is enqueued.
 * lipmpc_grid_frontier_regions_workspace_bytes: the bytes of `work`; LIPMPC_E_ARG or LIPMPC_E_UNSUPPORTED (negative) as above. */
int64_t lipmpc_grid_frontier_regions_workspace_bytes(int64_t F, int32_t W, int32_t H, int32_t R_max);
int lipmpc_grid_frontier_regions_batch(int device, int64_t F, int32_t W, int32_t H, const uint8_t* frontier, int32_t min_size,
                                       int32_t R_max, void* work, int64_t work_bytes, int32_t* label, int32_t* size, uint8_t* rep,
                                       int32_t* table, int32_t* n_regions, void* hip_stream);

/* NEIGHBOUR LDCBF ROWS (backward-compatible addition): the robots of one launch as each other's obstacles.  For every robot
 * the call finds its nearest neighbours among the B robots and appends one half-space row per neighbour to the robot's
 * c_eta, in the form lipmpc_plan_step_batch_c_eta solves against -- after the rows of a scan (first_slot = the scan's
 * n_inferred), or on their own.  All pointers are DEVICE pointers; asynchronous on hip_stream; no host synchronisation and no
 * allocation, so the call can be captured in a graph.  Evaluated in IEEE double, no contraction, division and square root
 * correctly rounded, every expression as written.
 *  state      [B,5]  only (p_x, p_y) are read
 *  radius     [B]    body radius of each robot
 *  group      [B] int32 or NULL (= one world): only robots of equal group see each other
 *  first_slot [B] int32 or NULL (= 0): first free slot of robot b's c_eta; values outside 0..n_obs_max are taken as the
 *             nearer end of that range
 *  workspace  lipmpc_neighbour_workspace_bytes(B) bytes, contents arbitrary on entry; calls sharing one must be stream-ordered
 * ABSENT: a robot with group < 0, a non-finite coordinate, or a negative or non-finite radius.  It neither sees nor is seen:
 *  n_rows = n_near = 0 (its slots from first_slot on are zeroed like everybody's).
 * RANGE AND ORDER: for present i != j of one group, dx = x_i - x_j, dy = y_i - y_j, d2 = dx*dx + dy*dy, dist = sqrt(d2);
 *  j is in range iff dist < sense_range (strictly, as the LiDAR's readings).  n_near[i] = the number in range.  Robot i's
 *  neighbours are the in-range j in ascending (d2, j) order; n_rows[i] = min(k_rows, n_obs_max - first_slot[i], n_near[i]).
 * ROW r of robot i, for its r-th neighbour j, at slot first_slot[i] + r:
 *    rs = r_i + r_j;  offset = rs + share * (dist - rs);  eta = (dx / dist, dy / dist);
 *    c = (x_j + offset * eta_x, y_j + offset * eta_y);  stored (c_x, c_y, eta_x, eta_y).
 *  share = 0.5 is the RECIPROCAL model (buffered Voronoi cell, Zhou et al. 2017): each robot of a pair may use its half of
 *  the free space between the two discs.  There eta.(p_i - c) = (dist - rs) / 2 at k = 0, which is >= 0 whenever the discs
 *  do not overlap -- the constant row cannot fail because the OTHER robot moved -- and the two half-spaces of a pair are
 *  disjoint and rs apart, so if both solves succeed the discs do not overlap at the next sample either.  share = 0 is the
 *  static disc, c = p_j + rs * eta, for neighbours known not to move (a neighbour that steps toward the robot violates that
 *  row).  dist == 0 gives eta = NaN: the step reports LIPMPC_STATUS_DEGENERATE, as for every producer's degenerate geometry.
 *  There is no inside flip: overlapping discs make the constant row negative and the step reports LIPMPC_STATUS_INFEASIBLE.
 * WRITTEN: slots below first_slot[i] are not touched; slots first_slot[i] + n_rows[i] .. n_obs_max - 1 are zeroed (in a
 *  replayed loop no row of the previous sample survives); n_rows [B], n_near [B]; neighbours [B,k_rows] int32 or NULL: j per
 *  row, -1 beyond n_rows.  n_near[i] > n_rows[i]: a neighbour in range got no row.
 * A robot's outputs are a function of the inputs alone -- not of the launch order, nor of how the races of the sort fell:
 *  two calls give identical bits.  Reproduced in numpy by tests/neighbour_oracle.py.
 * The search is a uniform grid of cells a hair wider than sense_range, hashed into a bucket table sized from B (counting
 *  sort: count, scan, scatter; then one lane per robot walks its 3 x 3 cells): linear in B at a given density.
 * LIPMPC_E_ARG: B outside 0..2^22, k_rows outside 1..16, n_obs_max outside 1..50, sense_range not positive and finite, share
 *  outside [0, 1], a null state, radius, workspace, c_eta, n_rows or n_near. */
int64_t lipmpc_neighbour_workspace_bytes(int64_t B);          /* < 0: B out of range */
int lipmpc_neighbour_c_eta_batch(int device, int64_t B, int32_t n_obs_max, int32_t k_rows,
                                 double sense_range, double share,
                                 const double* state, const double* radius, const int32_t* group,
                                 const int32_t* first_slot, void* workspace,
                                 double* c_eta, int32_t* n_rows, int32_t* n_near, int32_t* neighbours,
                                 void* hip_stream);

const char* lipmpc_strerror(int code);
int lipmpc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LIPMPC_H */
