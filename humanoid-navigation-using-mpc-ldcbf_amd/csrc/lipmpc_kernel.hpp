// lipmpc_kernel.hpp — batched LIP-MPC / LDCBF step solver for gfx950 (MI355X), C ABI in include/lipmpc.h.
//
// One QP per group of G lanes (G = 16 for N <= 8, 32 for N <= 16; 4 or 2 problems per
// 64-wide wavefront).  Lane l of a group owns decision variable l = 2a + c, i.e. coordinate c
// of the CoM position p_{a+1} (position form of the QP: H = 2I), and the
// inequality rows of "its" stage:
//   c = 0: leg-reach x (upper, lower), walking-velocity longitudinal (upper, lower), manoeuvrability
//   c = 1: leg-reach y (upper, lower), walking-velocity lateral (upper, lower)
//   LDCBF rows of stage a+1: obstacle j on lane c = j & 1.
// Rows are generated, never stored: G q, G^T w and K = 2I + G^T D G are applied through the
// problem's structure (rotation blocks, the alternating-sum velocity map, per-stage 2x2 LDCBF
// blocks), so a problem's live state is n + ~3 m doubles in registers.  For large obstacle sets
// (more than 7 LDCBF rows per lane) those rows are STREAMED instead: (s, z) per row in LDS, everything
// else recomputed in each pass (step_solve, STREAM).  Horizons up to 4 run the factorisation on 8 variable
// slots (NVAR = 8).
// A step = front_end (theta / omega, closest point and normal per obstacle, presolve of the LDCBF rows the leg-reach rows
// make redundant, compaction of the obstacles that still have a row) + step_solve<G, NOBS_L, NVAR> (interior point +
// certified primal active-set finish on NOBS_L row slots per lane); step_body picks the body: in the exact mode with the
// presolve the smallest of {1, 2, 7, the handle's} slots that holds the wave's neediest problem.  Kernels: plan_step_kernel
// (one step for B problems, optionally in the cost order of the previous launch: lipmpc_set_schedule; DISPATCH = with /
// without the small bodies), warm_step_kernel (the same step warm-started from and written back to caller-owned records:
// lipmpc_set_warm_start) and rollout_kernel (the whole closed loop per robot, one launch).
//
// Reference semantics followed (HumanoidNavigation/...):
//   theta/omega            MPC/HumanoidMpc.py:137-160
//   closest point / eta    Utils/ObstaclesUtils.py:50-109
//   rows                   MPC/HumanoidMpc.py:183-249, 252-294; HumanoidMPCCustomLCBF.py:30-31
//   cost                   MPC/HumanoidMpc.py:321-333
//   dynamics / advance     MPC/HumanoidMpc.py:34-48, 335-343, 432-447
// Solver: Mehrotra predictor-corrector on the normal equations + certified active-set finish
// (the algorithm of oracle/lipmpc_oracle.py, which is the parity checker, not a dependency).



#pragma once
#include "lipmpc_solve.hpp"

namespace lipmpc_dev {

// The whole MPC step of one problem on one group of G lanes: front end, then the SMALLEST solver body that holds the
// obstacles which still have a row after the presolve (1, 2, 7 or the handle's NOBS_L row slots per lane; the wave takes the
// body its neediest group needs).  On the BASELINE fields a step keeps 0-3 of 10 obstacles (N = 8) or 0-6 of 50 (N = 16), so
// the 2-slot body solves what the 5-slot / the 25-slot streamed body was sized for.  DISPATCH = false (the closed-loop kernel,
// whose callers run the interior mode, where every present obstacle keeps its rows): the handle's body only -- one body per
// kernel keeps that kernel's register allocation.  Output pointers may be null.
template <int G, int NOBS_L, int NVAR = G, bool DISPATCH = true, bool LEAN = false>
__device__ __forceinline__ StepOut step_body(
    const KArgs& P, const StepIn& in, const double* __restrict__ obs_xy, const int32_t* __restrict__ obs_nv,
    double* __restrict__ U, double* __restrict__ X, double* __restrict__ theta_out,
    double* __restrict__ omega_out, double* __restrict__ obj_out, int32_t* __restrict__ status_out,
    int32_t* __restrict__ iters_out, unsigned long long* __restrict__ active_out,
    unsigned long long* __restrict__ working_out, double* __restrict__ c_eta,
    double* __restrict__ diag, const double* __restrict__ c_eta_in = nullptr, WarmIO* __restrict__ warm = nullptr,
    int32_t* __restrict__ cost_out = nullptr) {
  constexpr int GPW = 64 / G;
  constexpr int MAXOBS = 2 * NOBS_L;
  // a problem's obstacle rings staged in LDS by one coalesced sweep of the group when they fit (n_obs x v_max vertices
  // <= RING_CAP: the 10 x 5 of BASELINE config 2 do): the edge walk of the closest-point step then reads LDS instead
  // of paying one global-memory latency per edge
  constexpr int RING_CAP = (G == 16) ? 64 : 256;
  __shared__ double lds_ring[GPW][MAXOBS > 0 ? RING_CAP : 1][2];
  __shared__ double lds_obs[GPW][MAXOBS > 0 ? MAXOBS : 1][4];   // eta_x, eta_y, b = eta.c + delta, kfirst
  __shared__ int lds_perm[GPW][MAXOBS > 0 ? MAXOBS : 1];
  __shared__ int lds_flag[GPW];
  __shared__ int lds_need[GPW];
  const int grp = threadIdx.x / G;
  const bool cold = (warm == nullptr) || (warm->lds == nullptr);
  const FrontOut<G> F = front_end<G, MAXOBS, !LEAN>(P, in, obs_xy, obs_nv, theta_out, omega_out, c_eta, c_eta_in, cold, lds_ring[grp],
                                                    lds_obs[grp], lds_perm[grp], &lds_flag[grp]);
#define LIPMPC_SOLVE(NL) step_solve<G, NL, NVAR, LEAN>(P, in, F, lds_obs[grp], lds_perm[grp], U, X, obj_out, status_out, iters_out, active_out, working_out, diag, warm, cost_out)
  if constexpr (DISPATCH && NOBS_L > 1) {
    if ((threadIdx.x & (G - 1)) == 0) lds_need[grp] = (F.n_rel + 1) >> 1;      // row slots per lane this group's obstacles need
    wave_sync();
    int need = 0;
#pragma unroll
    for (int g = 0; g < GPW; ++g) need = max(need, lds_need[g]);
    need = __builtin_amdgcn_readfirstlane(need);
    if (need <= 1) return LIPMPC_SOLVE(1);
    if constexpr (NOBS_L > 2) { if (need <= 2) return LIPMPC_SOLVE(2); }
    if constexpr (NOBS_L > 7) { if (need <= 7) return LIPMPC_SOLVE(7); }
  }
  return LIPMPC_SOLVE(NOBS_L);
#undef LIPMPC_SOLVE
}

// ------------------------------------------------------------------------------------------
// kernel 1: one MPC step for B problems (lipmpc_plan_step_batch)
// ------------------------------------------------------------------------------------------
// DISPATCH: the kernel holds the small solver bodies next to the handle's own and a wave picks the smallest that fits (exact
// mode with the presolve); false: the handle's body alone (interior mode / LIPMPC_FLAG_NO_PRESOLVE, where every present
// obstacle keeps its rows -- and where the streamed body keeps the register allocation it has when it is alone: inlined next
// to the small bodies it spills into its row sweeps, 59 instead of 36 us per iteration at N = 16 / 50 obstacles).
template <int G, int NOBS_L, int NVAR, bool DISPATCH>
__global__ __launch_bounds__(WAVE) void plan_step_kernel(
    KArgs P, long B, const double* __restrict__ state, const double* __restrict__ goal,
    const int8_t* __restrict__ first_foot, const double* __restrict__ delta_in,
    const double* __restrict__ obs_xy, const int32_t* __restrict__ obs_nv,
    double* __restrict__ U, double* __restrict__ X, double* __restrict__ theta_out,
    double* __restrict__ omega_out, double* __restrict__ obj_out, int32_t* __restrict__ status_out,
    int32_t* __restrict__ iters_out, unsigned long long* __restrict__ active_out,
    unsigned long long* __restrict__ working_out, double* __restrict__ c_eta,
    double* __restrict__ diag, const double* __restrict__ bounds, const double* __restrict__ c_eta_in,
    int32_t* __restrict__ sched, const int32_t* __restrict__ overflow_in) {
  constexpr int GPW = WAVE / G;
  static_assert(G == 16 || G == 32, "a problem is one or two DPP rows of one wavefront");
  if (blockDim.x != WAVE) __builtin_trap();          // wave_sync() and every group exchange assume a one-wave workgroup
  const long prob_raw = (long)blockIdx.x * GPW + threadIdx.x / G;
  // Which problem this group solves: its position in the launch, or -- on a schedule (lipmpc_set_schedule) -- the problem
  // the order left by the previous launch puts there: by descending cost (iterations + finish rounds).  That starts the
  // long solves first, and, as important, puts problems of like cost into the same wave: a wave lasts as long as the
  // slowest of its groups, and the mean of that maximum over four random problems is 12 % above the mean problem.
  long pb = prob_raw < B ? prob_raw : (B - 1);
  if (sched && sched[SCHED_VALID] == (int)B) {
    const long r = sched[SCHED_ORDER + pb];
    if (r >= 0 && r < B) pb = r;
  }
  const StepIn in = load_step_in(P, pb, prob_raw < B, state, goal, first_foot, delta_in, bounds, overflow_in);
  step_body<G, NOBS_L, NVAR, DISPATCH>(P, in, obs_xy, obs_nv, U, X, theta_out, omega_out, obj_out, status_out, iters_out, active_out,
                                       working_out, c_eta, diag, c_eta_in, nullptr, sched ? sched + SCHED_ORDER + B : nullptr);
}

// ------------------------------------------------------------------------------------------
// kernel 1c: one MPC step for B problems, each warm-started from its record (lipmpc_set_warm_start)
// ------------------------------------------------------------------------------------------
// The record of problem b (warm_rec + b * (1 + 2N + m_tot) doubles): word 0 = 1.0 when it holds a step result, then q of the
// interior-point phase (2N, stage-major) and its multipliers in canonical row order.  The kernel stages the record into the
// WarmIO block of its group in the lane layout the solver parks (q on lane l, slot i's multiplier on row 1 + i), the solver
// reads it back shifted by one stage exactly as in the closed-loop kernel, and after the solve the parked block goes back to the
// record in canonical order.  The body is the plain one with every row kept (LIPMPC_FLAG_WARM_START: no presolve); the front
// end keeps every obstacle in its own slot (cold = false: no compaction), so LDCBF slot 2t + c is obstacle 2t + c.  Register
// rows only (NOBS_L <= 7: the block holds WARM_ROWS slots), on 32 lanes NOBS_L <= 2 (lipmpc_inst.hip).  Every canonical word of a record is written by exactly one lane; padding
// groups (prob_raw >= B) start cold and write nothing.  Own instantiations of front_end and step_solve (template flag RECORD):
// sharing theirs with plan_step_kernel changed how that kernel compiles.
template <int G, int NOBS_L, int NVAR>
__global__ __launch_bounds__(WAVE) void warm_step_kernel(
    KArgs P, long B, const double* __restrict__ state, const double* __restrict__ goal,
    const int8_t* __restrict__ first_foot, const double* __restrict__ delta_in,
    const double* __restrict__ obs_xy, const int32_t* __restrict__ obs_nv,
    double* __restrict__ U, double* __restrict__ X, double* __restrict__ theta_out,
    double* __restrict__ omega_out, double* __restrict__ obj_out, int32_t* __restrict__ status_out,
    int32_t* __restrict__ iters_out, unsigned long long* __restrict__ active_out,
    unsigned long long* __restrict__ working_out, double* __restrict__ c_eta,
    double* __restrict__ diag, const double* __restrict__ bounds, const double* __restrict__ c_eta_in,
    int32_t* __restrict__ sched, const int32_t* __restrict__ overflow_in, double* __restrict__ warm_rec) {
  constexpr int GPW = WAVE / G;
  constexpr int MAXOBS = 2 * NOBS_L;
  constexpr int RING_CAP = (G == 16) ? 64 : 256;
  constexpr int NR = R_CBF + NOBS_L;
  static_assert(NR <= WARM_ROWS, "the warm-start block holds the register row slots only");
  if (blockDim.x != WAVE) __builtin_trap();          // see plan_step_kernel
  __shared__ double lds_ring[GPW][MAXOBS > 0 ? RING_CAP : 1][2];
  __shared__ double lds_obs[GPW][MAXOBS > 0 ? MAXOBS : 1][4];
  __shared__ int lds_perm[GPW][MAXOBS > 0 ? MAXOBS : 1];
  __shared__ int lds_flag[GPW];
  __shared__ double lds_warm[GPW][1 + WARM_ROWS][G];
  const int grp = threadIdx.x / G;
  const int lane = threadIdx.x & (G - 1);
  const long prob_raw = (long)blockIdx.x * GPW + grp;
  long pb = prob_raw < B ? prob_raw : (B - 1);        // (the schedule as in plan_step_kernel: records stay indexed by problem)
  if (sched && sched[SCHED_VALID] == (int)B) {
    const long r = sched[SCHED_ORDER + pb];
    if (r >= 0 && r < B) pb = r;
  }
  const StepIn in = load_step_in(P, pb, prob_raw < B, state, goal, first_foot, delta_in, bounds, overflow_in);
  const int N = P.N;
  const int a = lane >> 1, c = lane & 1;
  double* rec = warm_rec + pb * (long)(1 + 2 * N + P.m_tot);
  double* rec_z = rec + 1 + 2 * N;
  double* wl = &lds_warm[grp][0][0];
  const int* perm = lds_perm[grp];
  const CanonicalRows ci{a, c, N, P, perm};
  WarmIO ws;
  ws.lds = wl;
  ws.have = in.valid && rec[0] == 1.0;
  const FrontOut<G> F = front_end<G, MAXOBS, true, true>(P, in, obs_xy, obs_nv, theta_out, omega_out, c_eta, c_eta_in, false,
                                                         lds_ring[grp], lds_obs[grp], lds_perm[grp], &lds_flag[grp]);
  // does slot i of this lane name a canonical row?  (lanes past the horizon, the c = 1 manoeuvrability slot and obstacle slots
  // past n_obs do not)
  auto has_row = [&](int i) -> bool {
    if (a >= N) return false;
    if (i == R_M) return c == 0;
    if (i >= R_CBF) return perm[2 * (i - R_CBF) + c] < P.n_obs;
    return true;
  };
  if (ws.have) {
    wl[lane] = a < N ? rec[1 + lane] : 0.0;
#pragma unroll
    for (int i = 0; i < NR; ++i)
      wl[(1 + i) * G + lane] = has_row(i) ? rec_z[ci(i)] : 0.0;
  }
  wave_sync();
  const StepOut r = step_solve<G, NOBS_L, NVAR, false, true>(P, in, F, lds_obs[grp], lds_perm[grp], U, X, obj_out, status_out,
                                                             iters_out, active_out, working_out, diag, &ws,
                                                             sched ? sched + SCHED_ORDER + B : nullptr);
  // the solver parked this step's interior-point result in wl (absent rows as 0) and synchronised the wave: back to the record,
  // unshifted; the constant k = 0 rows are 0
  if (in.valid) {
    if (a < N) rec[1 + lane] = wl[lane];
#pragma unroll
    for (int i = 0; i < NR; ++i)
      if (has_row(i)) rec_z[ci(i)] = wl[(1 + i) * G + lane];
    for (int j = lane; j < P.n_obs; j += G) rec_z[9 * N + j] = 0.0;     // the constant k = 0 rows of obstacle j
    if (lane == 0) rec[0] = (r.status == LIPMPC_STATUS_SOLVED || r.status == LIPMPC_STATUS_UNCERTIFIED) ? 1.0 : 0.0;
  }
}

// ------------------------------------------------------------------------------------------
// kernels 1b: the split launch of one MPC step (see SPLIT_CLASSES above): classify -> bin -> one kernel per solver body
// ------------------------------------------------------------------------------------------
// The class of every problem: the front end alone (0.7 % of a step at N = 16 / 50 obstacles), one group of G lanes per
// problem exactly as the solving kernels run it -- the same code on the same inputs, hence the same count.
template <int G>
__global__ __launch_bounds__(WAVE) void classify_kernel(
    KArgs P, long B, const double* __restrict__ state, const double* __restrict__ goal, const double* __restrict__ delta_in,
    const double* __restrict__ obs_xy, const int32_t* __restrict__ obs_nv, const double* __restrict__ bounds,
    const double* __restrict__ c_eta_in, int32_t* __restrict__ ws) {
  constexpr int GPW = WAVE / G;
  constexpr int RING_CAP = (G == 16) ? 64 : 256;
  if (blockDim.x != WAVE) __builtin_trap();
  __shared__ double lds_ring[GPW][RING_CAP][2];
  __shared__ double lds_obs[GPW][SPLIT_MAXOBS][4];
  __shared__ int lds_perm[GPW][SPLIT_MAXOBS];
  __shared__ int lds_flag[GPW];
  const int grp = threadIdx.x / G;
  const long prob_raw = (long)blockIdx.x * GPW + grp;
  const long pb = prob_raw < B ? prob_raw : (B - 1);
  const StepIn in = load_step_in(P, pb, prob_raw < B, state, goal, nullptr, delta_in, bounds, nullptr);
  const FrontOut<G> F = front_end<G, SPLIT_MAXOBS>(P, in, obs_xy, obs_nv, nullptr, nullptr, nullptr, c_eta_in, true, lds_ring[grp],
                                                   lds_obs[grp], lds_perm[grp], &lds_flag[grp]);
  // sort key: class, then the cost hint's bucket (0 = dearest)
  if (in.valid && (threadIdx.x & (G - 1)) == 0)
    ws[SPLIT_HEAD + pb] = split_class_of((F.n_rel + 1) >> 1) * SPLIT_BUCKETS +
                          split_cost_bucket(F.h0_min, F.rows_kept, sqrt(in.v0x * in.v0x + in.v0y * in.v0y));
}

// One solver body over its class's list: the step kernel with NL row slots per lane and nothing else in its register
// allocation.  Launched with the grid of the whole batch (the counts live on the device); the blocks past the list's end leave
// at once.
template <int G, int NL, int NVAR>
__global__ __launch_bounds__(WAVE) void solve_list_kernel(
    KArgs P, long B, int cls, const int32_t* __restrict__ ws, const double* __restrict__ state, const double* __restrict__ goal,
    const int8_t* __restrict__ first_foot, const double* __restrict__ delta_in,
    const double* __restrict__ obs_xy, const int32_t* __restrict__ obs_nv,
    double* __restrict__ U, double* __restrict__ X, double* __restrict__ theta_out,
    double* __restrict__ omega_out, double* __restrict__ obj_out, int32_t* __restrict__ status_out,
    int32_t* __restrict__ iters_out, unsigned long long* __restrict__ active_out,
    unsigned long long* __restrict__ working_out, double* __restrict__ c_eta,
    double* __restrict__ diag, const double* __restrict__ bounds, const double* __restrict__ c_eta_in,
    int32_t* __restrict__ cost_out, const int32_t* __restrict__ overflow_in) {
  constexpr int GPW = WAVE / G;
  constexpr int RING_CAP = (G == 16) ? 64 : 256;
  if (blockDim.x != WAVE) __builtin_trap();
  const int count = ws[cls];
  if ((long)blockIdx.x * GPW >= count) return;                    // (wave-uniform; no loop over the list: a loop around the step
                                                                  // costs every body 200-500 B of scratch per lane)
  __shared__ double lds_ring[GPW][RING_CAP][2];
  __shared__ double lds_obs[GPW][SPLIT_MAXOBS][4];
  __shared__ int lds_perm[GPW][SPLIT_MAXOBS];
  __shared__ int lds_flag[GPW];
  const int grp = threadIdx.x / G;
  const long idx = (long)blockIdx.x * GPW + grp;
  const long pb = ws[SPLIT_HEAD + B * (1 + cls) + (idx < count ? idx : count - 1)];
  const StepIn in = load_step_in(P, pb, idx < count, state, goal, first_foot, delta_in, bounds, overflow_in);
  FrontOut<G> F = front_end<G, SPLIT_MAXOBS>(P, in, obs_xy, obs_nv, theta_out, omega_out, c_eta, c_eta_in, true, lds_ring[grp],
                                             lds_obs[grp], lds_perm[grp], &lds_flag[grp]);
  if (F.n_rel > 2 * NL) F.front_flag |= 8;
  step_solve<G, NL, NVAR, false>(P, in, F, lds_obs[grp], lds_perm[grp], U, X, obj_out, status_out, iters_out, active_out, working_out,
                                 diag, nullptr, cost_out);
}

// x+ = A_l x + B_l u of the CoM (px, vx, py, vy) under the input u = (ux, uy) (HumanoidMpc.py:34-48), in place
__device__ __forceinline__ void lip_advance(double ch, double sh_over_beta, double beta_sh, double ux, double uy, double& px,
                                            double& vx, double& py, double& vy) {
  const double px0 = px, vx0 = vx, py0 = py, vy0 = vy;
  px = ch * px0 + sh_over_beta * vx0 + (1.0 - ch) * ux;
  vx = beta_sh * px0 + ch * vx0 - beta_sh * ux;
  py = ch * py0 + sh_over_beta * vy0 + (1.0 - ch) * uy;
  vy = beta_sh * py0 + ch * vy0 - beta_sh * uy;
}

// ------------------------------------------------------------------------------------------
// kernel 2: the closed loop of HumanoidMPC.run_simulation on the device (lipmpc_rollout_batch),
// HumanoidMpc.py:380-459: per sample k: stop if the previous objective < 0.05 (:392); on MPC samples
// (k % mpc_step == 0) solve the step, keep u_0 (:432), advance x+ = A x + B u_0 (:441-442); on the
// other samples only the heading moves (:443-447); theta <- theta_1 (:447); the stance foot of MPC step
// number floor(k / mpc_step) alternates (:104-108, 401-403).  A failed solve ends the robot's run (:419-429).
// Each group owns one robot for the whole run: no host round trip, no batch-wide barrier per step.
// ------------------------------------------------------------------------------------------
template <int G, int NOBS_L, int NVAR>
__global__ __launch_bounds__(WAVE) void rollout_kernel(
    KArgs P, long B, int k_max, int mpc_step, double stop_obj, const double* __restrict__ state0,
    const double* __restrict__ goal, const int8_t* __restrict__ first_foot, const double* __restrict__ delta_in,
    const double* __restrict__ obs_xy, const int32_t* __restrict__ obs_nv, double* __restrict__ X_pred,
    double* __restrict__ U_pred, int32_t* __restrict__ n_steps, int32_t* __restrict__ last_status,
    int32_t* __restrict__ total_iters, const double* __restrict__ bounds) {
  constexpr int GPW = WAVE / G;
  if (blockDim.x != WAVE) __builtin_trap();          // see plan_step_kernel
  const int lane = threadIdx.x & (G - 1);
  const long prob_raw = (long)blockIdx.x * GPW + threadIdx.x / G;
  StepIn in;
  in.valid = prob_raw < B;
  const long pb = in.valid ? prob_raw : (B - 1);
  in.pb = pb;
  load_bounds(P, bounds, pb, in);
  in.p0x = state0[pb * 5 + 0]; in.v0x = state0[pb * 5 + 1]; in.p0y = state0[pb * 5 + 2]; in.v0y = state0[pb * 5 + 3];
  in.th0 = state0[pb * 5 + 4];
  in.gx = goal[pb * 2 + 0]; in.gy = goal[pb * 2 + 1];
  in.foot0 = (double)first_foot[pb];
  in.delta = delta_in ? delta_in[pb] : 0.0;
  double* Xp = X_pred + pb * (long)(k_max + 1) * 5;
  double* Up = U_pred + pb * (long)k_max * 3;
  if (in.valid && lane == 0) { Xp[0] = in.p0x; Xp[1] = in.v0x; Xp[2] = in.p0y; Xp[3] = in.v0y; Xp[4] = in.th0; }
  bool fin = false;
  int k_done = 0, st_last = LIPMPC_STATUS_SOLVED, it_sum = 0;
  double last_obj = INFINITY, ukx = 0.0, uky = 0.0;
  // warm start between MPC steps: register rows only (streamed instantiations start cold), horizons of 2 and more
  constexpr bool CAN_WARM = NOBS_L <= 7;
  const bool use_warm = CAN_WARM && (P.flags & LIPMPC_FLAG_WARM_START) && P.N >= 2;
  __shared__ double lds_warm[GPW][1 + WARM_ROWS][G];
  WarmIO ws;
  ws.lds = use_warm ? &lds_warm[threadIdx.x / G][0][0] : nullptr;
  ws.have = false;
  for (int k = 0; k < k_max; ++k) {
    if (!fin && last_obj < stop_obj) fin = true;
    if (__all(fin)) break;
    if (!fin) {
      const bool is_mpc = (k % mpc_step) == 0;
      double theta1, omega0;
      if (is_mpc) {     // group-uniform (k and mpc_step are wave-uniform)
        const StepOut r = step_body<G, NOBS_L, NVAR, false, true>(P, in, obs_xy, obs_nv, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ws);
        if (use_warm) ws.have = true;             // (a failed solve ends the run anyway)
        st_last = r.status;
        it_sum += r.iters;
        theta1 = r.theta1; omega0 = r.omega0;
        if (r.status != LIPMPC_STATUS_SOLVED && r.status != LIPMPC_STATUS_UNCERTIFIED) fin = true;
        else { last_obj = r.obj; ukx = r.ux; uky = r.uy; }
      } else {
        const double psi = atan2(in.gy - in.p0y, in.gx - in.p0x);
        omega0 = fmin(fmax(psi - in.th0, -in.omega_max), in.omega_max);
        theta1 = in.th0 + omega0 * P.tau;
      }
      if (!fin) {
        if (is_mpc) lip_advance(P.ch, P.sh_over_beta, P.beta_sh, ukx, uky, in.p0x, in.v0x, in.p0y, in.v0y);
        in.th0 = theta1;
        if ((k + 1) % mpc_step == 0) in.foot0 = -in.foot0;
        if (in.valid && lane == 0) {
          Up[3 * k] = ukx; Up[3 * k + 1] = uky; Up[3 * k + 2] = omega0;
          double* xo = Xp + (long)(k + 1) * 5;
          xo[0] = in.p0x; xo[1] = in.v0x; xo[2] = in.p0y; xo[3] = in.v0y; xo[4] = in.th0;
        }
        k_done = k + 1;
      }
    }
  }
  if (in.valid && lane == 0) { n_steps[pb] = k_done; last_status[pb] = st_last; total_iters[pb] = it_sum; }
}

// The buffers of one MPC step (lipmpc_plan_step_batch / _c_eta), in the order the step kernels take them.  Host side only: the
// launchers in lipmpc_inst.hip spell them out as kernel arguments, so every kernel keeps its own __restrict__ parameter list.
struct StepIO {
  const double* state; const double* goal; const int8_t* first_foot; const double* delta;
  const double* obs_xy; const int32_t* obs_nv;
  double* U; double* X; double* theta; double* omega; double* obj; int32_t* status; int32_t* iters;
  unsigned long long* active; unsigned long long* working; double* c_eta; double* diag;
  const double* bounds; const double* c_eta_in; const int32_t* overflow;
};

// host-side launchers of one instantiation (defined in lipmpc_inst.hip, one object per (G, NOBS_L, NVAR))
template <int G, int NOBS_L, int NVAR>
void launch_plan_step(const KArgs& k, long B, const StepIO& io, int32_t* sched, hipStream_t stream);
// the step with warm-start records (register-row instantiations only: NOBS_L <= 7)
template <int G, int NOBS_L, int NVAR>
void launch_warm_step(const KArgs& k, long B, const StepIO& io, int32_t* sched, double* warm_rec, hipStream_t stream);
template <int G, int NOBS_L, int NVAR>
void launch_rollout(const KArgs& k, long B, int k_max, int mpc_step, double stop_obj, const double* state0,
                    const double* goal, const int8_t* first_foot, const double* delta, const double* obs_xy,
                    const int32_t* obs_nv, double* X_pred, double* U_pred, int32_t* n_steps, int32_t* last_status,
                    int32_t* total_iters, const double* bounds, hipStream_t stream);
// one solver body of the split launch over its class's list (32 lanes per problem; defined in lipmpc_inst.hip)
template <int G, int NL, int NVAR>
void launch_solve_list(const KArgs& k, long B, int cls, const int32_t* ws, const StepIO& io, int32_t* cost_out, hipStream_t stream);

}  // namespace lipmpc_dev
