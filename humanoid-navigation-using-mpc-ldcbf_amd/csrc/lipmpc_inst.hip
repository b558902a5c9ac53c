// lipmpc_inst.hip — one explicit instantiation of the step kernel per object file:
// compiled with -DINST_G=<16|32> -DINST_NL=<0|2|5|7|13|25> -DINST_NV=<variable slots: INST_G, or 8 for horizons up to 4> (see Makefile).
// -DINST_LIST: the solver body of the split launch with INST_NL row slots per lane instead (solve_list_kernel: one kernel per
// body, each with its own register allocation).  The register-row objects (INST_NL <= 7; on 32 lanes INST_NL <= 2, the bodies
// that compile without scratch) also hold the step with warm-start records (warm_step_kernel).
#include "lipmpc_kernel.hpp"

namespace lipmpc_dev {

#ifdef INST_LIST
template <int G, int NL, int NVAR>
void launch_solve_list(const KArgs& k, long B, int cls, const int32_t* ws, const StepIO& io, int32_t* cost_out, hipStream_t stream) {
  constexpr int GPW = WAVE / G;
  const unsigned blocks = (unsigned)((B + GPW - 1) / GPW);      // the whole batch's grid: the list's length lives on the device
  hipLaunchKernelGGL((solve_list_kernel<G, NL, NVAR>), dim3(blocks), dim3(WAVE), 0, stream, k, B, cls, ws, io.state, io.goal,
                     io.first_foot, io.delta, io.obs_xy, io.obs_nv, io.U, io.X, io.theta, io.omega, io.obj, io.status, io.iters,
                     io.active, io.working, io.c_eta, io.diag, io.bounds, io.c_eta_in, cost_out, io.overflow);
}
template void launch_solve_list<INST_G, INST_NL, INST_NV>(const KArgs&, long, int, const int32_t*, const StepIO&, int32_t*, hipStream_t);
#else

template <int G, int NOBS_L, int NVAR>
void launch_plan_step(const KArgs& k, long B, const StepIO& io, int32_t* sched, hipStream_t stream) {
  constexpr int GPW = WAVE / G;
  const unsigned blocks = (unsigned)((B + GPW - 1) / GPW);
  // exact mode with the presolve: the kernel with the small solver bodies; otherwise the handle's body alone
  auto kernel = (k.flags & (LIPMPC_FLAG_INTERIOR | LIPMPC_FLAG_NO_PRESOLVE | LIPMPC_FLAG_WARM_START))
                    ? plan_step_kernel<G, NOBS_L, NVAR, false> : plan_step_kernel<G, NOBS_L, NVAR, true>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(WAVE), 0, stream, k, B, io.state, io.goal, io.first_foot, io.delta, io.obs_xy,
                     io.obs_nv, io.U, io.X, io.theta, io.omega, io.obj, io.status, io.iters, io.active, io.working, io.c_eta,
                     io.diag, io.bounds, io.c_eta_in, sched, io.overflow);
}
template void launch_plan_step<INST_G, INST_NL, INST_NV>(const KArgs&, long, const StepIO&, int32_t*, hipStream_t);

#if INST_NL <= (INST_G == 32 ? 2 : 7)      // (warm_capable in lipmpc_api.hip)
template <int G, int NOBS_L, int NVAR>
void launch_warm_step(const KArgs& k, long B, const StepIO& io, int32_t* sched, double* warm_rec, hipStream_t stream) {
  constexpr int GPW = WAVE / G;
  const unsigned blocks = (unsigned)((B + GPW - 1) / GPW);
  hipLaunchKernelGGL((warm_step_kernel<G, NOBS_L, NVAR>), dim3(blocks), dim3(WAVE), 0, stream, k, B, io.state, io.goal, io.first_foot,
                     io.delta, io.obs_xy, io.obs_nv, io.U, io.X, io.theta, io.omega, io.obj, io.status, io.iters, io.active,
                     io.working, io.c_eta, io.diag, io.bounds, io.c_eta_in, sched, io.overflow, warm_rec);
}
template void launch_warm_step<INST_G, INST_NL, INST_NV>(const KArgs&, long, const StepIO&, int32_t*, double*, hipStream_t);
#endif

template <int G, int NOBS_L, int NVAR>
void launch_rollout(const KArgs& k, long B, int k_max, int mpc_step, double stop_obj, const double* state0,
                    const double* goal, const int8_t* first_foot, const double* delta, const double* obs_xy,
                    const int32_t* obs_nv, double* X_pred, double* U_pred, int32_t* n_steps, int32_t* last_status,
                    int32_t* total_iters, const double* bounds, hipStream_t stream) {
  constexpr int GPW = WAVE / G;
  const unsigned blocks = (unsigned)((B + GPW - 1) / GPW);
  hipLaunchKernelGGL((rollout_kernel<G, NOBS_L, NVAR>), dim3(blocks), dim3(WAVE), 0, stream, k, B, k_max, mpc_step, stop_obj,
                     state0, goal, first_foot, delta, obs_xy, obs_nv, X_pred, U_pred, n_steps, last_status, total_iters, bounds);
}

template void launch_rollout<INST_G, INST_NL, INST_NV>(const KArgs&, long, int, int, double, const double*, const double*,
                                              const int8_t*, const double*, const double*, const int32_t*, double*,
                                              double*, int32_t*, int32_t*, int32_t*, const double*, hipStream_t);
#endif  // INST_LIST

}  // namespace lipmpc_dev
