// lipmpc_api.hip — C ABI (include/lipmpc.h): handle, parameter checks, kernel dispatch, state advance.
#include <type_traits>

#include "lipmpc_kernel.hpp"

using namespace lipmpc_dev;

namespace {
// state advance (HumanoidMpc.py:432-447)
__global__ void advance_kernel(long B, double ch, double sh_over_beta, double beta_sh, double* __restrict__ state,
                               int8_t* __restrict__ foot, const double* __restrict__ U, const double* __restrict__ theta,
                               const int32_t* __restrict__ status, int N) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int st = status[b];
  if (st != LIPMPC_STATUS_SOLVED && st != LIPMPC_STATUS_UNCERTIFIED) return;
  double* x = state + b * 5;
  const double ux = U[b * N * 2 + 0], uy = U[b * N * 2 + 1];
  lip_advance(ch, sh_over_beta, beta_sh, ux, uy, x[0], x[1], x[2], x[3]);
  x[4] = theta[b * (N + 1) + 1];
  foot[b] = (int8_t)(-foot[b]);
}

// one sample of a host-driven fleet loop (include/lipmpc.h: lipmpc_fleet_update_batch)
__global__ void fleet_update_kernel(long B, int k_max, double stop_obj, double ch, double sh_over_beta, double beta_sh, int N,
                                    double* __restrict__ state, int8_t* __restrict__ foot, int8_t* __restrict__ walking,
                                    double* __restrict__ last_obj, int32_t* __restrict__ n_steps,
                                    int32_t* __restrict__ last_status, int32_t* __restrict__ n_overflow,
                                    const int32_t* __restrict__ sample, double* __restrict__ X_pred,
                                    double* __restrict__ U_pred, const double* __restrict__ U,
                                    const double* __restrict__ theta, const double* __restrict__ omega,
                                    const double* __restrict__ obj, const int32_t* __restrict__ status,
                                    const int32_t* __restrict__ overflow) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int k = *sample;
  if (k >= k_max) return;
  bool w = walking[b] != 0 && last_obj[b] >= stop_obj;
  // a scan whose clusters did not fit the obstacle slots is a failed sample: planning against a truncated
  // obstacle list would let the robot walk through something it sensed
  const int st = (overflow && overflow[b]) ? LIPMPC_STATUS_SENSOR_OVERFLOW : status[b];
  if (w && overflow) n_overflow[b] += overflow[b];
  if (w) last_status[b] = st;
  w = w && (st == LIPMPC_STATUS_SOLVED || st == LIPMPC_STATUS_UNCERTIFIED);
  double* x = state + b * 5;
  const double ux = U[b * N * 2 + 0], uy = U[b * N * 2 + 1];
  if (w) {
    last_obj[b] = obj[b];
    lip_advance(ch, sh_over_beta, beta_sh, ux, uy, x[0], x[1], x[2], x[3]);
    x[4] = theta[b * (N + 1) + 1];
    foot[b] = (int8_t)(-foot[b]);
    n_steps[b] += 1;
  }
  walking[b] = w ? 1 : 0;
  double* up = U_pred + (b * (long)k_max + k) * 3;
  up[0] = ux; up[1] = uy; up[2] = omega[b * N];
  double* xp = X_pred + (b * (long)(k_max + 1) + k + 1) * 5;
  for (int i = 0; i < 5; ++i) xp[i] = x[i];
}
__global__ void fleet_next_sample_kernel(int32_t* sample) { *sample += 1; }

// The capture step of a robot whose solve failed (include/lipmpc.h: lipmpc_fleet_recover_update_batch), every expression as the
// contract writes it: the capture point, the least margin of the sample's rows at it, the heading rule of the step at k = 0.
struct CaptureStep { double cpx, cpy, margin, omega, theta; };
__device__ __forceinline__ CaptureStep capture_step(const double* __restrict__ x, double beta, double omega_max, double tau,
                                                    const double* __restrict__ goal, const double* __restrict__ rows, int n_obs,
                                                    double delta) {
#pragma clang fp contract(off)
  CaptureStep s;
  s.cpx = x[0] + x[1] / beta;
  s.cpy = x[2] + x[3] / beta;
  double margin = INFINITY;
  bool nan_row = false;
  for (int j = 0; j < n_obs; ++j) {
    const double cx = rows[4 * j], cy = rows[4 * j + 1], ex = rows[4 * j + 2], ey = rows[4 * j + 3];
    if (ex == 0.0 && ey == 0.0) continue;                  // an empty slot (a NaN in eta is a used row)
    const double m = (ex * (s.cpx - cx) + ey * (s.cpy - cy)) - delta;
    nan_row = nan_row || m != m;
    margin = fmin(margin, m);
  }
  s.margin = nan_row ? -INFINITY : margin;           // (NaN is kept for "not evaluated")
  s.omega = fmin(fmax(atan2(goal[1] - x[2], goal[0] - x[0]) - x[4], -omega_max), omega_max);
  s.theta = x[4] + s.omega * tau;
  return s;
}

// one sample of a host-driven fleet loop in which a failed solve costs a capture step instead of the robot
// (include/lipmpc.h: lipmpc_fleet_recover_update_batch); fleet_update_kernel's rule around it
__global__ void fleet_recover_update_kernel(long B, int k_max, double stop_obj, double ch, double sh_over_beta, double beta_sh,
                                            double beta, double omega_max, double tau, int N, int n_obs,
                                            double* __restrict__ state, int8_t* __restrict__ foot, int8_t* __restrict__ walking,
                                            double* __restrict__ last_obj, int32_t* __restrict__ n_steps,
                                            int32_t* __restrict__ last_status, int32_t* __restrict__ n_overflow,
                                            const int32_t* __restrict__ sample, double* __restrict__ X_pred,
                                            double* __restrict__ U_pred, const double* __restrict__ U,
                                            const double* __restrict__ theta, const double* __restrict__ omega,
                                            const double* __restrict__ obj, const int32_t* __restrict__ status,
                                            const int32_t* __restrict__ overflow, const double* __restrict__ goal,
                                            const double* __restrict__ c_eta, const double* __restrict__ delta, int max_recover,
                                            int32_t* __restrict__ recover_run, int32_t* __restrict__ n_recover,
                                            double* __restrict__ recover_margin) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int k = *sample;
  if (k >= k_max) return;
  bool w = walking[b] != 0 && last_obj[b] >= stop_obj;
  const int st = (overflow && overflow[b]) ? LIPMPC_STATUS_SENSOR_OVERFLOW : status[b];
  if (w && overflow) n_overflow[b] += overflow[b];
  if (w) last_status[b] = st;
  const bool solved = st == LIPMPC_STATUS_SOLVED || st == LIPMPC_STATUS_UNCERTIFIED;
  double* x = state + b * 5;
  double margin = NAN;
  bool recover = false;
  CaptureStep cs{};
  if (w && (st == LIPMPC_STATUS_INFEASIBLE || st == LIPMPC_STATUS_MAX_ITER) && recover_run[b] < max_recover &&
      isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(x[3])) {
    cs = capture_step(x, beta, omega_max, tau, goal + b * 2, c_eta ? c_eta + b * (long)n_obs * 4 : nullptr, c_eta ? n_obs : 0,
                      delta ? delta[b] : 0.0);
    margin = cs.margin;
    recover = margin >= 0.0;
  }
  double ux, uy, om;
  if (recover) {                                           // (the failed solve's outputs are NaN: not read)
    ux = cs.cpx; uy = cs.cpy; om = cs.omega;
    lip_advance(ch, sh_over_beta, beta_sh, ux, uy, x[0], x[1], x[2], x[3]);
    x[4] = cs.theta;
    foot[b] = (int8_t)(-foot[b]);
    recover_run[b] += 1;
    n_recover[b] += 1;
  } else {
    ux = U[b * N * 2 + 0]; uy = U[b * N * 2 + 1]; om = omega[b * N];
    w = w && solved;
    if (w) {
      last_obj[b] = obj[b];
      lip_advance(ch, sh_over_beta, beta_sh, ux, uy, x[0], x[1], x[2], x[3]);
      x[4] = theta[b * (N + 1) + 1];
      foot[b] = (int8_t)(-foot[b]);
      n_steps[b] += 1;
      if (max_recover > 0) recover_run[b] = 0;
    }
  }
  walking[b] = w ? 1 : 0;
  recover_margin[b] = margin;
  double* up = U_pred + (b * (long)k_max + k) * 3;
  up[0] = ux; up[1] = uy; up[2] = om;
  double* xp = X_pred + (b * (long)(k_max + 1) + k + 1) * 5;
  for (int i = 0; i < 5; ++i) xp[i] = x[i];
}

// The order of the NEXT step launch on a schedule from the costs this launch left: problems by descending cost (counting
// sort, one workgroup; which of two equally costly problems comes first is immaterial).
__global__ __launch_bounds__(1024) void order_by_cost_kernel(long B, int32_t* __restrict__ sched) {
  __shared__ int cursor_[SCHED_COST_BINS];
  const int32_t* w = sched + SCHED_ORDER + B;
  int32_t* order = sched + SCHED_ORDER;
  for (int k = threadIdx.x; k < SCHED_COST_BINS; k += blockDim.x) cursor_[k] = 0;
  __syncthreads();
  for (long i = threadIdx.x; i < B; i += blockDim.x) atomicAdd(&cursor_[SCHED_COST_BINS - 1 - min(max(w[i], 0), SCHED_COST_BINS - 1)], 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int k = 0; k < SCHED_COST_BINS; ++k) { const int c = cursor_[k]; cursor_[k] = run; run += c; }
  }
  __syncthreads();
  for (long i = threadIdx.x; i < B; i += blockDim.x)
    order[atomicAdd(&cursor_[SCHED_COST_BINS - 1 - min(max(w[i], 0), SCHED_COST_BINS - 1)], 1)] = (int32_t)i;
  if (threadIdx.x == 0) sched[SCHED_VALID] = (int32_t)B;
}

// Index lists per class from the sort keys (class, cost bucket): a STABLE counting sort in one workgroup -- every thread owns a
// contiguous run of problems and counts its keys (bytes in LDS); per key one wave scans the counts over the threads (eight
// threads' bytes per lane as one 64-bit word, a wave prefix sum over the lanes); then the writes -- so the lists, and with them
// which problems share a wave, are a function of the batch alone.  The list of a class is the concatenation of its buckets,
// dearest first.
constexpr int BIN_THREADS = 512;
constexpr int BIN_KEYS = SPLIT_CLASSES * SPLIT_BUCKETS;
constexpr long BIN_MAX_B = 255L * BIN_THREADS;          // a thread's run holds at most 255 problems (byte counters)
__device__ __forceinline__ int bin_key(int k) { return min(max(k, 0), BIN_KEYS - 1); }
__global__ __launch_bounds__(BIN_THREADS) void split_bin_kernel(long B, int32_t* __restrict__ ws) {
  __shared__ __attribute__((aligned(8))) unsigned char cnt_[BIN_KEYS][BIN_THREADS];
  __shared__ int start_[BIN_KEYS][BIN_THREADS / 8];      // problems with this key in the runs of the threads before lane's eight
  __shared__ int total_[BIN_KEYS], base_[BIN_KEYS];
  const int t = threadIdx.x;
  const long per = (B + BIN_THREADS - 1) / BIN_THREADS, lo = min((long)t * per, B), hi = min(lo + per, B);
  const int32_t* key = ws + SPLIT_HEAD;
  unsigned* z = reinterpret_cast<unsigned*>(&cnt_[0][0]);
  for (int i = t; i < BIN_KEYS * BIN_THREADS / 4; i += BIN_THREADS) z[i] = 0u;
  __syncthreads();
  for (long i = lo; i < hi; ++i) cnt_[bin_key(key[i])][t] += 1;      // (own column: no race)
  __syncthreads();
  const int wave = t >> 6, lane = t & 63;
  for (int k = wave; k < BIN_KEYS; k += BIN_THREADS / 64) {
    const unsigned long long w = *reinterpret_cast<const unsigned long long*>(&cnt_[k][8 * lane]);
    int mine = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) mine += (int)((w >> (8 * u)) & 0xffull);
    int incl = mine;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { const int o = __shfl_up(incl, m, 64); if (lane >= m) incl += o; }
    start_[k][lane] = incl - mine;
    if (lane == 63) total_[k] = incl;
  }
  __syncthreads();
  if (t < SPLIT_CLASSES) {
    int run = 0;
    for (int q = 0; q < SPLIT_BUCKETS; ++q) { base_[t * SPLIT_BUCKETS + q] = run; run += total_[t * SPLIT_BUCKETS + q]; }
    ws[t] = run;
  }
  __syncthreads();
  for (long i = lo; i < hi; ++i) {
    const int k = bin_key(key[i]);
    // position: the key's base inside its class list + the runs of the earlier threads + this thread's earlier problems of the key
    int pos = base_[k] + start_[k][t >> 3];
    for (int u = t & ~7; u < t; ++u) pos += cnt_[k][u];
    for (long j = lo; j < i; ++j) pos += (bin_key(key[j]) == k) ? 1 : 0;
    ws[SPLIT_HEAD + B * (1 + k / SPLIT_BUCKETS) + pos] = (int32_t)i;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
struct lipmpc_handle {
  lipmpc_params p;
  KArgs k;
  int device;
  int G;
  int nobs_l;
  int nvar;     // variable slots of the factorisation: G, or 8 (horizons up to 4, register-row instantiations)
  int32_t* sched;       // optional schedule buffer (lipmpc_set_schedule), device memory owned by the caller
  int64_t sched_cap;    // largest batch it holds
  int32_t* ws;          // optional split-launch workspace (lipmpc_set_workspace), device memory owned by the caller
  int64_t ws_cap;
  double* warm;         // optional warm-start records (lipmpc_set_warm_start), device memory owned by the caller
  int64_t warm_cap;     // problems they hold
  hipStream_t side[SPLIT_CLASSES - 1];     // the solver bodies of a split launch run side by side (created with the workspace)
  hipEvent_t fork_ev, join_ev[SPLIT_CLASSES - 1];
  bool have_streams;
};

// The instantiation table: f(G, NOBS_L, NVAR) as std::integral_constant arguments for the handle's (G, nobs_l, nvar), the last
// row slot count of a list taking every larger nobs_l.  The objects that hold these instantiations are the INST_OBJS of the
// Makefile: a triple added here needs its object there, and the reverse.
template <int V> using IntC = std::integral_constant<int, V>;
template <int G, int NVAR, int NL, int... MORE, class F>
static void dispatch_nl(int nobs_l, F& f) {
  if constexpr (sizeof...(MORE) == 0) f(IntC<G>{}, IntC<NL>{}, IntC<NVAR>{});
  else if (nobs_l == NL) f(IntC<G>{}, IntC<NL>{}, IntC<NVAR>{});
  else dispatch_nl<G, NVAR, MORE...>(nobs_l, f);
}
template <class F>
static void with_instantiation(const lipmpc_handle* h, F&& f) {
  if (h->G == 16 && h->nvar == 8) dispatch_nl<16, 8, 0, 2, 5, 7>(h->nobs_l, f);
  else if (h->G == 16) dispatch_nl<16, 16, 0, 2, 5, 7, 13, 25>(h->nobs_l, f);
  else dispatch_nl<32, 32, 0, 2, 5, 7, 13, 25>(h->nobs_l, f);
}

// The solver body of split class `cls` (split_slots(cls) row slots per lane) over its list: the objects list_32_<slots>.o, the
// LIST_NLS of the Makefile
static_assert(split_slots(0) == 1 && split_slots(1) == 2 && split_slots(2) == 4 && split_slots(3) == 13 && split_slots(4) == 25,
              "the Makefile's LIST_NLS builds the bodies of the classes");
template <int C = 0>
static void launch_class_body(int cls, const KArgs& k, long B, const int32_t* ws, const StepIO& io, int32_t* cost,
                              hipStream_t stream) {
  if constexpr (C + 1 < SPLIT_CLASSES) {
    if (cls != C) return launch_class_body<C + 1>(cls, k, B, ws, io, cost, stream);
  }
  launch_solve_list<32, split_slots(C), 32>(k, B, C, ws, io, cost, stream);
}

extern "C" {

int lipmpc_default_params(lipmpc_params* p) {
  if (!p) return LIPMPC_E_ARG;
  memset(p, 0, sizeof(*p));
  p->N = 3; p->n_obs_max = 0; p->v_max = 5; p->max_iter = 60; p->flags = 0; p->finish_rounds = 0;
  p->dt = 0.4; p->g = 9.81; p->h_com = 1.0; p->alpha = 3.6;
  p->l_max[0] = 0.10; p->l_max[1] = 0.10; p->l_min[0] = -0.1; p->l_min[1] = -0.1;
  p->v_min[0] = -0.1; p->v_min[1] = 0.1; p->v_max_xy[0] = 0.8; p->v_max_xy[1] = 0.4;
  p->omega_max = 0.156 * M_PI; p->ell = 0.05; p->sampling_time = 0.4;
  p->tol = 1e-11; p->tol_interior = 1e-9; p->k0_tol = 1e-5;
  return LIPMPC_OK;
}

int64_t lipmpc_num_rows(const lipmpc_params* p) { return p ? 9L * p->N + (long)(p->N + 1) * p->n_obs_max : LIPMPC_E_ARG; }
int64_t lipmpc_active_words(const lipmpc_params* p) { return p ? (lipmpc_num_rows(p) + 63) / 64 : LIPMPC_E_ARG; }

int lipmpc_create(const lipmpc_params* p, int device, lipmpc_handle** out) {
  if (!p || !out) return LIPMPC_E_ARG;
  if (p->N < 1 || p->N > 16 || p->n_obs_max < 0 || p->n_obs_max > 50 || p->v_max < 3 || p->v_max > 32 ||
      p->max_iter < 1 || p->finish_rounds < 0 || p->finish_rounds > 64 || !(p->tol > 0.0) || !(p->tol_interior > 0.0) || !(p->dt > 0.0) || !(p->h_com > 0.0) || !(p->g > 0.0))
    return LIPMPC_E_UNSUPPORTED;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return LIPMPC_E_HIP;
  lipmpc_handle* h = (lipmpc_handle*)calloc(1, sizeof(lipmpc_handle));
  if (!h) return LIPMPC_E_NOMEM;
  h->p = *p;
  h->device = device;
  h->G = (p->N <= 8) ? 16 : 32;
  const int need = (p->n_obs_max + 1) / 2;
  h->nobs_l = need == 0 ? 0 : need <= 2 ? 2 : need <= 5 ? 5 : need <= 7 ? 7 : need <= 13 ? 13 : 25;
  h->nvar = (h->G == 16 && p->N <= 4 && h->nobs_l <= 7) ? 8 : h->G;
  KArgs& k = h->k;
  k.N = p->N; k.n_obs = p->n_obs_max; k.nvert_max = p->v_max; k.max_iter = p->max_iter; k.flags = p->flags;
  k.fin_rounds = p->finish_rounds > 0 ? p->finish_rounds : (p->N <= 8 ? FIN_ROUNDS : FIN_ROUNDS_LONG);
  k.m_tot = (int)lipmpc_num_rows(p); k.words = (int)lipmpc_active_words(p);
  const double beta = sqrt(p->g / p->h_com), ch = cosh(beta * p->dt), sh = sinh(beta * p->dt);
  k.kappa = beta * sh / (ch - 1.0); k.ch = ch; k.sh_over_beta = sh / beta; k.inv_one_minus_ch = 1.0 / (1.0 - ch);
  k.beta_sh = beta * sh;
  for (int i = 0; i < 2; ++i) { k.l_max[i] = p->l_max[i]; k.l_min[i] = p->l_min[i]; k.v_min[i] = p->v_min[i]; k.v_max[i] = p->v_max_xy[i]; }
  k.alpha_over_pi = p->alpha / M_PI; k.omega_max = p->omega_max; k.ell = p->ell; k.tau = p->sampling_time;
  k.tol = (p->flags & LIPMPC_FLAG_INTERIOR) ? p->tol_interior : p->tol; k.k0_tol = p->k0_tol;
  {   // presolve bound (oracle: reach_step): the largest |p_{k+1} - p_k| the leg-reach rows allow
#pragma clang fp contract(off)
    const double dx = fmax(fabs(p->l_max[0]), fabs(p->l_min[0])), dy = fmax(fabs(p->l_max[1]), fabs(p->l_min[1])) + fabs(p->ell);
    k.reach_step = sqrt(dx * dx + dy * dy);
  }
  *out = h;
  return LIPMPC_OK;
}

static void drop_streams(lipmpc_handle* h) {
  if (!h->have_streams) return;
  (void)hipSetDevice(h->device);
  for (int i = 0; i < SPLIT_CLASSES - 1; ++i) { (void)hipStreamDestroy(h->side[i]); (void)hipEventDestroy(h->join_ev[i]); }
  (void)hipEventDestroy(h->fork_ev);
  h->have_streams = false;
}

void lipmpc_destroy(lipmpc_handle* h) {
  if (!h) return;
  drop_streams(h);
  free(h);
}

// does this handle's step run as a split launch when it has a workspace?  (32 lanes per problem, obstacles, presolve on)
static bool split_capable(const lipmpc_handle* h) {
  return h->G == 32 && h->nobs_l > 0 && !(h->p.flags & (LIPMPC_FLAG_INTERIOR | LIPMPC_FLAG_NO_PRESOLVE | LIPMPC_FLAG_WARM_START));
}

int64_t lipmpc_workspace_bytes(const lipmpc_handle* h, int64_t capacity) {
  if (!h || capacity < 0) return LIPMPC_E_ARG;
  return split_capable(h) ? (int64_t)sizeof(int32_t) * (SPLIT_HEAD + (1 + SPLIT_CLASSES) * capacity) : 0;
}

int lipmpc_set_workspace(lipmpc_handle* h, void* workspace, int64_t capacity) {
  if (!h || capacity < 0 || (workspace && capacity > 0x0fffffff)) return LIPMPC_E_ARG;
  h->ws = (capacity > 0 && split_capable(h)) ? (int32_t*)workspace : nullptr;
  h->ws_cap = h->ws ? capacity : 0;
  if (h->ws && !h->have_streams) {
    if (hipSetDevice(h->device) != hipSuccess) return LIPMPC_E_HIP;
    bool ok = hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming) == hipSuccess;
    // (plain streams: side streams of the highest priority, tried so that the dearer bodies' waves are placed first, made the
    // launch 35 % slower -- the high-priority queues delay the next launch's classification and the fork / join events)
    for (int i = 0; ok && i < SPLIT_CLASSES - 1; ++i)
      ok = hipStreamCreateWithFlags(&h->side[i], hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&h->join_ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) { h->ws = nullptr; h->ws_cap = 0; return LIPMPC_E_HIP; }      // (a partial set leaks a few handles at process scope only)
    h->have_streams = true;
  }
  return LIPMPC_OK;
}

// Split launch: classes -> lists -> one kernel per solver body, side by side.  The rare, long bodies go first on their own
// streams (a few waves each, they must not queue behind 2048 short ones); the caller's stream takes the 1-slot body and
// waits for the others.  A failure after the fork enqueues no further body, but every side stream that took the fork is still
// joined back to the caller's stream (nothing of this launch outlives the caller's stream; a capture stays joined).
static int split_step(lipmpc_handle* h, long B, const StepIO& io, int32_t* sched, hipStream_t stream) {
  constexpr int GPW = WAVE / 32;
  const unsigned blocks = (unsigned)((B + GPW - 1) / GPW);
  int32_t* ws = h->ws;
  int32_t* cost = sched ? sched + SCHED_ORDER + B : nullptr;
  hipLaunchKernelGGL((classify_kernel<32>), dim3(blocks), dim3(WAVE), 0, stream, h->k, B, io.state, io.goal, io.delta, io.obs_xy,
                     io.obs_nv, io.bounds, io.c_eta_in, ws);
  if (hipGetLastError() != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(split_bin_kernel, dim3(1), dim3(BIN_THREADS), 0, stream, B, ws);
  if (hipGetLastError() != hipSuccess) return LIPMPC_E_HIP;
  const int top = split_class_of((h->p.n_obs_max + 1) / 2);
  // Which body goes where: the waves of a kernel are placed in launch order and a kernel that starts first takes the free
  // SIMDs first.  The 1-slot body has the most problems and the cheapest ones: it goes LAST, on a side stream (a side
  // stream's kernel starts ~10 us after the caller's stream's: the fork event); the 2-slot body -- a third of the problems,
  // dearer ones -- takes the caller's stream and with it the first pick of the SIMDs; the rare bodies with more slots start
  // next to it.  (Measured at N = 16 / 50 obstacles, B = 4096: 1-slot body on the caller's stream 0.640 ms, this 0.6xx.)
  if (hipEventRecord(h->fork_ev, stream) != hipSuccess) return LIPMPC_E_HIP;
  const int on_main = top >= 1 ? 1 : 0;
  int joined[SPLIT_CLASSES - 1], n_joined = 0;        // side streams whose join event is recorded
  bool ok = true;
  for (int c = top; c >= 0 && ok; --c) {
    if (c == on_main) continue;
    const int si = c < on_main ? c : c - 1;                                // four side streams for the four other classes
    hipStream_t st = h->side[si];
    if (hipStreamWaitEvent(st, h->fork_ev, 0) != hipSuccess) { ok = false; break; }
    launch_class_body(c, h->k, B, ws, io, cost, st);
    ok = hipGetLastError() == hipSuccess;
    if (hipEventRecord(h->join_ev[si], st) == hipSuccess) joined[n_joined++] = si;
    else ok = false;
  }
  if (ok) {
    launch_class_body(on_main, h->k, B, ws, io, cost, stream);
    ok = hipGetLastError() == hipSuccess;
  }
  for (int i = 0; i < n_joined; ++i) ok = hipStreamWaitEvent(stream, h->join_ev[joined[i]], 0) == hipSuccess && ok;
  return ok ? LIPMPC_OK : LIPMPC_E_HIP;
}

static int plan_step_impl(lipmpc_handle* h, int64_t B, const StepIO& io, void* hip_stream) {
  if (!h || B < 0) return LIPMPC_E_ARG;
  if (B == 0) return LIPMPC_OK;
  if (!io.state || !io.goal || !io.first_foot || !io.U || !io.X || !io.theta || !io.omega || !io.obj || !io.status || !io.iters ||
      !io.active)
    return LIPMPC_E_ARG;
  if (h->p.n_obs_max > 0 && !io.c_eta_in && (!io.obs_xy || !io.obs_nv)) return LIPMPC_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t stream = (hipStream_t)hip_stream;
  int32_t* sched = (h->sched && B <= h->sched_cap) ? h->sched : nullptr;
  if (h->warm) {
    if (B > h->warm_cap) return LIPMPC_E_ARG;
    // (lipmpc_set_warm_start admits the warm_capable instantiations only; no other is ever launched here)
    with_instantiation(h, [&](auto G, auto NL, auto NV) {
      if constexpr (NL <= (G == 32 ? 2 : 7)) launch_warm_step<G, NL, NV>(h->k, (long)B, io, sched, h->warm, stream);
    });
  } else if (h->ws && B <= h->ws_cap && B <= BIN_MAX_B && split_capable(h)) {
    if (split_step(h, (long)B, io, sched, stream) != LIPMPC_OK) return LIPMPC_E_HIP;
  } else {
    with_instantiation(h, [&](auto G, auto NL, auto NV) { launch_plan_step<G, NL, NV>(h->k, (long)B, io, sched, stream); });
  }
  if (sched) hipLaunchKernelGGL(order_by_cost_kernel, dim3(1), dim3(1024), 0, stream, (long)B, sched);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}

int lipmpc_set_schedule(lipmpc_handle* h, int32_t* schedule, int64_t capacity) {
  if (!h || capacity < 0 || (schedule && capacity > 0x3fffffff)) return LIPMPC_E_ARG;
  h->sched = capacity > 0 ? schedule : nullptr;
  h->sched_cap = h->sched ? capacity : 0;
  return LIPMPC_OK;
}

int64_t lipmpc_schedule_words(int64_t B) { return B < 0 ? LIPMPC_E_ARG : SCHED_ORDER + 2L * B; }

// the instantiations with warm_step_kernel (lipmpc_inst.hip: WARM_INST): horizons of 2 and more, register rows, and on 32 lanes
// at most 2 row slots per lane -- the 32-lane bodies with 5 and 7 slots spill to scratch (240 B per lane at 7)
static bool warm_capable(const lipmpc_handle* h) { return h->p.N >= 2 && h->nobs_l <= (h->G == 32 ? 2 : 7); }

int64_t lipmpc_warm_words(const lipmpc_params* p) { return p ? 1L + 2L * p->N + lipmpc_num_rows(p) : LIPMPC_E_ARG; }

int lipmpc_set_warm_start(lipmpc_handle* h, double* record, int64_t capacity) {
  if (!h || capacity < 0) return LIPMPC_E_ARG;
  if (!record || capacity == 0) { h->warm = nullptr; h->warm_cap = 0; return LIPMPC_OK; }
  if (!(h->p.flags & LIPMPC_FLAG_WARM_START)) return LIPMPC_E_ARG;      // (warm => every row kept: the one presolve rule)
  if (!warm_capable(h)) return LIPMPC_E_UNSUPPORTED;
  h->warm = record;
  h->warm_cap = capacity;
  return LIPMPC_OK;
}

int lipmpc_plan_step_batch(lipmpc_handle* h, int64_t B, const double* state, const double* goal,
                           const int8_t* first_foot, const double* delta, const double* obs_xy,
                           const int32_t* obs_nv, double* U, double* X, double* theta, double* omega,
                           double* obj, int32_t* status, int32_t* iters, uint64_t* active, uint64_t* working, double* c_eta,
                           double* diag, const double* bounds, void* hip_stream) {
  const StepIO io{state, goal, first_foot, delta, obs_xy, obs_nv, U, X, theta, omega, obj, status, iters,
                  (unsigned long long*)active, (unsigned long long*)working, c_eta, diag, bounds, /*c_eta_in=*/nullptr,
                  /*overflow=*/nullptr};
  return plan_step_impl(h, B, io, hip_stream);
}

int lipmpc_plan_step_batch_c_eta(lipmpc_handle* h, int64_t B, const double* state, const double* goal,
                                 const int8_t* first_foot, const double* delta, const double* c_eta_in,
                                 const int32_t* overflow, double* U, double* X, double* theta, double* omega, double* obj,
                                 int32_t* status, int32_t* iters, uint64_t* active, uint64_t* working, double* diag,
                                 const double* bounds, void* hip_stream) {
  if (h && h->p.n_obs_max > 0 && !c_eta_in) return LIPMPC_E_ARG;
  const StepIO io{state, goal, first_foot, delta, /*obs_xy=*/nullptr, /*obs_nv=*/nullptr, U, X, theta, omega, obj, status, iters,
                  (unsigned long long*)active, (unsigned long long*)working, /*c_eta=*/nullptr, diag, bounds, c_eta_in, overflow};
  return plan_step_impl(h, B, io, hip_stream);
}

int lipmpc_rollout_batch(lipmpc_handle* h, int64_t B, int32_t k_max, int32_t mpc_step, double stop_obj,
                         const double* state0, const double* goal, const int8_t* first_foot, const double* delta,
                         const double* obs_xy, const int32_t* obs_nv, double* X_pred, double* U_pred,
                         int32_t* n_steps, int32_t* last_status, int32_t* total_iters, const double* bounds,
                         void* hip_stream) {
  if (!h || B < 0 || k_max < 1 || mpc_step < 1) return LIPMPC_E_ARG;
  if (B == 0) return LIPMPC_OK;
  if (!state0 || !goal || !first_foot || !X_pred || !U_pred || !n_steps || !last_status || !total_iters) return LIPMPC_E_ARG;
  if (h->p.n_obs_max > 0 && (!obs_xy || !obs_nv)) return LIPMPC_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t stream = (hipStream_t)hip_stream;
  with_instantiation(h, [&](auto G, auto NL, auto NV) {
    launch_rollout<G, NL, NV>(h->k, (long)B, k_max, mpc_step, stop_obj, state0, goal, first_foot, delta, obs_xy, obs_nv, X_pred,
                              U_pred, n_steps, last_status, total_iters, bounds, stream);
  });
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}

int lipmpc_sense_plan_step_batch(lipmpc_handle* h, int64_t B, int32_t resolution, int32_t n_env, int32_t v_env,
                                 int32_t env_shared, double lidar_range, double eps, int32_t min_samples,
                                 const double* state, const double* goal, const int8_t* first_foot, const double* delta,
                                 const double* env_xy, const int32_t* env_nv, const double* ray_table, const double* noise,
                                 double* c_eta, int32_t* n_inferred, int32_t* overflow, int32_t* schedule,
                                 double* U, double* X, double* theta, double* omega, double* obj, int32_t* status,
                                 int32_t* iters, uint64_t* active, uint64_t* working, double* diag, const double* bounds,
                                 void* hip_stream) {
  if (!h || B < 0) return LIPMPC_E_ARG;
  if (h->p.n_obs_max < 1) return LIPMPC_E_UNSUPPORTED;        // a handle without obstacle slots has nothing to sense into
  if (!c_eta || !goal || !first_foot || !U || !X || !theta || !omega || !obj || !status || !iters || !active) return LIPMPC_E_ARG;
  if (h->warm && B > h->warm_cap) return LIPMPC_E_ARG;       // (refused before the scan is enqueued)
  const int rc = lipmpc_lidar_c_eta_batch(h->device, B, resolution, n_env, v_env, env_shared, lidar_range, eps, min_samples,
                                          h->p.n_obs_max, h->p.v_max, state, env_xy, env_nv, ray_table, noise, c_eta, n_inferred,
                                          overflow, nullptr, nullptr, nullptr, nullptr, schedule, hip_stream);
  if (rc != LIPMPC_OK) return rc;
  // the scan's overflow flags go to the solve: a robot whose clusters did not fit the obstacle slots gets
  // LIPMPC_STATUS_SENSOR_OVERFLOW and NaN outputs instead of a plan against the truncated list
  return lipmpc_plan_step_batch_c_eta(h, B, state, goal, first_foot, delta, c_eta, overflow, U, X, theta, omega, obj, status, iters,
                                      active, working, diag, bounds, hip_stream);
}

int lipmpc_sense_grid_plan_step_batch(lipmpc_handle* h, int64_t B, int32_t resolution, int32_t W, int32_t H, int32_t grid_shared,
                                      const double* origin, const double* cell, double lidar_range, double eps,
                                      int32_t min_samples, const double* state, const double* goal, const int8_t* first_foot,
                                      const double* delta, const uint8_t* occ, const double* ray_table, const double* noise,
                                      double* c_eta, int32_t* n_inferred, int32_t* overflow,
                                      double* U, double* X, double* theta, double* omega, double* obj, int32_t* status,
                                      int32_t* iters, uint64_t* active, uint64_t* working, double* diag, const double* bounds,
                                      void* hip_stream) {
  if (!h || B < 0) return LIPMPC_E_ARG;
  if (h->p.n_obs_max < 1) return LIPMPC_E_UNSUPPORTED;        // a handle without obstacle slots has nothing to sense into
  if (!c_eta || !goal || !first_foot || !U || !X || !theta || !omega || !obj || !status || !iters || !active) return LIPMPC_E_ARG;
  if (h->warm && B > h->warm_cap) return LIPMPC_E_ARG;       // (refused before the scan is enqueued)
  const int rc = lipmpc_lidar_grid_c_eta_batch(h->device, B, resolution, W, H, grid_shared, origin, cell, lidar_range, eps, min_samples,
                                               h->p.n_obs_max, h->p.v_max, state, occ, ray_table, noise, c_eta, n_inferred, overflow,
                                               nullptr, nullptr, nullptr, nullptr, hip_stream);
  if (rc != LIPMPC_OK) return rc;
  // overflow: the clusters did not fit the obstacle slots, or the robot stands in a solid cell -- no plan either way
  return lipmpc_plan_step_batch_c_eta(h, B, state, goal, first_foot, delta, c_eta, overflow, U, X, theta, omega, obj, status, iters,
                                      active, working, diag, bounds, hip_stream);
}

int lipmpc_advance_batch(lipmpc_handle* h, int64_t B, double* state, int8_t* first_foot, const double* U,
                         const double* theta, const int32_t* status, void* hip_stream) {
  if (!h || B < 0) return LIPMPC_E_ARG;
  if (B == 0) return LIPMPC_OK;
  if (!state || !first_foot || !U || !theta || !status) return LIPMPC_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(advance_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                     (long)B, h->k.ch, h->k.sh_over_beta, h->k.beta_sh, state, first_foot, U, theta, status, h->k.N);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}

int lipmpc_fleet_update_batch(lipmpc_handle* h, int64_t B, int32_t k_max, double stop_obj, double* state,
                              int8_t* first_foot, int8_t* walking, double* last_obj, int32_t* n_steps,
                              int32_t* last_status, int32_t* n_overflow, int32_t* sample, double* X_pred, double* U_pred,
                              const double* U, const double* theta, const double* omega, const double* obj,
                              const int32_t* status, const int32_t* overflow, void* hip_stream) {
  if (!h || B < 0 || k_max < 1) return LIPMPC_E_ARG;
  if (B == 0) return LIPMPC_OK;
  if (!state || !first_foot || !walking || !last_obj || !n_steps || !last_status || !sample || !X_pred || !U_pred || !U ||
      !theta || !omega || !obj || !status || (overflow && !n_overflow))
    return LIPMPC_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(fleet_update_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, (long)B,
                     k_max, stop_obj, h->k.ch, h->k.sh_over_beta, h->k.beta_sh, h->k.N, state, first_foot, walking, last_obj,
                     n_steps, last_status, n_overflow, sample, X_pred, U_pred, U, theta, omega, obj, status, overflow);
  hipLaunchKernelGGL(fleet_next_sample_kernel, dim3(1), dim3(1), 0, (hipStream_t)hip_stream, sample);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}

int lipmpc_fleet_recover_update_batch(lipmpc_handle* h, int64_t B, int32_t k_max, double stop_obj, double* state,
                                      int8_t* first_foot, int8_t* walking, double* last_obj, int32_t* n_steps,
                                      int32_t* last_status, int32_t* n_overflow, int32_t* sample, double* X_pred,
                                      double* U_pred, const double* U, const double* theta, const double* omega,
                                      const double* obj, const int32_t* status, const int32_t* overflow, const double* goal,
                                      const double* c_eta, const double* delta, int32_t max_recover, int32_t* recover_run,
                                      int32_t* n_recover, double* recover_margin, void* hip_stream) {
  if (!h || B < 0 || k_max < 1 || max_recover < 0) return LIPMPC_E_ARG;
  if (B == 0) return LIPMPC_OK;
  if (!state || !first_foot || !walking || !last_obj || !n_steps || !last_status || !sample || !X_pred || !U_pred || !U ||
      !theta || !omega || !obj || !status || (overflow && !n_overflow) || !goal || !recover_run || !n_recover || !recover_margin)
    return LIPMPC_E_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(fleet_recover_update_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                     (long)B, k_max, stop_obj, h->k.ch, h->k.sh_over_beta, h->k.beta_sh, sqrt(h->p.g / h->p.h_com), h->k.omega_max,
                     h->k.tau, h->k.N, h->k.n_obs, state, first_foot, walking, last_obj, n_steps, last_status, n_overflow, sample,
                     X_pred, U_pred, U, theta, omega, obj, status, overflow, goal, c_eta, delta, max_recover, recover_run,
                     n_recover, recover_margin);
  hipLaunchKernelGGL(fleet_next_sample_kernel, dim3(1), dim3(1), 0, (hipStream_t)hip_stream, sample);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}

const char* lipmpc_strerror(int code) {
  switch (code) {
    case LIPMPC_OK: return "ok";
    case LIPMPC_E_ARG: return "invalid argument (null pointer or negative size)";
    case LIPMPC_E_UNSUPPORTED: return "unsupported parameters (N 1..16, n_obs_max 0..50, v_max 3..32)";
    case LIPMPC_E_HIP: return "HIP runtime error (no device, bad device index or launch failure)";
    case LIPMPC_E_NOMEM: return "out of host memory";
    default: return "unknown error";
  }
}

#ifdef LIPMPC_PHASE_TIMING      // an instrumented build writes phase counters where the product writes diag: not loadable as the product
int lipmpc_version(void) { return LIPMPC_ABI_VERSION + LIPMPC_VARIANT_BASE; }
#else
int lipmpc_version(void) { return LIPMPC_ABI_VERSION; }
#endif

}  // extern "C"
