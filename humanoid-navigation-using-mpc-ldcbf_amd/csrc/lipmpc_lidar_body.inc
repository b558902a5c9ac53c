// lipmpc_lidar_body.inc -- the body of the two sense kernels of lipmpc_lidar.hip, included once per kernel: LIDAR_GRID 0 = the map is the
// vertex rings env_xy / env_nv (lidar_sense_kernel), LIDAR_GRID 1 = the occupancy grid gm (lidar_grid_scan_kernel).  The two differ in
// section 1 only.  In: the kernel's arguments.
  // LDS: 10.1 KB per wave = 16 waves per CU (the 160 KB of a CU are what caps this kernel's occupancy, not its registers:
  // the scan is latency-bound, and went from 8 to 16 resident waves per CU with this layout).  One array of points, everything
  // a lane owns of its own points (coordinates, cluster root) in registers, and the three small tables of the three phases on
  // one another.
  __shared__ __attribute__((aligned(16))) double pint_[2 * RMAX];   // ray phase: staged edges; then the readings (x, y), compacted in ray order
#if !LIDAR_GRID
  double* const edge_ = pint_;                   // [ECAP][4]: g = b - a and f = robot - a of every staged edge ...
  double* const nua_ = pint_ + 4 * ECAP;         // [ECAP]:    ... and g x f, the ray-independent numerator of compute_intersection
#endif
  __shared__ __attribute__((aligned(16))) int comp_[RMAX];          // -1 = no reading; core: component root; else NO_ROOT; hull stage: cluster offsets
  __shared__ unsigned short cand_[RMAX];         // obstacles that can be hit from here, list order; then the ray of every reading; then member lists
#if !LIDAR_GRID
  __shared__ unsigned short eoff_[66];           // first staged edge of the chunk's candidates
#endif
  __shared__ __attribute__((aligned(16))) double small_[NCC * 3];   // one phase's small table at a time:
#if !LIDAR_GRID
  double (*const candc_)[3] = reinterpret_cast<double (*)[3]>(small_);            // rays: bounding circle (centre, radius) of the first NCC candidates
#endif
  double (*const bb16_)[4] = reinterpret_cast<double (*)[4]>(small_);             // neighbour rows: bounding box (x0, x1, y0, y1) of each run of 16 points
  int* const roots_ = reinterpret_cast<int*>(small_);                             // components on: cluster roots, ascending [64]
  unsigned short* const stagei_ = reinterpret_cast<unsigned short*>(small_ + 32); // hulls: [4][VSTAGE] vertices of the rings being marched, as point indices
  static_assert(NRUN * 4 * 8 <= NCC * 3 * 8 && 32 * 8 + 4 * VSTAGE * 2 <= NCC * 3 * 8, "the small tables share one area");

  const int lane = threadIdx.x;
  if ((long)blockIdx.x >= B) return;
  // Which robot this wave scans: the block index, or -- with an order buffer (include/lipmpc.h) -- the robot the order
  // kernel of THIS call put at this position: ranked by an estimate of its reading count (lidar_weight_kernel) and dealt out so
  // that the robots sharing a SIMD are a heavy one with light ones (lidar_order_kernel).  A scan's length varies 3x with the
  // number of readings, and with the whole batch resident the launch lasts as long as its most loaded SIMD: 94 us as the robots
  // come, 74 us ranked by the true counts, 85 us ranked by the estimate, ranking included (tools/lidar_order.py).  Any order
  // gives the same results.
  long b = blockIdx.x;
#if !LIDAR_GRID                   // (a grid is scanned in index order)
  if (sched && sched[SCHED_VALID] == (int)B) {
    const long r = sched[SCHED_ORDER + blockIdx.x];
    if (r >= 0 && r < B) b = r;
    // the robots of a SIMD come one from each round of `period` launch positions, the heaviest from the first: that one goes
    // first when the SIMD picks an instruction (the launch lasts as long as its longest scan)
    const int period = sched[SCHED_PERIOD];
    if (period > 0) {
      const long round = blockIdx.x / period;
      if (round == 0) __builtin_amdgcn_s_setprio(3);
      else if (round == 1) __builtin_amdgcn_s_setprio(1);
    }
  }
#endif
#ifdef LIPMPC_LIDAR_PHASES
  const unsigned long long t_enter = wall_clock64();
  if (dbg_stop == 8) {            // placement probe (tools/lidar_placement.py): where the dispatcher put launch position blockIdx.x
    if (lane == 0) {
      n_inferred[blockIdx.x] = (int)__builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_REG_HW_ID
      overflow[blockIdx.x] = (int)__builtin_amdgcn_s_getreg((31 << 11) | 20);       // HW_REG_XCC_ID
    }
    for (int i = 0; i < 16; ++i) __builtin_amdgcn_s_sleep(127);                     // stay resident while the grid is placed
    return;
  }
#endif
  const double x0 = state[b * 5 + 0], y0 = state[b * 5 + 2];
#if !LIDAR_GRID
  const double* exy = env_xy + b * env_stride * (long)n_env * v_env * 2;
  const int32_t* env = env_nv + b * env_stride * (long)n_env;
  int n_cand = 0;
#endif
  int in_ovf = 0;                 // inputs beyond what this kernel holds: more than RMAX obstacles in range, rings longer than v_env

  // 1. ray casting -> n_pts readings (hit + noise) compacted in ray order in pint_, the ray of reading k in cand_[k]
  int n_pts = 0;
#if LIDAR_GRID
#include "lipmpc_lidar_grid_rays.inc"
#else
#include "lipmpc_lidar_rays.inc"
#endif

  LIDAR_PHASE_END(1);
  // ---- 2. DBSCAN ------------------------------------------------------------------------------------
  // The launch lasts as long as its longest scan, and a scan with many readings (quadratically more pair tests, the longest hull)
  // shares its SIMD with three others: from here on it goes first when the SIMD picks an instruction.
  if (n_pts > 256) __builtin_amdgcn_s_setprio(3);
  else if (n_pts > 160) __builtin_amdgcn_s_setprio(2);
  else if (n_pts > 112) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
  const int NW = (n_pts + 63) >> 6;                      // words / passes actually in use (wave-uniform)
  const int npad = NW << 6;
  if (labels_out) for (int i = lane; i < R; i += 64) labels_out[b * R + i] = -2;      // -2 = no reading
  if (pieces_out) for (int i = lane; i < R; i += 64) pieces_out[b * R + i] = -2;
  const double eps2 = eps * eps;
  unsigned long long vmask[WORDS];                  // which points exist
#pragma unroll
  for (int w = 0; w < WORDS; ++w) {
    const int left = n_pts - w * 64;
    vmask[w] = left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
  }
  int touch[WORDS];                                  // smallest tree root point lane + 64 k touches (NO_ROOT: none)
#pragma unroll
  for (int w = 0; w < WORDS; ++w) touch[w] = NO_ROOT;
  // 2a. clustering by chains of consecutive readings, where that is provably DBSCAN's answer -> chains, comp_, touch
#include "lipmpc_lidar_chains.inc"
  if (chains) __syncthreads();
  if (!chains) {
  // 2. the general route: neighbour rows, core flags, connected components -> comp_, touch
#include "lipmpc_lidar_rows.inc"
  }      // (!chains)
  LIDAR_PHASE_END(4);
  // cluster root of every reading (of this lane's point of every word: nobody else asks for it): own component for cores,
  // smallest neighbouring core component for the rest
  int rootr[WORDS];
#pragma unroll
  for (int k = 0; k < WORDS; ++k) {
    const int ci = (k < NW) ? comp_[k * 64 + lane] : -1;
    rootr[k] = (ci < 0) ? NO_ROOT : ((ci != NO_ROOT) ? ci : touch[k]);
  }
  LIDAR_PHASE_END(5);
  // roots in ascending order = cluster labels 0, 1, ...
  int n_clusters = 0;
  for (int w = 0; w < NW; ++w) {
    const int i = w * 64 + lane;
    const bool is_root = comp_[i] == i;
    const unsigned long long ball = __ballot(is_root);
    if (is_root) {
      const int k = n_clusters + __popcll(ball & ((1ull << lane) - 1ull));
      if (k < 64) roots_[k] = i;
    }
    n_clusters += __popcll(ball);
  }
  __syncthreads();
  if (labels_out) {
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
      const int i = w * 64 + lane;
      if (i >= n_pts) continue;
      int lab = -1;                                           // -1 noise
      const int r = rootr[w];
      if (r != NO_ROOT) for (int k = 0; k < n_clusters && k < 64; ++k) if (roots_[k] == r) lab = k;
      labels_out[b * R + cand_[i]] = lab;
    }
  }

  LIDAR_PHASE_END(3);
  // 2b. (opt-in) clusters cut into pieces of at most split_rays rays, which take the clusters' place -> rootr, roots_, n_clusters
  if (split_rays > 0 || pieces_out) {                    // wave-uniform
    const int split = split_rays > 0 ? split_rays : R;   // (pieces asked for without splitting: every cluster is one piece)
#include "lipmpc_lidar_pieces.inc"
  }
  // 3 + 4. hull per cluster, constraint assembly -> obs_xy / obs_nv / c_eta, n_out, ovf
#include "lipmpc_lidar_hulls.inc"
  if (lane == 0) { n_inferred[b] = n_out; overflow[b] = ovf; }
#ifdef LIPMPC_LIDAR_PHASES
  if (dbg_stop == 10 && lane == 0) n_inferred[b] = chains ? 1 : 0;      // which route clustered this scan (tools/lidar_wave_times.py)
  if (dbg_stop == 9 && lane == 0) {      // wave timing (tools/lidar_wave_times.py): start and end on the 100 MHz wall clock, by robot
    n_inferred[b] = (int)(t_enter & 0x7fffffff);
    overflow[b] = (int)(wall_clock64() & 0x7fffffff);
  }
#endif
