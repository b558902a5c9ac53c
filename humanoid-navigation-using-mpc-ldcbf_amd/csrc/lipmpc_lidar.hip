// lipmpc_lidar.hip — unknown-environment front end (BASELINE config 5): per robot and MPC step, a 2-D LiDAR scan of the
// true map -> noisy readings -> DBSCAN clusters -> convex hull per cluster, i.e. the obstacle rings the step kernel
// consumes.  Restates
//   range_finder / compute_lidar_readings / retrieve_clusters / build_local_obstacles
//       HumanoidNavigation/RangeFinder/range_finder_wth_polygons_dbscan.py:26-63, 65-83, 100-126, 157-180
//   line_polygon_intersection (compute_intersection)      HumanoidNavigation/Utils/obstacles.py:95-139
//   the call site                                          HumanoidNavigation/MPC/HumanoidMPCVariants/HumanoidMPCUnknownEnvironment.py:30-68
// One wavefront (64 lanes) per robot; everything between the ray casting and the half-spaces stays in LDS / registers
// (10.1 KB of LDS and 128 registers per wave: 16 waves per CU, a whole batch of 4096 robots resident at once):
//   1. rays: lane l owns rays l, l+64, ...; the edges of the obstacles within range are staged once per robot in LDS
//      (edge vector, the robot's offset from the edge's first vertex and their cross product: the operands of
//      compute_intersection, no global / scalar load left in the ray loops) and every ray walks them in list order, keeping
//      the nearest hit strictly inside the range (contraction off: the hit points are bit-identical to the reference's)
//   2. DBSCAN(eps, min_samples) by its order-free characterisation (oracle/lidar_oracle.py), on the readings
//      compacted in ray order: neighbour bit rows (pruned by the bounding boxes of runs of 16 readings: far pairs of runs
//      skipped, pairs within eps corner to corner set without a test, the rest tested column by column with the verdict
//      shifted in through the carry), core flags, connected components of the core points (forest of "smallest core
//      neighbour" pointers + pointer jumping, then merging trees through ballot masks of tree membership — bit operations,
//      no sweeps over neighbours' labels), clusters numbered by their smallest core index, border points to the smallest
//      neighbouring cluster
//   2b. (opt-in: lipmpc_lidar_c_eta_split_batch, split_rays > 0) every cluster cut into pieces of at most split_rays consecutive
//      rays, in registers from the ballot masks of the cluster's members; the pieces take the clusters' place in 3 and 4 -- the
//      walls of a room are one cluster whose hull holds the robot, the hulls of sectors of at most half a turn cannot
//   3. hull per cluster: Jarvis march from the lexicographically smallest point, farthest point on collinear ties
//      (= the CCW ring of extreme points Qhull / monotone chain return, same rotation as np.unique + monotone chain);
//      four clusters march at once, one per 16-lane DPP row, every lane's candidates held in registers; a step's winner is
//      guessed by a single-precision turning key and proved with the exact predicate (exact reduction only when that fails)
//   4. constraint assembly (HumanoidMPCUnknownEnvironment.py:54-62 -> ObstaclesUtils.py:60-109): closest point c and
//      unit normal eta of every hull at the robot's CoM, one hull edge per lane, from the hull still staged in LDS --
//      the (c, eta) rows are what the step solver consumes (lipmpc_plan_step_batch_c_eta); the rings themselves go to
//      HBM only when the caller asks for them
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "lipmpc_kernel.hpp"      // DPP row exchanges (lipmpc_dev::row_xor)

namespace {

constexpr int RMAX = 384;            // rays per scan (reference: 360)
constexpr int WORDS = RMAX / 64;     // neighbour bit row
constexpr int NO_ROOT = 0x7fffffff;
constexpr int SOLO_MIN = 64;        // a cluster of at least this many points gets the whole wave in the hull stage
constexpr int NCC = 64;             // candidates whose bounding circle is kept for the per-pass sector test
constexpr int VFAST = 8;            // rings of at most this many vertices (v_env) are fetched in one round of loads
constexpr int VSTAGE = 64;          // hull vertices staged per cluster (v_max <= VSTAGE)
// order buffer (int32, scratch of ONE call): [B the order is valid for, -, order[B] (robot at launch position i), weight[B]]
constexpr int SCHED_VALID = 0, SCHED_PERIOD = 1, SCHED_ORDER = 2;
constexpr int NRUN = RMAX / 16;      // runs of 16 consecutive readings
constexpr int ECAP = 152;           // edges staged per chunk of the ray phase (5 doubles each, where the points go afterwards)
static_assert(ECAP * 5 <= 2 * RMAX && ECAP % 2 == 0, "the staged edges live in the point array");
static_assert(ECAP <= 65535 && RMAX <= 65535, "16-bit edge offsets and point indices");
constexpr int GRID_WINDOW_CELLS = 2 * RMAX * 8 * 8;      // grid maps: the window of cells around the robot, one bit each, where the edges are staged
constexpr int GRID_RAYS = 3;         // grid maps: rays a lane marches at once
constexpr int GRID_STAGE = 8;        // grid maps: window cells a lane fetches per trip of the staging loop

// The occupancy grid of a grid scan (lipmpc_lidar_grid_c_eta_batch)
struct GridArg {
  int W, H;                          // cells; cell (i, j) at occ[i * H + j]
  long stride;                       // W * H for a map per robot, 0 for a shared one
  double ox, oy, dx, dy;             // origin and cell size
  int nx, ny;                        // half-width of the staged window in cells: floor(range / cell) + 2
  const unsigned char* occ;
};

struct Cand { double x, y; int idx; };
#ifdef LIPMPC_LIDAR_PHASES
#define LIDAR_PHASE_END(n) if (dbg_stop == (n)) return
#else
#define LIDAR_PHASE_END(n)
#endif

// Is candidate b a better "next hull vertex" than a when standing on p?  (b strictly to the right of p->a, or collinear and
// farther; a.idx < 0 = no candidate yet.)  Candidates are given as OFFSETS from p (a.x = x_a - p_x ...), formed once per step
// instead of once per comparison.  Straight-line on purpose (the verdict assembled from masks): the march is a chain of
// dependent steps, and the nest of divergent branches the short-circuit form compiles to cost more than the arithmetic it
// skipped.  Exactly collinear pairs are rare enough for the tie-break to sit behind a wave-uniform branch.
__device__ __forceinline__ bool better_from(const Cand& a, const Cand& b) {
#pragma clang fp contract(off)
  const double cr = a.x * b.y - a.y * b.x;
  const bool both = (a.idx >= 0) & (b.idx >= 0);
  bool tie = false;
  if (__any(both & (cr == 0.0))) {
    const double da = a.x * a.x + a.y * a.y;
    const double db = b.x * b.x + b.y * b.y;
    tie = (db > da) | ((db == da) & (b.idx < a.idx));
  }
  const bool geo = (cr < 0.0) | ((cr == 0.0) & tie);
  return (b.idx >= 0) & ((a.idx < 0) | geo);
}
// the value lane l (wave-uniform) holds
__device__ __forceinline__ double lane_value(double v, int l) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, l), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), l);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// the value held 16 / 32 lanes away, by v_permlane16_swap / v_permlane32_swap (VALU, no trip through the LDS crossbar)
template <class T> __device__ __forceinline__ T wave_xor16(T v) { return lipmpc_dev::rowswap(v); }
__device__ __forceinline__ unsigned wave_xor32_u(unsigned u) {
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);      // {lanes 0-31 everywhere, lanes 32-63 everywhere}
  const unsigned lo = r[0], hi = r[1];
  return (lipmpc_dev::fresh(threadIdx.x) & 32) ? lo : hi;
}
template <class T> __device__ __forceinline__ T wave_xor32(T v) {
  if constexpr (sizeof(T) == 8) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = wave_xor32_u((unsigned)u), hi = wave_xor32_u((unsigned)(u >> 32));
    return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
  } else {
    return __builtin_bit_cast(T, wave_xor32_u(__builtin_bit_cast(unsigned, v)));
  }
}

// closest point of one hull edge (a -> b) to p and the crossing test of the edge (prev -> a) with the +X ray from p:
// the arithmetic of lipmpc_dev::closest_point_normal (ObstaclesUtils.py:50-109), one edge per call
struct EdgeCp { double d, qx, qy; bool degen, hit; };
__device__ __forceinline__ EdgeCp edge_closest(double pvx, double pvy, double ax, double ay, double bx, double by, double px,
                                               double py) {
#pragma clang fp contract(off)
  EdgeCp r;
  const double dx = bx - ax, dy = by - ay;
  const double nrm = sqrt(dx * dx + dy * dy);
  const double den = nrm * nrm;                      // sqrt-then-square, ObstaclesUtils.py:81
  r.degen = den == 0.0;
  double t = ((px - ax) * dx + (py - ay) * dy) / den;
  t = fmax(0.0, fmin(1.0, t));
  const double qx = ax + t * dx, qy = ay + t * dy;
  const double ux = qx - px, uy = qy - py;
  r.d = r.degen ? INFINITY : sqrt(ux * ux + uy * uy);
  r.qx = r.degen ? NAN : qx; r.qy = r.degen ? NAN : qy;
  const bool f0 = pvy >= py, f1 = ay >= py;
  r.hit = (f0 != f1) && (((ay - py) * (pvx - ax) >= (ax - px) * (pvy - ay)) == f1);
  return r;
}

// The two sense kernels share one body (lipmpc_lidar_body.inc), which differs in section 1 only: the rays are cast against vertex rings
// (lidar_sense_kernel) or marched through an occupancy grid (lidar_grid_scan_kernel).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void lidar_sense_kernel(
    long B, int R, int n_env, int v_env, long env_stride, double lidar_range, double eps, int min_samples,
    int n_obs_max, int v_max, const double* __restrict__ state, const double* __restrict__ env_xy,
    const int32_t* __restrict__ env_nv, const double* __restrict__ ray_table, const double* __restrict__ noise,
    double* __restrict__ obs_xy, int32_t* __restrict__ obs_nv, double* __restrict__ c_eta, int32_t* __restrict__ n_inferred,
    int32_t* __restrict__ overflow, double* __restrict__ hits_out, int32_t* __restrict__ labels_out,
    int32_t* __restrict__ sched, int dbg_stop, int split_rays, int32_t* __restrict__ pieces_out) {
#define LIDAR_GRID 0
#include "lipmpc_lidar_body.inc"
#undef LIDAR_GRID
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void lidar_grid_scan_kernel(
    long B, int R, double lidar_range, double eps, int min_samples, int n_obs_max, int v_max, const double* __restrict__ state,
    const double* __restrict__ ray_table, const double* __restrict__ noise, double* __restrict__ obs_xy,
    int32_t* __restrict__ obs_nv, double* __restrict__ c_eta, int32_t* __restrict__ n_inferred, int32_t* __restrict__ overflow,
    double* __restrict__ hits_out, int32_t* __restrict__ labels_out, int dbg_stop, GridArg gm, int split_rays,
    int32_t* __restrict__ pieces_out) {
#define LIDAR_GRID 1
#include "lipmpc_lidar_body.inc"
#undef LIDAR_GRID
}

// Weight of every robot for the launch order of its scan: an ESTIMATE of its reading count -- every ray, if the robot stands
// INSIDE an obstacle (the heaviest scans there are: all 360 readings in one dense cluster); otherwise, per obstacle in range, the
// rays its bounding circle of radius r at distance d subtends, R / (2 pi) * 2 asin(r / d) (the asin by its argument: the estimate
// only ranks), scaled by the share of the circle inside the range -- summed and capped at R.  Correlation 0.91 with the true
// counts on a CROWDED-style map, 93 % of the heaviest tenth in its top fifth (tools/lidar_order.py): it costs one obstacle per
// lane instead of the scan itself.  One wave per robot.
__global__ __launch_bounds__(64) void lidar_weight_kernel(long B, int R, int n_env, int v_env, long env_stride, double lidar_range,
                                                          const double* __restrict__ state, const double* __restrict__ env_xy,
                                                          const int32_t* __restrict__ env_nv, int32_t* __restrict__ sched) {
  const long b = blockIdx.x;
  if (b >= B) return;
  const int lane = threadIdx.x;
  const double x0 = state[b * 5 + 0], y0 = state[b * 5 + 2];
  const double* exy = env_xy + b * env_stride * (long)n_env * v_env * 2;
  const int32_t* env = env_nv + b * env_stride * (long)n_env;
  double w = 0.0;
  for (int j = lane; j < n_env; j += 64) {
    const int nv = min(env[j], v_env);
    if (nv <= 0) continue;
    const double* ring = exy + (long)j * v_env * 2;
    double mx = 0.0, my = 0.0, rad2 = 0.0;
    bool within = false;             // the robot stands INSIDE this obstacle: every ray returns a reading (the heaviest scans there are)
    auto crosses = [&](double ax, double ay, double bx, double by) {      // edge a -> b against the +x ray from the robot
      return ((ay > y0) != (by > y0)) && (x0 - ax) * fabs(by - ay) < (bx - ax) * (y0 - ay) * ((by > ay) ? 1.0 : -1.0);
    };
    if (v_env <= VFAST) {            // the whole ring in one round of loads
      double vx[VFAST], vy[VFAST];
#pragma unroll
      for (int e = 0; e < VFAST; ++e) { const int ee = e < nv ? e : 0; vx[e] = ring[2 * ee]; vy[e] = ring[2 * ee + 1]; }
#pragma unroll
      for (int e = 0; e < VFAST; ++e) if (e < nv) { mx += vx[e]; my += vy[e]; }
      mx /= nv; my /= nv;
#pragma unroll
      for (int e = 0; e < VFAST; ++e)
        if (e < nv) {
          const double dx = vx[e] - mx, dy = vy[e] - my;
          rad2 = fmax(rad2, dx * dx + dy * dy);
          const bool last = e + 1 == nv;
          within ^= crosses(vx[e], vy[e], last ? vx[0] : vx[(e + 1) % VFAST], last ? vy[0] : vy[(e + 1) % VFAST]);
        }
    } else {
      for (int e = 0; e < nv; ++e) { mx += ring[2 * e]; my += ring[2 * e + 1]; }
      mx /= nv; my /= nv;
      for (int e = 0; e < nv; ++e) {
        const double dx = ring[2 * e] - mx, dy = ring[2 * e + 1] - my;
        rad2 = fmax(rad2, dx * dx + dy * dy);
        const int f = e + 1 == nv ? 0 : e + 1;
        within ^= crosses(ring[2 * e], ring[2 * e + 1], ring[2 * f], ring[2 * f + 1]);
      }
    }
    const double rad = sqrt(rad2), d = sqrt((mx - x0) * (mx - x0) + (my - y0) * (my - y0));
    if (d > lidar_range + rad) continue;
    const double inside = (d + rad <= lidar_range) ? 1.0 : fmin(1.0, fmax(0.0, (lidar_range + rad - d) / (2.0 * rad + 1e-300)));
    w += within ? (double)R : (double)R * (1.0 / M_PI) * fmin(1.0, rad / fmax(d, 1e-300)) * inside;
  }
  for (int m = 1; m < 64; m <<= 1) w += __shfl_xor(w, m, 64);
  if (lane == 0) sched[SCHED_ORDER + B + b] = (int32_t)fmin(w, (double)R);
}

// The launch order of the scans from the weights: robots by descending weight (counting sort, one workgroup; which of two
// equally heavy robots comes first is immaterial).
__global__ __launch_bounds__(1024) void lidar_order_kernel(long B, int period, int32_t* __restrict__ sched) {
  constexpr int NBIN = 512;                                // >= RMAX + 1 weights; one thread per bin in the scan
  static_assert(RMAX + 1 <= NBIN, "one bin per weight");
  __shared__ int cursor_[NBIN];
  __shared__ int scan_[NBIN];
  const int32_t* w = sched + SCHED_ORDER + B;
  int32_t* order = sched + SCHED_ORDER;
  for (int k = threadIdx.x; k < NBIN; k += blockDim.x) cursor_[k] = 0;
  __syncthreads();
  for (long i = threadIdx.x; i < B; i += blockDim.x) atomicAdd(&cursor_[RMAX - min(max(w[i], 0), RMAX)], 1);
  __syncthreads();
  // exclusive prefix sum of the bin counts: each of the first NBIN / 64 waves scans its 64 bins in registers, the waves' totals
  // go through LDS once (two barriers; a serial loop of one thread, then a Hillis-Steele scan with a barrier pair per step,
  // were most of this kernel's time)
  const int t = threadIdx.x;
  {
    const int mine = t < NBIN ? cursor_[t] : 0;
    int acc = mine;                                   // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(acc, d, 64); if ((t & 63) >= d) acc += o; }
    if (t < NBIN && (t & 63) == 63) scan_[t >> 6] = acc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int k = 0; k < NBIN / 64; ++k) if (k < (t >> 6)) base += scan_[k];
    __syncthreads();
    if (t < NBIN) cursor_[t] = base + acc - mine;
  }
  __syncthreads();
  // Rank -> launch position.  While every wave of the grid is resident at once, launch positions `period` apart share a SIMD
  // (period = 4 x compute units: the dispatcher deals single-wave blocks round-robin, tools/lidar_placement.py), so the ranks go
  // out boustrophedon -- forwards on even rounds of `period` positions, backwards on odd ones: a SIMD's robots are one from each
  // quantile, the heaviest with the lightest.  (Beyond what is resident the dispatcher takes blocks as slots free up, and plain
  // heaviest-first is the right order there: the last, partial round stays as ranked.)
  for (long i = threadIdx.x; i < B; i += blockDim.x) {
    const long r = atomicAdd(&cursor_[RMAX - min(max(w[i], 0), RMAX)], 1);
    const long q = r / period, s2 = r % period;
    const long pos = ((q + 1) * period <= B && (q & 1)) ? q * period + (period - 1 - s2) : r;
    order[pos] = (int32_t)i;
  }
  if (threadIdx.x == 0) { sched[SCHED_VALID] = (int32_t)B; sched[SCHED_PERIOD] = period; }
}

}  // namespace

// SIMDs of the device (4 per compute unit), asked once per device
static int simd_count(int device) {
  static int cached[64];
  if (device < 0 || device >= 64) return 1024;
  if (cached[device] == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    cached[device] = 4 * cus;
  }
  return cached[device];
}

static int lidar_dbg_stop() {
#ifdef LIPMPC_LIDAR_PHASES
  // profiling build only (make CXXFLAGS+=-DLIPMPC_LIDAR_PHASES, tools/lidar_phases.py): LIPMPC_LIDAR_STOP=1..7 ends the
  // kernel after that phase (the grid scan: 6 = window staged, 1 = rays marched); outputs are then undefined.  The shipped
  // library has no such knob.
  static const int dbg_stop = getenv("LIPMPC_LIDAR_STOP") ? atoi(getenv("LIPMPC_LIDAR_STOP")) : 0;
  return dbg_stop;
#else
  return 0;
#endif
}

static int lidar_launch(int device, int64_t B, int32_t resolution, int32_t n_env, int32_t v_env, int32_t env_shared,
                        double lidar_range, double eps, int32_t min_samples, int32_t n_obs_max, int32_t v_max,
                        const double* state, const double* env_xy, const int32_t* env_nv, const double* ray_table,
                        const double* noise, double* obs_xy, int32_t* obs_nv, double* c_eta, int32_t* n_inferred,
                        int32_t* overflow, double* hits, int32_t* labels, int32_t* schedule, int32_t split_rays, int32_t* pieces,
                        void* hip_stream) {
  if (B < 0 || resolution < 1 || resolution > RMAX || n_env < 0 || v_env < 1 || n_obs_max < 1 || v_max < 3 || v_max > VSTAGE ||
      split_rays < 0 || split_rays > resolution / 2)
    return LIPMPC_E_ARG;
  if (n_env > 65535) return LIPMPC_E_UNSUPPORTED;      // obstacle indices are kept as 16 bits in LDS
  if (B == 0) return LIPMPC_OK;
  if (!state || !ray_table || !n_inferred || !overflow || (n_env > 0 && (!env_xy || !env_nv)) || (!obs_xy != !obs_nv) ||
      (!obs_xy && !c_eta))
    return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  const int dbg_stop = lidar_dbg_stop();
  if (schedule && n_env > 0) {
    // rank the robots first: estimate of the reading counts -> launch positions, a heavy robot with light ones on every SIMD
    hipLaunchKernelGGL(lidar_weight_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)hip_stream, (long)B, resolution, n_env, v_env,
                       (long)(env_shared ? 0 : 1), lidar_range, state, env_xy, env_nv, schedule);
    hipLaunchKernelGGL(lidar_order_kernel, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, (long)B, simd_count(device), schedule);
  } else {
    schedule = nullptr;
  }
  hipLaunchKernelGGL(lidar_sense_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)hip_stream, (long)B, resolution, n_env,
                     v_env, (long)(env_shared ? 0 : 1), lidar_range, eps, min_samples, n_obs_max, v_max, state, env_xy, env_nv,
                     ray_table, noise, obs_xy, obs_nv, c_eta, n_inferred, overflow, hits, labels, schedule, dbg_stop, split_rays, pieces);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}

extern "C" int lipmpc_lidar_sense_batch(int device, int64_t B, int32_t resolution, int32_t n_env, int32_t v_env,
                                        int32_t env_shared, double lidar_range, double eps, int32_t min_samples,
                                        int32_t n_obs_max, int32_t v_max, const double* state, const double* env_xy,
                                        const int32_t* env_nv, const double* ray_table, const double* noise,
                                        double* obs_xy, int32_t* obs_nv, int32_t* n_inferred, int32_t* overflow,
                                        double* hits, int32_t* labels, void* hip_stream) {
  if (!obs_xy || !obs_nv) return LIPMPC_E_ARG;
  return lidar_launch(device, B, resolution, n_env, v_env, env_shared, lidar_range, eps, min_samples, n_obs_max, v_max, state,
                      env_xy, env_nv, ray_table, noise, obs_xy, obs_nv, nullptr, n_inferred, overflow, hits, labels, nullptr, 0, nullptr, hip_stream);
}

extern "C" int lipmpc_lidar_c_eta_split_batch(int device, int64_t B, int32_t resolution, int32_t n_env, int32_t v_env,
                                              int32_t env_shared, double lidar_range, double eps, int32_t min_samples,
                                              int32_t n_obs_max, int32_t v_max, const double* state, const double* env_xy,
                                              const int32_t* env_nv, const double* ray_table, const double* noise,
                                              double* c_eta, int32_t* n_inferred, int32_t* overflow, double* obs_xy,
                                              int32_t* obs_nv, double* hits, int32_t* labels, int32_t* schedule,
                                              int32_t split_rays, int32_t* pieces, void* hip_stream) {
  if (!c_eta) return LIPMPC_E_ARG;
  if (schedule && B > 0x3fffffff) return LIPMPC_E_UNSUPPORTED;
  return lidar_launch(device, B, resolution, n_env, v_env, env_shared, lidar_range, eps, min_samples, n_obs_max, v_max, state,
                      env_xy, env_nv, ray_table, noise, obs_xy, obs_nv, c_eta, n_inferred, overflow, hits, labels, schedule,
                      split_rays, pieces, hip_stream);
}

extern "C" int lipmpc_lidar_c_eta_batch(int device, int64_t B, int32_t resolution, int32_t n_env, int32_t v_env,
                                        int32_t env_shared, double lidar_range, double eps, int32_t min_samples,
                                        int32_t n_obs_max, int32_t v_max, const double* state, const double* env_xy,
                                        const int32_t* env_nv, const double* ray_table, const double* noise,
                                        double* c_eta, int32_t* n_inferred, int32_t* overflow, double* obs_xy,
                                        int32_t* obs_nv, double* hits, int32_t* labels, int32_t* schedule,
                                        void* hip_stream) {
  return lipmpc_lidar_c_eta_split_batch(device, B, resolution, n_env, v_env, env_shared, lidar_range, eps, min_samples, n_obs_max,
                                        v_max, state, env_xy, env_nv, ray_table, noise, c_eta, n_inferred, overflow, obs_xy, obs_nv,
                                        hits, labels, schedule, 0, nullptr, hip_stream);
}

extern "C" int lipmpc_lidar_grid_c_eta_split_batch(int device, int64_t B, int32_t resolution, int32_t W, int32_t H,
                                                   int32_t grid_shared, const double* origin, const double* cell, double lidar_range,
                                                   double eps, int32_t min_samples, int32_t n_obs_max, int32_t v_max,
                                                   const double* state, const uint8_t* occ, const double* ray_table,
                                                   const double* noise, double* c_eta, int32_t* n_inferred, int32_t* overflow,
                                                   double* obs_xy, int32_t* obs_nv, double* hits, int32_t* labels, int32_t split_rays,
                                                   int32_t* pieces, void* hip_stream) {
  if (B < 0 || resolution < 1 || resolution > RMAX || W < 1 || H < 1 || n_obs_max < 1 || v_max < 3 || v_max > VSTAGE || !origin ||
      !cell || !c_eta || split_rays < 0 || split_rays > resolution / 2)
    return LIPMPC_E_ARG;
  const double ox = origin[0], oy = origin[1], dx = cell[0], dy = cell[1];
  if (!(dx > 0.0) || !(dy > 0.0) || !(dx < INFINITY) || !(dy < INFINITY) || !(fabs(ox) < INFINITY) || !(fabs(oy) < INFINITY) ||
      !(lidar_range >= 0.0) || !(lidar_range < INFINITY))
    return LIPMPC_E_ARG;
  // the window of cells within range of a robot is staged as a bitmap in LDS: (range, cell) pairs whose window does not fit are refused
  const double nx = floor(lidar_range / dx) + 2.0, ny = floor(lidar_range / dy) + 2.0;
  if ((2.0 * nx + 1.0) * (2.0 * ny + 1.0) > (double)GRID_WINDOW_CELLS) return LIPMPC_E_UNSUPPORTED;
  if (B == 0) return LIPMPC_OK;
  if (!state || !occ || !ray_table || !n_inferred || !overflow || (!obs_xy != !obs_nv)) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  const GridArg gm{W, H, grid_shared ? 0L : (long)W * H, ox, oy, dx, dy, (int)nx, (int)ny, occ};
  hipLaunchKernelGGL(lidar_grid_scan_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)hip_stream, (long)B, resolution, lidar_range, eps,
                     min_samples, n_obs_max, v_max, state, ray_table, noise, obs_xy, obs_nv, c_eta, n_inferred, overflow, hits, labels,
                     lidar_dbg_stop(), gm, split_rays, pieces);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}

extern "C" int lipmpc_lidar_grid_c_eta_batch(int device, int64_t B, int32_t resolution, int32_t W, int32_t H, int32_t grid_shared,
                                             const double* origin, const double* cell, double lidar_range, double eps,
                                             int32_t min_samples, int32_t n_obs_max, int32_t v_max, const double* state,
                                             const uint8_t* occ, const double* ray_table, const double* noise, double* c_eta,
                                             int32_t* n_inferred, int32_t* overflow, double* obs_xy, int32_t* obs_nv, double* hits,
                                             int32_t* labels, void* hip_stream) {
  return lipmpc_lidar_grid_c_eta_split_batch(device, B, resolution, W, H, grid_shared, origin, cell, lidar_range, eps, min_samples,
                                             n_obs_max, v_max, state, occ, ray_table, noise, c_eta, n_inferred, overflow, obs_xy, obs_nv,
                                             hits, labels, 0, nullptr, hip_stream);
}

extern "C" int64_t lipmpc_lidar_schedule_words(int64_t B) { return B < 0 ? LIPMPC_E_ARG : SCHED_ORDER + 2L * B; }
