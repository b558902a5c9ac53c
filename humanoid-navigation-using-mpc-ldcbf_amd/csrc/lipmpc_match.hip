// lipmpc_match.hip -- correlative scan matching against the occupancy-evidence grid (lipmpc_scan_match_batch, include/lipmpc.h).
//
// Where is the robot on the map it builds?  One call scores, per robot, a window of candidate poses (whole-cell shifts a, b and a
// table of yaws k) by the evidence under the scan's hit cells and returns the best one.  One launch on the caller's stream:
//   scan_match_kernel  one workgroup (256 lanes) per robot.
//     stage      the evidence of the map update's window grown by (n_x, n_y), clamped to +-clamp, one signed byte per cell in
//                LDS, 0 outside the map; the end points of the readings (the map update's, NaN = none) in LDS.
//     per yaw    cells: the used readings' cells as offsets into that byte window (the ONLY floating point of the call: one
//                evaluation per reading and yaw), compacted through an LDS counter (a sum does not mind the order);
//                correlate: lanes own candidates, consecutive lanes consecutive b = consecutive bytes; every lane walks the
//                list of offsets and adds the byte at offset + its own shift; fold the packed key of each candidate.
//     select     the smallest key of the workgroup through LDS; lane 0 applies the acceptance test and writes the outputs.
// Every compared value is an integer and the key is a total order: the result does not depend on thread order.  The contract
// is restated in numpy by tests/scan_match_oracle.py.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lipmpc.h"

#pragma clang fp contract(off)

namespace {

constexpr int RMAX = 384;                           // rays per scan, as the scans
constexpr int MATCH_WINDOW_CELLS = 49152;           // the grown window, one byte per cell in LDS
constexpr int N_MAX = 16;                           // largest search half-width (cells, yaw steps)
constexpr int CLAMP_MAX = 127;
constexpr int LANES = 256;
constexpr int PER_LANE_MAX = ((2 * N_MAX + 1) * (2 * N_MAX + 1) + LANES - 1) / LANES;      // candidates (a, b) a lane can own: 5
constexpr int SCORE_BIAS = RMAX * CLAMP_MAX;        // |score| <= 48768: bias - score is 0..97536, 17 bits
constexpr double CELL_LIMIT = 1073741824.0;         // 2^30, as the map update's

struct MatchArg {
  int W, H;                          // cells; cell (i, j) at evidence[i * H + j]
  long stride;                       // W * H for a map per robot, 0 for a shared one
  double ox, oy, dx, dy;             // origin and cell size
  int mx, my;                        // the map update's window half-widths
  int nx, ny, nyaw;                  // the search half-widths
  int clamp, min_score, min_gain;
};

struct MatchOut {
  int32_t* offset_cells; int32_t* yaw_index; double* offset; int32_t* score; int32_t* n_used; int8_t* matched;
};

// key of candidate (k, idx) with score s, SMALLER IS BETTER: (-score, a^2 + b^2, |k - n_yaw|, k, idx) packed most significant first
__device__ __forceinline__ uint64_t pack_key(int s, int d2, int k, int nyaw, int idx) {
  const int dk = k > nyaw ? k - nyaw : nyaw - k;
  return ((uint64_t)(unsigned)(SCORE_BIAS - s) << 32) | ((uint64_t)(unsigned)d2 << 22) | ((uint64_t)(unsigned)dk << 17) |
         ((uint64_t)(unsigned)k << 11) | (uint64_t)(unsigned)idx;
}

// one yaw's correlation for the NP candidates of this lane: every lane walks the same list of offsets (an LDS broadcast) and adds
// the byte at offset + shift; shift[] of a candidate the lane does not own is 0 (in bounds, its sum is dropped by the caller)
template <int NP>
__device__ __forceinline__ void correlate(const int8_t* __restrict__ V, const int* __restrict__ cells, int n, const int (&shift)[PER_LANE_MAX],
                                          int (&acc)[PER_LANE_MAX]) {
#pragma unroll
  for (int p = 0; p < PER_LANE_MAX; ++p) acc[p] = 0;
  for (int r = 0; r < n; ++r) {
    const int base = cells[r];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] += (int)V[base + shift[p]];
  }
}

__global__ void __launch_bounds__(LANES) scan_match_kernel(int R, double depth, const double* __restrict__ state,
                                                           const double* __restrict__ hits, const double* __restrict__ rot_table,
                                                           const int32_t* __restrict__ mask, const int32_t* __restrict__ evidence,
                                                           MatchOut out, MatchArg gm) {
  __shared__ int8_t V_[MATCH_WINDOW_CELLS];          // the grown window: cell (gi, gj) at gi * gh + gj
  __shared__ double ex_[RMAX], ey_[RMAX];            // the end points, NaN = the reading is not valid
  __shared__ int cells_[2][RMAX];                    // yaw k's used cells as offsets into V_ (shift (-n_x, -n_y)), in cells_[k & 1]
  __shared__ int count_[2 * N_MAX + 1];              // ... and how many they are
  __shared__ uint64_t keys_[LANES];
  __shared__ int used0_, zero_;
  const long b = blockIdx.x;
  const int tid = threadIdx.x;
  const double cdx = gm.dx, cdy = gm.dy, ox = gm.ox, oy = gm.oy;
  bool live = !(mask && mask[b] == 0);               // uniform over the workgroup
  double x0 = 0.0, y0 = 0.0, fi = 0.0, fj = 0.0;
  if (live) {
    x0 = state[5 * b]; y0 = state[5 * b + 2];
    fi = floor((x0 - ox) / cdx); fj = floor((y0 - oy) / cdy);
    live = (fabs(fi) < CELL_LIMIT) & (fabs(fj) < CELL_LIMIT);
  }
  if (!live) {                                       // no cell, or masked: zeros
    if (tid == 0) {
      out.offset_cells[2 * b] = 0; out.offset_cells[2 * b + 1] = 0; out.yaw_index[b] = 0;
      out.offset[2 * b] = 0.0; out.offset[2 * b + 1] = 0.0;
      out.score[2 * b] = 0; out.score[2 * b + 1] = 0; out.n_used[b] = 0; out.matched[b] = 0;
    }
    return;
  }
  const int ci = (int)fi, cj = (int)fj;
  const int mx = gm.mx, my = gm.my, nx = gm.nx, ny = gm.ny, nyaw = gm.nyaw;
  const int W = gm.W, H = gm.H, clampv = gm.clamp;
  const int gw = 2 * (mx + nx) + 1, gh = 2 * (my + ny) + 1, gcell = gw * gh;      // <= MATCH_WINDOW_CELLS (the host refuses more)
  const int gi0 = ci - mx - nx, gj0 = cj - my - ny;

  // ---- stage: the clamped evidence of the grown window, and the readings' end points ----------------------------
  const int32_t* const ev = evidence + b * gm.stride;
  for (int c = tid; c < gcell; c += LANES) {
    const int gi = c / gh, gj = c - gi * gh;
    const int i = gi0 + gi, j = gj0 + gj;
    int v = 0;
    if (i >= 0 && i < W && j >= 0 && j < H) {
      v = ev[(long)i * H + j];
      v = v < -clampv ? -clampv : (v > clampv ? clampv : v);
    }
    V_[c] = (int8_t)v;
  }
  for (int r = tid; r < R; r += LANES) {
    const double qx = hits[(b * R + r) * 2], qy = hits[(b * R + r) * 2 + 1];
    // the end point of the map update: the reading pushed `depth` along its ray
    const double ddx = qx - x0, ddy = qy - y0;
    const double L = sqrt(ddx * ddx + ddy * ddy);
    const double s = depth / L;
    const double ex = qx + s * ddx, ey = qy + s * ddy;
    const bool valid = !((qx != qx) | (qy != qy)) & (L != 0.0) & (fabs(L) < INFINITY) & (fabs(ex) < INFINITY) & (fabs(ey) < INFINITY);
    ex_[r] = valid ? ex : NAN; ey_[r] = ey;
  }
  if (tid < 2 * N_MAX + 1) count_[tid] = 0;
  __syncthreads();

  // ---- the candidates of this lane: idx = (a + n_x) * (2 n_y + 1) + (b + n_y) = tid + p * LANES -----------------
  const int nb = 2 * ny + 1, ncand = (2 * nx + 1) * nb;
  const int nper = (ncand + LANES - 1) / LANES;      // uniform, 1..PER_LANE_MAX
  int shift[PER_LANE_MAX], d2[PER_LANE_MAX];
#pragma unroll
  for (int p = 0; p < PER_LANE_MAX; ++p) {
    const int idx = tid + p * LANES;
    const bool mine = idx < ncand;
    const int ai = mine ? idx / nb : 0, bi = mine ? idx - ai * nb : 0;
    shift[p] = ai * gh + bi;                          // (a + n_x) * gh + (b + n_y) >= 0
    d2[p] = (ai - nx) * (ai - nx) + (bi - ny) * (bi - ny);
  }
  const int zero_idx = nx * nb + ny;
  uint64_t best = ~(uint64_t)0;

  const int T = 2 * nyaw + 1;
  for (int k = 0; k < T; ++k) {
    // the cells: at k == n_yaw the end point itself, no arithmetic -- exactly the cells the map update would raise
    double c = 1.0, s = 0.0;
    if (k != nyaw) { c = rot_table[2 * k]; s = rot_table[2 * k + 1]; }
    for (int r = tid; r < R; r += LANES) {
      const double ex = ex_[r], ey = ey_[r];
      if (ex != ex) continue;
      double x = ex, y = ey;
      if (k != nyaw) {
        const double rx = ex - x0, ry = ey - y0;
        x = x0 + (c * rx - s * ry); y = y0 + (s * rx + c * ry);
      }
      const double hi = floor((x - ox) / cdx) - fi, hj = floor((y - oy) / cdy) - fj;
      if ((fabs(hi) <= (double)mx) & (fabs(hj) <= (double)my)) {
        const int li = (int)hi + mx, lj = (int)hj + my;          // the window cell; shift (0, 0) of the grown window is (-n_x, -n_y)
        cells_[k & 1][atomicAdd(&count_[k], 1)] = li * gh + lj;
      }
    }
    // the one barrier of the yaw: the lists alternate, so a wave that is ahead fills the other one
    __syncthreads();
    const int n = count_[k];
    const int* const cells = cells_[k & 1];
    int acc[PER_LANE_MAX];
    switch (nper) {
      case 1: correlate<1>(V_, cells, n, shift, acc); break;
      case 2: correlate<2>(V_, cells, n, shift, acc); break;
      case 3: correlate<3>(V_, cells, n, shift, acc); break;
      case 4: correlate<4>(V_, cells, n, shift, acc); break;
      default: correlate<PER_LANE_MAX>(V_, cells, n, shift, acc); break;
    }
#pragma unroll
    for (int p = 0; p < PER_LANE_MAX; ++p) {
      const int idx = tid + p * LANES;
      if (idx < ncand) {
        const uint64_t key = pack_key(acc[p], d2[p], k, nyaw, idx);
        best = key < best ? key : best;
        if (k == nyaw && idx == zero_idx) { zero_ = acc[p]; used0_ = n; }
      }
    }
  }

  // ---- select: the smallest key of the workgroup ----------------------------------------------------------------
  keys_[tid] = best;
  __syncthreads();
  for (int h = LANES / 2; h > 0; h >>= 1) {
    if (tid < h) { const uint64_t o = keys_[tid + h]; if (o < keys_[tid]) keys_[tid] = o; }
    __syncthreads();
  }
  if (tid == 0) {
    const uint64_t key = keys_[0];
    const int s_best = SCORE_BIAS - (int)(unsigned)(key >> 32), s_zero = zero_;
    int k = (int)((key >> 11) & 63u) - nyaw;
    const int idx = (int)(key & 2047u);
    int a = idx / nb - nx, bb = idx - (idx / nb) * nb - ny;
    const bool accepted = (s_best >= gm.min_score) & (s_best - s_zero >= gm.min_gain);
    if (!accepted) { a = 0; bb = 0; k = 0; }
    out.offset_cells[2 * b] = a; out.offset_cells[2 * b + 1] = bb; out.yaw_index[b] = k;
    out.offset[2 * b] = (double)a * cdx; out.offset[2 * b + 1] = (double)bb * cdy;
    out.score[2 * b] = s_best; out.score[2 * b + 1] = s_zero;
    out.n_used[b] = used0_;
    out.matched[b] = (int8_t)(accepted & ((a != 0) | (bb != 0) | (k != 0)));
  }
}

}  // namespace

extern "C" int lipmpc_scan_match_batch(int device, int64_t B, int32_t resolution, int32_t W, int32_t H, int32_t grid_shared,
                                       const double* origin, const double* cell, double lidar_range, double depth, int32_t n_x,
                                       int32_t n_y, int32_t n_yaw, const double* rot_table, int32_t clamp, int32_t min_score,
                                       int32_t min_gain, const double* state, const double* hits, const int32_t* mask,
                                       const int32_t* evidence, int32_t* offset_cells, int32_t* yaw_index, double* offset,
                                       int32_t* score, int32_t* n_used, int8_t* matched, void* hip_stream) {
  if (B < 0 || B > 0x7fffffff || resolution < 1 || resolution > RMAX || W < 1 || H < 1 || !origin || !cell || n_x < 0 ||
      n_x > N_MAX || n_y < 0 || n_y > N_MAX || n_yaw < 0 || n_yaw > N_MAX || clamp < 1 || clamp > CLAMP_MAX || min_gain < 0 ||
      (n_yaw > 0 && !rot_table))
    return LIPMPC_E_ARG;
  const double ox = origin[0], oy = origin[1], dx = cell[0], dy = cell[1];
  if (!(dx > 0.0) || !(dy > 0.0) || !(dx < INFINITY) || !(dy < INFINITY) || !(fabs(ox) < INFINITY) || !(fabs(oy) < INFINITY) ||
      !(lidar_range >= 0.0) || !(lidar_range < INFINITY) || !(depth >= 0.0) || !(depth < INFINITY))
    return LIPMPC_E_ARG;
  // the map update's window grown by the search half-widths is kept as bytes in LDS: what does not fit is refused
  const double mx = floor((lidar_range + depth) / dx) + 2.0, my = floor((lidar_range + depth) / dy) + 2.0;
  if (!((2.0 * (mx + n_x) + 1.0) * (2.0 * (my + n_y) + 1.0) <= (double)MATCH_WINDOW_CELLS)) return LIPMPC_E_UNSUPPORTED;
  if (B == 0) return LIPMPC_OK;
  if (!state || !hits || !evidence || !offset_cells || !yaw_index || !offset || !score || !n_used || !matched) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  const MatchArg gm{W, H, grid_shared ? 0L : (long)W * H, ox, oy, dx, dy, (int)mx, (int)my, n_x, n_y, n_yaw, clamp, min_score, min_gain};
  const MatchOut out{offset_cells, yaw_index, offset, score, n_used, matched};
  hipLaunchKernelGGL(scan_match_kernel, dim3((unsigned)B), dim3(LANES), 0, (hipStream_t)hip_stream, resolution, depth, state, hits,
                     rot_table, mask, evidence, out, gm);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}
