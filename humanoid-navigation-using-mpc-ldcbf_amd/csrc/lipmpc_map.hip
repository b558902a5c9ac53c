// lipmpc_map.hip -- LiDAR scans integrated into an occupancy-evidence grid on the device (lipmpc_map_update_batch,
// include/lipmpc.h).
//
// The memory between the scan and the planner: one call adds one scan per robot to an int32 evidence grid, +w_hit on the cells
// the readings lie in, -w_miss on the cells the rays passed through.  One launch on the caller's stream:
//   map_update_kernel  one wavefront per robot.  The window of cells a ray can reach is kept as TWO bitmaps in LDS (passed,
//                      hit); every lane marches its rays through the window (the grid scan's march: crossings recomputed from
//                      the boundary's index, x on a tie) and sets bits with LDS OR-atomics; after a barrier the wave sweeps the
//                      window, 64 consecutive cells per trip (consecutive j = consecutive words of the grid), and adds into
//                      global memory -- a plain read-modify-write on a per-robot map (the wave owns it), an integer atomic on
//                      a shared one.
// A cell is updated once per robot and call however many rays met it (the bitmaps), and integer addition commutes: the result
// does not depend on the launch order, two calls give identical bits.
// The contract is restated in numpy by tests/map_oracle.py; every compared quantity is a sum, product, quotient, floor or
// square root of the inputs evaluated as written, so the evidence is the oracle's integer for integer.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lipmpc.h"

#pragma clang fp contract(off)

namespace {

constexpr int RMAX = 384;                           // rays per scan, as the scans
constexpr int MAP_WINDOW_CELLS = 49152;             // the window of cells a ray can reach, one bit each in either bitmap
constexpr int MAP_WORDS = MAP_WINDOW_CELLS / 32;    // 2 x 6 KiB of LDS per wave
constexpr double CELL_LIMIT = 1073741824.0;         // 2^30: a robot must have a cell index below this in magnitude

struct MapArg {
  int W, H;                          // cells; cell (i, j) at evidence[i * H + j]
  long stride;                       // W * H for a map per robot, 0 for a shared one
  double ox, oy, dx, dy;             // origin and cell size
  int nx, ny;                        // half-width of the window in cells: floor((range + depth) / cell) + 2
};

__global__ void __launch_bounds__(64) map_update_kernel(int R, double lidar_range, double depth, int w_hit, int w_miss,
                                                        const double* __restrict__ state, const double* __restrict__ hits,
                                                        const double* __restrict__ ray_table, const int32_t* __restrict__ mask,
                                                        int32_t* evidence, MapArg gm) {
  __shared__ unsigned passed_[MAP_WORDS], hit_[MAP_WORDS];
  const long b = blockIdx.x;
  const int lane = threadIdx.x;
  if (mask && mask[b] == 0) return;
  const int W = gm.W, H = gm.H;
  const double ox = gm.ox, oy = gm.oy, cdx = gm.dx, cdy = gm.dy;
  const double x0 = state[5 * b], y0 = state[5 * b + 2];
  // the robot's cell, as the grid scan's; a robot that cannot be given one (far away, NaN, infinite) contributes nothing
  const double fi = floor((x0 - ox) / cdx), fj = floor((y0 - oy) / cdy);
  if (!((fabs(fi) < CELL_LIMIT) & (fabs(fj) < CELL_LIMIT))) return;
  const int ci = (int)fi, cj = (int)fj;
  const int nx = gm.nx, ny = gm.ny;
  const int ww = 2 * nx + 1, wh = 2 * ny + 1, ncell = ww * wh;
  const int wi0 = ci - nx, wj0 = cj - ny;
  if (!(wi0 < W && wi0 + ww > 0 && wj0 < H && wj0 + wh > 0)) return;      // no cell of the window is a cell of the grid
  const int nw = (ncell + 31) >> 5;
  for (int w = lane; w < nw; w += 64) { passed_[w] = 0u; hit_[w] = 0u; }
  __syncthreads();

  // ---- the rays: window cell (li, lj) = grid cell (wi0 + li, wj0 + lj) is bit li * wh + lj ----------------------
  for (int i = lane; i < R; i += 64) {
    const double qx = hits[(b * R + i) * 2], qy = hits[(b * R + i) * 2 + 1];
    const bool reading = !((qx != qx) | (qy != qy));
    double ex, ey;
    int hli = -1, hlj = -1;                          // the hit cell in window coordinates, if it is in the window
    if (reading) {
      // the end point: the reading pushed `depth` along the ray, into the wall whose face it lies on
      const double ddx = qx - x0, ddy = qy - y0;
      const double L = sqrt(ddx * ddx + ddy * ddy);
      const double s = depth / L;
      ex = qx + s * ddx; ey = qy + s * ddy;
      if (!((L != 0.0) & (fabs(L) < INFINITY) & (fabs(ex) < INFINITY) & (fabs(ey) < INFINITY))) continue;
      const double hi = floor((ex - ox) / cdx) - fi, hj = floor((ey - oy) / cdy) - fj;
      if ((fabs(hi) <= (double)nx) & (fabs(hj) <= (double)ny)) { hli = (int)hi + nx; hlj = (int)hj + ny; }
    } else {
      ex = x0 + lidar_range * ray_table[2 * i]; ey = y0 + lidar_range * ray_table[2 * i + 1];
    }
    // the march from p0 to e (the grid scan's): t_x, t_y = the parameters at which the ray crosses the next cell boundary in
    // x / in y, each from the boundary's INDEX; the smaller is taken (x on a tie), the ray is then in the next cell of that axis
    const double rdx = ex - x0, rdy = ey - y0;
    const double ivx = 1.0 / rdx, ivy = 1.0 / rdy;
    const bool upx = rdx > 0.0, upy = rdy > 0.0;
    double ax = (double)(ci + (upx ? 1 : 0)), ay = (double)(cj + (upy ? 1 : 0));
    double tx = rdx != 0.0 ? ((ox + ax * cdx) - x0) * ivx : INFINITY;
    double ty = rdy != 0.0 ? ((oy + ay * cdy) - y0) * ivy : INFINITY;
    int ri = nx, rj = ny, rk = nx * wh + ny;
    if (!(ri == hli && rj == hlj)) atomicOr(&passed_[rk >> 5], 1u << (rk & 31));      // the robot's own cell
    for (;;) {
      const bool xs = tx <= ty;
      const double t = xs ? tx : ty;
      if (xs) {
        ri += upx ? 1 : -1; rk += upx ? wh : -wh; ax += upx ? 1.0 : -1.0;
        tx = ((ox + ax * cdx) - x0) * ivx;
      } else {
        rj += upy ? 1 : -1; rk += upy ? 1 : -1; ay += upy ? 1.0 : -1.0;
        ty = ((oy + ay * cdy) - y0) * ivy;
      }
      if (!(t <= 1.0)) break;                                     // beyond the end point (a NaN parameter stops the ray)
      if ((ri < 0) | (ri >= ww) | (rj < 0) | (rj >= wh)) break;   // out of the window
      if (ri == hli && rj == hlj) break;                          // the hit cell ends the ray and is not passed
      atomicOr(&passed_[rk >> 5], 1u << (rk & 31));
    }
    if (hli >= 0) {
      const int hk = hli * wh + hlj;
      atomicOr(&hit_[hk >> 5], 1u << (hk & 31));
    }
  }
  __syncthreads();

  // ---- the flush: one update per touched cell, hit wins over passed ---------------------------------------------
  int32_t* const ev = evidence + b * gm.stride;
  const bool shared = gm.stride == 0;
  const int q64 = 64 / wh, r64 = 64 % wh;
  int li = lane / wh, lj = lane % wh;                 // window cell of bit k
  for (int k = lane; k < ncell; k += 64) {
    const bool h = (hit_[k >> 5] >> (k & 31)) & 1u, p = (passed_[k >> 5] >> (k & 31)) & 1u;
    const int gi = wi0 + li, gj = wj0 + lj;
    if ((h | p) && gi >= 0 && gi < W && gj >= 0 && gj < H) {
      const int v = h ? w_hit : -w_miss;
      int32_t* const a = ev + ((long)gi * H + gj);
      if (shared) atomicAdd(a, v);
      else *a += v;
    }
    li += q64; lj += r64;
    if (lj >= wh) { lj -= wh; ++li; }
  }
}

}  // namespace

extern "C" int lipmpc_map_update_batch(int device, int64_t B, int32_t resolution, int32_t W, int32_t H, int32_t grid_shared,
                                       const double* origin, const double* cell, double lidar_range, double depth,
                                       int32_t w_hit, int32_t w_miss, const double* state, const double* hits,
                                       const double* ray_table, const int32_t* mask, int32_t* evidence, void* hip_stream) {
  if (B < 0 || B > 0x7fffffff || resolution < 1 || resolution > RMAX || W < 1 || H < 1 || w_hit < 1 || w_hit > 32767 ||
      w_miss < 1 || w_miss > 32767 || !origin || !cell)
    return LIPMPC_E_ARG;
  const double ox = origin[0], oy = origin[1], dx = cell[0], dy = cell[1];
  if (!(dx > 0.0) || !(dy > 0.0) || !(dx < INFINITY) || !(dy < INFINITY) || !(fabs(ox) < INFINITY) || !(fabs(oy) < INFINITY) ||
      !(lidar_range >= 0.0) || !(lidar_range < INFINITY) || !(depth >= 0.0) || !(depth < INFINITY))
    return LIPMPC_E_ARG;
  // the window of cells within reach of a robot is kept as two bitmaps in LDS: (range, cell) pairs whose window does not fit are refused
  const double nx = floor((lidar_range + depth) / dx) + 2.0, ny = floor((lidar_range + depth) / dy) + 2.0;
  if (!((2.0 * nx + 1.0) * (2.0 * ny + 1.0) <= (double)MAP_WINDOW_CELLS)) return LIPMPC_E_UNSUPPORTED;
  if (B == 0) return LIPMPC_OK;
  if (!state || !hits || !ray_table || !evidence) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  const MapArg gm{W, H, grid_shared ? 0L : (long)W * H, ox, oy, dx, dy, (int)nx, (int)ny};
  hipLaunchKernelGGL(map_update_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)hip_stream, resolution, lidar_range, depth,
                     w_hit, w_miss, state, hits, ray_table, mask, evidence, gm);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}
