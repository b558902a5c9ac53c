// lipmpc_neighbours.hip -- neighbour LDCBF rows on the device (lipmpc_neighbour_c_eta_batch, include/lipmpc.h).
//
// The robots of one launch as each other's obstacles: every robot's nearest neighbours among the B robots, one half-space
// row per neighbour appended to its c_eta.  A uniform grid of cells a hair wider than sense_range, hashed into a table of
// NB buckets (a power of two, sized from B), as a counting sort -- six launches on the caller's stream:
//   nb_clear_kernel    the bucket counts and the run allocator to zero (the workspace's contents are arbitrary on entry)
//   nb_bin_kernel      one lane per robot: present?  cell, bucket, count (integer atomic); an absent robot's counts
//   nb_runs_kernel     one lane per bucket: a contiguous run of the sorted array for every bucket -- exclusive scan of the
//                      counts inside the workgroup, the workgroup's base from one atomic on the allocator (the runs need not
//                      follow each other in bucket order, so no scan crosses workgroups)
//   nb_scatter_kernel  one lane per robot: a 32-byte record (x, y, cell, group, index) into the bucket's run (atomic cursor)
//   nb_search_kernel   one lane per SORTED robot (lanes of a wave are neighbours in space: their walks read the same runs):
//                      the 3 x 3 cells around it, the best K candidates by (d2, j) in registers -> n_near, n_rows, indices
//   nb_rows_kernel     one lane per (robot, slot): the row of that slot, or zeros; `neighbours`
// Where a bucket's run lies, and where a robot lands inside it, depends on how the atomics fell; nothing that is written does:
// the walk counts EVERY in-range candidate and keeps the K smallest under the total order (d2, j), whatever order it meets
// them in.
// The contract is restated in numpy by tests/neighbour_oracle.py; every compared quantity is a sum, product, quotient or
// square root of the inputs evaluated as written, so the outputs are the oracle's bit for bit.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lipmpc.h"

#pragma clang fp contract(off)

namespace {

constexpr int NB_THREADS = 256;
constexpr int NB_MIN = 1024;                        // buckets at least (a multiple of NB_THREADS)
constexpr int K_MAX = 16;                           // rows per robot at most; stride of the workspace's index lists
constexpr int64_t B_MAX = int64_t(1) << 22;
constexpr double CELL_CLAMP = 1073741824.0;         // 2^30: cell coordinates are clamped to +-2^30 (int32, room for +-1)

// THE 3 x 3 CELLS SUFFICE.  Claim: if dist < R in floating point then the cell coordinates of x_i and x_j differ by at most 1
// (y likewise), with cell(v) = clamp(floor(fl(v / w))) and w = max(fl(R (1 + 2^-20)), 2^-500).
//  - With u = 2^-53: fl(x_i - x_j) = (x_i - x_j)(1 + e), |e| <= u; fl(dx dx) >= dx^2 (1 - u) unless it is below 2^-1022;
//    d2 >= fl(dx dx) (adding fl(dy dy) >= 0 and rounding are monotone); sqrt and its rounding are monotone and lose at most
//    another (1 - u): dist >= |x_i - x_j| (1 - 4u).  So dist < R gives |x_i - x_j| < R (1 + 5u) < w (1 - 2^-21).  If dx dx is
//    below 2^-1022 then |x_i - x_j| < 2^-510 < w (1 - 2^-21) by the floor on w.
//  - Let a < b be the true quotients x / w, b - a < 1 - 2^-21, and suppose floor(fl(b)) >= floor(fl(a)) + 2: there is an
//    integer n with fl(a) < n + 1 and fl(b) >= n + 2.  Rounding is monotone and integers below 2^53 are doubles, so a < n + 1
//    and b >= (n + 2)(1 - u), hence b - a > 1 - |n + 2| u >= 1 - 2^-21 for |n + 2| <= 2^32: a contradiction.  Beyond
//    +-2^30 the clamp, which is monotone too, puts everything into one cell.
//  - w = inf (R near the largest double) makes every quotient 0: one cell.
__device__ inline int cell_of(double v, double w) {
  double q = floor(v / w);
  q = q < -CELL_CLAMP ? -CELL_CLAMP : (q > CELL_CLAMP ? CELL_CLAMP : q);
  return (int)q;
}

// bucket of cell (cx, cy) in world g: distinct cells share buckets, so the walk compares the cell (and g) of every candidate
__device__ inline uint32_t bucket_of(int cx, int cy, int g, uint32_t mask) {
  uint32_t h = (uint32_t)cx * 0x9E3779B1u ^ (uint32_t)cy * 0x85EBCA77u ^ (uint32_t)g * 0xC2B2AE3Du;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
  return h & mask;
}

__host__ __device__ inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }

struct alignas(16) Rec {                            // a robot in the sorted array: two 16-byte loads
  double x, y;
  int32_t cx, cy, g, idx;
};

struct Layout {                                     // byte offsets into the workspace
  int64_t nb;                                       // buckets
  int64_t run, total, bucket, cell, rec, nbr, bytes;
};

inline Layout layout(int64_t B) {
  Layout L;
  L.nb = NB_MIN;
  while (L.nb < 2 * B) L.nb <<= 1;
  L.run = 0;                                        // int2 [nb]: (count, -) -> (begin, cursor) -> after the scatter (begin, end)
  L.total = L.run + align256(L.nb * 8);             // int32: the run allocator; after nb_runs_kernel the robots present
  L.bucket = L.total + 256;                         // int32 [B]: bucket of robot b, -1 = absent
  L.cell = L.bucket + align256(B * 4);              // int2 [B]
  L.rec = L.cell + align256(B * 8);                 // Rec [B]: the sorted array
  L.nbr = L.rec + align256(B * (int64_t)sizeof(Rec));   // int32 [B, K_MAX]: neighbour indices in (d2, j) order
  L.bytes = L.nbr + align256(B * K_MAX * 4);
  return L;
}

struct Ws {
  int2* run;
  int32_t *total, *bucket, *nbr;
  int2* cell;
  Rec* rec;
  uint32_t mask;
};

__device__ inline int clamp_slot(const int32_t* first_slot, int i, int n_obs_max) {
  const int f = first_slot ? first_slot[i] : 0;
  return f < 0 ? 0 : (f > n_obs_max ? n_obs_max : f);
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ void nb_clear_kernel(Ws ws, int nb) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nb) ws.run[t] = make_int2(0, 0);
  if (t == 0) *ws.total = 0;
}

__global__ void nb_bin_kernel(int B, double w, const double* __restrict__ state, const double* __restrict__ radius,
                              const int32_t* __restrict__ group, Ws ws, int32_t* __restrict__ n_rows,
                              int32_t* __restrict__ n_near) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const double x = state[5 * (int64_t)i], y = state[5 * (int64_t)i + 2], r = radius[i];
  const int g = group ? group[i] : 0;
  if (!(g >= 0 && isfinite(x) && isfinite(y) && isfinite(r) && !(r < 0.0))) {
    ws.bucket[i] = -1;
    n_rows[i] = 0;
    n_near[i] = 0;
    return;
  }
  const int cx = cell_of(x, w), cy = cell_of(y, w);
  const uint32_t b = bucket_of(cx, cy, g, ws.mask);
  ws.bucket[i] = (int32_t)b;
  ws.cell[i] = make_int2(cx, cy);
  atomicAdd(&ws.run[b].x, 1);
}

// run of bucket t: [begin, begin + count) with begin = the workgroup's base + the exclusive scan of the counts inside the
// workgroup; nb is a multiple of NB_THREADS
__global__ __launch_bounds__(NB_THREADS) void nb_runs_kernel(Ws ws) {
  __shared__ int32_t part[NB_THREADS];
  __shared__ int32_t base;
  const int t = threadIdx.x, b = blockIdx.x * NB_THREADS + t;
  const int32_t count = ws.run[b].x;
  part[t] = count;
  __syncthreads();
  for (int off = 1; off < NB_THREADS; off <<= 1) {
    const int32_t v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  if (t == NB_THREADS - 1) base = part[t] ? atomicAdd(ws.total, part[t]) : 0;
  __syncthreads();
  const int32_t begin = base + part[t] - count;     // <= the robots present <= B
  ws.run[b] = make_int2(begin, begin);
}

__global__ void nb_scatter_kernel(int B, const double* __restrict__ state, const int32_t* __restrict__ group, Ws ws) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const int32_t b = ws.bucket[i];
  if (b < 0) return;
  const int pos = atomicAdd(&ws.run[b].y, 1);       // inside the bucket's run: < the robots present <= B
  const int2 c = ws.cell[i];
  Rec r;
  r.x = state[5 * (int64_t)i];
  r.y = state[5 * (int64_t)i + 2];
  r.cx = c.x; r.cy = c.y; r.g = group ? group[i] : 0; r.idx = i;
  ws.rec[pos] = r;
}

// after the scatter run[b] = (begin, end) of bucket b's run; *total = robots present
template <int K>
__global__ __launch_bounds__(NB_THREADS) void nb_search_kernel(int B, int n_obs_max, int k_rows, double R,
                                                               const int32_t* __restrict__ first_slot, Ws ws,
                                                               int32_t* __restrict__ n_rows, int32_t* __restrict__ n_near) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B || t >= *ws.total) return;
  const Rec me = ws.rec[t];
  const double xi = me.x, yi = me.y;
  const int g = me.g, i = me.idx;
  double bd[K];
  int bj[K];
#pragma unroll
  for (int s = 0; s < K; ++s) { bd[s] = INFINITY; bj[s] = INT_MAX; }
  int near = 0;
  int2 run[9];                                      // the nine runs first: independent loads, one latency
#pragma unroll
  for (int o = 0; o < 9; ++o) run[o] = ws.run[bucket_of(me.cx + o % 3 - 1, me.cy + o / 3 - 1, g, ws.mask)];
#pragma unroll
  for (int o = 0; o < 9; ++o) {
    const int cx = me.cx + o % 3 - 1, cy = me.cy + o / 3 - 1;
    for (int p = run[o].x; p < run[o].y; ++p) {
      const Rec c = ws.rec[p];
      if (c.cx != cx || c.cy != cy || c.g != g || c.idx == i) continue;
      const double dx = xi - c.x, dy = yi - c.y;
      const double d2 = dx * dx + dy * dy;
      if (!(sqrt(d2) < R)) continue;
      ++near;
      double cd = d2;
      int cj = c.idx;
      if (cd < bd[K - 1] || (cd == bd[K - 1] && cj < bj[K - 1])) {
#pragma unroll
        for (int s = 0; s < K; ++s) {               // insertion by compare-and-swap down the sorted list: static indices
          const bool lt = cd < bd[s] || (cd == bd[s] && cj < bj[s]);
          const double td = lt ? bd[s] : cd;
          const int tj = lt ? bj[s] : cj;
          bd[s] = lt ? cd : bd[s];
          bj[s] = lt ? cj : bj[s];
          cd = td;
          cj = tj;
        }
      }
    }
  }
  const int room = n_obs_max - clamp_slot(first_slot, i, n_obs_max);
  int n = near < k_rows ? near : k_rows;
  n = n < room ? n : room;
  n_near[i] = near;
  n_rows[i] = n;
  int32_t* out = ws.nbr + (int64_t)i * K_MAX;
#pragma unroll
  for (int s = 0; s < K; ++s)
    if (s < n) out[s] = bj[s];
}

__global__ void nb_rows_kernel(int B, int n_obs_max, int k_rows, int S, double share, const double* __restrict__ state,
                               const double* __restrict__ radius, const int32_t* __restrict__ first_slot,
                               const int32_t* __restrict__ nbr, const int32_t* __restrict__ n_rows,
                               double* __restrict__ c_eta, int32_t* __restrict__ neighbours) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)B * S) return;
  const int i = (int)(id / S), s = (int)(id % S);
  const int fs = clamp_slot(first_slot, i, n_obs_max), nr = n_rows[i];
  if (neighbours && s < k_rows) neighbours[(int64_t)i * k_rows + s] = s < nr ? nbr[(int64_t)i * K_MAX + s] : -1;
  if (s >= n_obs_max || s < fs) return;
  double4 row = make_double4(0.0, 0.0, 0.0, 0.0);
  if (s - fs < nr) {
    const int j = nbr[(int64_t)i * K_MAX + (s - fs)];
    const double xj = state[5 * (int64_t)j], yj = state[5 * (int64_t)j + 2];
    const double dx = state[5 * (int64_t)i] - xj, dy = state[5 * (int64_t)i + 2] - yj;
    const double d2 = dx * dx + dy * dy;
    const double dist = sqrt(d2);
    const double rs = radius[i] + radius[j];
    const double offset = rs + share * (dist - rs);
    const double ex = dx / dist, ey = dy / dist;
    row = make_double4(xj + offset * ex, yj + offset * ey, ex, ey);
  }
  *reinterpret_cast<double4*>(c_eta + ((int64_t)i * n_obs_max + s) * 4) = row;
}

}  // namespace

extern "C" int64_t lipmpc_neighbour_workspace_bytes(int64_t B) {
  if (B < 0 || B > B_MAX) return LIPMPC_E_ARG;
  return layout(B).bytes;
}

extern "C" int lipmpc_neighbour_c_eta_batch(int device, int64_t B, int32_t n_obs_max, int32_t k_rows, double sense_range,
                                            double share, const double* state, const double* radius, const int32_t* group,
                                            const int32_t* first_slot, void* workspace, double* c_eta, int32_t* n_rows,
                                            int32_t* n_near, int32_t* neighbours, void* hip_stream) {
  if (B < 0 || B > B_MAX || k_rows < 1 || k_rows > K_MAX || n_obs_max < 1 || n_obs_max > 50) return LIPMPC_E_ARG;
  if (!(sense_range > 0.0) || !isfinite(sense_range) || !(share >= 0.0 && share <= 1.0)) return LIPMPC_E_ARG;
  if (!state || !radius || !workspace || !c_eta || !n_rows || !n_near) return LIPMPC_E_ARG;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const Layout L = layout(B);
  char* base = (char*)workspace;
  Ws ws;
  ws.run = (int2*)(base + L.run);
  ws.total = (int32_t*)(base + L.total);
  ws.bucket = (int32_t*)(base + L.bucket);
  ws.cell = (int2*)(base + L.cell);
  ws.rec = (Rec*)(base + L.rec);
  ws.nbr = (int32_t*)(base + L.nbr);
  ws.mask = (uint32_t)(L.nb - 1);
  // cells a hair wider than the range, and never narrower than 2^-500 (the argument at cell_of)
  double w = sense_range * (1.0 + 0x1p-20);
  if (w < 0x1p-500) w = 0x1p-500;
  const int nb = (int)L.nb, n = (int)B;
  const unsigned per_robot = (unsigned)((B + NB_THREADS - 1) / NB_THREADS);
  hipLaunchKernelGGL(nb_clear_kernel, dim3((unsigned)(nb / NB_THREADS)), dim3(NB_THREADS), 0, s, ws, nb);
  hipLaunchKernelGGL(nb_bin_kernel, dim3(per_robot), dim3(NB_THREADS), 0, s, n, w, state, radius, group, ws, n_rows, n_near);
  hipLaunchKernelGGL(nb_runs_kernel, dim3((unsigned)(nb / NB_THREADS)), dim3(NB_THREADS), 0, s, ws);
  hipLaunchKernelGGL(nb_scatter_kernel, dim3(per_robot), dim3(NB_THREADS), 0, s, n, state, group, ws);
  if (k_rows <= 4)
    hipLaunchKernelGGL(nb_search_kernel<4>, dim3(per_robot), dim3(NB_THREADS), 0, s, n, n_obs_max, k_rows, sense_range,
                       first_slot, ws, n_rows, n_near);
  else
    hipLaunchKernelGGL(nb_search_kernel<K_MAX>, dim3(per_robot), dim3(NB_THREADS), 0, s, n, n_obs_max, k_rows, sense_range,
                       first_slot, ws, n_rows, n_near);
  const int S = n_obs_max > k_rows ? n_obs_max : k_rows;
  const int64_t lanes = B * S;
  hipLaunchKernelGGL(nb_rows_kernel, dim3((unsigned)((lanes + NB_THREADS - 1) / NB_THREADS)), dim3(NB_THREADS), 0, s, n,
                     n_obs_max, k_rows, S, share, state, radius, first_slot, ws.nbr, n_rows, c_eta, neighbours);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}
