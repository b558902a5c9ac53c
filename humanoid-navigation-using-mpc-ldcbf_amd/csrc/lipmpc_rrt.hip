// lipmpc_rrt.hip -- batched RRT* sub-goal planner on the device (lipmpc_rrt_plan_batch, include/lipmpc.h).
//
// The global planner of the reference's HumanoidMPCWithRRT (HumanoidMPCVariants/HumanoidMPCWithRRT.py:21-135), one
// problem per (obstacle set, start, goal, seed), in five launches on the caller's stream:
//   rrt_setup_kernel   one thread per problem: bounds, grid dims, start / goal cells (:32-65, 103-105)
//   rrt_grid_kernel    one thread per cell: occupancy from the convex hulls of the ROUNDED vertices (:67-88), ballot ->
//                      bitmap words; the hulls (monotone chain) are built in LDS by every workgroup
//   rrt_edt_col_kernel one thread per grid column: 1-D distance along y
//   rrt_edt_row_kernel one thread per grid row: lower envelope of parabolas (Meijster) along x -> exact integer d2,
//                      C = exp(-sqrt(d2)) (:107-112)
//   rrt_star_kernel    one workgroup per problem: RRT* (:116-128) with the tree and the occupancy bitmap in LDS, then the
//                      tree path as world sub-goals (:129-135)
// lipmpc_rrt_plan_grid_batch plans on a GIVEN occupancy grid: rrt_setup_grid_kernel and rrt_pack_grid_kernel (bounds from the
// grid's geometry, occupancy bytes -> bitmap words) stand in for the first two launches, the other three run unchanged.
// The contract (sampler, ties, rewiring, segment rasterisation) is spelled out at lipmpc_rrt_plan_batch in lipmpc.h and
// restated in numpy by tests/rrt_oracle.py.  Every comparison the tree makes is between exactly computed values (integers,
// correctly rounded sqrt, separate multiply and add), so given C the tree is the oracle's bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lipmpc.h"

#pragma clang fp contract(off)

namespace {

constexpr int RRT_THREADS = 256;                    // rrt_star_kernel: 4 waves per problem (64 and 128: slower)
constexpr int RRT_WAVES = RRT_THREADS / 64;
constexpr int GRID_THREADS = 256;
constexpr int MAX_SIDE = 4096;                      // cells per grid side: coordinates pack into 16 bits, d2 < 2^25
constexpr int64_t LDS_LIMIT = 160 * 1024;

struct RrtHdr {                                     // per-problem header at the start of its workspace slot
  double min_x, max_x, min_y, max_y;
  int32_t W, H, ncells, status;                     // status: FOUND (0) = grid built, or GRID_TOO_LARGE
  int32_t any_occ, start_cell, goal_cell, pad;
};

struct Slot {                                       // per-problem workspace layout
  int64_t bytes, bitmap, g, C;
};

__host__ __device__ inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }

__host__ __device__ inline Slot slot_layout(int64_t max_cells) {
  Slot s;
  s.bitmap = align256(sizeof(RrtHdr));
  s.g = s.bitmap + align256(((max_cells + 63) / 64) * 8);
  s.C = s.g + align256(max_cells * 4);
  s.bytes = s.C + align256(max_cells * 8);
  return s;
}

__host__ __device__ inline int64_t rrt_lds_bytes(int n_samples, int64_t max_cells) {
  const int64_t nv = n_samples + 1;                 // root + one vertex per sample at most
  return nv * (8 + 8 + 4 + 4 + 4) + ((max_cells + 63) / 64) * 8 + 256;
}

__device__ inline int floor_div(int a, int b) {     // b > 0
  int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

__device__ inline bool occ_bit(const uint32_t* bm, int c) { return (bm[c >> 5] >> (c & 31)) & 1u; }

__device__ inline int to_cell(double v, double lo, double hi, int n) {
  return (int)rint(((v - lo) / (hi - lo)) * (double)n);
}

__device__ inline double to_world(int i, double lo, double hi, int n) {
  return lo + (((double)i * (hi - lo)) / (double)n);
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ void rrt_setup_kernel(int64_t B, lipmpc_rrt_params p, const double* __restrict__ obs_xy,
                                 const int32_t* __restrict__ obs_nv, int n_obs_max, int v_max,
                                 const double* __restrict__ start, const double* __restrict__ goal, char* ws,
                                 int64_t slot_bytes, int32_t* grid_dims) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double sx = start ? start[2 * b] : 0.0, sy = start ? start[2 * b + 1] : 0.0;
  const double gx = goal[2 * b], gy = goal[2 * b + 1];
  double lx = fmin(sx, gx), hx = fmax(sx, gx), ly = fmin(sy, gy), hy = fmax(sy, gy);
  for (int o = 0; o < n_obs_max; ++o) {
    int nv = obs_nv[b * n_obs_max + o];
    nv = nv > v_max ? v_max : nv;
    const double* r = obs_xy + ((b * n_obs_max + o) * v_max) * 2;
    for (int k = 0; k < nv; ++k) {
      lx = fmin(lx, r[2 * k]); hx = fmax(hx, r[2 * k]);
      ly = fmin(ly, r[2 * k + 1]); hy = fmax(hy, r[2 * k + 1]);
    }
  }
  RrtHdr* h = (RrtHdr*)(ws + b * slot_bytes);
  h->min_x = lx - p.margin; h->max_x = hx + p.margin;
  h->min_y = ly - p.margin; h->max_y = hy + p.margin;
  const double Hd = ceil((double)p.width * ((h->max_y - h->min_y) / (h->max_x - h->min_x)));
  const bool too_large = !(Hd + 1.0 <= (double)MAX_SIDE) || (double)(p.width + 1) * (Hd + 1.0) > (double)p.max_cells;
  const int H = too_large ? 0 : (int)Hd;
  h->W = p.width;
  h->H = H;
  h->ncells = too_large ? 0 : (p.width + 1) * (H + 1);
  h->status = too_large ? LIPMPC_RRT_GRID_TOO_LARGE : LIPMPC_RRT_FOUND;
  h->any_occ = 0;
  if (!too_large) {
    h->start_cell = to_cell(sx, h->min_x, h->max_x, p.width) * (H + 1) + to_cell(sy, h->min_y, h->max_y, H);
    h->goal_cell = to_cell(gx, h->min_x, h->max_x, p.width) * (H + 1) + to_cell(gy, h->min_y, h->max_y, H);
  }
  if (grid_dims) {
    grid_dims[2 * b] = p.width + 1;
    grid_dims[2 * b + 1] = too_large ? (int)fmin(Hd + 1.0, 2147483647.0) : H + 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Occupancy.  blockIdx.x = problem, blockIdx.y = chunk of GRID_THREADS cells.  LDS: per obstacle 3 * v_max packed cells
// (v_max sorted rounded vertices, 2 * v_max for the monotone chain) + the hull size and the half-open box.
__global__ void __launch_bounds__(GRID_THREADS) rrt_grid_kernel(const double* __restrict__ obs_xy,
                                                                const int32_t* __restrict__ obs_nv, int n_obs_max,
                                                                int v_max, char* ws, int64_t slot_bytes,
                                                                int64_t off_bitmap) {
  extern __shared__ uint32_t lds_u32[];
  const int64_t b = blockIdx.x;
  RrtHdr* h = (RrtHdr*)(ws + b * slot_bytes);
  if (h->status != LIPMPC_RRT_FOUND) return;
  const int ncells = h->ncells, H1 = h->H + 1;
  const int c0 = blockIdx.y * GRID_THREADS;
  if (c0 >= ncells) return;
  uint32_t* pts = lds_u32;                                   // [n_obs_max][v_max]
  uint32_t* hull = pts + n_obs_max * v_max;                  // [n_obs_max][2 v_max]
  int* hinfo = (int*)(hull + 2 * n_obs_max * v_max);         // [n_obs_max][5]: hull size, x0, x1, y0, y1
  for (int o = threadIdx.x; o < n_obs_max; o += blockDim.x) {
    int nv = obs_nv[b * n_obs_max + o];
    nv = nv > v_max ? v_max : nv;
    int* inf = hinfo + 5 * o;
    if (nv <= 0) { inf[0] = 0; continue; }
    const double* r = obs_xy + ((b * n_obs_max + o) * v_max) * 2;
    uint32_t* P = pts + o * v_max;
    uint32_t* Hh = hull + o * 2 * v_max;                     // first the unsorted rounded vertices, then the hull
    int x0 = 1 << 30, x1 = -1, y0 = 1 << 30, y1 = -1;
    for (int k = 0; k < nv; ++k) {                           // rounded vertices packed x << 16 | y (orders
      const int xi = to_cell(r[2 * k], h->min_x, h->max_x, h->W);        // lexicographically)
      const int yi = to_cell(r[2 * k + 1], h->min_y, h->max_y, h->H);
      x0 = min(x0, xi); x1 = max(x1, xi); y0 = min(y0, yi); y1 = max(y1, yi);
      Hh[k] = ((uint32_t)xi << 16) | (uint32_t)yi;
    }
    for (int k = 0; k < nv; ++k) {                           // rank sort
      const uint32_t key = Hh[k];
      int rank = 0;
      for (int q = 0; q < nv; ++q) rank += (Hh[q] < key) || (Hh[q] == key && q < k);
      P[rank] = key;
    }
    int nu = 0;                                              // drop duplicates
    for (int k = 0; k < nv; ++k)
      if (nu == 0 || P[k] != P[nu - 1]) P[nu++] = P[k];
    int m = 0;
    if (nu <= 2) {
      for (int k = 0; k < nu; ++k) Hh[k] = P[k];
      m = nu;
    } else {                                                 // Andrew's monotone chain, collinear points dropped
      auto cr = [](uint32_t o_, uint32_t a, uint32_t c) {
        const int ox = o_ >> 16, oy = o_ & 0xffff, ax = a >> 16, ay = a & 0xffff, cx = c >> 16, cy = c & 0xffff;
        return (ax - ox) * (cy - oy) - (ay - oy) * (cx - ox);
      };
      for (int k = 0; k < nu; ++k) {
        while (m >= 2 && cr(Hh[m - 2], Hh[m - 1], P[k]) <= 0) --m;
        Hh[m++] = P[k];
      }
      const int t = m + 1;
      for (int k = nu - 2; k >= 0; --k) {
        while (m >= t && cr(Hh[m - 2], Hh[m - 1], P[k]) <= 0) --m;
        Hh[m++] = P[k];
      }
      m -= 1;
    }
    inf[0] = m; inf[1] = x0; inf[2] = x1; inf[3] = y0; inf[4] = y1;
  }
  __syncthreads();
  const int c = c0 + threadIdx.x;
  bool occ = false;
  if (c < ncells) {
    const int i = c / H1, j = c - (c / H1) * H1;
    for (int o = 0; o < n_obs_max && !occ; ++o) {
      const int* inf = hinfo + 5 * o;
      const int m = inf[0];
      if (m == 0 || !(inf[1] <= i && i < inf[2] && inf[3] <= j && j < inf[4])) continue;
      const uint32_t* Hh = hull + o * 2 * v_max;
      bool in = true;
      for (int e = 0; e < m && in; ++e) {
        const uint32_t a = Hh[e], bb = Hh[e + 1 == m ? 0 : e + 1];
        const int ax = a >> 16, ay = a & 0xffff, bx = bb >> 16, by = bb & 0xffff;
        in = (bx - ax) * (j - ay) - (by - ay) * (i - ax) >= 0;
      }
      occ = in;
    }
  }
  const uint64_t mask = __ballot(occ);
  if ((threadIdx.x & 63) == 0 && c < ncells) {
    uint32_t* bm = (uint32_t*)(ws + b * slot_bytes + off_bitmap);
    const int w = c >> 5;                                     // c is a multiple of 64
    bm[w] = (uint32_t)mask;
    bm[w + 1] = (uint32_t)(mask >> 32);
    if (mask) atomicOr(&h->any_occ, 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Planning on a GIVEN occupancy grid (lipmpc_rrt_plan_grid_batch): the two kernels that stand in for rrt_setup_kernel and
// rrt_grid_kernel; the distance transform and the tree run behind them unchanged.
// The planner's cells are the CENTRES of the grid's W x H cells: bounds min = origin + cell / 2, max = origin + (W - 1/2) cell,
// W_p = W - 1, H_p = H - 1 -- the inverse of GridMap.from_planner.  One thread per problem.
__global__ void rrt_setup_grid_kernel(int64_t B, lipmpc_rrt_params p, int W, int H, double ox, double oy, double cdx, double cdy,
                                      const double* __restrict__ start, const double* __restrict__ goal, char* ws,
                                      int64_t slot_bytes, int32_t* grid_dims) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double sx = start ? start[2 * b] : 0.0, sy = start ? start[2 * b + 1] : 0.0;
  const double gx = goal[2 * b], gy = goal[2 * b + 1];
  RrtHdr* h = (RrtHdr*)(ws + b * slot_bytes);
  h->min_x = ox + cdx / 2.0; h->max_x = ox + ((double)W - 0.5) * cdx;
  h->min_y = oy + cdy / 2.0; h->max_y = oy + ((double)H - 0.5) * cdy;
  const bool too_large = W > MAX_SIDE || H > MAX_SIDE || (int64_t)W * H > (int64_t)p.max_cells;
  h->W = W - 1;
  h->H = too_large ? 0 : H - 1;
  h->ncells = too_large ? 0 : W * H;
  h->any_occ = 0;
  h->start_cell = 0; h->goal_cell = 0;
  int st = too_large ? LIPMPC_RRT_GRID_TOO_LARGE : LIPMPC_RRT_FOUND;
  if (!too_large) {
    // the rounded cells as doubles first: a start or goal that rounds outside the grid (NaN included) has no cell
    const double si = rint(((sx - h->min_x) / (h->max_x - h->min_x)) * (double)(W - 1));
    const double sj = rint(((sy - h->min_y) / (h->max_y - h->min_y)) * (double)(H - 1));
    const double gi = rint(((gx - h->min_x) / (h->max_x - h->min_x)) * (double)(W - 1));
    const double gj = rint(((gy - h->min_y) / (h->max_y - h->min_y)) * (double)(H - 1));
    const bool inside = (si >= 0.0) & (si <= (double)(W - 1)) & (sj >= 0.0) & (sj <= (double)(H - 1)) &
                        (gi >= 0.0) & (gi <= (double)(W - 1)) & (gj >= 0.0) & (gj <= (double)(H - 1));
    if (inside) {
      h->start_cell = (int)si * H + (int)sj;
      h->goal_cell = (int)gi * H + (int)gj;
    } else {
      st = LIPMPC_RRT_OUTSIDE_GRID;
    }
  }
  h->status = st;
  if (grid_dims) { grid_dims[2 * b] = W; grid_dims[2 * b + 1] = H; }
}

// Occupancy bytes -> bitmap words.  blockIdx.x = problem, blockIdx.y = chunk of GRID_THREADS cells; the grid's own layout
// (cell (i, j) at i * H + j) is the planner's, so a wave's ballot over 64 consecutive bytes is the word pair.
__global__ void __launch_bounds__(GRID_THREADS) rrt_pack_grid_kernel(const uint8_t* __restrict__ occ, int64_t occ_stride, char* ws,
                                                                     int64_t slot_bytes, int64_t off_bitmap) {
  const int64_t b = blockIdx.x;
  RrtHdr* h = (RrtHdr*)(ws + b * slot_bytes);
  if (h->status != LIPMPC_RRT_FOUND) return;
  const int ncells = h->ncells;
  const int c0 = blockIdx.y * GRID_THREADS;
  if (c0 >= ncells) return;
  const int c = c0 + threadIdx.x;
  const bool o = c < ncells && occ[b * occ_stride + c] != 0;
  const uint64_t mask = __ballot(o);
  if ((threadIdx.x & 63) == 0 && c < ncells) {
    uint32_t* bm = (uint32_t*)(ws + b * slot_bytes + off_bitmap);
    const int w = c >> 5;                                     // c is a multiple of 64
    bm[w] = (uint32_t)mask;
    bm[w + 1] = (uint32_t)(mask >> 32);
    if (mask) atomicOr(&h->any_occ, 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// EDT pass 1: g[x][y] = distance along y to the nearest occupied cell of column x (big if none).
__global__ void rrt_edt_col_kernel(char* ws, int64_t slot_bytes, Slot sl) {
  const int64_t b = blockIdx.x;
  const RrtHdr* h = (const RrtHdr*)(ws + b * slot_bytes);
  const int x = blockIdx.y * blockDim.x + threadIdx.x;
  if (h->status != LIPMPC_RRT_FOUND || x > h->W) return;
  const int H1 = h->H + 1, big = h->W + h->H + 4;
  const uint32_t* bm = (const uint32_t*)(ws + b * slot_bytes + sl.bitmap);
  int32_t* g = (int32_t*)(ws + b * slot_bytes + sl.g) + (int64_t)x * H1;
  int run = big;
  for (int y = 0; y < H1; ++y) {
    run = occ_bit(bm, x * H1 + y) ? 0 : min(run + 1, big);
    g[y] = run;
  }
  run = big;
  for (int y = H1 - 1; y >= 0; --y) {
    run = occ_bit(bm, x * H1 + y) ? 0 : min(run + 1, big);
    g[y] = min(g[y], run);
  }
}

// EDT pass 2 along x for row y (Meijster, Roerdink & Hesselink 2000): d2[x][y] = min_x' (x - x')^2 + g[x'][y]^2, exact in
// integers, then C = exp(-sqrt(d2)).  The envelope's (site, start) pairs live in the row's own C slots, which the final
// sweep overwrites from the right: it reads pair q <= u before it writes slot u.
__global__ void rrt_edt_row_kernel(char* ws, int64_t slot_bytes, Slot sl, int64_t max_cells, int32_t* occ_d2,
                                   double* cost_grid) {
  const int64_t b = blockIdx.x;
  const RrtHdr* h = (const RrtHdr*)(ws + b * slot_bytes);
  const int y = blockIdx.y * blockDim.x + threadIdx.x;
  if (h->status != LIPMPC_RRT_FOUND || y > h->H) return;
  const int W = h->W, H1 = h->H + 1;
  const bool any = h->any_occ != 0;
  const int32_t* g = (const int32_t*)(ws + b * slot_bytes + sl.g) + y;
  double* Cg = (double*)(ws + b * slot_bytes + sl.C) + y;
  int2* st = (int2*)Cg;                                     // st[q * H1] = (s[q], t[q])
  auto G2 = [&](int i) { const int v = g[(int64_t)i * H1]; return v * v; };
  auto F = [&](int x, int i) { return (x - i) * (x - i) + G2(i); };
  int q = 0;
  st[0] = make_int2(0, 0);
  for (int u = 1; u <= W; ++u) {
    int2 sq = st[(int64_t)q * H1];
    while (q >= 0 && F(sq.y, sq.x) > F(sq.y, u)) {
      --q;
      if (q >= 0) sq = st[(int64_t)q * H1];
    }
    if (q < 0) {
      q = 0;
      st[0] = make_int2(u, 0);
    } else {
      const int w = 1 + floor_div(u * u - sq.x * sq.x + G2(u) - G2(sq.x), 2 * (u - sq.x));
      if (w <= W) {
        ++q;
        st[(int64_t)q * H1] = make_int2(u, w);
      }
    }
  }
  for (int u = W; u >= 0; --u) {
    const int2 sq = st[(int64_t)q * H1];
    const int d2 = F(u, sq.x);
    const int64_t c = (int64_t)u * H1;
    Cg[c] = any ? exp(-sqrt((double)d2)) : __builtin_nan("");
    if (occ_d2) occ_d2[b * max_cells + c + y] = any ? d2 : -1;
    if (cost_grid) cost_grid[b * max_cells + c + y] = Cg[c];
    if (u == sq.y) --q;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
__device__ inline uint64_t splitmix_cell(uint64_t seed, int64_t k, uint32_t ncells) {
  uint64_t z = seed + (uint64_t)(k + 1) * 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return ((z >> 32) * (uint64_t)ncells) >> 32;
}

__device__ inline int dist2(uint32_t a, int bx, int by) {
  const int dx = (int)(a >> 16) - bx, dy = (int)(a & 0xffff) - by;
  return dx * dx + dy * dy;
}

// the cells a + floor((2 k d + m) / (2 m)), k = 0..m, of the segment with its endpoints in lexicographic order, walked
// incrementally by one lane (the major axis moves by one cell per step, the minor one keeps quotient and remainder)
__device__ inline bool seg_free_lane(const uint32_t* bm, int H1, int ax, int ay, int bx, int by) {
  if (bx < ax || (bx == ax && by < ay)) {
    int t = ax; ax = bx; bx = t;
    t = ay; ay = by; by = t;
  }
  const int dx = bx - ax, dy = by - ay;
  const int m = max(abs(dx), abs(dy));
  if (m == 0) return !occ_bit(bm, ax * H1 + ay);
  const int two_m = 2 * m, first = ax * H1 + ay;
  int qx = 0, rx = m, qy = 0, ry = m;
  for (int k0 = 0; k0 <= m; k0 += 8) {
    // eight cells per trip: eight independent LDS reads in flight instead of one dependent read per cell (cells past
    // the end read the first cell again)
    uint32_t hit = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = k0 + u <= m ? (ax + qx) * H1 + ay + qy : first;
      hit |= bm[c >> 5] >> (c & 31);
      rx += 2 * dx; ry += 2 * dy;
      if (rx >= two_m) { rx -= two_m; ++qx; } else if (rx < 0) { rx += two_m; --qx; }
      if (ry >= two_m) { ry -= two_m; ++qy; } else if (ry < 0) { ry += two_m; --qy; }
    }
    if (hit & 1u) return false;
  }
  return true;
}

struct Red {                                               // reduction slots, two sets used alternately
  uint64_t key[2][RRT_WAVES];
  double c[2][RRT_WAVES];
  int v[2][RRT_WAVES];
};

// OR over the workgroup through the reduction slots (__syncthreads_or would bring 256 bytes of static LDS of its own, which
// the LDS limit of rrt_lds_bytes does not count)
__device__ inline bool block_or(int x, Red* red, int& ph) {
  const bool w_any = __ballot(x != 0) != 0;
  if ((threadIdx.x & 63) == 0) red->v[ph][threadIdx.x >> 6] = w_any;
  __syncthreads();
  int r = red->v[ph][0];
  for (int i = 1; i < RRT_WAVES; ++i) r |= red->v[ph][i];
  ph ^= 1;
  return r != 0;
}

// the same cells split over the workgroup (one segment, every lane a stride of its cells): true if free
__device__ inline bool seg_free_block(const uint32_t* bm, int H1, int ax, int ay, int bx, int by, Red* red, int& ph) {
  if (bx < ax || (bx == ax && by < ay)) {
    int t = ax; ax = bx; bx = t;
    t = ay; ay = by; by = t;
  }
  const int dx = bx - ax, dy = by - ay;
  const int m = max(abs(dx), abs(dy));
  int hit = 0;
  if (m == 0) {
    hit = occ_bit(bm, ax * H1 + ay);
  } else {
    for (int k = threadIdx.x; k <= m && !hit; k += RRT_THREADS) {
      const int cx = ax + floor_div(2 * k * dx + m, 2 * m), cy = ay + floor_div(2 * k * dy + m, 2 * m);
      hit = occ_bit(bm, cx * H1 + cy);
    }
  }
  return !block_or(hit, red, ph);
}

__device__ inline uint64_t block_min_u64(uint64_t x, Red* red, int& ph) {
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)x, o), hi = __shfl_xor((uint32_t)(x >> 32), o);
    const uint64_t y = ((uint64_t)hi << 32) | lo;
    x = y < x ? y : x;
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red->key[ph][w] = x;
  __syncthreads();
  uint64_t r = red->key[ph][0];
  for (int i = 1; i < RRT_WAVES; ++i) r = red->key[ph][i] < r ? red->key[ph][i] : r;
  ph ^= 1;
  return r;
}

// lexicographic (cost, index) minimum over the workgroup
__device__ inline void block_argmin(double& c, int& v, Red* red, int& ph) {
  for (int o = 32; o >= 1; o >>= 1) {
    const double c2 = __shfl_xor(c, o);
    const int v2 = __shfl_xor(v, o);
    if (c2 < c || (c2 == c && v2 < v)) { c = c2; v = v2; }
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red->c[ph][w] = c; red->v[ph][w] = v; }
  __syncthreads();
  c = red->c[ph][0];
  v = red->v[ph][0];
  for (int i = 1; i < RRT_WAVES; ++i) {
    const double c2 = red->c[ph][i];
    const int v2 = red->v[ph][i];
    if (c2 < c || (c2 == c && v2 < v)) { c = c2; v = v2; }
  }
  ph ^= 1;
}

// One workgroup per problem.  LDS: cost, C, packed cell, parent, BFS mark per vertex; the occupancy bitmap; Red.
__global__ void __launch_bounds__(RRT_THREADS) rrt_star_kernel(lipmpc_rrt_params p, const uint64_t* __restrict__ seeds,
                                                               char* ws, int64_t slot_bytes, Slot sl, int S_max,
                                                               double* sub_goals, int32_t* n_sub, int32_t* status,
                                                               double* path_cost, double* tree) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const RrtHdr* h = (const RrtHdr*)(ws + b * slot_bytes);
  const int NV = p.n_samples + 1;
  double* cost = (double*)lds;
  double* Cv = cost + NV;
  uint32_t* cell = (uint32_t*)(Cv + NV);
  int32_t* par = (int32_t*)(cell + NV);
  int32_t* mark = par + NV;
  uint32_t* bm = (uint32_t*)(mark + NV + (NV & 1));            // 8-byte aligned
  const int words = (p.max_cells + 63) / 64 * 2;
  Red* red = (Red*)(bm + words);

  int st = h->status;
  const int ncells = h->ncells, H1 = h->H + 1;
  const double* Cg = (const double*)(ws + b * slot_bytes + sl.C);
  if (st == LIPMPC_RRT_FOUND) {
    const uint32_t* bmg = (const uint32_t*)(ws + b * slot_bytes + sl.bitmap);
    for (int w = tid; w < (ncells + 63) / 64 * 2; w += RRT_THREADS) bm[w] = bmg[w];
    __syncthreads();
    if (!h->any_occ) st = LIPMPC_RRT_NO_OBSTACLE_GRID;
    else if (occ_bit(bm, h->start_cell)) st = LIPMPC_RRT_START_OCCUPIED;
    else if (occ_bit(bm, h->goal_cell)) st = LIPMPC_RRT_GOAL_OCCUPIED;
  }
  if (st != LIPMPC_RRT_FOUND) {
    if (tid == 0) {
      status[b] = st; n_sub[b] = 0; path_cost[b] = __builtin_nan("");
      if (tree) { double* t = tree + b * (int64_t)(NV + 1) * 4; t[0] = 0; t[1] = -1; t[2] = 0; t[3] = 0; }
    }
    return;
  }
  const int sc = h->start_cell, gc = h->goal_cell;
  const int r2 = p.r_rewire * p.r_rewire;
  const uint64_t seed = seeds[b];
  const int64_t cap = 64 * (int64_t)p.n_samples;
  if (tid == 0) {
    cell[0] = ((uint32_t)(sc / H1) << 16) | (uint32_t)(sc % H1);
    par[0] = -1; cost[0] = 0.0; Cv[0] = Cg[sc]; mark[0] = 0;
  }
  __syncthreads();
  int nv = 1, samples = 0, ph = 0, tag = 1;
  int64_t k = 0;
  const int lane = tid & 63;
  while (samples < p.n_samples && k < cap) {
    // next valid draw: every wave runs the same 64-draw windows, so all agree without a barrier
    int c = -1;
    while (k < cap) {
      const int64_t kk = k + lane;
      bool ok = false;
      int ci = 0;
      if (kk < cap) {
        ci = (int)splitmix_cell(seed, kk, (uint32_t)ncells);
        ok = !occ_bit(bm, ci) && ci != sc && ci != gc;
      }
      const uint64_t m = __ballot(ok);
      if (m) {
        const int l = __ffsll((unsigned long long)m) - 1;
        c = __shfl(ci, l);
        k += l + 1;
        break;
      }
      k = k + 64 < cap ? k + 64 : cap;                        // a window that straddles the cap holds cap - k draws
    }
    if (c < 0) break;
    ++samples;
    const int xi = c / H1, xj = c - (c / H1) * H1;
    // nearest vertex (lowest index on ties)
    uint64_t key = ~0ull;
    for (int v = tid; v < nv; v += RRT_THREADS) {
      const uint64_t kv = ((uint64_t)(uint32_t)dist2(cell[v], xi, xj) << 32) | (uint32_t)v;
      key = kv < key ? kv : key;
    }
    key = block_min_u64(key, red, ph);
    const int vn = (int)(key & 0xffffffffu), dmin = (int)(key >> 32);
    if (dmin == 0) continue;
    if (!seg_free_block(bm, H1, cell[vn] >> 16, cell[vn] & 0xffff, xi, xj, red, ph)) continue;
    // parent: cheapest near vertex with a free segment; the cost test first, the segment only if it could win
    const double Cx = Cg[c];
    double bc = __builtin_inf();
    int bv = 0x7fffffff;
    for (int v = tid; v < nv; v += RRT_THREADS) {
      const int d2 = dist2(cell[v], xi, xj);
      if (d2 > r2 && v != vn) continue;
      const double cc = cost[v] + Cx * sqrt((double)d2);
      if (cc < bc && seg_free_lane(bm, H1, cell[v] >> 16, cell[v] & 0xffff, xi, xj)) { bc = cc; bv = v; }
    }
    block_argmin(bc, bv, red, ph);
    const int xv = nv;
    if (tid == 0) {
      cell[xv] = ((uint32_t)xi << 16) | (uint32_t)xj;
      par[xv] = bv; cost[xv] = bc; Cv[xv] = Cx; mark[xv] = tag;
    }
    // rewire against the costs before this sample (no cost changes until the barrier below)
    int any = 0;
    for (int u = tid; u < nv; u += RRT_THREADS) {
      if (u == bv) continue;
      const int d2 = dist2(cell[u], xi, xj);
      if (d2 > r2 && u != vn) continue;
      const double nc = bc + Cv[u] * sqrt((double)d2);
      if (nc < cost[u] && seg_free_lane(bm, H1, cell[u] >> 16, cell[u] & 0xffff, xi, xj)) { par[u] = xv; any = 1; }
    }
    nv += 1;
    if (block_or(any, red, ph)) {
      // costs top-down through x's subtree, one level per pass: level L+1 = the vertices whose parent carries tag L
      for (;;) {
        int found = 0;
        for (int v = tid; v < nv; v += RRT_THREADS) {
          const int pv = par[v];
          if (pv >= 0 && mark[pv] == tag) {
            const uint32_t cp = cell[pv];
            cost[v] = cost[pv] + Cv[v] * sqrt((double)dist2(cell[v], cp >> 16, cp & 0xffff));
            mark[v] = tag + 1;
            found = 1;
          }
        }
        ++tag;
        if (!block_or(found, red, ph)) break;
      }
    }
    ++tag;
  }
  // goal: cheapest vertex within r_rewire with a free segment
  const int gi = gc / H1, gj = gc - (gc / H1) * H1;
  const double Cgoal = Cg[gc];
  double bc = __builtin_inf();
  int bv = 0x7fffffff;
  for (int v = tid; v < nv; v += RRT_THREADS) {
    const int d2 = dist2(cell[v], gi, gj);
    if (d2 > r2) continue;
    const double cc = cost[v] + Cgoal * sqrt((double)d2);
    if (cc < bc && seg_free_lane(bm, H1, cell[v] >> 16, cell[v] & 0xffff, gi, gj)) { bc = cc; bv = v; }
  }
  block_argmin(bc, bv, red, ph);
  const bool found = bv != 0x7fffffff;
  if (tree) {
    double* t = tree + b * (int64_t)(NV + 1) * 4;
    for (int v = tid; v < nv; v += RRT_THREADS) {
      double* r = t + 4 * (v + 1);
      r[0] = (double)(cell[v] >> 16); r[1] = (double)(cell[v] & 0xffff); r[2] = (double)par[v]; r[3] = cost[v];
    }
    if (tid == 0) { t[0] = nv; t[1] = found ? bv : -1; t[2] = (double)k; t[3] = samples; }
  }
  if (tid != 0) return;
  if (!found) {
    status[b] = LIPMPC_RRT_NO_PATH; n_sub[b] = 0; path_cost[b] = __builtin_nan("");
    return;
  }
  int L = 1;
  for (int v = bv; v > 0; v = par[v]) ++L;
  path_cost[b] = bc;
  if (L > S_max) {
    status[b] = LIPMPC_RRT_PATH_OVERFLOW; n_sub[b] = 0;
    return;
  }
  double* sg = sub_goals + b * (int64_t)S_max * 2;
  sg[2 * (L - 1)] = to_world(gi, h->min_x, h->max_x, h->W);
  sg[2 * (L - 1) + 1] = to_world(gj, h->min_y, h->max_y, h->H);
  int i = L - 2;
  for (int v = bv; v > 0; v = par[v], --i) {
    sg[2 * i] = to_world(cell[v] >> 16, h->min_x, h->max_x, h->W);
    sg[2 * i + 1] = to_world(cell[v] & 0xffff, h->min_y, h->max_y, h->H);
  }
  status[b] = LIPMPC_RRT_FOUND;
  n_sub[b] = L;
}

bool params_ok(const lipmpc_rrt_params* p) {
  return p && p->width >= 1 && p->width < MAX_SIDE && p->n_samples >= 1 && p->r_rewire >= 1 && p->r_rewire <= 8192 &&
         p->max_cells >= 1 && p->max_cells <= (1 << 22) && p->margin > 0.0 &&
         rrt_lds_bytes(p->n_samples, p->max_cells) <= LDS_LIMIT;
}

// the parameters the tree and the distance transform read (a given grid has no width and no margin)
bool tree_params_ok(const lipmpc_rrt_params* p) {
  return p && p->n_samples >= 1 && p->r_rewire >= 1 && p->r_rewire <= 8192 && p->max_cells >= 1 && p->max_cells <= (1 << 22) &&
         rrt_lds_bytes(p->n_samples, p->max_cells) <= LDS_LIMIT;
}

}  // namespace

extern "C" int lipmpc_rrt_default_params(lipmpc_rrt_params* p) {
  if (!p) return LIPMPC_E_ARG;
  p->width = 250;
  p->n_samples = 1500;
  p->r_rewire = 80;
  p->max_cells = 1 << 17;
  p->margin = 3.0;
  return LIPMPC_OK;
}

extern "C" int64_t lipmpc_rrt_workspace_bytes(const lipmpc_rrt_params* p, int64_t B) {
  if (!params_ok(p) || B < 0) return LIPMPC_E_ARG;
  return B * slot_layout(p->max_cells).bytes;
}

extern "C" int lipmpc_rrt_plan_batch(int device, const lipmpc_rrt_params* p, int64_t B, const double* obs_xy,
                                     const int32_t* obs_nv, int32_t n_obs_max, int32_t v_max, const double* start,
                                     const double* goal, const uint64_t* seed, void* workspace, double* sub_goals,
                                     int32_t* n_sub, int32_t* status, double* path_cost, int32_t* grid_dims,
                                     int32_t* occ_d2, double* cost_grid, double* tree, int32_t S_max,
                                     void* hip_stream) {
  if (!params_ok(p) || B < 0 || B > 0x7fffffff || n_obs_max < 0 || v_max < 1 || v_max > 64 || S_max < 1) return LIPMPC_E_ARG;
  if (B == 0) return LIPMPC_OK;
  if (!goal || !seed || !workspace || !sub_goals || !n_sub || !status || !path_cost) return LIPMPC_E_ARG;
  if (n_obs_max > 0 && (!obs_xy || !obs_nv)) return LIPMPC_E_ARG;
  const size_t lds_grid = (size_t)n_obs_max * v_max * 3 * 4 + (size_t)n_obs_max * 5 * 4;
  if (lds_grid > 64 * 1024) return LIPMPC_E_UNSUPPORTED;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const Slot sl = slot_layout(p->max_cells);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(rrt_setup_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, B, *p, obs_xy, obs_nv, n_obs_max,
                     v_max, start, goal, ws, sl.bytes, grid_dims);
  // (without obstacle slots the grid kernel writes an empty bitmap: the problem ends NO_OBSTACLE_GRID)
  hipLaunchKernelGGL(rrt_grid_kernel, dim3((unsigned)B, (unsigned)((p->max_cells + GRID_THREADS - 1) / GRID_THREADS)),
                     dim3(GRID_THREADS), lds_grid, s, obs_xy, obs_nv, n_obs_max, v_max, ws, sl.bytes, sl.bitmap);
  const int64_t h1_cap = p->max_cells / (p->width + 1);
  const int max_h1 = (int)(h1_cap < MAX_SIDE ? h1_cap : MAX_SIDE);
  hipLaunchKernelGGL(rrt_edt_col_kernel, dim3((unsigned)B, (unsigned)((p->width + 64) / 64)), dim3(64), 0, s, ws,
                     sl.bytes, sl);
  hipLaunchKernelGGL(rrt_edt_row_kernel, dim3((unsigned)B, (unsigned)((max_h1 + 63) / 64)), dim3(64), 0, s, ws,
                     sl.bytes, sl, (int64_t)p->max_cells, occ_d2, cost_grid);
  const size_t lds_tree = (size_t)rrt_lds_bytes(p->n_samples, p->max_cells);
  if (lds_tree > 64 * 1024 &&
      hipFuncSetAttribute((const void*)rrt_star_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_tree) != hipSuccess)
    return LIPMPC_E_HIP;
  hipLaunchKernelGGL(rrt_star_kernel, dim3((unsigned)B), dim3(RRT_THREADS), lds_tree, s, *p, seed, ws, sl.bytes, sl,
                     S_max, sub_goals, n_sub, status, path_cost, tree);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}

extern "C" int lipmpc_rrt_plan_grid_batch(int device, const lipmpc_rrt_params* p, int64_t B, int32_t W, int32_t H,
                                          int32_t grid_shared, const double* origin, const double* cell, const uint8_t* occ,
                                          const double* start, const double* goal, const uint64_t* seed, void* workspace,
                                          double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                          int32_t* grid_dims, int32_t* occ_d2, double* cost_grid, double* tree, int32_t S_max,
                                          void* hip_stream) {
  if (!tree_params_ok(p) || B < 0 || B > 0x7fffffff || W < 2 || H < 2 || S_max < 1 || !origin || !cell) return LIPMPC_E_ARG;
  const double ox = origin[0], oy = origin[1], dx = cell[0], dy = cell[1];
  if (!(dx > 0.0) || !(dy > 0.0) || !(dx < INFINITY) || !(dy < INFINITY) || !(fabs(ox) < INFINITY) || !(fabs(oy) < INFINITY))
    return LIPMPC_E_ARG;
  if (B == 0) return LIPMPC_OK;
  if (!occ || !goal || !seed || !workspace || !sub_goals || !n_sub || !status || !path_cost) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const Slot sl = slot_layout(p->max_cells);
  char* ws = (char*)workspace;
  // a grid beyond the caps is refused per problem by the setup kernel (GRID_TOO_LARGE); the launches behind it then find nothing to do
  const bool fits = W <= MAX_SIDE && H <= MAX_SIDE && (int64_t)W * H <= (int64_t)p->max_cells;
  const int64_t ncells = fits ? (int64_t)W * H : 1;
  const int w1 = fits ? W : 1, h1 = fits ? H : 1;
  hipLaunchKernelGGL(rrt_setup_grid_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, B, *p, W, H, ox, oy, dx, dy, start,
                     goal, ws, sl.bytes, grid_dims);
  hipLaunchKernelGGL(rrt_pack_grid_kernel, dim3((unsigned)B, (unsigned)((ncells + GRID_THREADS - 1) / GRID_THREADS)),
                     dim3(GRID_THREADS), 0, s, occ, grid_shared ? (int64_t)0 : (int64_t)W * H, ws, sl.bytes, sl.bitmap);
  hipLaunchKernelGGL(rrt_edt_col_kernel, dim3((unsigned)B, (unsigned)((w1 + 63) / 64)), dim3(64), 0, s, ws, sl.bytes, sl);
  hipLaunchKernelGGL(rrt_edt_row_kernel, dim3((unsigned)B, (unsigned)((h1 + 63) / 64)), dim3(64), 0, s, ws, sl.bytes, sl,
                     (int64_t)p->max_cells, occ_d2, cost_grid);
  const size_t lds_tree = (size_t)rrt_lds_bytes(p->n_samples, p->max_cells);
  if (lds_tree > 64 * 1024 &&
      hipFuncSetAttribute((const void*)rrt_star_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_tree) != hipSuccess)
    return LIPMPC_E_HIP;
  hipLaunchKernelGGL(rrt_star_kernel, dim3((unsigned)B), dim3(RRT_THREADS), lds_tree, s, *p, seed, ws, sl.bytes, sl, S_max,
                     sub_goals, n_sub, status, path_cost, tree);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}
