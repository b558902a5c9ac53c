// lipmpc_field.hip -- the grid field planner (lipmpc_grid_field_batch, lipmpc_grid_path_batch, include/lipmpc.h): a complete,
// deterministic global planner on an occupancy grid.
//   grid_field_*_kernel  one workgroup per field: solid bytes -> bitmap, the bitmap dilated by the disc of r_inflate -> blocked
//                        bitmap, then the cost-to-go from the goal cell (axial 5, diagonal 7) by chaotic relaxation to the fixed
//                        point.  The field lives in LDS (sized to the map) when it fits beside the blocked bitmap, else in the
//                        output buffer itself.
//   grid_path_kernel     one lane per robot: snap, steepest descent down a field, sub-goals by string pulling.
// Everything the two kernels compare is an integer but the two floors that name a cell; the cell centres are one multiply and
// one add, contraction off.  tests/field_oracle.py restates both contracts (Dijkstra) and the GPU tests hold every output to it
// bit for bit.
//
// WHY RELAXATION GIVES DIJKSTRA'S FIELD.  Every value a cell ever holds is the cost of a real path to the goal, values only fall,
// and each cell has one owner, so a round of sweeps in which no thread lowered anything has read final values only: a fixed
// point of  f(c) = min over legal moves c -> n of f(n) + cost,  f(goal) = 0.  Its finite values are path costs, so >= the least
// cost; by induction along a least-cost path they are <= it.  The least cost is unique, hence the bits are whatever order the
// races fell in.  The diagonal rule is judged on the FIELD (both side cells finite) instead of the bitmap: a side cell of a legal
// diagonal is unblocked and an axial neighbour of n, so it is finite wherever n is once the sweeps have settled -- the same fixed
// point, and a sweep reads nine field words and one bit per cell.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lipmpc.h"

#pragma clang fp contract(off)

namespace {

constexpr int FIELD_THREADS = 1024;                 // one workgroup per field: 16 waves, two workgroups fill a CU
constexpr int PATH_THREADS = 64;
constexpr int MAX_SIDE = 4096;                      // the RRT planner's caps
constexpr int64_t MAX_CELLS = 1 << 17;
constexpr int64_t LDS_LIMIT = 160 * 1024;
constexpr int64_t LDS_SLACK = 256;                  // the workgroup reduction's own words
constexpr uint32_t INF = 0xFFFFFFFFu;
constexpr int R_INFLATE_MAX = 16;
constexpr uint32_t AXIAL = 5, DIAGONAL = 7;

// bitmap words of n cells: whole 64-cell ballots, + 2 so that a 64-bit window may start in the last word
__host__ __device__ inline int64_t bitmap_words(int64_t ncells) { return ((ncells + 63) / 64) * 2 + 2; }

// LDS of the field kernels: the blocked bitmap, then the field (whose first words hold the solid bitmap until the blocked one
// is made) -- or, with the field in global memory, the solid bitmap alone
__host__ __device__ inline int64_t field_lds_bytes(int64_t ncells, bool in_lds) {
  return 4 * (bitmap_words(ncells) + (in_lds ? ncells : bitmap_words(ncells)));
}

inline bool field_fits_lds(int64_t ncells) { return field_lds_bytes(ncells, true) + LDS_SLACK <= LDS_LIMIT; }

__device__ inline bool bit_of(const uint32_t* bm, int c) { return (bm[c >> 5] >> (c & 31)) & 1u; }

// the floor rule (the grid scan's robot cell); false for a cell outside the grid, NaN included
__device__ inline bool cell_of(double x, double y, double ox, double oy, double dx, double dy, int W, int H, int& i, int& j) {
  const double fi = floor((x - ox) / dx), fj = floor((y - oy) / dy);
  if (!(fi >= 0.0 && fi < (double)W && fj >= 0.0 && fj < (double)H)) return false;
  i = (int)fi;
  j = (int)fj;
  return true;
}

// relaxed accesses of workgroup scope: the sweeps race on purpose (a reader gets the old or the new word, both path costs)
template <typename P> __device__ inline uint32_t ld(P p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
template <typename P> __device__ inline void st(P p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// blockIdx.x = field.  `fld`: the field's working copy ([W*H], LDS or the output itself); `solid`: bitmap scratch, free to
// overlap fld; `blk`: the blocked bitmap.
template <bool COPY_OUT, typename FieldPtr>
__device__ inline void field_body(FieldPtr fld, uint32_t* solid, uint32_t* blk, int W, int H, int64_t occ_stride, double ox, double oy,
                                  double dx, double dy, const uint8_t* __restrict__ occ, const double* __restrict__ goal,
                                  int r_inflate, uint32_t* field_out, int32_t* __restrict__ field_status) {
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int ncells = W * H, words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  const uint8_t* oc = occ + f * occ_stride;
  uint32_t* out = field_out + f * (int64_t)ncells;

  // solid bytes -> bitmap words: a wave's ballot over 64 consecutive cells is a word pair
  for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
    const int c = c0 + lane;
    const uint64_t m = __ballot(c < ncells && oc[c] != 0);
    if (lane == 0) { solid[c0 >> 5] = (uint32_t)m; solid[(c0 >> 5) + 1] = (uint32_t)(m >> 32); }
  }
  if (tid < 2) { solid[words - 2 + tid] = 0; blk[words - 2 + tid] = 0; }
  __syncthreads();
  // blocked = solid dilated by the disc: per row i + di the cells j - w .. j + w, w = floor(sqrt(r^2 - di^2)), are at most 33
  // consecutive bits of the bitmap (layout i * H + j), one 64-bit window
  const int r2 = r_inflate * r_inflate;
  for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
    const int c = c0 + lane;
    bool b = false;
    if (c < ncells) {
      const int i = c / H, j = c - i * H;
      for (int di = -r_inflate; di <= r_inflate; ++di) {
        const int ii = i + di, rem = r2 - di * di;
        if (ii < 0 || ii >= W) continue;
        int w = (int)sqrtf((float)rem);
        while (w * w > rem) --w;
        while ((w + 1) * (w + 1) <= rem) ++w;
        const int lo = max(j - w, 0), hi = min(j + w, H - 1);
        const int c1 = ii * H + lo, n = hi - lo + 1;
        const uint64_t win = (((uint64_t)solid[(c1 >> 5) + 1] << 32) | solid[c1 >> 5]) >> (c1 & 31);
        b |= (win & ((1ull << n) - 1)) != 0;
      }
    }
    const uint64_t m = __ballot(b);
    if (lane == 0) { blk[c0 >> 5] = (uint32_t)m; blk[(c0 >> 5) + 1] = (uint32_t)(m >> 32); }
  }
  __syncthreads();                                    // (the solid bitmap is dead from here: the field may take its place)

  int gi = 0, gj = 0;
  const bool inside = cell_of(goal[2 * f], goal[2 * f + 1], ox, oy, dx, dy, W, H, gi, gj);
  const int gc = gi * H + gj;
  const int status = !inside ? LIPMPC_FIELD_GOAL_OUTSIDE : bit_of(blk, gc) ? LIPMPC_FIELD_GOAL_BLOCKED : LIPMPC_FIELD_OK;
  if (tid == 0) field_status[f] = status;
  if (status != LIPMPC_FIELD_OK) {
    for (int c = tid; c < ncells; c += FIELD_THREADS) out[c] = INF;
    return;
  }
  for (int c = tid; c < ncells; c += FIELD_THREADS) st(fld + c, c == gc ? 0u : INF);
  __syncthreads();

  // sweeps: thread t owns the cells t, t + T, ...; (i, j) advance by T = qi * H + rj without a division
  const int qi = FIELD_THREADS / H, rj = FIELD_THREADS - qi * H, i0 = tid / H, j0 = tid - i0 * H;
  for (;;) {
    int changed = 0;
    for (int c = tid, i = i0, j = j0; c < ncells; c += FIELD_THREADS) {
      if (!bit_of(blk, c)) {
        const bool up = i > 0, dn = i < W - 1, lf = j > 0, rt = j < H - 1;
        auto rd = [&](bool in, int n) { const uint32_t v = ld(fld + (in ? n : c)); return in ? v : INF; };
        const uint32_t cur = ld(fld + c);
        const uint32_t a_up = rd(up, c - H), a_dn = rd(dn, c + H), a_lf = rd(lf, c - 1), a_rt = rd(rt, c + 1);
        const uint32_t d_ul = rd(up & lf, c - H - 1), d_ur = rd(up & rt, c - H + 1);
        const uint32_t d_dl = rd(dn & lf, c + H - 1), d_dr = rd(dn & rt, c + H + 1);
        const bool p_up = a_up != INF, p_dn = a_dn != INF, p_lf = a_lf != INF, p_rt = a_rt != INF;
        const uint32_t ax = min(min(a_up, a_dn), min(a_lf, a_rt));
        const uint32_t dg = min(min(p_up & p_lf ? d_ul : INF, p_up & p_rt ? d_ur : INF),
                                min(p_dn & p_lf ? d_dl : INF, p_dn & p_rt ? d_dr : INF));
        // (a finite value is below 7 * 2^17: the additions cannot wrap)
        const uint32_t best = min(ax == INF ? INF : ax + AXIAL, dg == INF ? INF : dg + DIAGONAL);
        if (best < cur) { st(fld + c, best); changed = 1; }
      }
      i += qi; j += rj;
      if (j >= H) { j -= H; ++i; }
    }
    if (!__syncthreads_or(changed)) break;
  }
  if (COPY_OUT)
    for (int c = tid; c < ncells; c += FIELD_THREADS) out[c] = ld(fld + c);
}

__global__ void __launch_bounds__(FIELD_THREADS) grid_field_lds_kernel(int W, int H, int64_t occ_stride, double ox, double oy, double dx,
                                                                       double dy, const uint8_t* __restrict__ occ,
                                                                       const double* __restrict__ goal, int r_inflate,
                                                                       uint32_t* __restrict__ field, int32_t* __restrict__ field_status) {
  extern __shared__ uint32_t field_lds[];
  uint32_t* fld = field_lds + bitmap_words((int64_t)W * H);
  field_body<true>(fld, fld, field_lds, W, H, occ_stride, ox, oy, dx, dy, occ, goal, r_inflate, field, field_status);
}

__global__ void __launch_bounds__(FIELD_THREADS) grid_field_global_kernel(int W, int H, int64_t occ_stride, double ox, double oy, double dx,
                                                                          double dy, const uint8_t* __restrict__ occ,
                                                                          const double* __restrict__ goal, int r_inflate,
                                                                          uint32_t* field, int32_t* __restrict__ field_status) {
  extern __shared__ uint32_t field_lds[];
  uint32_t* fld = field + (int64_t)blockIdx.x * W * H;
  field_body<false>(fld, field_lds + bitmap_words((int64_t)W * H), field_lds, W, H, occ_stride, ox, oy, dx, dy, occ, goal, r_inflate, field,
             field_status);
}

// ---------------------------------------------------------------------------------------------------------------------
// the planner's segment rule on passable cells, walked incrementally (quotient and remainder per axis)
__device__ inline bool los(const uint32_t* __restrict__ fld, int H, int a, int b) {
  if (b < a) { const int t = a; a = b; b = t; }       // (index order i * H + j is the lexicographic order of (i, j))
  const int ai = a / H, aj = a - ai * H, bi = b / H, bj = b - bi * H;
  const int di = bi - ai, dj = bj - aj;
  const int m = max(abs(di), abs(dj)), two_m = 2 * m;
  if (m == 0) return fld[a] != INF;
  int qi = 0, ri = m, qj = 0, rj = m;
  for (int k = 0; k <= m; ++k) {
    if (fld[(ai + qi) * H + aj + qj] == INF) return false;
    ri += 2 * di; rj += 2 * dj;
    if (ri >= two_m) { ri -= two_m; ++qi; } else if (ri < 0) { ri += two_m; --qi; }
    if (rj >= two_m) { rj -= two_m; ++qj; } else if (rj < 0) { rj += two_m; --qj; }
  }
  return true;
}

// the descent's next cell: the first neighbour in the contract's order with field[n] + cost == field[c]; -1 if none (not a field)
__device__ inline int descend(const uint32_t* __restrict__ fld, int W, int H, int c) {
  const int i = c / H, j = c - i * H;
  const uint32_t fc = fld[c];
  for (int di = -1; di <= 1; ++di)
    for (int dj = -1; dj <= 1; ++dj) {
      if ((di == 0 && dj == 0) || (unsigned)(i + di) >= (unsigned)W || (unsigned)(j + dj) >= (unsigned)H) continue;
      const int n = c + di * H + dj;
      const uint32_t v = fld[n];
      if (v == INF) continue;
      const bool diag = di != 0 && dj != 0;
      if (diag && (fld[c + di * H] == INF || fld[c + dj] == INF)) continue;
      if (v < fc && fc - v == (diag ? DIAGONAL : AXIAL)) return n;
    }
  return -1;
}

// One lane per robot.
__global__ void __launch_bounds__(PATH_THREADS) grid_path_kernel(int64_t B, int one_field, int W, int H, int64_t occ_stride, double ox,
                                                                 double oy, double dx, double dy, const uint8_t* __restrict__ occ,
                                                                 const uint32_t* __restrict__ field,
                                                                 const int32_t* __restrict__ field_status,
                                                                 const double* __restrict__ goal, const double* __restrict__ start,
                                                                 int r_inflate, int max_seg, int S_max, double* __restrict__ sub_goals,
                                                                 int32_t* __restrict__ n_sub, int32_t* __restrict__ status,
                                                                 double* __restrict__ path_cost) {
  const int64_t b = (int64_t)blockIdx.x * PATH_THREADS + threadIdx.x;
  if (b >= B) return;
  const int64_t f = one_field ? 0 : b;
  const int ncells = W * H;
  const uint32_t* fld = field + f * (int64_t)ncells;
  auto done = [&](int st_, int n, double cost) { status[b] = st_; n_sub[b] = n; path_cost[b] = cost; };
  const double nan = __builtin_nan("");
  const int fs = field_status[f];
  if (fs == LIPMPC_FIELD_GOAL_OUTSIDE) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan);
  if (fs == LIPMPC_FIELD_GOAL_BLOCKED) return done(LIPMPC_RRT_GOAL_OCCUPIED, 0, nan);
  int si = 0, sj = 0;
  if (!cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj)) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan);
  int s = si * H + sj;
  if (occ[f * occ_stride + s] != 0) return done(LIPMPC_RRT_START_OCCUPIED, 0, nan);
  if (fld[s] == INF) {
    // snap: the finite cell of the window with the least (d^2, field, index); ascending index, so only a smaller pair replaces
    const int n = r_inflate + 1;
    uint64_t best = ~0ull;
    int at = -1;
    for (int i = max(si - n, 0); i <= min(si + n, W - 1); ++i)
      for (int j = max(sj - n, 0); j <= min(sj + n, H - 1); ++j) {
        const uint32_t v = fld[i * H + j];
        if (v == INF) continue;
        const uint64_t key = ((uint64_t)(uint32_t)((i - si) * (i - si) + (j - sj) * (j - sj)) << 32) | v;
        if (key < best) { best = key; at = i * H + j; }
      }
    if (at < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan);
    s = at;
  }
  double* sg = sub_goals + b * (int64_t)S_max * 2;
  // the walk, twice: count the sub-goals, then -- if they fit -- write them (rows past n_sub stay untouched)
  auto walk = [&](bool write) {
    int count = 0;
    auto emit = [&](int c) {
      if (write) {
        const int i = c / H, j = c - i * H;
        sg[2 * count] = ox + ((double)i + 0.5) * dx;
        sg[2 * count + 1] = oy + ((double)j + 0.5) * dy;
      }
      ++count;
    };
    if (fld[s] != 0) {
      int a = s, prev = s, cur = descend(fld, W, H, s);
      while (cur >= 0) {
        const bool last = fld[cur] == 0;
        if (!los(fld, H, a, cur) || fld[a] - fld[cur] >= (uint32_t)max_seg) {
          if (prev != a) { emit(prev); a = prev; continue; }          // cur is looked at again from the new anchor
          if (last) break;
          emit(cur); a = cur;
        }
        if (last) break;
        prev = cur;
        cur = descend(fld, W, H, cur);
      }
      if (cur < 0) return -1;
    }
    return count + 1;                                                 // + the goal itself
  };
  const int n = walk(false);
  if (n < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan);                 // (a `field` that is no cost-to-go field of this map)
  const double cost = (double)fld[s] / 5.0;
  if (n > S_max) return done(LIPMPC_RRT_PATH_OVERFLOW, 0, cost);
  walk(true);
  sg[2 * (n - 1)] = goal[2 * f];
  sg[2 * (n - 1) + 1] = goal[2 * f + 1];
  done(LIPMPC_RRT_FOUND, n, cost);
}

// what both entry points refuse about the grid: E_ARG, then the caps
int grid_refusal(int32_t W, int32_t H, const double* origin, const double* cell, int32_t r_inflate) {
  if (W < 2 || H < 2 || !origin || !cell || r_inflate < 0 || r_inflate > R_INFLATE_MAX) return LIPMPC_E_ARG;
  const double ox = origin[0], oy = origin[1], dx = cell[0], dy = cell[1];
  if (!(dx > 0.0) || !(dy > 0.0) || !(dx < INFINITY) || !(dy < INFINITY) || !(fabs(ox) < INFINITY) || !(fabs(oy) < INFINITY))
    return LIPMPC_E_ARG;
  if (W > MAX_SIDE || H > MAX_SIDE || (int64_t)W * H > MAX_CELLS) return LIPMPC_E_UNSUPPORTED;
  return LIPMPC_OK;
}

}  // namespace

extern "C" int lipmpc_grid_field_batch(int device, int64_t F, int32_t W, int32_t H, int32_t grid_shared, const double* origin,
                                       const double* cell, const uint8_t* occ, const double* goal, int32_t r_inflate,
                                       uint32_t* field, int32_t* field_status, void* hip_stream) {
  if (F < 0 || F > 0x7fffffff) return LIPMPC_E_ARG;
  if (const int rc = grid_refusal(W, H, origin, cell, r_inflate)) return rc;
  if (F == 0) return LIPMPC_OK;
  if (!occ || !goal || !field || !field_status) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t ncells = (int64_t)W * H, stride = grid_shared ? 0 : ncells;
  const bool in_lds = field_fits_lds(ncells);
  const size_t lds = (size_t)field_lds_bytes(ncells, in_lds);
  if (in_lds) {
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)grid_field_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds) != hipSuccess)
      return LIPMPC_E_HIP;
    hipLaunchKernelGGL(grid_field_lds_kernel, dim3((unsigned)F), dim3(FIELD_THREADS), lds, s, W, H, stride, origin[0], origin[1],
                       cell[0], cell[1], occ, goal, r_inflate, field, field_status);
  } else {
    hipLaunchKernelGGL(grid_field_global_kernel, dim3((unsigned)F), dim3(FIELD_THREADS), lds, s, W, H, stride, origin[0], origin[1],
                       cell[0], cell[1], occ, goal, r_inflate, field, field_status);
  }
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}

extern "C" int lipmpc_grid_path_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin, const double* cell,
                                      const uint8_t* occ, int32_t grid_shared, const uint32_t* field, const int32_t* field_status,
                                      const double* goal, const double* start, int32_t r_inflate, int32_t max_seg, int32_t S_max,
                                      double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, void* hip_stream) {
  if (B < 0 || B > 0x7fffffff || (F != 1 && F != B) || max_seg < 5 || S_max < 1) return LIPMPC_E_ARG;
  if (const int rc = grid_refusal(W, H, origin, cell, r_inflate)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (!occ || !field || !field_status || !goal || !start || !sub_goals || !n_sub || !status || !path_cost) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(grid_path_kernel, dim3((unsigned)((B + PATH_THREADS - 1) / PATH_THREADS)), dim3(PATH_THREADS), 0,
                     (hipStream_t)hip_stream, B, (int)(F == 1), W, H, grid_shared ? (int64_t)0 : (int64_t)W * H, origin[0], origin[1],
                     cell[0], cell[1], occ, field, field_status, goal, start, r_inflate, max_seg, S_max, sub_goals, n_sub, status,
                     path_cost);
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}
