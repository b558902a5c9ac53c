// lipmpc_field.hip -- the grid field planner (lipmpc_grid_field_batch, lipmpc_grid_path_batch, include/lipmpc.h): a complete,
// deterministic global planner on an occupancy grid.
//   grid_field_*_kernel  one workgroup per field: solid bytes -> bitmap, the bitmap dilated by the disc of r_inflate -> blocked
//                        bitmap, then the cost-to-go from the goal cell (axial 5, diagonal 7) by chaotic relaxation to the fixed
//                        point.  The field lives in LDS (sized to the map) when it fits beside the blocked bitmap, else in the
//                        output buffer itself.
//   grid_path_kernel     one lane per robot: snap, steepest descent down a field, sub-goals by string pulling.
// and the frontier explorer (lipmpc_grid_frontier_field_batch, lipmpc_grid_frontier_path_batch) on an evidence grid:
//   frontier_field_*_kernel  one workgroup per map: evidence -> solid and unknown bitmaps, blocked = unknown | solid dilated,
//                            frontier = unblocked with enough unknown neighbours, then the same relaxation from EVERY frontier
//                            cell at once: the cost-to-go to the nearest frontier.
//   frontier_path_kernel     grid_path_kernel's snap, descent and string pulling, ending at the first frontier cell reached.
//   frontier_assign_*_kernel ONE workgroup for a fleet on a shared map (lipmpc_grid_frontier_assign_batch): round by round the
//                            relaxation from what is left of the frontier, the nearest robot's claim and path, its disc cleared.
// and the informed explorer (lipmpc_grid_frontier_gain_batch, lipmpc_grid_frontier_utility_field_batch,
// lipmpc_grid_frontier_utility_path_batch):
//   frontier_gain_kernel          a wave per frontier cell, a lane per ray of the fan: the distinct unknown cells seen from it.
//   frontier_utility_*_kernel     one workgroup per map: the same relaxation from sources that start at a gain-dependent seed.
//   frontier_utility_path_kernel  frontier_path_kernel down that field, ending at the first source that holds its own seed.
// and the same two fields on LARGE maps (lipmpc_grid_field_tiled_batch, lipmpc_grid_frontier_field_tiled_batch and their path calls),
// at the end of this file:
//   tiled_*_kernel                set-up by many workgroups, then ROUNDS of one workgroup per (field, tile) that relax a tile in LDS with
//                                 a one-cell halo held, ordered by kernel boundaries alone; the path kernels with one more rule in front.
// and the informed and the coordinated explorer on LARGE maps (lipmpc_grid_frontier_gain_tiled_batch,
// lipmpc_grid_frontier_utility_field_tiled_batch, lipmpc_grid_frontier_utility_path_tiled_batch,
// lipmpc_grid_frontier_assign_tiled_batch), after them:
//   tile_gain_kernel              one workgroup per (map, tile): the fan against bitmaps of the tile grown by r_view.
//   tile_utility_*_kernel         the utility field's seeds for the rounds above; the path kernel with one more rule in front.
//   claim_*_kernel                frontier_assign_*_kernel's rounds cut into kernels, each round's field relaxed by the rounds above.
// and soft clearance (lipmpc_grid_clearance_cost_batch, lipmpc_grid_field_weighted_batch, lipmpc_grid_frontier_field_weighted_batch
// and their path calls), at the very end:
//   soft_cost_kernel              one workgroup per (map, tile): a byte per cell that decays with the distance to the nearest solid cell.
//   soft_round_kernel             the tiled round with that byte added to what a cell takes; soft_*_descent_kernel walk down such a field.
// Everything the kernels compare is an integer but the two floors that name a cell; the cell centres are one multiply and
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
// SEVERAL SOURCES change nothing in that argument: with f(s) = 0 on every frontier cell s, a value is the cost of a real path to
// SOME source, the fixed point's finite values are >= the least cost to any source and, along a least-cost path to the nearest
// one, <= it.  The frontier field is as unique as the goal field, whatever order the races fell in.
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
constexpr int THRESHOLD_MAX = 1 << 30;                // of the frontier calls' t_free and t_occ: -t_free is an int32
constexpr uint32_t AXIAL = 5, DIAGONAL = 7;

// bitmap words of n cells: whole 64-cell ballots, + 2 so that a 64-bit window may start in the last word
__host__ __device__ inline int64_t bitmap_words(int64_t ncells) { return ((ncells + 63) / 64) * 2 + 2; }

// LDS of the field kernels: the blocked bitmap, then the field (whose first words hold the solid bitmap until the blocked one
// is made) -- or, with the field in global memory, the solid bitmap alone
__host__ __device__ inline int64_t field_lds_bytes(int64_t ncells, bool in_lds) {
  return 4 * (bitmap_words(ncells) + (in_lds ? ncells : bitmap_words(ncells)));
}

inline bool field_fits_lds(int64_t ncells) { return field_lds_bytes(ncells, true) + LDS_SLACK <= LDS_LIMIT; }

// LDS of the frontier field kernels: three bitmaps (blocked, solid, unknown: the frontier test reads the last two while the
// field is seeded, so the field does not take their place), the frontier count (a word pair: the field stays 8-byte aligned),
// then the field -- or bitmaps and count alone
__host__ __device__ inline int64_t frontier_bitmap_words(int64_t ncells) { return 3 * bitmap_words(ncells) + 2; }
__host__ __device__ inline int64_t frontier_lds_bytes(int64_t ncells, bool in_lds) {
  return 4 * (frontier_bitmap_words(ncells) + (in_lds ? ncells : 0));
}

inline bool frontier_fits_lds(int64_t ncells) { return frontier_lds_bytes(ncells, true) + LDS_SLACK <= LDS_LIMIT; }

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

// 64 bits of a bitmap from cell c on (layout i * H + j; a bitmap has two spare words, so the pair is always inside)
__device__ inline uint64_t window(const uint32_t* bm, int c) { return (((uint64_t)bm[(c >> 5) + 1] << 32) | bm[c >> 5]) >> (c & 31); }

// some solid cell of the grid within the disc of r_inflate around (i, j): per row i + di the cells j - w .. j + w,
// w = floor(sqrt(r^2 - di^2)), are at most 33 consecutive bits of the bitmap, one 64-bit window
__device__ inline bool disc_hits(const uint32_t* solid, int W, int H, int i, int j, int r_inflate) {
  const int r2 = r_inflate * r_inflate;
  bool b = false;
  for (int di = -r_inflate; di <= r_inflate; ++di) {
    const int ii = i + di, rem = r2 - di * di;
    if (ii < 0 || ii >= W) continue;
    int w = (int)sqrtf((float)rem);
    while (w * w > rem) --w;
    while ((w + 1) * (w + 1) <= rem) ++w;
    const int lo = max(j - w, 0), hi = min(j + w, H - 1);
    b |= (window(solid, ii * H + lo) & ((1ull << (hi - lo + 1)) - 1)) != 0;
  }
  return b;
}

// the sweeps, from a field that holds 0 on its sources and INF elsewhere, to the fixed point: thread t owns the cells t, t + T,
// ...; (i, j) advance by T = qi * H + rj without a division
template <typename FieldPtr> __device__ inline void relax(FieldPtr fld, const uint32_t* blk, int W, int H) {
  const int tid = threadIdx.x, ncells = W * H;
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
}

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
  // blocked = solid dilated by the disc
  for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
    const int c = c0 + lane;
    bool b = false;
    if (c < ncells) {
      const int i = c / H, j = c - i * H;
      b = disc_hits(solid, W, H, i, j, r_inflate);
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

  relax(fld, blk, W, H);
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
// blockIdx.x = map.  `fld`: the field's working copy ([W*H], LDS or the output itself); `bm`: three bitmaps and the count's
// word, apart from fld.
template <bool COPY_OUT, typename FieldPtr>
__device__ inline void frontier_body(FieldPtr fld, uint32_t* bm, int W, int H, const int32_t* __restrict__ evidence, int t_free,
                                     int t_occ, int r_inflate, int min_unknown, uint8_t* __restrict__ frontier, uint32_t* field_out,
                                     int32_t* __restrict__ n_frontier) {
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int ncells = W * H, words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  uint32_t *blk = bm, *solid = bm + words, *unk = bm + 2 * words, *n_front = bm + 3 * words;
  const int32_t* ev = evidence + f * (int64_t)ncells;
  uint32_t* out = field_out + f * (int64_t)ncells;
  uint8_t* fr_out = frontier ? frontier + f * (int64_t)ncells : nullptr;

  // evidence -> solid and unknown bitmaps (t_free, t_occ >= 1: the two plain comparisons hold for every int32, and never both)
  for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
    const int c = c0 + lane;
    const int e = c < ncells ? ev[c] : 0;
    const bool is_solid = c < ncells && e >= t_occ, is_free = e <= -t_free;
    const uint64_t ms = __ballot(is_solid), mu = __ballot(c < ncells && !is_solid && !is_free);
    if (lane == 0) {
      solid[c0 >> 5] = (uint32_t)ms; solid[(c0 >> 5) + 1] = (uint32_t)(ms >> 32);
      unk[c0 >> 5] = (uint32_t)mu; unk[(c0 >> 5) + 1] = (uint32_t)(mu >> 32);
    }
  }
  if (tid < 2) { solid[words - 2 + tid] = 0; unk[words - 2 + tid] = 0; blk[words - 2 + tid] = 0; }
  if (tid == 0) *n_front = 0;
  __syncthreads();
  // blocked = not free, or within the disc of a solid cell = unknown | solid dilated (the disc holds its own centre)
  for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
    const int c = c0 + lane;
    bool b = false;
    if (c < ncells) {
      const int i = c / H, j = c - i * H;
      b = bit_of(unk, c) | disc_hits(solid, W, H, i, j, r_inflate);
    }
    const uint64_t m = __ballot(b);
    if (lane == 0) { blk[c0 >> 5] = (uint32_t)m; blk[(c0 >> 5) + 1] = (uint32_t)(m >> 32); }
  }
  __syncthreads();
  // frontier = unblocked with >= min_unknown unknown cells among the neighbours inside the grid: per row i - 1, i, i + 1 the
  // cells j - 1 .. j + 1, clipped to the row, are up to three bits of one window (the cell itself is unblocked, so not unknown).
  // Every frontier cell is a source of the field.
  int mine = 0;
  for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
    const int c = c0 + lane;
    bool fr = false;
    if (c < ncells) {
      if (!bit_of(blk, c)) {
        const int i = c / H, j = c - i * H;
        const int lo = max(j - 1, 0), hi = min(j + 1, H - 1);
        const uint64_t mask = (1ull << (hi - lo + 1)) - 1;
        int cnt = __popcll(window(unk, c - j + lo) & mask);
        if (i > 0) cnt += __popcll(window(unk, c - H - j + lo) & mask);
        if (i < W - 1) cnt += __popcll(window(unk, c + H - j + lo) & mask);
        fr = cnt >= min_unknown;
      }
      st(fld + c, fr ? 0u : INF);
      if (fr_out) fr_out[c] = fr;
    }
    mine += __popcll(__ballot(fr));
  }
  if (lane == 0 && mine) atomicAdd(n_front, (uint32_t)mine);     // (integers: the sum is the same in any order)
  __syncthreads();
  const int n = (int)*n_front;
  if (tid == 0) n_frontier[f] = n;
  if (n) relax(fld, blk, W, H);                          // (no frontier: the field is INF as it stands)
  if (COPY_OUT)
    for (int c = tid; c < ncells; c += FIELD_THREADS) out[c] = ld(fld + c);
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_field_lds_kernel(int W, int H, const int32_t* __restrict__ evidence, int t_free,
                                                                           int t_occ, int r_inflate, int min_unknown,
                                                                           uint8_t* __restrict__ frontier, uint32_t* __restrict__ field,
                                                                           int32_t* __restrict__ n_frontier) {
  extern __shared__ uint32_t field_lds[];
  frontier_body<true>(field_lds + frontier_bitmap_words((int64_t)W * H), field_lds, W, H, evidence, t_free, t_occ, r_inflate, min_unknown,
                      frontier, field, n_frontier);
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_field_global_kernel(int W, int H, const int32_t* __restrict__ evidence,
                                                                              int t_free, int t_occ, int r_inflate, int min_unknown,
                                                                              uint8_t* __restrict__ frontier, uint32_t* field,
                                                                              int32_t* __restrict__ n_frontier) {
  extern __shared__ uint32_t field_lds[];
  frontier_body<false>(field + (int64_t)blockIdx.x * W * H, field_lds, W, H, evidence, t_free, t_occ, r_inflate, min_unknown, frontier,
                       field, n_frontier);
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

// snap: the finite cell of the window round (si, sj) with the least (d^2, field, index); ascending index, so only a smaller pair
// replaces; -1 if the window has none
__device__ inline int snap(const uint32_t* __restrict__ fld, int W, int H, int si, int sj, int r_inflate) {
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
  return at;
}

__device__ inline void centre(int c, int H, double ox, double oy, double dx, double dy, double* p) {
  const int i = c / H, j = c - i * H;
  p[0] = ox + ((double)i + 0.5) * dx;
  p[1] = oy + ((double)j + 0.5) * dy;
}

// the walk from s down the field to the first cell whose field is 0 (`last`): the number of sub-goals, that cell's included (its
// row is the caller's to write), or -1 where no neighbour satisfies the descent.  `sg`: where to write them, or null to count.
__device__ inline int walk(const uint32_t* __restrict__ fld, int W, int H, int s, int max_seg, double ox, double oy, double dx, double dy,
                           double* sg, int& last_cell) {
  int count = 0;
  auto emit = [&](int c) {
    if (sg) centre(c, H, ox, oy, dx, dy, sg + 2 * count);
    ++count;
  };
  last_cell = s;
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
    last_cell = cur;
  }
  return count + 1;
}

// (the weighted walk of SOFT CLEARANCE, below)
__device__ inline int soft_walk(const uint32_t* __restrict__ fld, const uint8_t* __restrict__ kc, int W, int H, int s, int max_seg,
                                double ox, double oy, double dx, double dy, double* sg, int& last_cell);

// One lane per robot.  `settled`: null, or the tiled field calls' word per field -- a robot whose field is not settled gets
// LIPMPC_RRT_FIELD_UNSETTLED before any other rule.  WEIGHTED: the walk is soft_walk() down a weighted field, on the cost layer
// `cost` (shared exactly when the map is); else `cost` is not read.
template <bool WEIGHTED>
__device__ __forceinline__ void grid_path_body(int64_t B, int one_field, int W, int H, int64_t occ_stride, double ox, double oy, double dx,
                                               double dy, const uint8_t* __restrict__ occ, const uint8_t* __restrict__ cost,
                                               const uint32_t* __restrict__ field,
                                               const int32_t* __restrict__ field_status, const int32_t* __restrict__ settled,
                                               const double* __restrict__ goal, const double* __restrict__ start, int r_inflate,
                                               int max_seg, int S_max, double* __restrict__ sub_goals, int32_t* __restrict__ n_sub,
                                               int32_t* __restrict__ status, double* __restrict__ path_cost) {
  const int64_t b = (int64_t)blockIdx.x * PATH_THREADS + threadIdx.x;
  if (b >= B) return;
  const int64_t f = one_field ? 0 : b;
  const int ncells = W * H;
  const uint32_t* fld = field + f * (int64_t)ncells;
  const uint8_t* kc = WEIGHTED ? cost + f * occ_stride : nullptr;   // (the layer is shared exactly when the map is)
  auto done = [&](int st_, int n, double c) { status[b] = st_; n_sub[b] = n; path_cost[b] = c; };
  const double nan = __builtin_nan("");
  if ((WEIGHTED || settled) && settled[f] == 0) return done(LIPMPC_RRT_FIELD_UNSETTLED, 0, nan);       // (a weighted field has the word)
  const int fs = field_status[f];
  if (fs == LIPMPC_FIELD_GOAL_OUTSIDE) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan);
  if (fs == LIPMPC_FIELD_GOAL_BLOCKED) return done(LIPMPC_RRT_GOAL_OCCUPIED, 0, nan);
  int si = 0, sj = 0;
  if (!cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj)) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan);
  int s = si * H + sj;
  if (occ[f * occ_stride + s] != 0) return done(LIPMPC_RRT_START_OCCUPIED, 0, nan);
  if (fld[s] == INF) s = snap(fld, W, H, si, sj, r_inflate);
  if (s < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan);
  double* sg = sub_goals + b * (int64_t)S_max * 2;
  // the walk, twice: count the sub-goals, then -- if they fit -- write them (rows past n_sub stay untouched)
  int last_cell;
  int n;
  if constexpr (WEIGHTED) n = soft_walk(fld, kc, W, H, s, max_seg, ox, oy, dx, dy, nullptr, last_cell);
  else n = walk(fld, W, H, s, max_seg, ox, oy, dx, dy, nullptr, last_cell);
  if (n < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan);                 // (a `field` that is no cost-to-go field of this map and layer)
  const double total = (double)fld[s] / 5.0;                          // penalties included
  if (n > S_max) return done(LIPMPC_RRT_PATH_OVERFLOW, 0, total);
  if constexpr (WEIGHTED) soft_walk(fld, kc, W, H, s, max_seg, ox, oy, dx, dy, sg, last_cell);
  else walk(fld, W, H, s, max_seg, ox, oy, dx, dy, sg, last_cell);
  sg[2 * (n - 1)] = goal[2 * f];                                      // the goal itself, not its cell's centre
  sg[2 * (n - 1) + 1] = goal[2 * f + 1];
  done(LIPMPC_RRT_FOUND, n, total);
}

__global__ void __launch_bounds__(PATH_THREADS) grid_path_kernel(int64_t B, int one_field, int W, int H, int64_t occ_stride, double ox,
                                                                 double oy, double dx, double dy, const uint8_t* __restrict__ occ,
                                                                 const uint32_t* __restrict__ field,
                                                                 const int32_t* __restrict__ field_status,
                                                                 const double* __restrict__ goal, const double* __restrict__ start,
                                                                 int r_inflate, int max_seg, int S_max, double* __restrict__ sub_goals,
                                                                 int32_t* __restrict__ n_sub, int32_t* __restrict__ status,
                                                                 double* __restrict__ path_cost) {
  grid_path_body<false>(B, one_field, W, H, occ_stride, ox, oy, dx, dy, occ, nullptr, field, field_status, nullptr, goal, start, r_inflate,
                        max_seg, S_max, sub_goals, n_sub, status, path_cost);
}

// One lane per robot: grid_path_kernel down a frontier field, to the centre of the first frontier cell reached.  `settled`: as
// grid_path_body's, and so are WEIGHTED and `cost` (a layer per field).
template <bool WEIGHTED>
__device__ __forceinline__ void frontier_path_body(int64_t B, int one_field, int W, int H, double ox, double oy, double dx, double dy,
                                                   const int32_t* __restrict__ evidence, const uint8_t* __restrict__ cost, int t_occ,
                                                   const uint32_t* __restrict__ field,
                                                   const int32_t* __restrict__ n_frontier, const int32_t* __restrict__ settled,
                                                   const double* __restrict__ start, int r_inflate, int max_seg, int S_max,
                                                   double* __restrict__ sub_goals, int32_t* __restrict__ n_sub,
                                                   int32_t* __restrict__ status, double* __restrict__ path_cost,
                                                   int32_t* __restrict__ target_cell) {
  const int64_t b = (int64_t)blockIdx.x * PATH_THREADS + threadIdx.x;
  if (b >= B) return;
  const int64_t f = one_field ? 0 : b;
  const int ncells = W * H;
  const uint32_t* fld = field + f * (int64_t)ncells;
  auto done = [&](int st_, int n, double c, int target) { status[b] = st_; n_sub[b] = n; path_cost[b] = c; target_cell[b] = target; };
  const double nan = __builtin_nan("");
  if ((WEIGHTED || settled) && settled[f] == 0) return done(LIPMPC_RRT_FIELD_UNSETTLED, 0, nan, -1);
  int si = 0, sj = 0;
  if (!cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj)) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan, -1);
  int s = si * H + sj;
  if (evidence[f * (int64_t)ncells + s] >= t_occ) return done(LIPMPC_RRT_START_OCCUPIED, 0, nan, -1);
  if (n_frontier[f] == 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);
  if (fld[s] == INF) s = snap(fld, W, H, si, sj, r_inflate);
  if (s < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);
  double* sg = sub_goals + b * (int64_t)S_max * 2;
  int last_cell;
  int n;
  if constexpr (WEIGHTED) n = soft_walk(fld, cost + f * (int64_t)ncells, W, H, s, max_seg, ox, oy, dx, dy, nullptr, last_cell);
  else n = walk(fld, W, H, s, max_seg, ox, oy, dx, dy, nullptr, last_cell);
  if (n < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);             // (a `field` that is no frontier field of this map and layer)
  const double total = (double)fld[s] / 5.0;                          // penalties included
  if (n > S_max) return done(LIPMPC_RRT_PATH_OVERFLOW, 0, total, last_cell);
  if constexpr (WEIGHTED) soft_walk(fld, cost + f * (int64_t)ncells, W, H, s, max_seg, ox, oy, dx, dy, sg, last_cell);
  else walk(fld, W, H, s, max_seg, ox, oy, dx, dy, sg, last_cell);
  centre(last_cell, H, ox, oy, dx, dy, sg + 2 * (n - 1));
  done(LIPMPC_RRT_FOUND, n, total, last_cell);
}

__global__ void __launch_bounds__(PATH_THREADS) frontier_path_kernel(int64_t B, int one_field, int W, int H, double ox, double oy, double dx,
                                                                     double dy, const int32_t* __restrict__ evidence, int t_occ,
                                                                     const uint32_t* __restrict__ field,
                                                                     const int32_t* __restrict__ n_frontier,
                                                                     const double* __restrict__ start, int r_inflate, int max_seg,
                                                                     int S_max, double* __restrict__ sub_goals, int32_t* __restrict__ n_sub,
                                                                     int32_t* __restrict__ status, double* __restrict__ path_cost,
                                                                     int32_t* __restrict__ target_cell) {
  frontier_path_body<false>(B, one_field, W, H, ox, oy, dx, dy, evidence, nullptr, t_occ, field, n_frontier, nullptr, start, r_inflate,
                            max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell);
}

// ---------------------------------------------------------------------------------------------------------------------
// the coordinated claim (lipmpc_grid_frontier_assign_batch): ONE workgroup for the whole call, a sequential round per claim.
// Its field is relaxed anew every round, in LDS or in `work`, so the path functions above come once more in a form that takes
// whatever pointer the field lives behind and reads it with the sweeps' own loads: the same rules, word for word.
template <typename FieldPtr> __device__ __forceinline__ bool los_in(FieldPtr fld, int H, int a, int b) {
  if (b < a) { const int t = a; a = b; b = t; }
  const int ai = a / H, aj = a - ai * H, bi = b / H, bj = b - bi * H;
  const int di = bi - ai, dj = bj - aj;
  const int m = max(abs(di), abs(dj)), two_m = 2 * m;
  if (m == 0) return ld(fld + a) != INF;
  int qi = 0, ri = m, qj = 0, rj = m;
  for (int k = 0; k <= m; ++k) {
    if (ld(fld + ((ai + qi) * H + aj + qj)) == INF) return false;
    ri += 2 * di; rj += 2 * dj;
    if (ri >= two_m) { ri -= two_m; ++qi; } else if (ri < 0) { ri += two_m; --qi; }
    if (rj >= two_m) { rj -= two_m; ++qj; } else if (rj < 0) { rj += two_m; --qj; }
  }
  return true;
}

template <typename FieldPtr> __device__ __forceinline__ int descend_in(FieldPtr fld, int W, int H, int c) {
  const int i = c / H, j = c - i * H;
  const uint32_t fc = ld(fld + c);
  // (not unrolled: eight neighbours' conditions at once fill the scalar file, and one lane walks)
#pragma unroll 1
  for (int di = -1; di <= 1; ++di)
#pragma unroll 1
    for (int dj = -1; dj <= 1; ++dj) {
      if ((di == 0 && dj == 0) || (unsigned)(i + di) >= (unsigned)W || (unsigned)(j + dj) >= (unsigned)H) continue;
      const int n = c + di * H + dj;
      const uint32_t v = ld(fld + n);
      if (v == INF) continue;
      const bool diag = di != 0 && dj != 0;
      if (diag && (ld(fld + (c + di * H)) == INF || ld(fld + (c + dj)) == INF)) continue;
      if (v < fc && fc - v == (diag ? DIAGONAL : AXIAL)) return n;
    }
  return -1;
}

template <typename FieldPtr> __device__ __forceinline__ int snap_in(FieldPtr fld, int W, int H, int si, int sj, int r_inflate) {
  const int n = r_inflate + 1;
  uint64_t best = ~0ull;
  int at = -1;
  for (int i = max(si - n, 0); i <= min(si + n, W - 1); ++i)
    for (int j = max(sj - n, 0); j <= min(sj + n, H - 1); ++j) {
      const uint32_t v = ld(fld + (i * H + j));
      if (v == INF) continue;
      const uint64_t key = ((uint64_t)(uint32_t)((i - si) * (i - si) + (j - sj) * (j - sj)) << 32) | v;
      if (key < best) { best = key; at = i * H + j; }
    }
  return at;
}

template <typename FieldPtr>
__device__ __forceinline__ int walk_in(FieldPtr fld, int W, int H, int s, int max_seg, double ox, double oy, double dx, double dy, double* sg,
                              int& last_cell) {
  int count = 0;
  auto emit = [&](int c) {
    if (sg) centre(c, H, ox, oy, dx, dy, sg + 2 * count);
    ++count;
  };
  last_cell = s;
  if (ld(fld + s) != 0) {
    int a = s, prev = s, cur = descend_in(fld, W, H, s);
    while (cur >= 0) {
      const bool last = ld(fld + cur) == 0;
      if (!los_in(fld, H, a, cur) || ld(fld + a) - ld(fld + cur) >= (uint32_t)max_seg) {
        if (prev != a) { emit(prev); a = prev; continue; }
        if (last) break;
        emit(cur); a = cur;
      }
      if (last) break;
      prev = cur;
      cur = descend_in(fld, W, H, cur);
    }
    if (cur < 0) return -1;
    last_cell = cur;
  }
  return count + 1;
}

// LDS of the assign kernels: two bitmaps (impassable, sources), then ASSIGN_WORDS words -- the winner's key (64 bits: 2
// bitmap_words() is even, so it is 8-byte aligned), the winner's target cell (a word pair), and what only the winner's lane needs,
// the placement's four doubles and the five pointers of its output rows: held in scalar registers through every loop of the
// rounds they would overfill that file (the bar is no spill of either kind); the lane that walks reads them from here -- then
// the field (8-byte aligned), or bitmaps and words alone with the field in `work`
constexpr int ASSIGN_WORDS = 22;
__host__ __device__ inline int64_t assign_bitmap_words(int64_t ncells) { return 2 * bitmap_words(ncells) + ASSIGN_WORDS; }
__host__ __device__ inline int64_t assign_lds_bytes(int64_t ncells, bool in_lds) {
  return 4 * (assign_bitmap_words(ncells) + (in_lds ? ncells : 0));
}

inline bool assign_fits_lds(int64_t ncells) { return assign_lds_bytes(ncells, true) + LDS_SLACK <= LDS_LIMIT; }

// where a robot whose start cell is (si, sj) enters the round's field: that cell if finite there, else the snap; -1 if neither
template <typename FieldPtr> __device__ __forceinline__ int claim_cell(FieldPtr fld, int W, int H, int cell, int r_inflate) {
  if (ld(fld + cell) != INF) return cell;
  const int si = cell / H;
  return snap_in(fld, W, H, si, cell - si * H, r_inflate);
}

// The whole call.  `fld`: the round's field ([W*H], LDS or `work`); `bm`: the two bitmaps and the ASSIGN_WORDS, apart from fld.
// While the rounds run, claim_round[b] of a robot of U holds -2 - (its start cell): the floor rule's two divisions are done once
// and a round reads one word per robot.  It is read back after the winner's lane wrote it: every barrier orders the workgroup's
// global accesses.
template <typename FieldPtr>
__device__ __forceinline__ void assign_body(FieldPtr fld, uint32_t* bm, int64_t B, int W, int H, double ox, double oy, double dx, double dy,
                                            const uint8_t* __restrict__ frontier, const uint32_t* __restrict__ field,
                                            const double* __restrict__ start, const int8_t* __restrict__ may_claim, int r_inflate,
                                            int r_claim, int max_claims, int max_seg, int S_max, double* __restrict__ sub_goals,
                                            int32_t* __restrict__ n_sub, int32_t* __restrict__ status, double* __restrict__ path_cost,
                                            int32_t* __restrict__ target_cell, int32_t* claim_round, int32_t* __restrict__ n_claims) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int ncells = W * H, words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  uint32_t *blk = bm, *src = bm + words, *tgt = bm + 2 * words + 2;
  unsigned long long* key = (unsigned long long*)(bm + 2 * words);
  uint32_t* parked = bm + 2 * words + 4;                  // 64-bit values as word pairs
  auto park = [&](int slot, unsigned long long v) { parked[2 * slot] = (uint32_t)v; parked[2 * slot + 1] = (uint32_t)(v >> 32); };
  auto unpark = [&](int slot) { return ((unsigned long long)parked[2 * slot + 1] << 32) | parked[2 * slot]; };

  // U_0, each robot with its start cell
  for (int64_t b = tid; b < B; b += FIELD_THREADS) {
    const int sb = status[b];
    int si = 0, sj = 0, v = -1;
    if (max_claims > 0 && (sb == LIPMPC_RRT_FOUND || sb == LIPMPC_RRT_PATH_OVERFLOW) && (!may_claim || may_claim[b]) &&
        cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj))
      v = -2 - (si * H + sj);
    claim_round[b] = v;
  }
  int claims = 0;
  if (max_claims > 0) {
    // impassable = the given field is INF; sources = the given frontier, on passable cells
    for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
      const int c = c0 + lane;
      const bool pass = c < ncells && field[c] != INF;
      const uint64_t mb = __ballot(c < ncells && !pass), ms = __ballot(pass && frontier[c] != 0);
      if (lane == 0) {
        blk[c0 >> 5] = (uint32_t)mb; blk[(c0 >> 5) + 1] = (uint32_t)(mb >> 32);
        src[c0 >> 5] = (uint32_t)ms; src[(c0 >> 5) + 1] = (uint32_t)(ms >> 32);
      }
    }
    if (tid < 2) { blk[words - 2 + tid] = 0; src[words - 2 + tid] = 0; }
    if (tid == 0) {
      *key = ~0ull;
      park(0, __double_as_longlong(ox)); park(1, __double_as_longlong(oy)); park(2, __double_as_longlong(dx));
      park(3, __double_as_longlong(dy));
      park(4, (unsigned long long)sub_goals); park(5, (unsigned long long)n_sub); park(6, (unsigned long long)status);
      park(7, (unsigned long long)path_cost); park(8, (unsigned long long)target_cell);
    }
    __syncthreads();

    for (int k = 0;; ++k) {
      // field_k: 0 on what is left of the sources, relaxed to the fixed point
      int any = 0;
      for (int c = tid; c < ncells; c += FIELD_THREADS) {
        const bool s = bit_of(src, c);
        st(fld + c, s ? 0u : INF);
        any |= s;
      }
      if (!__syncthreads_or(any)) break;
      relax(fld, blk, W, H);
      // the candidates of U_k, and the least (cost, b) among them
      unsigned long long mine = ~0ull;
      int eligible = 0;
      for (int64_t b = tid; b < B; b += FIELD_THREADS) {
        const int v = claim_round[b];
        if (v > -2) continue;
        ++eligible;
        const int s = claim_cell(fld, W, H, -2 - v, r_inflate);
        if (s >= 0) mine = min(mine, ((unsigned long long)ld(fld + s) << 32) | (unsigned long long)b);
      }
      for (int o = 32; o; o >>= 1) mine = min(mine, (unsigned long long)__shfl_xor(mine, o));
      if (lane == 0 && mine != ~0ull) atomicMin(key, mine);
      __syncthreads();
      const unsigned long long win = *key;
      if (win == ~0ull) break;                            // no candidate: the rounds end
      const int64_t wb = (int64_t)(win & 0xFFFFFFFFull);
      if (tid == 0) {
        // one lane walks the winner's path, twice: count, then -- if the sub-goals fit -- write (rows past n_sub stay untouched)
        const int s = claim_cell(fld, W, H, -2 - claim_round[wb], r_inflate);
        const double wox = __longlong_as_double(unpark(0)), woy = __longlong_as_double(unpark(1));
        const double wdx = __longlong_as_double(unpark(2)), wdy = __longlong_as_double(unpark(3));
        double* sg = (double*)unpark(4) + wb * (int64_t)S_max * 2;
        int last_cell = s, n = 0;
        for (int pass = 0; pass < 2 && n >= 0 && n <= S_max; ++pass)
          n = walk_in(fld, W, H, s, max_seg, wox, woy, wdx, wdy, pass ? sg : nullptr, last_cell);
        if (n > 0) {
          if (n <= S_max) centre(last_cell, H, wox, woy, wdx, wdy, sg + 2 * (n - 1));
          ((int32_t*)unpark(6))[wb] = n <= S_max ? LIPMPC_RRT_FOUND : LIPMPC_RRT_PATH_OVERFLOW;
          ((int32_t*)unpark(5))[wb] = n <= S_max ? n : 0;
          ((double*)unpark(7))[wb] = (double)ld(fld + s) / 5.0;
          ((int32_t*)unpark(8))[wb] = last_cell;
          claim_round[wb] = k;
        }
        *tgt = n > 0 ? (uint32_t)last_cell : INF;         // (a fixed point always has a descent: INF cannot happen)
      }
      if ((wb & (FIELD_THREADS - 1)) == tid) --eligible;
      const int more = __syncthreads_or(eligible);
      const uint32_t t = *tgt;
      if (tid == 0) *key = ~0ull;                         // (everybody has read it; the next minimum comes two barriers on)
      if (t == INF) break;
      ++claims;
      if (!more || k + 1 >= max_claims) break;            // U or the allowance is used up
      // S_{k+1}: the sources outside the winner's disc, clipped to the grid
      const int ti = (int)t / H, tj = (int)t - ti * H, r2 = r_claim * r_claim;
      const int i_lo = max(ti - r_claim, 0), i_hi = min(ti + r_claim, W - 1);
      for (int c = i_lo * H + tid; c < (i_hi + 1) * H; c += FIELD_THREADS) {
        const int i = c / H, j = c - i * H;
        if (bit_of(src, c) && (i - ti) * (i - ti) + (j - tj) * (j - tj) <= r2) atomicAnd(src + (c >> 5), ~(1u << (c & 31)));
      }
      __syncthreads();
    }
    // the followers: still in U
    __syncthreads();
    for (int64_t b = tid; b < B; b += FIELD_THREADS)
      if (claim_round[b] < -1) claim_round[b] = -1;
  }
  if (tid == 0) n_claims[0] = claims;
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_assign_lds_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ frontier,
    const uint32_t* __restrict__ field, const double* __restrict__ start, const int8_t* __restrict__ may_claim, int r_inflate, int r_claim,
    int max_claims, int max_seg, int S_max, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell,
    int32_t* claim_round, int32_t* __restrict__ n_claims) {
  extern __shared__ uint32_t field_lds[];
  assign_body(field_lds + assign_bitmap_words((int64_t)W * H), field_lds, B, W, H, ox, oy, dx, dy, frontier, field, start, may_claim,
              r_inflate, r_claim, max_claims, max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell, claim_round, n_claims);
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_assign_global_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ frontier,
    const uint32_t* __restrict__ field, const double* __restrict__ start, const int8_t* __restrict__ may_claim, int r_inflate, int r_claim,
    int max_claims, int max_seg, int S_max, uint32_t* work, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
    int32_t* target_cell, int32_t* claim_round, int32_t* __restrict__ n_claims) {
  extern __shared__ uint32_t field_lds[];
  assign_body(work, field_lds, B, W, H, ox, oy, dx, dy, frontier, field, start, may_claim, r_inflate, r_claim, max_claims, max_seg, S_max,
              sub_goals, n_sub, status, path_cost, target_cell, claim_round, n_claims);
}

// ---------------------------------------------------------------------------------------------------------------------
// claim hysteresis (lipmpc_grid_frontier_assign_keep_batch): a KEEP PHASE ahead of the greedy rounds, on a body of its own -- the
// two kernels above and their code objects stay what they were.  A robot with a previous target keeps what is left of it (the
// ANCHOR: the source nearest to it within r_keep) when the single-source field from the anchor says that it is reachable and not
// much farther than the robot's nearest frontier; a keeper's disc leaves the sources as a winner's does.  Every relaxation of the
// map, keep attempt or greedy round, is a SLOT, and a call makes at most max_claims of them.
// LDS: the assign kernels' layout with KEEP_WORDS in place of ASSIGN_WORDS -- the spare word 3 is the next keep candidate of the
// chunk; after the nine parked pairs come three more pointers (kept, the given field, prev_target), four scalars of the lane
// that walks (keep_ratio16, keep_slack, max_seg, S_max), the slot's entry cell and the count of U
constexpr int KEEP_WORDS = 34;
constexpr int R_KEEP_MAX = 64, KEEP_RATIO_MIN = 16, KEEP_RATIO_MAX = 1024, KEEP_SLACK_MAX = 4096;
__host__ __device__ inline int64_t keep_bitmap_words(int64_t ncells) { return 2 * bitmap_words(ncells) + KEEP_WORDS; }
__host__ __device__ inline int64_t keep_lds_bytes(int64_t ncells, bool in_lds) {
  return 4 * (keep_bitmap_words(ncells) + (in_lds ? ncells : 0));
}

inline bool keep_fits_lds(int64_t ncells) { return keep_lds_bytes(ncells, true) + LDS_SLACK <= LDS_LIMIT; }

// what the one-workgroup body and the tiled kernels share of the keep rule.
// the anchor search, a workgroup of FIELD_THREADS: this thread's wave's least (d^2 << 32 | cell) over the sources within r_keep of
// the previous target pt (the window clipped to the grid), ~0 for none; the caller reduces the waves with a 64-bit atomicMin
__device__ __forceinline__ unsigned long long anchor_key(const uint32_t* src, int pt, int r_keep, int W, int H) {
  const int pi = pt / H, pj = pt - pi * H;
  const int i_lo = max(pi - r_keep, 0), i_hi = min(pi + r_keep, W - 1), j_lo = max(pj - r_keep, 0), j_hi = min(pj + r_keep, H - 1);
  const int nj = j_hi - j_lo + 1, count = (i_hi - i_lo + 1) * nj;
  unsigned long long mine = ~0ull;
  for (int idx = threadIdx.x; idx < count; idx += FIELD_THREADS) {
    const int q = idx / nj, i = i_lo + q, j = j_lo + idx - q * nj, c = i * H + j;
    const int d2 = (i - pi) * (i - pi) + (j - pj) * (j - pj);
    if (d2 <= r_keep * r_keep && bit_of(src, c)) mine = min(mine, ((unsigned long long)(uint32_t)d2 << 32) | (uint32_t)c);
  }
  for (int o = 32; o; o >>= 1) mine = min(mine, (unsigned long long)__shfl_xor(mine, o));
  return mine;
}

// a previous target that is a cell of the grid (anything else is "none")
__device__ __forceinline__ bool is_cell(int32_t prev, int ncells) { return (uint32_t)prev < (uint32_t)ncells; }

// THE TEST (one lane): the robot whose start cell is `cell` enters the slot's field at s (-1: nowhere); it keeps iff it also
// enters the given field, at e, and 16 keepfield[s] <= keep_ratio16 given[e] + 80 keep_slack in 64 bits
template <typename FieldPtr>
__device__ __forceinline__ bool keep_passes(FieldPtr fld, const uint32_t* __restrict__ given, int W, int H, int cell, int s, int r_inflate,
                                            uint32_t keep_ratio16, uint32_t keep_slack) {
  const int ci = cell / H;
  const int e = given[cell] != INF ? cell : snap(given, W, H, ci, cell - ci * H, r_inflate);
  const unsigned long long cost = ld(fld + max(s, 0)), near = given[max(e, 0)];
  return s >= 0 && e >= 0 && 16ull * cost <= (unsigned long long)keep_ratio16 * near + 80ull * (unsigned long long)keep_slack;
}

template <typename FieldPtr>
__device__ __forceinline__ void assign_keep_body(FieldPtr fld, uint32_t* bm, int64_t B, int W, int H, double ox, double oy, double dx,
                                                 double dy, const uint8_t* __restrict__ frontier, const uint32_t* __restrict__ field,
                                                 const double* __restrict__ start, const int8_t* __restrict__ may_claim,
                                                 const int32_t* __restrict__ prev_target, int r_inflate, int r_claim, int r_keep,
                                                 int keep_ratio16, int keep_slack, int max_claims, int max_seg, int S_max,
                                                 double* __restrict__ sub_goals, int32_t* __restrict__ n_sub, int32_t* __restrict__ status,
                                                 double* __restrict__ path_cost, int32_t* __restrict__ target_cell, int32_t* claim_round,
                                                 int32_t* __restrict__ n_claims, int8_t* __restrict__ kept, int32_t* __restrict__ n_kept) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int ncells = W * H, words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  uint32_t *blk = bm, *src = bm + words, *tgt = bm + 2 * words + 2, *next = bm + 2 * words + 3;
  unsigned long long* key = (unsigned long long*)(bm + 2 * words);
  uint32_t* parked = bm + 2 * words + 4;                  // 64-bit values as word pairs
  auto park = [&](int slot, unsigned long long v) { parked[2 * slot] = (uint32_t)v; parked[2 * slot + 1] = (uint32_t)(v >> 32); };
  auto unpark = [&](int slot) { return ((unsigned long long)parked[2 * slot + 1] << 32) | parked[2 * slot]; };

  // U_0, each robot with its start cell (assign_body's encoding in claim_round); nobody has kept anything yet
  int in_u = 0;
  for (int64_t b = tid; b < B; b += FIELD_THREADS) {
    const int sb = status[b];
    int si = 0, sj = 0, v = -1;
    if (max_claims > 0 && (sb == LIPMPC_RRT_FOUND || sb == LIPMPC_RRT_PATH_OVERFLOW) && (!may_claim || may_claim[b]) &&
        cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj))
      v = -2 - (si * H + sj);
    claim_round[b] = v;
    kept[b] = 0;
    in_u += v <= -2;
  }
  int claims = 0, keeps = 0, slots = 0;
  if (max_claims > 0) {
    for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
      const int c = c0 + lane;
      const bool pass = c < ncells && field[c] != INF;
      const uint64_t mb = __ballot(c < ncells && !pass), ms = __ballot(pass && frontier[c] != 0);
      if (lane == 0) {
        blk[c0 >> 5] = (uint32_t)mb; blk[(c0 >> 5) + 1] = (uint32_t)(mb >> 32);
        src[c0 >> 5] = (uint32_t)ms; src[(c0 >> 5) + 1] = (uint32_t)(ms >> 32);
      }
    }
    if (tid < 2) { blk[words - 2 + tid] = 0; src[words - 2 + tid] = 0; }
    if (tid == 0) {
      *key = ~0ull;
      *next = INF;
      parked[29] = 0;
      park(0, __double_as_longlong(ox)); park(1, __double_as_longlong(oy)); park(2, __double_as_longlong(dx));
      park(3, __double_as_longlong(dy));
      park(4, (unsigned long long)sub_goals); park(5, (unsigned long long)n_sub); park(6, (unsigned long long)status);
      park(7, (unsigned long long)path_cost); park(8, (unsigned long long)target_cell);
      park(9, (unsigned long long)kept); park(10, (unsigned long long)field); park(11, (unsigned long long)prev_target);
      parked[24] = (uint32_t)keep_ratio16; parked[25] = (uint32_t)keep_slack; parked[26] = (uint32_t)max_seg; parked[27] = (uint32_t)S_max;
    }
    __syncthreads();
    // |U|: counted once, one less with every winner -- when the last of U has won, kept or claimed, no further slot is begun
    if (in_u) atomicAdd(parked + 29, (uint32_t)in_u);
    __syncthreads();
    int left = (int)parked[29];

    // (one lane) the rows of robot wb, who enters the slot's field at s and wins as number k: the path rule, as assign_body
    // writes a winner's.  Returns the target cell, or -1 (a fixed point always has a descent: it cannot happen)
    auto write_rows = [&](int64_t wb, int s, int k) {
      const double wox = __longlong_as_double(unpark(0)), woy = __longlong_as_double(unpark(1));
      const double wdx = __longlong_as_double(unpark(2)), wdy = __longlong_as_double(unpark(3));
      const int S_max = (int)parked[27], max_seg = (int)parked[26];
      double* sg = (double*)unpark(4) + wb * (int64_t)S_max * 2;
      int last_cell = s, n = 0;
      for (int pass = 0; pass < 2 && n >= 0 && n <= S_max; ++pass)
        n = walk_in(fld, W, H, s, max_seg, wox, woy, wdx, wdy, pass ? sg : nullptr, last_cell);
      if (n <= 0) return -1;
      if (n <= S_max) centre(last_cell, H, wox, woy, wdx, wdy, sg + 2 * (n - 1));
      ((int32_t*)unpark(6))[wb] = n <= S_max ? LIPMPC_RRT_FOUND : LIPMPC_RRT_PATH_OVERFLOW;
      ((int32_t*)unpark(5))[wb] = n <= S_max ? n : 0;
      ((double*)unpark(7))[wb] = (double)ld(fld + s) / 5.0;
      ((int32_t*)unpark(8))[wb] = last_cell;
      claim_round[wb] = k;
      return last_cell;
    };
    // the sources outside the disc of r_claim round cell t, clipped to the grid
    auto take_disc = [&](int t) {
      const int ti = t / H, tj = t - ti * H, r2 = r_claim * r_claim;
      const int i_lo = max(ti - r_claim, 0), i_hi = min(ti + r_claim, W - 1);
      for (int c = i_lo * H + tid; c < (i_hi + 1) * H; c += FIELD_THREADS) {
        const int i = c / H, j = c - i * H;
        if (bit_of(src, c) && (i - ti) * (i - ti) + (j - tj) * (j - tj) <= r2) atomicAnd(src + (c >> 5), ~(1u << (c & 31)));
      }
      __syncthreads();
    };

    // THE SLOTS.  One loop serves both phases, so that the relaxation and the walk are compiled once.  While `keeping`, a slot
    // belongs to the next robot of U_0 whose previous target has an anchor -- ascending index: a chunk of FIELD_THREADS robots at
    // a time, a thread per robot, `next` hands out the chunk's candidates one by one; after the last of them, to a greedy round of
    // assign_body (a = -1).
    auto is_candidate = [&](int64_t b) {
      return b < B && claim_round[b] <= -2 && is_cell(((const int32_t*)unpark(11))[b], ncells);
    };
    int64_t base = 0;
    int cursor = 0;
    bool keeping = true, candidate = is_candidate(tid);
    while (slots < max_claims && left > 0) {
      int a = -1;
      int64_t wb = 0;
      while (keeping) {
        if (candidate && tid >= cursor) atomicMin(next, (uint32_t)tid);
        __syncthreads();
        const uint32_t nx = *next;
        __syncthreads();                                  // everybody has read it
        if (nx == INF) {                                  // the chunk is done
          base += FIELD_THREADS;
          cursor = 0;
          keeping = base < B;
          candidate = keeping && is_candidate(base + tid);
          continue;
        }
        if (tid == 0) *next = INF;                        // (the next minimum comes at least two barriers on)
        cursor = (int)nx + 1;
        wb = base + nx;
        // the anchor: the source within r_keep of the previous target with the least (d^2, cell)
        const unsigned long long mine = anchor_key(src, ((const int32_t*)unpark(11))[wb], r_keep, W, H);
        if (lane == 0 && mine != ~0ull) atomicMin(key, mine);
        __syncthreads();
        const unsigned long long found = *key;
        __syncthreads();                                  // everybody has read it
        if (found == ~0ull) continue;                     // nothing is left of the target: no slot is spent
        if (tid == 0) *key = ~0ull;
        a = (int)(found & 0xFFFFFFFFull);
        break;
      }
      ++slots;
      // the slot's field: the least cost to the anchor alone, or to what is left of the sources
      int any = 0;
      for (int c = tid; c < ncells; c += FIELD_THREADS) {
        const bool s = a >= 0 ? c == a : bit_of(src, c);
        st(fld + c, s ? 0u : INF);
        any |= s;
      }
      if (!__syncthreads_or(any)) break;
      relax(fld, blk, W, H);
      if (a < 0) {
        // the candidates of U, and the least (cost, b) among them
        unsigned long long mine = ~0ull;
        for (int64_t b = tid; b < B; b += FIELD_THREADS) {
          const int v = claim_round[b];
          if (v > -2) continue;
          const int s = claim_cell(fld, W, H, -2 - v, r_inflate);
          if (s >= 0) mine = min(mine, ((unsigned long long)ld(fld + s) << 32) | (unsigned long long)b);
        }
        for (int o = 32; o; o >>= 1) mine = min(mine, (unsigned long long)__shfl_xor(mine, o));
        if (lane == 0 && mine != ~0ull) atomicMin(key, mine);
        __syncthreads();
        const unsigned long long win = *key;
        if (win == ~0ull) break;                          // no candidate: the rounds end
        wb = (int64_t)(win & 0xFFFFFFFFull);
      }
      if (tid == 0) {
        // where wb enters the slot's field; a keeper also has to pass the test, against the given field at its entry into that
        const int cell = -2 - claim_round[wb];
        const int s = claim_cell(fld, W, H, cell, r_inflate);
        bool ok = s >= 0;
        if (a >= 0) ok = keep_passes(fld, (const uint32_t*)unpark(10), W, H, cell, s, r_inflate, parked[24], parked[25]);
        parked[28] = ok ? (uint32_t)s : INF;
      }
      __syncthreads();
      const uint32_t entry = parked[28];
      if (tid == 0) *key = ~0ull;                         // (everybody has read it; the next minimum comes two barriers on)
      if (entry == INF) {
        if (a >= 0) continue;                             // not kept: the robot stays in U, the slot is spent
        break;
      }
      if (tid == 0) {
        const int last = write_rows(wb, (int)entry, claims);
        if (last >= 0 && a >= 0) ((int8_t*)unpark(9))[wb] = 1;
        *tgt = last >= 0 ? (uint32_t)last : INF;          // (a fixed point always has a descent: INF cannot happen)
      }
      __syncthreads();
      const uint32_t t = *tgt;
      if (t == INF) break;
      ++claims;
      if (a >= 0) ++keeps;
      if (--left == 0) break;                             // U is used up
      if (slots >= max_claims) break;
      take_disc((int)t);
    }
    // the followers: still in U
    __syncthreads();
    for (int64_t b = tid; b < B; b += FIELD_THREADS)
      if (claim_round[b] < -1) claim_round[b] = -1;
  }
  if (tid == 0) { n_claims[0] = claims; n_kept[0] = keeps; }
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_assign_keep_lds_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ frontier,
    const uint32_t* __restrict__ field, const double* __restrict__ start, const int8_t* __restrict__ may_claim,
    const int32_t* __restrict__ prev_target, int r_inflate, int r_claim, int r_keep, int keep_ratio16, int keep_slack, int max_claims,
    int max_seg, int S_max, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell,
    int32_t* claim_round, int32_t* __restrict__ n_claims, int8_t* __restrict__ kept, int32_t* __restrict__ n_kept) {
  extern __shared__ uint32_t field_lds[];
  assign_keep_body(field_lds + keep_bitmap_words((int64_t)W * H), field_lds, B, W, H, ox, oy, dx, dy, frontier, field, start, may_claim,
                   prev_target, r_inflate, r_claim, r_keep, keep_ratio16, keep_slack, max_claims, max_seg, S_max, sub_goals, n_sub, status,
                   path_cost, target_cell, claim_round, n_claims, kept, n_kept);
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_assign_keep_global_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ frontier,
    const uint32_t* __restrict__ field, const double* __restrict__ start, const int8_t* __restrict__ may_claim,
    const int32_t* __restrict__ prev_target, int r_inflate, int r_claim, int r_keep, int keep_ratio16, int keep_slack, int max_claims,
    int max_seg, int S_max, uint32_t* work, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell,
    int32_t* claim_round, int32_t* __restrict__ n_claims, int8_t* __restrict__ kept, int32_t* __restrict__ n_kept) {
  extern __shared__ uint32_t field_lds[];
  assign_keep_body(work, field_lds, B, W, H, ox, oy, dx, dy, frontier, field, start, may_claim, prev_target, r_inflate, r_claim, r_keep,
                   keep_ratio16, keep_slack, max_claims, max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell, claim_round,
                   n_claims, kept, n_kept);
}

// ---------------------------------------------------------------------------------------------------------------------
// the informed explorer (lipmpc_grid_frontier_gain_batch, lipmpc_grid_frontier_utility_field_batch,
// lipmpc_grid_frontier_utility_path_batch): what a robot would see from a frontier cell, the cost-to-go field whose sources start
// ahead by what they reveal, and the paths down it.
constexpr int R_VIEW_MAX = 64;
constexpr int W_GAIN_MAX = 65535, G_CAP_MAX = 16384;
constexpr int GAIN_THREADS = 1024, GAIN_WAVES = GAIN_THREADS / 64;
constexpr int GAIN_CHUNK = 2048;                      // cells of a map per workgroup: blockIdx.x = map, blockIdx.y = chunk

// words of a wave's visibility window, (2 r + 1)^2 bits, kept even
__host__ __device__ inline int64_t gain_window_words(int r_view) {
  const int64_t side = 2 * (int64_t)r_view + 1;
  return ((side * side + 63) / 64) * 2;
}

// LDS of the gain kernel: the whole map's solid and unknown bitmaps, the chunk's frontier count (a word pair), the chunk's
// frontier cells, one window per wave
__host__ __device__ inline int64_t gain_lds_bytes(int64_t ncells, int r_view) {
  return 4 * (2 * bitmap_words(ncells) + 2 + GAIN_CHUNK + GAIN_WAVES * gain_window_words(r_view));
}

// Work follows the frontier: the workgroup of a chunk compacts the chunk's frontier cells into a list (everything else gets its 0
// on the way), then a wave takes one frontier cell at a time and its lanes the 8 r rays of the fan, 64 at a time.  A ray walks
// outward by the planners' LOS expression -- quotient and remainder per axis, as los() -- and ORs the unknown cells it crosses
// into the wave's window; the gain is the window's popcount: a set's size, whatever order lanes and rays fell in.
__global__ void __launch_bounds__(GAIN_THREADS) frontier_gain_kernel(int W, int H, const int32_t* __restrict__ evidence, int t_free,
                                                                     int t_occ, const uint8_t* __restrict__ frontier, int r_view,
                                                                     int32_t* __restrict__ gain) {
  extern __shared__ uint32_t field_lds[];
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncells = W * H, words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  const int ww = (int)gain_window_words(r_view);
  uint32_t *solid = field_lds, *unk = field_lds + words, *count = field_lds + 2 * words, *list = count + 2;
  uint32_t* win = list + GAIN_CHUNK + wave * ww;
  const int32_t* ev = evidence + f * (int64_t)ncells;
  const uint8_t* fr = frontier + f * (int64_t)ncells;
  int32_t* out = gain + f * (int64_t)ncells;

  // evidence -> solid and unknown bitmaps, as the frontier field kernel classifies
  for (int c0 = tid - lane; c0 < padded; c0 += GAIN_THREADS) {
    const int c = c0 + lane;
    const int e = c < ncells ? ev[c] : 0;
    const bool is_solid = c < ncells && e >= t_occ, is_free = e <= -t_free;
    const uint64_t ms = __ballot(is_solid), mu = __ballot(c < ncells && !is_solid && !is_free);
    if (lane == 0) {
      solid[c0 >> 5] = (uint32_t)ms; solid[(c0 >> 5) + 1] = (uint32_t)(ms >> 32);
      unk[c0 >> 5] = (uint32_t)mu; unk[(c0 >> 5) + 1] = (uint32_t)(mu >> 32);
    }
  }
  if (tid < 2) { solid[words - 2 + tid] = 0; unk[words - 2 + tid] = 0; }
  if (tid == 0) *count = 0;
  __syncthreads();
  // the chunk's frontier cells (in whatever order: each cell's gain is its own)
  const int c_lo = (int)blockIdx.y * GAIN_CHUNK, c_hi = min(c_lo + GAIN_CHUNK, ncells);
  for (int c = c_lo + tid; c < c_hi; c += GAIN_THREADS) {
    if (fr[c] != 0) list[atomicAdd(count, 1u)] = (uint32_t)c;
    else out[c] = 0;
  }
  __syncthreads();
  const int n = (int)*count, r = r_view, r2 = r * r, two_r = 2 * r, side = two_r + 1, n_rays = 8 * r;
  for (int k = wave; k < n; k += GAIN_WAVES) {
    const int s = (int)list[k], si = s / H, sj = s - si * H;
    for (int w = lane; w < ww; w += 64) win[w] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int q = lane; q < n_rays; q += 64) {
      // the end cell: the ring of Chebyshev radius r, side by side
      const int edge = q / two_r, t = q - edge * two_r;
      const int di = edge == 0 ? -r : edge == 1 ? t - r : edge == 2 ? r : r - t;
      const int dj = edge == 0 ? t - r : edge == 1 ? r : edge == 2 ? r - t : -r;
      int qi = 0, ri = r, qj = 0, rj = r;
      for (int step = 1; step <= r; ++step) {
        ri += 2 * di; rj += 2 * dj;
        if (ri >= two_r) { ri -= two_r; ++qi; } else if (ri < 0) { ri += two_r; --qi; }
        if (rj >= two_r) { rj -= two_r; ++qj; } else if (rj < 0) { rj += two_r; --qj; }
        const int i = si + qi, j = sj + qj;
        if (qi * qi + qj * qj > r2 || (unsigned)i >= (unsigned)W || (unsigned)j >= (unsigned)H) break;
        const int c = i * H + j;
        if (bit_of(solid, c)) break;
        if (bit_of(unk, c)) {
          const int b = (qi + r) * side + qj + r;
          atomicOr(win + (b >> 5), 1u << (b & 31));
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int seen = 0;
    for (int w = lane; w < ww; w += 64) seen += __popc(win[w]);
    for (int o = 32; o; o >>= 1) seen += __shfl_xor(seen, o);
    if (lane == 0) out[s] = seen;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the window is read before the next cell clears it)
    __builtin_amdgcn_wave_barrier();
  }
}

// what a source starts with: sixteenths of a cost unit per cell it reveals less than g_cap (at most 2^26: no sum wraps)
__device__ inline uint32_t gain_seed(int g, int w_gain, int g_cap) {
  return ((uint32_t)w_gain * (uint32_t)(g_cap - min(max(g, 0), g_cap))) >> 4;
}

// LDS of the utility field kernels: the impassable bitmap, the source count (a word pair: the field stays 8-byte aligned), then
// the field -- or bitmap and count alone
__host__ __device__ inline int64_t utility_bitmap_words(int64_t ncells) { return bitmap_words(ncells) + 2; }
__host__ __device__ inline int64_t utility_lds_bytes(int64_t ncells, bool in_lds) {
  return 4 * (utility_bitmap_words(ncells) + (in_lds ? ncells : 0));
}

inline bool utility_fits_lds(int64_t ncells) { return utility_lds_bytes(ncells, true) + LDS_SLACK <= LDS_LIMIT; }

// blockIdx.x = map.  `fld`: the field's working copy ([W*H], LDS or the output itself); `bm`: the bitmap and the count's word.
// The sweeps converge from any seeds by monotone minimum: a value is the cost of a real path to some source plus that source's
// seed, values only fall, and the fixed point is the least such sum -- unique, whatever order the races fell in.
template <bool COPY_OUT, typename FieldPtr>
__device__ inline void utility_body(FieldPtr fld, uint32_t* bm, int W, int H, const uint8_t* __restrict__ frontier,
                                    const uint32_t* __restrict__ field, const int32_t* __restrict__ gain, int w_gain, int g_cap,
                                    int min_gain, uint32_t* ufield, int32_t* __restrict__ n_sources) {
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int ncells = W * H, words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  uint32_t *blk = bm, *n_src = bm + words;
  const uint8_t* fr = frontier + f * (int64_t)ncells;
  const uint32_t* given = field + f * (int64_t)ncells;
  const int32_t* gn = gain + f * (int64_t)ncells;
  uint32_t* out = ufield + f * (int64_t)ncells;

  if (tid < 2) blk[words - 2 + tid] = 0;
  if (tid == 0) *n_src = 0;
  __syncthreads();
  int mine = 0;
  for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
    const int c = c0 + lane;
    const bool pass = c < ncells && given[c] != INF;
    bool src = false;
    if (pass && fr[c] != 0) {
      const int g = gn[c];
      src = g >= min_gain;
      if (src) st(fld + c, gain_seed(g, w_gain, g_cap));
    }
    if (c < ncells && !src) st(fld + c, INF);
    const uint64_t mb = __ballot(c < ncells && !pass);
    if (lane == 0) { blk[c0 >> 5] = (uint32_t)mb; blk[(c0 >> 5) + 1] = (uint32_t)(mb >> 32); }
    mine += __popcll(__ballot(src));
  }
  if (lane == 0 && mine) atomicAdd(n_src, (uint32_t)mine);
  __syncthreads();
  const int n = (int)*n_src;
  if (tid == 0) n_sources[f] = n;
  if (n) relax(fld, blk, W, H);                          // (no source: the field is INF as it stands)
  if (COPY_OUT)
    for (int c = tid; c < ncells; c += FIELD_THREADS) out[c] = ld(fld + c);
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_utility_lds_kernel(int W, int H, const uint8_t* __restrict__ frontier,
                                                                             const uint32_t* __restrict__ field,
                                                                             const int32_t* __restrict__ gain, int w_gain, int g_cap,
                                                                             int min_gain, uint32_t* __restrict__ ufield,
                                                                             int32_t* __restrict__ n_sources) {
  extern __shared__ uint32_t field_lds[];
  utility_body<true>(field_lds + utility_bitmap_words((int64_t)W * H), field_lds, W, H, frontier, field, gain, w_gain, g_cap, min_gain,
                     ufield, n_sources);
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_utility_global_kernel(int W, int H, const uint8_t* __restrict__ frontier,
                                                                                const uint32_t* __restrict__ field,
                                                                                const int32_t* __restrict__ gain, int w_gain, int g_cap,
                                                                                int min_gain, uint32_t* ufield,
                                                                                int32_t* __restrict__ n_sources) {
  extern __shared__ uint32_t field_lds[];
  utility_body<false>(ufield + (int64_t)blockIdx.x * W * H, field_lds, W, H, frontier, field, gain, w_gain, g_cap, min_gain, ufield,
                      n_sources);
}

// walk() down a utility field: the same descent and string pulling, ending at the first TERMINAL cell -- a source that holds its
// own seed -- instead of the first 0; the test comes before a descending neighbour is looked for
template <typename Terminal>
__device__ inline int walk_to(const uint32_t* __restrict__ fld, int W, int H, int s, int max_seg, double ox, double oy, double dx, double dy,
                              double* sg, int& last_cell, Terminal terminal) {
  int count = 0;
  auto emit = [&](int c) {
    if (sg) centre(c, H, ox, oy, dx, dy, sg + 2 * count);
    ++count;
  };
  last_cell = s;
  if (!terminal(s)) {
    int a = s, prev = s, cur = descend(fld, W, H, s);
    while (cur >= 0) {
      const bool last = terminal(cur);
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
    last_cell = cur;
  }
  return count + 1;
}

// One lane per robot: frontier_path_kernel down a utility field, to the centre of the first terminal cell reached.
// (tile_utility_descent_kernel, further down, holds a COPY of this body behind one more rule: a fix here belongs there too.)
__global__ void __launch_bounds__(PATH_THREADS) frontier_utility_path_kernel(
    int64_t B, int one_field, int W, int H, double ox, double oy, double dx, double dy, const int32_t* __restrict__ evidence, int t_occ,
    const uint8_t* __restrict__ frontier, const int32_t* __restrict__ gain, const uint32_t* __restrict__ ufield,
    const int32_t* __restrict__ n_sources, int w_gain, int g_cap, int min_gain, const double* __restrict__ start, int r_inflate, int max_seg,
    int S_max, double* __restrict__ sub_goals, int32_t* __restrict__ n_sub, int32_t* __restrict__ status, double* __restrict__ path_cost,
    int32_t* __restrict__ target_cell, int32_t* __restrict__ target_gain) {
  const int64_t b = (int64_t)blockIdx.x * PATH_THREADS + threadIdx.x;
  if (b >= B) return;
  const int64_t f = one_field ? 0 : b;
  const int ncells = W * H;
  const uint32_t* fld = ufield + f * (int64_t)ncells;
  const uint8_t* fr = frontier + f * (int64_t)ncells;
  const int32_t* gn = gain + f * (int64_t)ncells;
  auto done = [&](int st_, int n, double cost, int target) {
    status[b] = st_; n_sub[b] = n; path_cost[b] = cost; target_cell[b] = target; target_gain[b] = target >= 0 ? gn[target] : -1;
  };
  // (a source is passable: its field is finite, which the comparison with a seed says too)
  auto terminal = [&](int c) {
    if (fr[c] == 0) return false;
    const int g = gn[c];
    return g >= min_gain && fld[c] == gain_seed(g, w_gain, g_cap);
  };
  const double nan = __builtin_nan("");
  int si = 0, sj = 0;
  if (!cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj)) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan, -1);
  int s = si * H + sj;
  if (evidence[f * (int64_t)ncells + s] >= t_occ) return done(LIPMPC_RRT_START_OCCUPIED, 0, nan, -1);
  if (n_sources[f] == 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);
  if (fld[s] == INF) s = snap(fld, W, H, si, sj, r_inflate);
  if (s < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);
  double* sg = sub_goals + b * (int64_t)S_max * 2;
  int last_cell;
  const int n = walk_to(fld, W, H, s, max_seg, ox, oy, dx, dy, nullptr, last_cell, terminal);
  if (n < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);             // (a `ufield` that is no utility field of this map)
  const double cost = (double)(fld[s] - fld[last_cell]) / 5.0;
  if (n > S_max) return done(LIPMPC_RRT_PATH_OVERFLOW, 0, cost, last_cell);
  walk_to(fld, W, H, s, max_seg, ox, oy, dx, dy, sg, last_cell, terminal);
  centre(last_cell, H, ox, oy, dx, dy, sg + 2 * (n - 1));
  done(LIPMPC_RRT_FOUND, n, cost, last_cell);
}

// ---------------------------------------------------------------------------------------------------------------------
// gain-seeded claims (lipmpc_grid_frontier_assign_utility_batch): the coordinated claim's rounds with the utility field's seeds
// on what is left of the sources and the utility path's terminal test where the winner walks -- on a body of its own: the assign
// and keep kernels above and their code objects stay what they were.  The source bitmap holds S_k (frontier, passable,
// gain >= min_gain, outside every disc so far), so the terminal test is "a bit of S_k that holds its own seed" and `gain` is read
// at source cells only; it stays in global memory.
// LDS: the assign kernels' layout with UCLAIM_WORDS in place of ASSIGN_WORDS -- after the nine parked pairs come two more
// pointers (gain, target_gain), four scalars -- the seed's w_gain and g_cap, which the round's seeding reads from here too (a
// lane's registers hold them then, not the scalar file through every loop), and the walking lane's max_seg and S_max -- then
// n_claims' pointer and the two scalars of a round's end, r_claim and max_claims
constexpr int UCLAIM_WORDS = 34;
__host__ __device__ inline int64_t uclaim_bitmap_words(int64_t ncells) { return 2 * bitmap_words(ncells) + UCLAIM_WORDS; }
__host__ __device__ inline int64_t uclaim_lds_bytes(int64_t ncells, bool in_lds) {
  return 4 * (uclaim_bitmap_words(ncells) + (in_lds ? ncells : 0));
}

inline bool uclaim_fits_lds(int64_t ncells) { return uclaim_lds_bytes(ncells, true) + LDS_SLACK <= LDS_LIMIT; }

// walk_to() on whatever pointer the round's field lives behind, read with the sweeps' own loads
template <typename FieldPtr, typename Terminal>
__device__ __forceinline__ int walk_in_to(FieldPtr fld, int W, int H, int s, int max_seg, double ox, double oy, double dx, double dy,
                                          double* sg, int& last_cell, Terminal terminal) {
  int count = 0;
  auto emit = [&](int c) {
    if (sg) centre(c, H, ox, oy, dx, dy, sg + 2 * count);
    ++count;
  };
  last_cell = s;
  if (!terminal(s)) {
    int a = s, prev = s, cur = descend_in(fld, W, H, s);
    while (cur >= 0) {
      const bool last = terminal(cur);
      if (!los_in(fld, H, a, cur) || ld(fld + a) - ld(fld + cur) >= (uint32_t)max_seg) {
        if (prev != a) { emit(prev); a = prev; continue; }
        if (last) break;
        emit(cur); a = cur;
      }
      if (last) break;
      prev = cur;
      cur = descend_in(fld, W, H, cur);
    }
    if (cur < 0) return -1;
    last_cell = cur;
  }
  return count + 1;
}

// The whole call: assign_body with the three differences named above.  claim_round[b] holds -2 - (start cell) while b is in U.
template <typename FieldPtr>
__device__ __forceinline__ void assign_utility_body(FieldPtr fld, uint32_t* bm, int64_t B, int W, int H, double ox, double oy, double dx,
                                                    double dy, const uint8_t* __restrict__ frontier, const uint32_t* __restrict__ field,
                                                    const int32_t* __restrict__ gain, int w_gain, int g_cap, int min_gain,
                                                    const double* __restrict__ start, const int8_t* __restrict__ may_claim,
                                                    int r_inflate, int r_claim, int max_claims, int max_seg, int S_max,
                                                    double* __restrict__ sub_goals, int32_t* __restrict__ n_sub,
                                                    int32_t* __restrict__ status, double* __restrict__ path_cost,
                                                    int32_t* __restrict__ target_cell, int32_t* __restrict__ target_gain,
                                                    int32_t* claim_round, int32_t* __restrict__ n_claims) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int ncells = W * H, words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  uint32_t *blk = bm, *src = bm + words, *tgt = bm + 2 * words + 2;
  unsigned long long* key = (unsigned long long*)(bm + 2 * words);
  uint32_t* parked = bm + 2 * words + 4;                  // 64-bit values as word pairs, then the two scalars
  auto park = [&](int slot, unsigned long long v) { parked[2 * slot] = (uint32_t)v; parked[2 * slot + 1] = (uint32_t)(v >> 32); };
  auto unpark = [&](int slot) { return ((unsigned long long)parked[2 * slot + 1] << 32) | parked[2 * slot]; };

  // U_0, each robot with its start cell
  for (int64_t b = tid; b < B; b += FIELD_THREADS) {
    const int sb = status[b];
    int si = 0, sj = 0, v = -1;
    if (max_claims > 0 && (sb == LIPMPC_RRT_FOUND || sb == LIPMPC_RRT_PATH_OVERFLOW) && (!may_claim || may_claim[b]) &&
        cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj))
      v = -2 - (si * H + sj);
    claim_round[b] = v;
  }
  int claims = 0;
  if (max_claims > 0) {
    // impassable = the given field is INF; sources = the utility field's: the given frontier, passable, gain >= min_gain
    for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
      const int c = c0 + lane;
      const bool pass = c < ncells && field[c] != INF;
      bool s = false;
      if (pass && frontier[c] != 0) s = gain[c] >= min_gain;
      const uint64_t mb = __ballot(c < ncells && !pass), ms = __ballot(s);
      if (lane == 0) {
        blk[c0 >> 5] = (uint32_t)mb; blk[(c0 >> 5) + 1] = (uint32_t)(mb >> 32);
        src[c0 >> 5] = (uint32_t)ms; src[(c0 >> 5) + 1] = (uint32_t)(ms >> 32);
      }
    }
    if (tid < 2) { blk[words - 2 + tid] = 0; src[words - 2 + tid] = 0; }
    if (tid == 0) {
      *key = ~0ull;
      park(0, __double_as_longlong(ox)); park(1, __double_as_longlong(oy)); park(2, __double_as_longlong(dx));
      park(3, __double_as_longlong(dy));
      park(4, (unsigned long long)sub_goals); park(5, (unsigned long long)n_sub); park(6, (unsigned long long)status);
      park(7, (unsigned long long)path_cost); park(8, (unsigned long long)target_cell);
      park(9, (unsigned long long)gain); park(10, (unsigned long long)target_gain);
      parked[22] = (uint32_t)w_gain; parked[23] = (uint32_t)g_cap; parked[24] = (uint32_t)max_seg; parked[25] = (uint32_t)S_max;
      park(13, (unsigned long long)n_claims); parked[28] = (uint32_t)r_claim; parked[29] = (uint32_t)max_claims;
      tgt[1] = (uint32_t)r_inflate;                       // (the spare word beside the target)
    }
    __syncthreads();

    for (int k = 0;; ++k) {
      // ufield_k: its seed on what is left of the sources, relaxed to the fixed point
      int any = 0;
      {
        const int32_t* gn = (const int32_t*)unpark(9);
        const int ww = (int)parked[22], wcap = (int)parked[23];
        for (int c = tid; c < ncells; c += FIELD_THREADS) {
          const bool s = bit_of(src, c);
          st(fld + c, s ? gain_seed(gn[c], ww, wcap) : INF);
          any |= s;
        }
      }
      if (!__syncthreads_or(any)) break;
      relax(fld, blk, W, H);
      // the candidates of U_k, and the least (cost, b) among them
      unsigned long long mine = ~0ull;
      int eligible = 0;
      for (int64_t b = tid; b < B; b += FIELD_THREADS) {
        const int v = claim_round[b];
        if (v > -2) continue;
        ++eligible;
        const int s = claim_cell(fld, W, H, -2 - v, (int)tgt[1]);
        if (s >= 0) mine = min(mine, ((unsigned long long)ld(fld + s) << 32) | (unsigned long long)b);
      }
      for (int o = 32; o; o >>= 1) mine = min(mine, (unsigned long long)__shfl_xor(mine, o));
      if (lane == 0 && mine != ~0ull) atomicMin(key, mine);
      __syncthreads();
      const unsigned long long win = *key;
      if (win == ~0ull) break;                            // no candidate: the rounds end
      const int64_t wb = (int64_t)(win & 0xFFFFFFFFull);
      if (tid == 0) {
        // one lane walks the winner's path, twice: count, then -- if the sub-goals fit -- write (rows past n_sub stay untouched)
        const int s = claim_cell(fld, W, H, -2 - claim_round[wb], (int)tgt[1]);
        const double wox = __longlong_as_double(unpark(0)), woy = __longlong_as_double(unpark(1));
        const double wdx = __longlong_as_double(unpark(2)), wdy = __longlong_as_double(unpark(3));
        const int wseg = (int)parked[24], wmax = (int)parked[25];
        double* sg = (double*)unpark(4) + wb * (int64_t)wmax * 2;
        const int32_t* wgain = (const int32_t*)unpark(9);
        const int ww = (int)parked[22], wcap = (int)parked[23];
        auto terminal = [&](int c) { return bit_of(src, c) && ld(fld + c) == gain_seed(wgain[c], ww, wcap); };
        int last_cell = s, n = 0;
        for (int pass = 0; pass < 2 && n >= 0 && n <= wmax; ++pass)
          n = walk_in_to(fld, W, H, s, wseg, wox, woy, wdx, wdy, pass ? sg : nullptr, last_cell, terminal);
        if (n > 0) {
          if (n <= wmax) centre(last_cell, H, wox, woy, wdx, wdy, sg + 2 * (n - 1));
          ((int32_t*)unpark(6))[wb] = n <= wmax ? LIPMPC_RRT_FOUND : LIPMPC_RRT_PATH_OVERFLOW;
          ((int32_t*)unpark(5))[wb] = n <= wmax ? n : 0;
          ((double*)unpark(7))[wb] = (double)(ld(fld + s) - ld(fld + last_cell)) / 5.0;
          ((int32_t*)unpark(8))[wb] = last_cell;
          ((int32_t*)unpark(10))[wb] = wgain[last_cell];
          claim_round[wb] = k;
        }
        *tgt = n > 0 ? (uint32_t)last_cell : INF;         // (a fixed point always has a descent: INF cannot happen)
      }
      if ((wb & (FIELD_THREADS - 1)) == tid) --eligible;
      const int more = __syncthreads_or(eligible);
      const uint32_t t = *tgt;
      if (tid == 0) *key = ~0ull;                         // (everybody has read it; the next minimum comes two barriers on)
      if (t == INF) break;
      ++claims;
      if (!more || k + 1 >= (int)parked[29]) break;       // U or the allowance is used up
      // S_{k+1}: the sources outside the winner's disc, clipped to the grid
      const int rc = (int)parked[28];
      const int ti = (int)t / H, tj = (int)t - ti * H, r2 = rc * rc;
      const int i_lo = max(ti - rc, 0), i_hi = min(ti + rc, W - 1);
      for (int c = i_lo * H + tid; c < (i_hi + 1) * H; c += FIELD_THREADS) {
        const int i = c / H, j = c - i * H;
        if (bit_of(src, c) && (i - ti) * (i - ti) + (j - tj) * (j - tj) <= r2) atomicAnd(src + (c >> 5), ~(1u << (c & 31)));
      }
      __syncthreads();
    }
    // the followers: still in U
    __syncthreads();
    for (int64_t b = tid; b < B; b += FIELD_THREADS)
      if (claim_round[b] < -1) claim_round[b] = -1;
    if (tid == 0) ((int32_t*)unpark(13))[0] = claims;
  } else if (tid == 0) {
    n_claims[0] = 0;
  }
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_assign_utility_lds_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ frontier,
    const uint32_t* __restrict__ field, const int32_t* __restrict__ gain, int w_gain, int g_cap, int min_gain,
    const double* __restrict__ start, const int8_t* __restrict__ may_claim, int r_inflate, int r_claim, int max_claims, int max_seg,
    int S_max, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell, int32_t* target_gain,
    int32_t* claim_round, int32_t* __restrict__ n_claims) {
  extern __shared__ uint32_t field_lds[];
  assign_utility_body(field_lds + uclaim_bitmap_words((int64_t)W * H), field_lds, B, W, H, ox, oy, dx, dy, frontier, field, gain, w_gain,
                      g_cap, min_gain, start, may_claim, r_inflate, r_claim, max_claims, max_seg, S_max, sub_goals, n_sub, status,
                      path_cost, target_cell, target_gain, claim_round, n_claims);
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_assign_utility_global_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ frontier,
    const uint32_t* __restrict__ field, const int32_t* __restrict__ gain, int w_gain, int g_cap, int min_gain,
    const double* __restrict__ start, const int8_t* __restrict__ may_claim, int r_inflate, int r_claim, int max_claims, int max_seg,
    int S_max, uint32_t* work, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell,
    int32_t* target_gain, int32_t* claim_round, int32_t* __restrict__ n_claims) {
  extern __shared__ uint32_t field_lds[];
  assign_utility_body(work, field_lds, B, W, H, ox, oy, dx, dy, frontier, field, gain, w_gain, g_cap, min_gain, start, may_claim,
                      r_inflate, r_claim, max_claims, max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell, target_gain,
                      claim_round, n_claims);
}

// ---------------------------------------------------------------------------------------------------------------------
// claim hysteresis for the gain-seeded claims (lipmpc_grid_frontier_assign_keep_utility_batch): assign_keep_body's slot loop with
// assign_utility_body's sources, seeds, terminal walk and target_gain -- on a body of its own: every kernel above and its code
// object stays what it was.  A keep slot's field is a single source, the anchor, that starts at ITS seed, so both sides of the
// test are utilities: the given `ufield` at the robot's entry into it stands where the keep call reads the given field.
// LDS: the assign kernels' layout with KEEPU_WORDS in place of ASSIGN_WORDS -- the key, the target and the chunk's next candidate
// as in the keep kernels; then sixteen parked pairs (the keep body's twelve with `ufield` where the given field was, then gain,
// target_gain, n_claims and n_kept), ten scalars (keep_ratio16, keep_slack, max_seg, S_max, w_gain, g_cap, r_claim, r_keep,
// r_inflate, max_claims: what the slot loop reads once a slot), the slot's entry cell and the count of U
constexpr int KEEPU_WORDS = 48;
__host__ __device__ inline int64_t keepu_bitmap_words(int64_t ncells) { return 2 * bitmap_words(ncells) + KEEPU_WORDS; }
__host__ __device__ inline int64_t keepu_lds_bytes(int64_t ncells, bool in_lds) {
  return 4 * (keepu_bitmap_words(ncells) + (in_lds ? ncells : 0));
}

inline bool keepu_fits_lds(int64_t ncells) { return keepu_lds_bytes(ncells, true) + LDS_SLACK <= LDS_LIMIT; }

// a value a lane holds for itself, in a vector register: the entry cell and the anchor are the same in all lanes, and with the walk's
// arithmetic on them done in the scalar file they would overfill it (the bar is no spill of either kind).  No instruction.
__device__ __forceinline__ int per_lane(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

template <typename FieldPtr>
__device__ __forceinline__ void assign_keep_utility_body(
    FieldPtr fld, uint32_t* bm, int64_t B, int W, int H, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ frontier,
    const uint32_t* __restrict__ field, const int32_t* __restrict__ gain, const uint32_t* __restrict__ ufield, int w_gain, int g_cap,
    int min_gain, const double* __restrict__ start, const int8_t* __restrict__ may_claim, const int32_t* __restrict__ prev_target,
    int r_inflate, int r_claim, int r_keep, int keep_ratio16, int keep_slack, int max_claims, int max_seg, int S_max,
    double* __restrict__ sub_goals, int32_t* __restrict__ n_sub, int32_t* __restrict__ status, double* __restrict__ path_cost,
    int32_t* __restrict__ target_cell, int32_t* __restrict__ target_gain, int32_t* claim_round, int32_t* __restrict__ n_claims,
    int8_t* __restrict__ kept, int32_t* __restrict__ n_kept) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int ncells = W * H, words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  uint32_t *blk = bm, *src = bm + words, *tgt = bm + 2 * words + 2, *next = bm + 2 * words + 3;
  unsigned long long* key = (unsigned long long*)(bm + 2 * words);
  uint32_t* parked = bm + 2 * words + 4;                  // 64-bit values as word pairs, then the scalars
  auto park = [&](int slot, unsigned long long v) { parked[2 * slot] = (uint32_t)v; parked[2 * slot + 1] = (uint32_t)(v >> 32); };
  auto unpark = [&](int slot) { return ((unsigned long long)parked[2 * slot + 1] << 32) | parked[2 * slot]; };

  // U_0, each robot with its start cell (assign_body's encoding in claim_round); nobody has kept anything yet
  int in_u = 0;
  for (int64_t b = tid; b < B; b += FIELD_THREADS) {
    const int sb = status[b];
    int si = 0, sj = 0, v = -1;
    if (max_claims > 0 && (sb == LIPMPC_RRT_FOUND || sb == LIPMPC_RRT_PATH_OVERFLOW) && (!may_claim || may_claim[b]) &&
        cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj))
      v = -2 - (si * H + sj);
    claim_round[b] = v;
    kept[b] = 0;
    in_u += v <= -2;
  }
  int claims = 0, keeps = 0, slots = 0;
  if (max_claims > 0) {
    // impassable = the given field is INF; sources = the utility field's: the given frontier, passable, gain >= min_gain
    for (int c0 = tid - lane; c0 < padded; c0 += FIELD_THREADS) {
      const int c = c0 + lane;
      const bool pass = c < ncells && field[c] != INF;
      bool s = false;
      if (pass && frontier[c] != 0) s = gain[c] >= min_gain;
      const uint64_t mb = __ballot(c < ncells && !pass), ms = __ballot(s);
      if (lane == 0) {
        blk[c0 >> 5] = (uint32_t)mb; blk[(c0 >> 5) + 1] = (uint32_t)(mb >> 32);
        src[c0 >> 5] = (uint32_t)ms; src[(c0 >> 5) + 1] = (uint32_t)(ms >> 32);
      }
    }
    if (tid < 2) { blk[words - 2 + tid] = 0; src[words - 2 + tid] = 0; }
    if (tid == 0) {
      *key = ~0ull;
      *next = INF;
      parked[43] = 0;
      park(0, __double_as_longlong(ox)); park(1, __double_as_longlong(oy)); park(2, __double_as_longlong(dx));
      park(3, __double_as_longlong(dy));
      park(4, (unsigned long long)sub_goals); park(5, (unsigned long long)n_sub); park(6, (unsigned long long)status);
      park(7, (unsigned long long)path_cost); park(8, (unsigned long long)target_cell);
      park(9, (unsigned long long)kept); park(10, (unsigned long long)ufield); park(11, (unsigned long long)prev_target);
      park(12, (unsigned long long)gain); park(13, (unsigned long long)target_gain);
      park(14, (unsigned long long)n_claims); park(15, (unsigned long long)n_kept);
      parked[32] = (uint32_t)keep_ratio16; parked[33] = (uint32_t)keep_slack; parked[34] = (uint32_t)max_seg; parked[35] = (uint32_t)S_max;
      parked[36] = (uint32_t)w_gain; parked[37] = (uint32_t)g_cap; parked[38] = (uint32_t)r_claim; parked[39] = (uint32_t)r_keep;
      parked[40] = (uint32_t)r_inflate; parked[41] = (uint32_t)max_claims;
    }
    __syncthreads();
    // |U|: counted once, one less with every winner -- when the last of U has won, kept or claimed, no further slot is begun
    if (in_u) atomicAdd(parked + 43, (uint32_t)in_u);
    __syncthreads();
    int left = (int)parked[43];

    // (one lane) the rows of robot wb, who enters the slot's field at s and wins as number k: the utility winner's path rule --
    // in a keep slot (a >= 0) the walk ends at the anchor and nowhere else, in a greedy round at the first source of what is
    // left that holds its own seed.  Returns the target cell, or -1 (a fixed point always has a descent: it cannot happen)
    auto write_rows = [&](int64_t wb, int s, int k, int a) {
      const double wox = __longlong_as_double(unpark(0)), woy = __longlong_as_double(unpark(1));
      const double wdx = __longlong_as_double(unpark(2)), wdy = __longlong_as_double(unpark(3));
      const int wmax = (int)parked[35], wseg = (int)parked[34];
      const int32_t* wgain = (const int32_t*)unpark(12);
      const int ww = (int)parked[36], wcap = (int)parked[37];
      auto terminal = [&](int c) { return a >= 0 ? c == a : bit_of(src, c) && ld(fld + c) == gain_seed(wgain[c], ww, wcap); };
      double* sg = (double*)unpark(4) + wb * (int64_t)wmax * 2;
      int last_cell = s, n = 0;
      for (int pass = 0; pass < 2 && n >= 0 && n <= wmax; ++pass)
        n = walk_in_to(fld, W, H, s, wseg, wox, woy, wdx, wdy, pass ? sg : nullptr, last_cell, terminal);
      if (n <= 0) return -1;
      if (n <= wmax) centre(last_cell, H, wox, woy, wdx, wdy, sg + 2 * (n - 1));
      ((int32_t*)unpark(6))[wb] = n <= wmax ? LIPMPC_RRT_FOUND : LIPMPC_RRT_PATH_OVERFLOW;
      ((int32_t*)unpark(5))[wb] = n <= wmax ? n : 0;
      ((double*)unpark(7))[wb] = (double)(ld(fld + s) - ld(fld + last_cell)) / 5.0;
      ((int32_t*)unpark(8))[wb] = last_cell;
      ((int32_t*)unpark(13))[wb] = wgain[last_cell];
      claim_round[wb] = k;
      return last_cell;
    };
    // the sources outside the disc of r_claim round cell t, clipped to the grid
    auto take_disc = [&](int t) {
      const int rc = (int)parked[38];
      const int ti = t / H, tj = t - ti * H, r2 = rc * rc;
      const int i_lo = max(ti - rc, 0), i_hi = min(ti + rc, W - 1);
      for (int c = i_lo * H + tid; c < (i_hi + 1) * H; c += FIELD_THREADS) {
        const int i = c / H, j = c - i * H;
        if (bit_of(src, c) && (i - ti) * (i - ti) + (j - tj) * (j - tj) <= r2) atomicAnd(src + (c >> 5), ~(1u << (c & 31)));
      }
      __syncthreads();
    };

    // THE SLOTS: assign_keep_body's loop, one for both phases, so that the relaxation and the walk are compiled once
    auto is_candidate = [&](int64_t b) {
      return b < B && claim_round[b] <= -2 && is_cell(((const int32_t*)unpark(11))[b], ncells);
    };
    int64_t base = 0;
    int cursor = 0;
    bool keeping = true, candidate = is_candidate(tid);
    while (slots < (int)parked[41] && left > 0) {
      int a = -1;
      int64_t wb = 0;
      while (keeping) {
        if (candidate && tid >= cursor) atomicMin(next, (uint32_t)tid);
        __syncthreads();
        const uint32_t nx = *next;
        __syncthreads();                                  // everybody has read it
        if (nx == INF) {                                  // the chunk is done
          base += FIELD_THREADS;
          cursor = 0;
          keeping = base < B;
          candidate = keeping && is_candidate(base + tid);
          continue;
        }
        if (tid == 0) *next = INF;                        // (the next minimum comes at least two barriers on)
        cursor = (int)nx + 1;
        wb = base + nx;
        // the anchor: the source within r_keep of the previous target with the least (d^2, cell)
        const unsigned long long mine = anchor_key(src, ((const int32_t*)unpark(11))[wb], (int)parked[39], W, H);
        if (lane == 0 && mine != ~0ull) atomicMin(key, mine);
        __syncthreads();
        const unsigned long long found = *key;
        __syncthreads();                                  // everybody has read it
        if (found == ~0ull) continue;                     // nothing is left of the target: no slot is spent
        if (tid == 0) *key = ~0ull;
        a = (int)(found & 0xFFFFFFFFull);
        break;
      }
      ++slots;
      // the slot's field: the anchor alone at its seed, or what is left of the sources at theirs
      int any = 0;
      {
        const int32_t* gn = (const int32_t*)unpark(12);
        const int ww = (int)parked[36], wcap = (int)parked[37];
        for (int c = tid; c < ncells; c += FIELD_THREADS) {
          const bool s = a >= 0 ? c == a : bit_of(src, c);
          st(fld + c, s ? gain_seed(gn[c], ww, wcap) : INF);
          any |= s;
        }
      }
      if (!__syncthreads_or(any)) break;
      relax(fld, blk, W, H);
      if (a < 0) {
        // the candidates of U, and the least (cost, b) among them
        unsigned long long mine = ~0ull;
        for (int64_t b = tid; b < B; b += FIELD_THREADS) {
          const int v = claim_round[b];
          if (v > -2) continue;
          const int s = claim_cell(fld, W, H, -2 - v, (int)parked[40]);
          if (s >= 0) mine = min(mine, ((unsigned long long)ld(fld + s) << 32) | (unsigned long long)b);
        }
        for (int o = 32; o; o >>= 1) mine = min(mine, (unsigned long long)__shfl_xor(mine, o));
        if (lane == 0 && mine != ~0ull) atomicMin(key, mine);
        __syncthreads();
        const unsigned long long win = *key;
        if (win == ~0ull) break;                          // no candidate: the rounds end
        wb = (int64_t)(win & 0xFFFFFFFFull);
      }
      if (tid == 0) {
        // where wb enters the slot's field; a keeper also has to pass the test, against the given ufield at its entry into that
        const int cell = -2 - claim_round[wb];
        const int wr = (int)parked[40];
        const int s = claim_cell(fld, W, H, cell, wr);
        bool ok = s >= 0;
        if (a >= 0) ok = keep_passes(fld, (const uint32_t*)unpark(10), W, H, cell, s, wr, parked[32], parked[33]);
        parked[42] = ok ? (uint32_t)s : INF;
      }
      __syncthreads();
      const uint32_t entry = parked[42];
      if (tid == 0) *key = ~0ull;                         // (everybody has read it; the next minimum comes two barriers on)
      if (entry == INF) {
        if (a >= 0) continue;                             // not kept: the robot stays in U, the slot is spent
        break;
      }
      if (tid == 0) {
        const int last = write_rows(wb, per_lane((int)entry), claims, per_lane(a));
        if (last >= 0 && a >= 0) ((int8_t*)unpark(9))[wb] = 1;
        *tgt = last >= 0 ? (uint32_t)last : INF;          // (a fixed point always has a descent: INF cannot happen)
      }
      __syncthreads();
      const uint32_t t = *tgt;
      if (t == INF) break;
      ++claims;
      if (a >= 0) ++keeps;
      if (--left == 0) break;                             // U is used up
      if (slots >= (int)parked[41]) break;
      take_disc((int)t);
    }
    // the followers: still in U
    __syncthreads();
    for (int64_t b = tid; b < B; b += FIELD_THREADS)
      if (claim_round[b] < -1) claim_round[b] = -1;
    if (tid == 0) { ((int32_t*)unpark(14))[0] = claims; ((int32_t*)unpark(15))[0] = keeps; }
  } else if (tid == 0) {
    n_claims[0] = 0; n_kept[0] = 0;
  }
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_assign_keep_utility_lds_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ frontier,
    const uint32_t* __restrict__ field, const int32_t* __restrict__ gain, const uint32_t* __restrict__ ufield, int w_gain, int g_cap,
    int min_gain, const double* __restrict__ start, const int8_t* __restrict__ may_claim, const int32_t* __restrict__ prev_target,
    int r_inflate, int r_claim, int r_keep, int keep_ratio16, int keep_slack, int max_claims, int max_seg, int S_max, double* sub_goals,
    int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell, int32_t* target_gain, int32_t* claim_round,
    int32_t* __restrict__ n_claims, int8_t* __restrict__ kept, int32_t* __restrict__ n_kept) {
  extern __shared__ uint32_t field_lds[];
  assign_keep_utility_body(field_lds + keepu_bitmap_words((int64_t)W * H), field_lds, B, W, H, ox, oy, dx, dy, frontier, field, gain,
                           ufield, w_gain, g_cap, min_gain, start, may_claim, prev_target, r_inflate, r_claim, r_keep, keep_ratio16,
                           keep_slack, max_claims, max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell, target_gain,
                           claim_round, n_claims, kept, n_kept);
}

__global__ void __launch_bounds__(FIELD_THREADS) frontier_assign_keep_utility_global_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ frontier,
    const uint32_t* __restrict__ field, const int32_t* __restrict__ gain, const uint32_t* __restrict__ ufield, int w_gain, int g_cap,
    int min_gain, const double* __restrict__ start, const int8_t* __restrict__ may_claim, const int32_t* __restrict__ prev_target,
    int r_inflate, int r_claim, int r_keep, int keep_ratio16, int keep_slack, int max_claims, int max_seg, int S_max, uint32_t* work,
    double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell, int32_t* target_gain,
    int32_t* claim_round, int32_t* __restrict__ n_claims, int8_t* __restrict__ kept, int32_t* __restrict__ n_kept) {
  extern __shared__ uint32_t field_lds[];
  assign_keep_utility_body(work, field_lds, B, W, H, ox, oy, dx, dy, frontier, field, gain, ufield, w_gain, g_cap, min_gain, start,
                           may_claim, prev_target, r_inflate, r_claim, r_keep, keep_ratio16, keep_slack, max_claims, max_seg, S_max,
                           sub_goals, n_sub, status, path_cost, target_cell, target_gain, claim_round, n_claims, kept, n_kept);
}

// =====================================================================================================================
// WHAT A CALL REFUSES, for every entry point of this translation unit.  A call decides in this order: LIPMPC_E_ARG, LIPMPC_E_UNSUPPORTED
// (a shape beyond the caps), a zero count returns LIPMPC_OK, then the device is selected -- the first HIP call: nothing is enqueued
// before.  Each family of arguments states its legal range ONCE, as a bad_*() predicate that is true for E_ARG; an entry point is a
// short list of families, a cap and its launches.  All E_ARG share one code, so their order cannot be seen; what CAN be seen, and
// differs from call to call, is whether the pointers are tested EARLY or only behind the caps and the zero count (LATE): each call
// says which where it does it, and tests/test_field_refusals_build.py pins all of it.
constexpr int64_t TILED_MAX_CELLS = 1 << 24;          // of the tiled calls: a finite value stays below 7 * 2^24, the additions cannot wrap
constexpr int64_t TILED_MAX_THREADS = (int64_t)1 << 31;                   // of one launch: F * (W * H + 64) stays within it
constexpr int MAX_ROUNDS = 65536;
constexpr int64_t CLAIM_MAX_LAUNCHES = 1 << 20;       // max_claims * max_rounds of one tiled claim call

template <typename... P> inline bool any_null(const P*... p) { return (... || !p); }

inline bool bad_count(int64_t n) { return n < 0 || n > 0x7fffffff; }
inline bool bad_shape(int32_t W, int32_t H) { return W < 2 || H < 2; }
inline bool bad_grid(int32_t W, int32_t H, int32_t r_inflate) { return bad_shape(W, H) || r_inflate < 0 || r_inflate > R_INFLATE_MAX; }
// a grid's placement, read on the host
bool bad_placement(const double* origin, const double* cell) {
  if (!origin || !cell) return true;
  const double ox = origin[0], oy = origin[1], dx = cell[0], dy = cell[1];
  return !(dx > 0.0) || !(dy > 0.0) || !(dx < INFINITY) || !(dy < INFINITY) || !(fabs(ox) < INFINITY) || !(fabs(oy) < INFINITY);
}
inline bool bad_placed_grid(int32_t W, int32_t H, const double* origin, const double* cell, int32_t r_inflate) {
  return bad_grid(W, H, r_inflate) || bad_placement(origin, cell);
}
inline bool bad_threshold(int32_t t) { return t < 1 || t > THRESHOLD_MAX; }            // t_free, t_occ
inline bool bad_min_unknown(int32_t min_unknown) { return min_unknown < 1 || min_unknown > 8; }
inline bool bad_view(int32_t r_view) { return r_view < 1 || r_view > R_VIEW_MAX; }
inline bool bad_walk(int32_t max_seg, int32_t S_max) { return max_seg < 5 || S_max < 1; }
// a path call: B robots down one shared field or down a field each
inline bool bad_path(int64_t B, int64_t F, int32_t max_seg, int32_t S_max) {
  return bad_count(B) || (F != 1 && F != B) || bad_walk(max_seg, S_max);
}
// a claim call, one-workgroup or tiled: its scalars and the pointers that the form needs (never `may_claim`), EARLY in every form
template <typename... P> bool bad_claim(int64_t B, int32_t r_claim, int32_t max_claims, int32_t max_seg, int32_t S_max, const P*... needed) {
  return bad_count(B) || r_claim < 0 || r_claim > MAX_SIDE || max_claims < 0 || max_claims > 4096 || bad_walk(max_seg, S_max) ||
         any_null(needed...);
}
inline bool bad_keep(int32_t r_keep, int32_t keep_ratio16, int32_t keep_slack) {
  return r_keep < 0 || r_keep > R_KEEP_MAX || keep_ratio16 < KEEP_RATIO_MIN || keep_ratio16 > KEEP_RATIO_MAX || keep_slack < 0 ||
         keep_slack > KEEP_SLACK_MAX;
}
inline bool bad_gain(int32_t w_gain, int32_t g_cap, int32_t min_gain) {
  return w_gain < 0 || w_gain > W_GAIN_MAX || g_cap < 1 || g_cap > G_CAP_MAX || min_gain < 0 || min_gain > G_CAP_MAX;
}
// the rounds of a tiled call: max_rounds, and `resume` where the call has it
inline bool bad_rounds(int32_t rounds, int32_t resume = 0) { return rounds < 1 || rounds > MAX_ROUNDS || (resume != 0 && resume != 1); }
// what a claim call on a large map adds: a workspace that starts on 8 bytes (its 64-bit keys) and the rounds ...
bool bad_claim_rounds(const void* work, int32_t rounds, int32_t resume = 0) { return ((uintptr_t)work & 7) != 0 || bad_rounds(rounds, resume); }
// ... and, where every claim relaxes a field of its own, max_claims * max_rounds launches
inline bool too_many_launches(int32_t max_claims, int32_t max_rounds) { return (int64_t)max_claims * max_rounds > CLAIM_MAX_LAUNCHES; }

// the caps, behind every E_ARG: of the one-workgroup calls ...
int group_cap_refusal(int32_t W, int32_t H) {
  return W > MAX_SIDE || H > MAX_SIDE || (int64_t)W * H > MAX_CELLS ? LIPMPC_E_UNSUPPORTED : LIPMPC_OK;
}
// ... and of the tiled calls, for F fields of the shape
int tiled_cap_refusal(int64_t F, int32_t W, int32_t H) {
  if (W > MAX_SIDE || H > MAX_SIDE || (int64_t)W * H > TILED_MAX_CELLS) return LIPMPC_E_UNSUPPORTED;
  if (F > 0 && F * ((int64_t)W * H + 64) > TILED_MAX_THREADS) return LIPMPC_E_UNSUPPORTED;
  return LIPMPC_OK;
}
// what the one-workgroup calls with a placed grid refuse about it: E_ARG, then the caps
int grid_refusal(int32_t W, int32_t H, const double* origin, const double* cell, int32_t r_inflate) {
  return bad_placed_grid(W, H, origin, cell, r_inflate) ? LIPMPC_E_ARG : group_cap_refusal(W, H);
}
// what the path calls on large maps (tiled, weighted, wave) refuse about their shape: E_ARG, then the tiled caps for F fields -- a
// path call needs no LDS sized to the map
int tiled_path_refusal(int64_t B, int64_t F, int32_t W, int32_t H, const double* origin, const double* cell, int32_t r_inflate,
                       int32_t max_seg, int32_t S_max) {
  if (bad_path(B, F, max_seg, S_max) || bad_placed_grid(W, H, origin, cell, r_inflate)) return LIPMPC_E_ARG;
  return tiled_cap_refusal(F, W, H);
}

// LAUNCH SET-UP.  A kernel's dynamic LDS above 64 KiB needs leave; false where the runtime refuses it (LIPMPC_E_HIP)
template <typename Kernel> bool lds_allowed(Kernel kernel, size_t lds) {
  return lds <= 64 * 1024 || hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}
inline int launched() { return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP; }
inline dim3 path_grid(int64_t B) { return dim3((unsigned)((B + PATH_THREADS - 1) / PATH_THREADS)); }
// one of a pair of FIELD_THREADS kernels with the same arguments: the field in LDS (`lds` bytes, sized to the map) or in global memory
template <typename Kernel, typename... Args>
int launch_field(bool in_lds, Kernel lds_kernel, Kernel global_kernel, int64_t F, size_t lds, void* hip_stream, Args... args) {
  if (in_lds && !lds_allowed(lds_kernel, lds)) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(in_lds ? lds_kernel : global_kernel, dim3((unsigned)F), dim3(FIELD_THREADS), lds, (hipStream_t)hip_stream, args...);
  return launched();
}

}  // namespace

extern "C" int lipmpc_grid_field_batch(int device, int64_t F, int32_t W, int32_t H, int32_t grid_shared, const double* origin,
                                       const double* cell, const uint8_t* occ, const double* goal, int32_t r_inflate,
                                       uint32_t* field, int32_t* field_status, void* hip_stream) {
  if (bad_count(F)) return LIPMPC_E_ARG;
  if (const int rc = grid_refusal(W, H, origin, cell, r_inflate)) return rc;
  if (F == 0) return LIPMPC_OK;
  if (any_null(occ, goal, field, field_status)) return LIPMPC_E_ARG;          // LATE: F == 0 passes with any of them null
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  const int64_t ncells = (int64_t)W * H, stride = grid_shared ? 0 : ncells;
  const bool in_lds = field_fits_lds(ncells);
  return launch_field(in_lds, grid_field_lds_kernel, grid_field_global_kernel, F, (size_t)field_lds_bytes(ncells, in_lds), hip_stream, W, H,
                      stride, origin[0], origin[1], cell[0], cell[1], occ, goal, r_inflate, field, field_status);
}

extern "C" int lipmpc_grid_path_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin, const double* cell,
                                      const uint8_t* occ, int32_t grid_shared, const uint32_t* field, const int32_t* field_status,
                                      const double* goal, const double* start, int32_t r_inflate, int32_t max_seg, int32_t S_max,
                                      double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, void* hip_stream) {
  if (bad_path(B, F, max_seg, S_max)) return LIPMPC_E_ARG;
  if (const int rc = grid_refusal(W, H, origin, cell, r_inflate)) return rc;
  if (B == 0) return LIPMPC_OK;
  // LATE: B == 0 passes with any of them null
  if (any_null(occ, field, field_status, goal, start, sub_goals, n_sub, status, path_cost)) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(grid_path_kernel, path_grid(B), dim3(PATH_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H,
                     grid_shared ? (int64_t)0 : (int64_t)W * H, origin[0], origin[1], cell[0], cell[1], occ, field, field_status, goal, start,
                     r_inflate, max_seg, S_max, sub_goals, n_sub, status, path_cost);
  return launched();
}

extern "C" int lipmpc_grid_frontier_field_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence, int32_t t_free,
                                                int32_t t_occ, int32_t r_inflate, int32_t min_unknown, uint8_t* frontier,
                                                uint32_t* field, int32_t* n_frontier, void* hip_stream) {
  // (the pointers EARLY, unlike lipmpc_grid_field_batch: a null one is E_ARG whatever the shape and F; `frontier` may be null)
  if (bad_count(F) || bad_grid(W, H, r_inflate) || bad_threshold(t_free) || bad_threshold(t_occ) || bad_min_unknown(min_unknown) ||
      any_null(evidence, field, n_frontier))
    return LIPMPC_E_ARG;
  if (const int rc = group_cap_refusal(W, H)) return rc;
  if (F == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  const int64_t ncells = (int64_t)W * H;
  const bool in_lds = frontier_fits_lds(ncells);
  return launch_field(in_lds, frontier_field_lds_kernel, frontier_field_global_kernel, F, (size_t)frontier_lds_bytes(ncells, in_lds),
                      hip_stream, W, H, evidence, t_free, t_occ, r_inflate, min_unknown, frontier, field, n_frontier);
}

extern "C" int lipmpc_grid_frontier_path_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                               const double* cell, const int32_t* evidence, int32_t t_occ, const uint32_t* field,
                                               const int32_t* n_frontier, const double* start, int32_t r_inflate, int32_t max_seg,
                                               int32_t S_max, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                               int32_t* target_cell, void* hip_stream) {
  if (bad_path(B, F, max_seg, S_max) || bad_threshold(t_occ)) return LIPMPC_E_ARG;
  if (const int rc = grid_refusal(W, H, origin, cell, r_inflate)) return rc;
  if (B == 0) return LIPMPC_OK;
  // LATE: B == 0 passes with any of them null
  if (any_null(evidence, field, n_frontier, start, sub_goals, n_sub, status, path_cost, target_cell)) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(frontier_path_kernel, path_grid(B), dim3(PATH_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H, origin[0],
                     origin[1], cell[0], cell[1], evidence, t_occ, field, n_frontier, start, r_inflate, max_seg, S_max, sub_goals, n_sub,
                     status, path_cost, target_cell);
  return launched();
}

extern "C" int lipmpc_grid_frontier_assign_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                                 const uint8_t* frontier, const uint32_t* field, const double* start,
                                                 const int8_t* may_claim, int32_t r_inflate, int32_t r_claim, int32_t max_claims,
                                                 int32_t max_seg, int32_t S_max, uint32_t* work, double* sub_goals, int32_t* n_sub,
                                                 int32_t* status, double* path_cost, int32_t* target_cell, int32_t* claim_round,
                                                 int32_t* n_claims, void* hip_stream) {
  // (the pointers EARLY in every claim call, `work` included even where the field will fit LDS)
  if (bad_claim(B, r_claim, max_claims, max_seg, S_max, frontier, field, start, work, sub_goals, n_sub, status, path_cost, target_cell,
                claim_round, n_claims))
    return LIPMPC_E_ARG;
  if (const int rc = grid_refusal(W, H, origin, cell, r_inflate)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t ncells = (int64_t)W * H;
  const bool in_lds = assign_fits_lds(ncells);
  const size_t lds = (size_t)assign_lds_bytes(ncells, in_lds);
  if (in_lds) {                                         // (the pair differs by `work`: two launches)
    if (!lds_allowed(frontier_assign_lds_kernel, lds)) return LIPMPC_E_HIP;
    hipLaunchKernelGGL(frontier_assign_lds_kernel, dim3(1), dim3(FIELD_THREADS), lds, s, B, W, H, origin[0], origin[1], cell[0], cell[1],
                       frontier, field, start, may_claim, r_inflate, r_claim, max_claims, max_seg, S_max, sub_goals, n_sub, status,
                       path_cost, target_cell, claim_round, n_claims);
  } else {
    hipLaunchKernelGGL(frontier_assign_global_kernel, dim3(1), dim3(FIELD_THREADS), lds, s, B, W, H, origin[0], origin[1], cell[0],
                       cell[1], frontier, field, start, may_claim, r_inflate, r_claim, max_claims, max_seg, S_max, work, sub_goals,
                       n_sub, status, path_cost, target_cell, claim_round, n_claims);
  }
  return launched();
}

extern "C" int lipmpc_grid_frontier_assign_keep_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                                      const uint8_t* frontier, const uint32_t* field, const double* start,
                                                      const int8_t* may_claim, const int32_t* prev_target, int32_t r_inflate,
                                                      int32_t r_claim, int32_t r_keep, int32_t keep_ratio16, int32_t keep_slack,
                                                      int32_t max_claims, int32_t max_seg, int32_t S_max, uint32_t* work,
                                                      double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                                      int32_t* target_cell, int32_t* claim_round, int32_t* n_claims, int8_t* kept,
                                                      int32_t* n_kept, void* hip_stream) {
  if (bad_claim(B, r_claim, max_claims, max_seg, S_max, frontier, field, start, prev_target, work, sub_goals, n_sub, status, path_cost,
                target_cell, claim_round, n_claims, kept, n_kept) ||
      bad_keep(r_keep, keep_ratio16, keep_slack))
    return LIPMPC_E_ARG;
  if (const int rc = grid_refusal(W, H, origin, cell, r_inflate)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t ncells = (int64_t)W * H;
  const bool in_lds = keep_fits_lds(ncells);
  const size_t lds = (size_t)keep_lds_bytes(ncells, in_lds);
  if (in_lds) {
    if (!lds_allowed(frontier_assign_keep_lds_kernel, lds)) return LIPMPC_E_HIP;
    hipLaunchKernelGGL(frontier_assign_keep_lds_kernel, dim3(1), dim3(FIELD_THREADS), lds, s, B, W, H, origin[0], origin[1], cell[0],
                       cell[1], frontier, field, start, may_claim, prev_target, r_inflate, r_claim, r_keep, keep_ratio16, keep_slack,
                       max_claims, max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell, claim_round, n_claims, kept, n_kept);
  } else {
    hipLaunchKernelGGL(frontier_assign_keep_global_kernel, dim3(1), dim3(FIELD_THREADS), lds, s, B, W, H, origin[0], origin[1], cell[0],
                       cell[1], frontier, field, start, may_claim, prev_target, r_inflate, r_claim, r_keep, keep_ratio16, keep_slack,
                       max_claims, max_seg, S_max, work, sub_goals, n_sub, status, path_cost, target_cell, claim_round, n_claims, kept,
                       n_kept);
  }
  return launched();
}

extern "C" int lipmpc_grid_frontier_gain_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence, int32_t t_free,
                                               int32_t t_occ, const uint8_t* frontier, int32_t r_view, int32_t* gain, void* hip_stream) {
  if (bad_count(F) || bad_shape(W, H) || bad_threshold(t_free) || bad_threshold(t_occ) || bad_view(r_view) ||
      any_null(evidence, frontier, gain))                 // (the pointers EARLY)
    return LIPMPC_E_ARG;
  if (const int rc = group_cap_refusal(W, H)) return rc;
  if (F == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  const int64_t ncells = (int64_t)W * H;
  const size_t lds = (size_t)gain_lds_bytes(ncells, r_view);
  if (!lds_allowed(frontier_gain_kernel, lds)) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(frontier_gain_kernel, dim3((unsigned)F, (unsigned)((ncells + GAIN_CHUNK - 1) / GAIN_CHUNK)), dim3(GAIN_THREADS), lds,
                     (hipStream_t)hip_stream, W, H, evidence, t_free, t_occ, frontier, r_view, gain);
  return launched();
}

extern "C" int lipmpc_grid_frontier_utility_field_batch(int device, int64_t F, int32_t W, int32_t H, const uint8_t* frontier,
                                                        const uint32_t* field, const int32_t* gain, int32_t w_gain, int32_t g_cap,
                                                        int32_t min_gain, uint32_t* ufield, int32_t* n_sources, void* hip_stream) {
  if (bad_count(F) || bad_shape(W, H) || bad_gain(w_gain, g_cap, min_gain) || any_null(frontier, field, gain, ufield, n_sources))
    return LIPMPC_E_ARG;                                  // (the pointers EARLY)
  if (const int rc = group_cap_refusal(W, H)) return rc;
  if (F == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  const int64_t ncells = (int64_t)W * H;
  const bool in_lds = utility_fits_lds(ncells);
  return launch_field(in_lds, frontier_utility_lds_kernel, frontier_utility_global_kernel, F, (size_t)utility_lds_bytes(ncells, in_lds),
                      hip_stream, W, H, frontier, field, gain, w_gain, g_cap, min_gain, ufield, n_sources);
}

extern "C" int lipmpc_grid_frontier_utility_path_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                                       const double* cell, const int32_t* evidence, int32_t t_occ, const uint8_t* frontier,
                                                       const int32_t* gain, const uint32_t* ufield, const int32_t* n_sources,
                                                       int32_t w_gain, int32_t g_cap, int32_t min_gain, const double* start,
                                                       int32_t r_inflate, int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub,
                                                       int32_t* status, double* path_cost, int32_t* target_cell, int32_t* target_gain,
                                                       void* hip_stream) {
  // (the pointers EARLY, unlike the two path calls above: B == 0 with a null one is E_ARG)
  if (bad_path(B, F, max_seg, S_max) || bad_threshold(t_occ) || bad_gain(w_gain, g_cap, min_gain) ||
      any_null(evidence, frontier, gain, ufield, n_sources, start, sub_goals, n_sub, status, path_cost, target_cell, target_gain))
    return LIPMPC_E_ARG;
  if (const int rc = grid_refusal(W, H, origin, cell, r_inflate)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(frontier_utility_path_kernel, path_grid(B), dim3(PATH_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H,
                     origin[0], origin[1], cell[0], cell[1], evidence, t_occ, frontier, gain, ufield, n_sources, w_gain, g_cap, min_gain,
                     start, r_inflate, max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell, target_gain);
  return launched();
}

extern "C" int lipmpc_grid_frontier_assign_utility_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin,
                                                         const double* cell, const uint8_t* frontier, const uint32_t* field,
                                                         const double* start, const int8_t* may_claim, int32_t r_inflate,
                                                         int32_t r_claim, int32_t max_claims, int32_t max_seg, int32_t S_max,
                                                         uint32_t* work, double* sub_goals, int32_t* n_sub, int32_t* status,
                                                         double* path_cost, int32_t* target_cell, int32_t* claim_round,
                                                         int32_t* n_claims, const int32_t* gain, int32_t w_gain, int32_t g_cap,
                                                         int32_t min_gain, int32_t* target_gain, void* hip_stream) {
  if (bad_claim(B, r_claim, max_claims, max_seg, S_max, frontier, field, start, work, sub_goals, n_sub, status, path_cost, target_cell,
                claim_round, n_claims, gain, target_gain) ||
      bad_gain(w_gain, g_cap, min_gain))
    return LIPMPC_E_ARG;
  if (const int rc = grid_refusal(W, H, origin, cell, r_inflate)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t ncells = (int64_t)W * H;
  const bool in_lds = uclaim_fits_lds(ncells);
  const size_t lds = (size_t)uclaim_lds_bytes(ncells, in_lds);
  if (in_lds) {
    if (!lds_allowed(frontier_assign_utility_lds_kernel, lds)) return LIPMPC_E_HIP;
    hipLaunchKernelGGL(frontier_assign_utility_lds_kernel, dim3(1), dim3(FIELD_THREADS), lds, s, B, W, H, origin[0], origin[1], cell[0],
                       cell[1], frontier, field, gain, w_gain, g_cap, min_gain, start, may_claim, r_inflate, r_claim, max_claims, max_seg,
                       S_max, sub_goals, n_sub, status, path_cost, target_cell, target_gain, claim_round, n_claims);
  } else {
    hipLaunchKernelGGL(frontier_assign_utility_global_kernel, dim3(1), dim3(FIELD_THREADS), lds, s, B, W, H, origin[0], origin[1], cell[0],
                       cell[1], frontier, field, gain, w_gain, g_cap, min_gain, start, may_claim, r_inflate, r_claim, max_claims, max_seg,
                       S_max, work, sub_goals, n_sub, status, path_cost, target_cell, target_gain, claim_round, n_claims);
  }
  return launched();
}

extern "C" int lipmpc_grid_frontier_assign_keep_utility_batch(
    int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell, const uint8_t* frontier, const uint32_t* field,
    const double* start, const int8_t* may_claim, const int32_t* prev_target, int32_t r_inflate, int32_t r_claim, int32_t r_keep,
    int32_t keep_ratio16, int32_t keep_slack, int32_t max_claims, int32_t max_seg, int32_t S_max, uint32_t* work, double* sub_goals,
    int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell, int32_t* claim_round, int32_t* n_claims, int8_t* kept,
    int32_t* n_kept, const int32_t* gain, const uint32_t* ufield, int32_t w_gain, int32_t g_cap, int32_t min_gain, int32_t* target_gain,
    void* hip_stream) {
  if (bad_claim(B, r_claim, max_claims, max_seg, S_max, frontier, field, start, prev_target, work, sub_goals, n_sub, status, path_cost,
                target_cell, claim_round, n_claims, kept, n_kept, gain, ufield, target_gain) ||
      bad_keep(r_keep, keep_ratio16, keep_slack) || bad_gain(w_gain, g_cap, min_gain))
    return LIPMPC_E_ARG;
  if (const int rc = grid_refusal(W, H, origin, cell, r_inflate)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t ncells = (int64_t)W * H;
  const bool in_lds = keepu_fits_lds(ncells);
  const size_t lds = (size_t)keepu_lds_bytes(ncells, in_lds);
  if (in_lds) {
    if (!lds_allowed(frontier_assign_keep_utility_lds_kernel, lds)) return LIPMPC_E_HIP;
    hipLaunchKernelGGL(frontier_assign_keep_utility_lds_kernel, dim3(1), dim3(FIELD_THREADS), lds, s, B, W, H, origin[0], origin[1],
                       cell[0], cell[1], frontier, field, gain, ufield, w_gain, g_cap, min_gain, start, may_claim, prev_target, r_inflate,
                       r_claim, r_keep, keep_ratio16, keep_slack, max_claims, max_seg, S_max, sub_goals, n_sub, status, path_cost,
                       target_cell, target_gain, claim_round, n_claims, kept, n_kept);
  } else {
    hipLaunchKernelGGL(frontier_assign_keep_utility_global_kernel, dim3(1), dim3(FIELD_THREADS), lds, s, B, W, H, origin[0], origin[1],
                       cell[0], cell[1], frontier, field, gain, ufield, w_gain, g_cap, min_gain, start, may_claim, prev_target, r_inflate,
                       r_claim, r_keep, keep_ratio16, keep_slack, max_claims, max_seg, S_max, work, sub_goals, n_sub, status, path_cost,
                       target_cell, target_gain, claim_round, n_claims, kept, n_kept);
  }
  return launched();
}

// =====================================================================================================================
// THE TILED FIELD (lipmpc_grid_field_tiled_batch, lipmpc_grid_frontier_field_tiled_batch and their path calls): the same two
// cost-to-go fields relaxed by MANY workgroups, with no cap below 2^24 cells.  The map is cut into tiles of TILE_W x TILE_H
// cells (i x j, j contiguous).  A ROUND is one launch of tiled_round_kernel with one workgroup per (field, tile):
//   - a tile whose flag in the round's `cur` array is 0 returns at once;
//   - an active tile clears its flag, stages its field words and blocked bits with a one-cell halo in LDS, relaxes its own cells
//     to the local fixed point with the halo held, writes back the cells that fell and, for every part of its rim on which a
//     cell fell, sets the flag of the neighbouring tile behind it in the round's `next` array.
// The two flag arrays change places from round to round; workgroups are ordered by the kernel boundaries of the caller's stream
// and by nothing else: nobody waits for a word that another workgroup writes.
//
// WHY THE TILES GIVE DIJKSTRA'S FIELD.  As above, every value a cell ever holds is the cost of a real path to a source and values
// only fall; a cell is written by the workgroup of its own tile only.  A halo word is read (relaxed, agent scope) while its
// owner may be lowering it: the reader gets the old or the new word, both path costs, so what it derives is a path cost too.
// INVARIANT: after every round, a tile whose flag is not set for the next round is at its local fixed point for the halo words
// as they stand at the end of the round.  For if it ran, it reached the fixed point for the halo it read, and a halo word that
// differs at the end of the round fell in this round, on the rim of its owner, which then set this tile's flag; if it did not
// run, it was at its fixed point before and the same holds of its halo.  (Before the first round the flags are set on every
// tile whose cells or halo hold a seed; any other tile holds INF beside INF.)  Hence NO FLAG SET <=> every tile is at its fixed
// point for final halo words <=> the whole map is a fixed point of  f(c) = min over legal moves c -> n of f(n) + cost  with
// f = 0 on the sources: by the argument above that is the least cost, which is unique -- whatever order the races fell in.
// A diagonal move is judged on the BLOCKED BITS of its two side cells, halo included, not on their field words: a side cell in
// another tile may still hold INF although it is unblocked, and the move must be taken all the same (the same fixed point as the
// one-workgroup kernels', where both rules agree once the sweeps have settled).
// THE ROUND GUARANTEE: after R rounds in total a cell holds its final value if some least-cost path from it to a source changes
// tile at most R - 1 times.  By induction on R.  Let the path leave the cell's tile T for the first time by the move x -> y (y
// in another tile; none if the path stays in T).  The rest of the path from y is a least-cost path that changes tile at most
// R - 2 times, so y holds its final value after round R - 1: either from the start (a source, then T's flag was set for round 1)
// or since it fell in some round r <= R - 1, on the rim beside T, which set T's flag for round r + 1.  In the first round in
// which T runs after that, it stages y's final word and relaxes to its local fixed point; the moves of the path inside T are
// legal by blocked bits alone, so every cell of the path in T comes out <= the path's cost, which is the least: final, by
// round R at the latest.
namespace {

constexpr int TILE_W = 32, TILE_H = 64;               // cells of a tile along i and along j
constexpr int TILE_THREADS = 256, TILE_ROWS = TILE_THREADS / TILE_H;      // a thread owns cell (4 k + tid / 64, tid % 64), k = 0..7
constexpr int TILE_OWN = TILE_W / TILE_ROWS;
constexpr int HALO_H = TILE_H + 2, HALO_CELLS = (TILE_W + 2) * HALO_H;    // 34 x 66 = 2244 words, 9 KiB: many workgroups per CU
constexpr int HALO_PADDED = ((HALO_CELLS + 63) / 64) * 64;
constexpr int SETUP_THREADS = 256;
static_assert(TILE_H == 64 && TILE_OWN * TILE_ROWS == TILE_W && TILE_OWN == 8, "the ownership rule and the 8-bit move masks");

// relaxed accesses of agent scope: the global field and the tile flags, read by one workgroup while another writes
__device__ inline uint32_t ld_agent(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void st_agent(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__host__ __device__ inline int tiles_along(int n, int side) { return (n + side - 1) / side; }

// The workspace: per field three bitmaps (solid, unknown, blocked; the goal field uses the first and the last, of map 0 alone on
// a shared grid), then the two flag arrays [F, tiles] each.
// what the rounds read of a workspace, whatever its layout: the tiles of a field, the blocked bitmap, the two flag arrays
struct RoundBuffers {
  int64_t tiles;
  uint32_t *blocked, *flags0, *flags1;
};
template <typename Layout> RoundBuffers round_buffers(const Layout& l, uint32_t* w) { return {l.tiles, w + l.blocked, w + l.flags0, w + l.flags1}; }

struct TiledLayout {
  int64_t bm_words, tiles, solid, unknown, blocked, flags0, flags1, words;
};
inline TiledLayout tiled_layout(int64_t F, int64_t W, int64_t H) {
  TiledLayout l;
  l.bm_words = bitmap_words(W * H);
  l.tiles = (int64_t)tiles_along((int)W, TILE_W) * tiles_along((int)H, TILE_H);
  l.solid = 0;
  l.unknown = F * l.bm_words;
  l.blocked = 2 * F * l.bm_words;
  l.flags0 = 3 * F * l.bm_words;
  l.flags1 = l.flags0 + F * l.tiles;
  l.words = l.flags1 + F * l.tiles;
  return l;
}
// (of a shape within the caps: F * (W * H + 64) <= 2^31, so nothing wraps)
inline int64_t tiled_bytes(int64_t F, int64_t W, int64_t H) { return 4 * tiled_layout(F, W, H).words + 256; }

// set-up, one wave per 64 cells of a map (blockIdx.x = map * chunks + chunk): solid (and unknown) bytes -> bitmap words; both
// flag arrays and n_frontier cleared.  KIND 0: occ bytes; KIND 1: evidence.
template <int KIND>
__global__ void __launch_bounds__(SETUP_THREADS) tiled_bitmaps_kernel(int ncells, int chunks, int64_t F, int64_t tiles,
                                                                      const uint8_t* __restrict__ occ,
                                                                      const int32_t* __restrict__ evidence, int t_free, int t_occ,
                                                                      uint32_t* __restrict__ solid, uint32_t* __restrict__ unk,
                                                                      uint32_t* __restrict__ flags, int32_t* __restrict__ n_frontier) {
  const int64_t m = blockIdx.x / chunks;
  const int chunk = blockIdx.x - (int)m * chunks, tid = threadIdx.x, lane = tid & 63;
  const int words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  const int c = chunk * SETUP_THREADS + tid, c0 = c - lane;
  uint32_t* so = solid + m * words;
  if (c0 < padded) {
    bool is_solid, is_unknown = false;
    if (KIND == 0) {
      is_solid = c < ncells && occ[m * ncells + c] != 0;
    } else {
      const int e = c < ncells ? evidence[m * ncells + c] : 0;
      is_solid = c < ncells && e >= t_occ;
      is_unknown = c < ncells && !is_solid && !(e <= -t_free);
    }
    const uint64_t ms = __ballot(is_solid), mu = __ballot(is_unknown);
    if (lane == 0) {
      so[c0 >> 5] = (uint32_t)ms; so[(c0 >> 5) + 1] = (uint32_t)(ms >> 32);
      if (KIND == 1) { unk[m * words + (c0 >> 5)] = (uint32_t)mu; unk[m * words + (c0 >> 5) + 1] = (uint32_t)(mu >> 32); }
    }
  }
  if (chunk == 0 && tid < 2) {
    so[words - 2 + tid] = 0;
    if (KIND == 1) unk[m * words + words - 2 + tid] = 0;
  }
  if (KIND == 1 && chunk == 0 && tid == 2) n_frontier[m] = 0;
  // the flags of all F fields, both arrays (contiguous), by the blocks of map 0 .. : a grid-stride loop over the whole launch
  const int64_t total = 2 * F * tiles, step = (int64_t)gridDim.x * SETUP_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * SETUP_THREADS + tid; k < total; k += step) flags[k] = 0;
}

// set-up: blocked = solid dilated by the disc (| unknown), on the global bitmaps
template <int KIND>
__global__ void __launch_bounds__(SETUP_THREADS) tiled_blocked_kernel(int W, int H, int chunks, int r_inflate,
                                                                      const uint32_t* __restrict__ solid,
                                                                      const uint32_t* __restrict__ unk, uint32_t* __restrict__ blk) {
  const int64_t m = blockIdx.x / chunks;
  const int chunk = blockIdx.x - (int)m * chunks, tid = threadIdx.x, lane = tid & 63;
  const int ncells = W * H, words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  const int c = chunk * SETUP_THREADS + tid, c0 = c - lane;
  if (c0 < padded) {
    bool b = false;
    if (c < ncells) {
      const int i = c / H, j = c - i * H;
      b = disc_hits(solid + m * words, W, H, i, j, r_inflate);
      if (KIND == 1) b |= bit_of(unk + m * words, c);
    }
    const uint64_t mb = __ballot(b);
    if (lane == 0) { blk[m * words + (c0 >> 5)] = (uint32_t)mb; blk[m * words + (c0 >> 5) + 1] = (uint32_t)(mb >> 32); }
  }
  if (chunk == 0 && tid < 2) blk[m * words + words - 2 + tid] = 0;
}

// a seed at (i, j): the flags of every tile that holds it among its cells or in its halo
__device__ inline void flag_round_seed(uint32_t* flags, int W, int H, int tiles_j, int i, int j) {
  for (int di = -1; di <= 1; ++di)
    for (int dj = -1; dj <= 1; ++dj) {
      const int ii = i + di, jj = j + dj;
      if ((unsigned)ii < (unsigned)W && (unsigned)jj < (unsigned)H) st_agent(flags + (ii / TILE_W) * tiles_j + jj / TILE_H, 1u);
    }
}

// set-up of the goal field: the status, 0 at the goal cell and INF elsewhere, the flags round the goal
__global__ void __launch_bounds__(SETUP_THREADS) tiled_goal_seed_kernel(int W, int H, int chunks, int64_t blk_stride, double ox, double oy,
                                                                        double dx, double dy, const double* __restrict__ goal,
                                                                        const uint32_t* __restrict__ blk, uint32_t* __restrict__ field,
                                                                        int32_t* __restrict__ field_status, uint32_t* __restrict__ flags,
                                                                        int64_t tiles) {
  const int64_t f = blockIdx.x / chunks;
  const int chunk = blockIdx.x - (int)f * chunks, ncells = W * H;
  const int c = chunk * SETUP_THREADS + threadIdx.x;
  int gi = 0, gj = 0;
  const bool inside = cell_of(goal[2 * f], goal[2 * f + 1], ox, oy, dx, dy, W, H, gi, gj);
  const int gc = gi * H + gj;
  const int status = !inside ? LIPMPC_FIELD_GOAL_OUTSIDE : bit_of(blk + f * blk_stride, gc) ? LIPMPC_FIELD_GOAL_BLOCKED : LIPMPC_FIELD_OK;
  if (c == 0) field_status[f] = status;
  if (c >= ncells) return;
  const bool seed = status == LIPMPC_FIELD_OK && c == gc;
  field[f * ncells + c] = seed ? 0u : INF;
  if (seed) flag_round_seed(flags + f * tiles, W, H, tiles_along(H, TILE_H), gi, gj);
}

// set-up of the frontier field: the frontier test of frontier_body on the global bitmaps, 0 on frontier cells and INF elsewhere,
// their count by integer atomics (n_frontier was cleared a kernel earlier), the flags round every frontier cell
__global__ void __launch_bounds__(SETUP_THREADS) tiled_frontier_seed_kernel(int W, int H, int chunks, int min_unknown,
                                                                            const uint32_t* __restrict__ unk,
                                                                            const uint32_t* __restrict__ blk,
                                                                            uint8_t* __restrict__ frontier, uint32_t* __restrict__ field,
                                                                            int32_t* __restrict__ n_frontier, uint32_t* __restrict__ flags,
                                                                            int64_t tiles) {
  const int64_t f = blockIdx.x / chunks;
  const int chunk = blockIdx.x - (int)f * chunks, lane = threadIdx.x & 63;
  const int ncells = W * H, words = (int)bitmap_words(ncells);
  const int c = chunk * SETUP_THREADS + threadIdx.x;
  const uint32_t *un = unk + f * words, *bl = blk + f * words;
  bool fr = false;
  if (c < ncells) {
    const int i = c / H, j = c - i * H;
    if (!bit_of(bl, c)) {
      const int lo = max(j - 1, 0), hi = min(j + 1, H - 1);
      const uint64_t mask = (1ull << (hi - lo + 1)) - 1;
      int cnt = __popcll(window(un, c - j + lo) & mask);
      if (i > 0) cnt += __popcll(window(un, c - H - j + lo) & mask);
      if (i < W - 1) cnt += __popcll(window(un, c + H - j + lo) & mask);
      fr = cnt >= min_unknown;
    }
    field[f * ncells + c] = fr ? 0u : INF;
    if (frontier) frontier[f * ncells + c] = fr;
    if (fr) flag_round_seed(flags + f * tiles, W, H, tiles_along(H, TILE_H), i, j);
  }
  const int mine = __popcll(__ballot(fr));
  if (lane == 0 && mine) atomicAdd(n_frontier + f, mine);            // (integers: the sum is the same in any order)
}

// the byte a path pays for leaving cell c, on top of the step (SOFT CLEARANCE, below)
__device__ inline uint32_t soft_k(const uint8_t* __restrict__ cost, int c) { return min((uint32_t)cost[c], (uint32_t)LIPMPC_COST_MAX); }

// ONE ROUND.  blockIdx.x = field * tiles + tile.  WEIGHTED: the eight cost bytes of a thread's cells ride in one more register and
// are added to what a cell takes; a source holds 0 and never falls, so it pays nothing.  Else `cost` is not read.
template <bool WEIGHTED>
__device__ __forceinline__ void round_body(int W, int H, int tiles_j, int tiles, int64_t blk_stride, const uint32_t* __restrict__ blk,
                                           int64_t cost_stride, const uint8_t* __restrict__ cost, uint32_t* field, uint32_t* cur,
                                           uint32_t* next) {
  __shared__ uint32_t lf[HALO_CELLS];                 // field words, local index l = (li + 1) * HALO_H + lj + 1
  __shared__ uint32_t lb[HALO_PADDED / 32 + 2];       // blocked bits by l; a cell outside the grid is blocked
  __shared__ uint32_t rim;
  const int64_t f = blockIdx.x / tiles;
  const int tile = blockIdx.x - (int)f * tiles, tid = threadIdx.x, lane = tid & 63;
  uint32_t* my_flag = cur + f * tiles + tile;
  if (ld_agent(my_flag) == 0) return;                 // (one word for the whole workgroup: uniform)
  const int ti = tile / tiles_j, tj = tile - ti * tiles_j, i0 = ti * TILE_W, j0 = tj * TILE_H;
  const uint32_t* bl = blk + f * blk_stride;
  uint32_t* fld = field + f * (int64_t)W * H;

  for (int l0 = tid - lane; l0 < HALO_PADDED; l0 += TILE_THREADS) {
    const int l = l0 + lane, li = l / HALO_H, lj = l - li * HALO_H;
    const int gi = i0 + li - 1, gj = j0 + lj - 1;
    const bool in = l < HALO_CELLS && (unsigned)gi < (unsigned)W && (unsigned)gj < (unsigned)H;
    const int gc = in ? gi * H + gj : 0;
    const uint32_t v = ld_agent(fld + gc);
    const uint64_t mb = __ballot(!in || bit_of(bl, gc));
    if (l < HALO_CELLS) lf[l] = in ? v : INF;
    if (lane == 0) { lb[l0 >> 5] = (uint32_t)mb; lb[(l0 >> 5) + 1] = (uint32_t)(mb >> 32); }
  }
  if (tid == 0) rim = 0;
  __syncthreads();                                    // (everybody has read the flag: it is cleared for the round after next)
  if (tid == 0) st_agent(my_flag, 0u);

  // the legal moves of my eight cells, a byte per cell, bit d = neighbour (-1,-1), (-1,0), (-1,1), (0,-1), (0,1), (1,-1), (1,0),
  // (1,1): the neighbour unblocked and, for a diagonal, both side cells unblocked.  0 for a blocked cell.  WEIGHTED: beside them
  // the cells' eight cost bytes, clamped.
  const int l_first = ((tid >> 6) + 1) * HALO_H + (tid & 63) + 1;
  auto open_at = [&](int l) { return ((lb[l >> 5] >> (l & 31)) & 1u) ^ 1u; };       // 1 = unblocked (integers: no lane masks to keep)
  uint64_t moves = 0, costs = 0;
#pragma unroll 1
  for (int k = 0; k < TILE_OWN; ++k) {
    const int l = l_first + k * TILE_ROWS * HALO_H;
    const uint32_t up = open_at(l - HALO_H), dn = open_at(l + HALO_H), lt = open_at(l - 1), rt = open_at(l + 1);
    const uint32_t m = (open_at(l - HALO_H - 1) & up & lt) | up << 1 | (open_at(l - HALO_H + 1) & up & rt) << 2 | lt << 3 | rt << 4 |
                       (open_at(l + HALO_H - 1) & dn & lt) << 5 | dn << 6 | (open_at(l + HALO_H + 1) & dn & rt) << 7;
    const uint32_t mine = m * open_at(l);
    moves |= (uint64_t)mine << (8 * k);
    if constexpr (WEIGHTED) {
      const int gi = i0 + k * TILE_ROWS + (tid >> 6), gj = j0 + (tid & 63);          // (an unblocked cell is inside the grid)
      if (mine) costs |= (uint64_t)soft_k(cost + f * cost_stride, gi * H + gj) << (8 * k);
    }
  }

  // the sweeps of relax(), on my cells, the halo held.
  // WHY THE WEIGHTED ROUNDS GIVE WEIGHTED DIJKSTRA'S FIELD.  The argument of THE TILED FIELD carries over word for word; the cell
  // cost enters in ONE place: a value a cell takes is  k(c) + f(n) + step  for a legal move c -> n, which is the cost of the real
  // path "leave c, then n's path" in the metric where leaving c costs k(c) more.  Values are still path costs and still only fall,
  // so no flag set <=> a fixed point of  f(c) = k(c) + min over legal moves of f(n) + step,  f = 0 on the sources; its finite values
  // are >= the least cost (they are path costs) and <= it (induction along a least-cost path); k >= 0 is an integer, so the least
  // cost is unique and the bits are Dijkstra's.  The round guarantee's induction uses "the rest of a least-cost path is a least-cost
  // path" and "a tile relaxes to its local fixed point", both of which hold in the weighted metric.
  // NO WRAP: a stored value is the cost of a SIMPLE path (a value derived through the cell itself would be larger than the one it
  // holds), at most 2^24 - 1 moves of at most 7 + 248 each; a candidate adds one more: <= 255 * 2^24 < 2^32 - 1 = INF.
  uint32_t fell = 0;
  for (;;) {
    int changed = 0;
#pragma unroll 1
    for (int k = 0; k < TILE_OWN; ++k) {                // (not unrolled: eight cells' lane masks at once overfill the scalar file)
      const uint32_t m = (uint32_t)(moves >> (8 * k)) & 0xFFu;
      if (m) {
        const int l = l_first + k * TILE_ROWS * HALO_H;
        auto via = [&](int bit, int off, uint32_t step) {
          const uint32_t v = ld(lf + l + off);
          return ((m >> bit) & 1u) && v != INF ? v + step : INF;
        };
        const uint32_t cur_v = ld(lf + l);
        uint32_t best = min(min(min(via(0, -HALO_H - 1, DIAGONAL), via(1, -HALO_H, AXIAL)), min(via(2, -HALO_H + 1, DIAGONAL), via(3, -1, AXIAL))),
                            min(min(via(4, 1, AXIAL), via(5, HALO_H - 1, DIAGONAL)), min(via(6, HALO_H, AXIAL), via(7, HALO_H + 1, DIAGONAL))));
        if constexpr (WEIGHTED) best = best == INF ? INF : best + ((uint32_t)(costs >> (8 * k)) & 0xFFu);      // THE CELL COST ENTERS HERE
        if (best < cur_v) { st(lf + l, best); changed = 1; fell |= 1u << k; }
      }
    }
    if (!__syncthreads_or(changed)) break;
  }

  // write back what fell; which parts of the rim fell: bit 0 top, 1 bottom, 2 left, 3 right, 4..7 the corners
  uint32_t r = 0;
  const int lj = tid & 63;
#pragma unroll
  for (int k = 0; k < TILE_OWN; ++k)
    if ((fell >> k) & 1u) {
      const int li = k * TILE_ROWS + (tid >> 6);
      st_agent(fld + (i0 + li) * H + j0 + lj, lf[l_first + k * TILE_ROWS * HALO_H]);
      const bool top = li == 0, bot = li == TILE_W - 1, lft = lj == 0, rgt = lj == TILE_H - 1;
      r |= (uint32_t)top | (uint32_t)bot << 1 | (uint32_t)lft << 2 | (uint32_t)rgt << 3 | (uint32_t)(top & lft) << 4 |
           (uint32_t)(top & rgt) << 5 | (uint32_t)(bot & lft) << 6 | (uint32_t)(bot & rgt) << 7;
    }
  if (r) atomicOr(&rim, r);
  __syncthreads();
  if (tid < 8 && ((rim >> tid) & 1u)) {
    const int di = tid == 0 || tid == 4 || tid == 5 ? -1 : tid == 1 || tid == 6 || tid == 7 ? 1 : 0;
    const int dj = tid == 2 || tid == 4 || tid == 6 ? -1 : tid == 3 || tid == 5 || tid == 7 ? 1 : 0;
    const int ni = ti + di, nj = tj + dj;
    if ((unsigned)ni < (unsigned)(tiles / tiles_j) && (unsigned)nj < (unsigned)tiles_j) st_agent(next + f * tiles + ni * tiles_j + nj, 1u);
  }
}

__global__ void __launch_bounds__(TILE_THREADS) tiled_round_kernel(
    int W, int H, int tiles_j, int tiles, int64_t blk_stride, const uint32_t* __restrict__ blk, uint32_t* field, uint32_t* cur,
    uint32_t* next) {
  round_body<false>(W, H, tiles_j, tiles, blk_stride, blk, 0, nullptr, field, cur, next);
}

__global__ void __launch_bounds__(TILE_THREADS) soft_round_kernel(
    int W, int H, int tiles_j, int tiles, int64_t blk_stride, const uint32_t* __restrict__ blk, int64_t cost_stride,
    const uint8_t* __restrict__ cost, uint32_t* field, uint32_t* cur, uint32_t* next) {
  round_body<true>(W, H, tiles_j, tiles, blk_stride, blk, cost_stride, cost, field, cur, next);
}

// after the call's last round: settled[f] = no flag of field f set in `live`; with `swap` the flags move to array 0, where the
// next call's first round reads them.  blockIdx.x = field.
__global__ void __launch_bounds__(SETUP_THREADS) tiled_settle_kernel(int tiles, int swap, uint32_t* flags0, uint32_t* flags1,
                                                                     int32_t* __restrict__ settled) {
  const int64_t f = blockIdx.x;
  uint32_t *a0 = flags0 + f * tiles, *a1 = flags1 + f * tiles;
  int any = 0;
  for (int t = threadIdx.x; t < tiles; t += SETUP_THREADS) {
    const uint32_t v = swap ? a1[t] : a0[t];
    if (swap) { a0[t] = v; a1[t] = 0; }
    any |= v != 0;
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) settled[f] = !any;
}

__global__ void __launch_bounds__(PATH_THREADS) tiled_goal_descent_kernel(int64_t B, int one_field, int W, int H, int64_t occ_stride,
                                                                          double ox, double oy, double dx, double dy,
                                                                          const uint8_t* __restrict__ occ,
                                                                          const uint32_t* __restrict__ field,
                                                                          const int32_t* __restrict__ field_status,
                                                                          const int32_t* __restrict__ settled,
                                                                          const double* __restrict__ goal, const double* __restrict__ start,
                                                                          int r_inflate, int max_seg, int S_max,
                                                                          double* __restrict__ sub_goals, int32_t* __restrict__ n_sub,
                                                                          int32_t* __restrict__ status, double* __restrict__ path_cost) {
  grid_path_body<false>(B, one_field, W, H, occ_stride, ox, oy, dx, dy, occ, nullptr, field, field_status, settled, goal, start, r_inflate,
                        max_seg, S_max, sub_goals, n_sub, status, path_cost);
}

__global__ void __launch_bounds__(PATH_THREADS) tiled_frontier_descent_kernel(int64_t B, int one_field, int W, int H, double ox, double oy,
                                                                              double dx, double dy, const int32_t* __restrict__ evidence,
                                                                              int t_occ, const uint32_t* __restrict__ field,
                                                                              const int32_t* __restrict__ n_frontier,
                                                                              const int32_t* __restrict__ settled,
                                                                              const double* __restrict__ start, int r_inflate, int max_seg,
                                                                              int S_max, double* __restrict__ sub_goals,
                                                                              int32_t* __restrict__ n_sub, int32_t* __restrict__ status,
                                                                              double* __restrict__ path_cost,
                                                                              int32_t* __restrict__ target_cell) {
  frontier_path_body<false>(B, one_field, W, H, ox, oy, dx, dy, evidence, nullptr, t_occ, field, n_frontier, settled, start, r_inflate,
                            max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell);
}

// the two path bodies, WEIGHTED (SOFT CLEARANCE, below)
__global__ void __launch_bounds__(PATH_THREADS) soft_goal_descent_kernel(
    int64_t B, int one_field, int W, int H, int64_t occ_stride, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ occ,
    const uint8_t* __restrict__ cost, const uint32_t* __restrict__ field, const int32_t* __restrict__ field_status,
    const int32_t* __restrict__ settled, const double* __restrict__ goal, const double* __restrict__ start, int r_inflate, int max_seg,
    int S_max, double* __restrict__ sub_goals, int32_t* __restrict__ n_sub, int32_t* __restrict__ status, double* __restrict__ path_cost) {
  grid_path_body<true>(B, one_field, W, H, occ_stride, ox, oy, dx, dy, occ, cost, field, field_status, settled, goal, start, r_inflate,
                       max_seg, S_max, sub_goals, n_sub, status, path_cost);
}

__global__ void __launch_bounds__(PATH_THREADS) soft_frontier_descent_kernel(
    int64_t B, int one_field, int W, int H, double ox, double oy, double dx, double dy, const int32_t* __restrict__ evidence,
    const uint8_t* __restrict__ cost, int t_occ, const uint32_t* __restrict__ field, const int32_t* __restrict__ n_frontier,
    const int32_t* __restrict__ settled, const double* __restrict__ start, int r_inflate, int max_seg, int S_max,
    double* __restrict__ sub_goals, int32_t* __restrict__ n_sub, int32_t* __restrict__ status, double* __restrict__ path_cost,
    int32_t* __restrict__ target_cell) {
  frontier_path_body<true>(B, one_field, W, H, ox, oy, dx, dy, evidence, cost, t_occ, field, n_frontier, settled, start, r_inflate, max_seg,
                           S_max, sub_goals, n_sub, status, path_cost, target_cell);
}

// what the two tiled field calls add to their refusals: E_ARG, then the caps; a `work` too small for a shape within the caps is
// E_ARG (beyond them no size is defined)
int tiled_refusal(int64_t F, int32_t W, int32_t H, const void* work, int64_t work_bytes, int32_t max_rounds, int32_t resume,
                  const int32_t* settled) {
  if (any_null(work, settled) || bad_rounds(max_rounds, resume)) return LIPMPC_E_ARG;
  if (const int rc = tiled_cap_refusal(F, W, H)) return rc;
  return work_bytes < tiled_bytes(F, W, H) ? LIPMPC_E_ARG : LIPMPC_OK;
}

// the rounds and the settle kernel; with a cost layer (`cost` not null, `cost_stride` bytes from field to field) the weighted rounds
int tiled_rounds(hipStream_t s, int64_t F, int W, int H, int64_t blk_stride, const RoundBuffers& b, uint32_t* field, int max_rounds,
                 int32_t* settled, const uint8_t* cost = nullptr, int64_t cost_stride = 0) {
  const int tiles = (int)b.tiles, tiles_j = tiles_along(H, TILE_H);
  const dim3 grid((unsigned)(F * tiles)), block(TILE_THREADS);
  uint32_t* flags[2] = {b.flags0, b.flags1};
  for (int r = 0; r < max_rounds; ++r) {
    if (cost)
      hipLaunchKernelGGL(soft_round_kernel, grid, block, 0, s, W, H, tiles_j, tiles, blk_stride, b.blocked, cost_stride, cost, field,
                         flags[r & 1], flags[(r + 1) & 1]);
    else
      hipLaunchKernelGGL(tiled_round_kernel, grid, block, 0, s, W, H, tiles_j, tiles, blk_stride, b.blocked, field, flags[r & 1],
                         flags[(r + 1) & 1]);
  }
  hipLaunchKernelGGL(tiled_settle_kernel, dim3((unsigned)F), dim3(SETUP_THREADS), 0, s, tiles, max_rounds & 1, flags[0], flags[1], settled);
  return launched();
}

// what a tiled field call derives from its shape: the workspace's layout, the set-up launches' blocks per map (a wave per 64 cells
// of the padded map), the maps to set up and the stride of their blocked bitmaps (one map, stride 0, on a shared grid)
struct TiledCall {
  TiledLayout l;
  int ncells, chunks;
  int64_t maps, blk_stride;
  uint32_t* w;
};
TiledCall tiled_call(int64_t F, int W, int H, bool shared, void* work) {
  const TiledLayout l = tiled_layout(F, W, H);
  return {l, W * H, ((int)(l.bm_words - 2) * 32 + SETUP_THREADS - 1) / SETUP_THREADS, shared ? 1 : F, shared ? 0 : l.bm_words, (uint32_t*)work};
}

// the first two set-up launches of the frontier kind (the frontier and the utility field): the bitmaps of the evidence, `counter`
// cleared, then the blocked bitmap
void frontier_bitmaps(hipStream_t s, const TiledCall& t, int64_t F, int W, int H, const int32_t* evidence, int t_free, int t_occ,
                      int r_inflate, int32_t* counter) {
  const TiledLayout& l = t.l;
  const dim3 grid((unsigned)(F * t.chunks)), block(SETUP_THREADS);
  hipLaunchKernelGGL(tiled_bitmaps_kernel<1>, grid, block, 0, s, t.ncells, t.chunks, F, l.tiles, (const uint8_t*)nullptr, evidence, t_free,
                     t_occ, t.w + l.solid, t.w + l.unknown, t.w + l.flags0, counter);
  hipLaunchKernelGGL(tiled_blocked_kernel<1>, grid, block, 0, s, W, H, t.chunks, r_inflate, t.w + l.solid, t.w + l.unknown, t.w + l.blocked);
}

// lipmpc_grid_field_tiled_batch and, `weighted`, lipmpc_grid_field_weighted_batch: a null `cost` is E_ARG for the latter alone
int goal_field(int device, int64_t F, int32_t W, int32_t H, int32_t grid_shared, const double* origin, const double* cell,
               const uint8_t* occ, bool weighted, const uint8_t* cost, const double* goal, int32_t r_inflate, uint32_t* field,
               int32_t* field_status, void* work, int64_t work_bytes, int32_t max_rounds, int32_t resume, int32_t* settled,
               void* hip_stream) {
  // (the pointers EARLY, unlike lipmpc_grid_field_batch)
  if (bad_count(F) || bad_placed_grid(W, H, origin, cell, r_inflate) || any_null(occ, goal, field, field_status) || (weighted && !cost))
    return LIPMPC_E_ARG;
  if (const int rc = tiled_refusal(F, W, H, work, work_bytes, max_rounds, resume, settled)) return rc;
  if (F == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const TiledCall t = tiled_call(F, W, H, grid_shared != 0, work);
  const TiledLayout& l = t.l;
  if (!resume) {
    const dim3 maps((unsigned)(t.maps * t.chunks)), block(SETUP_THREADS);
    hipLaunchKernelGGL(tiled_bitmaps_kernel<0>, maps, block, 0, s, t.ncells, t.chunks, F, l.tiles, occ, (const int32_t*)nullptr, 0, 0,
                       t.w + l.solid, t.w + l.unknown, t.w + l.flags0, (int32_t*)nullptr);
    hipLaunchKernelGGL(tiled_blocked_kernel<0>, maps, block, 0, s, W, H, t.chunks, r_inflate, t.w + l.solid, t.w + l.unknown,
                       t.w + l.blocked);
    hipLaunchKernelGGL(tiled_goal_seed_kernel, dim3((unsigned)(F * t.chunks)), block, 0, s, W, H, t.chunks, t.blk_stride, origin[0],
                       origin[1], cell[0], cell[1], goal, t.w + l.blocked, field, field_status, t.w + l.flags0, l.tiles);
  }
  return tiled_rounds(s, F, W, H, t.blk_stride, round_buffers(l, t.w), field, max_rounds, settled, weighted ? cost : nullptr,
                      grid_shared ? (int64_t)0 : (int64_t)t.ncells);
}

// lipmpc_grid_frontier_field_tiled_batch and, `weighted`, lipmpc_grid_frontier_field_weighted_batch
int frontier_field(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence, bool weighted, const uint8_t* cost, int32_t t_free,
                   int32_t t_occ, int32_t r_inflate, int32_t min_unknown, uint8_t* frontier, uint32_t* field, int32_t* n_frontier,
                   void* work, int64_t work_bytes, int32_t max_rounds, int32_t resume, int32_t* settled, void* hip_stream) {
  if (bad_count(F) || bad_grid(W, H, r_inflate) || bad_threshold(t_free) || bad_threshold(t_occ) || bad_min_unknown(min_unknown) ||
      any_null(evidence, field, n_frontier) || (weighted && !cost))       // (`frontier` may be null)
    return LIPMPC_E_ARG;
  if (const int rc = tiled_refusal(F, W, H, work, work_bytes, max_rounds, resume, settled)) return rc;
  if (F == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const TiledCall t = tiled_call(F, W, H, false, work);
  const TiledLayout& l = t.l;
  if (!resume) {
    frontier_bitmaps(s, t, F, W, H, evidence, t_free, t_occ, r_inflate, n_frontier);
    hipLaunchKernelGGL(tiled_frontier_seed_kernel, dim3((unsigned)(F * t.chunks)), dim3(SETUP_THREADS), 0, s, W, H, t.chunks, min_unknown,
                       t.w + l.unknown, t.w + l.blocked, frontier, field, n_frontier, t.w + l.flags0, l.tiles);
  }
  return tiled_rounds(s, F, W, H, t.blk_stride, round_buffers(l, t.w), field, max_rounds, settled, weighted ? cost : nullptr, t.ncells);
}

}  // namespace

extern "C" int lipmpc_grid_tiled_info(int32_t* tile_w, int32_t* tile_h, int64_t* max_cells) {
  if (!tile_w || !tile_h || !max_cells) return LIPMPC_E_ARG;
  *tile_w = TILE_W;
  *tile_h = TILE_H;
  *max_cells = TILED_MAX_CELLS;
  return LIPMPC_OK;
}

extern "C" int64_t lipmpc_grid_tiled_workspace_bytes(int64_t F, int32_t W, int32_t H) {
  if (bad_count(F) || bad_shape(W, H)) return LIPMPC_E_ARG;
  if (const int rc = tiled_cap_refusal(F, W, H)) return rc;
  return tiled_bytes(F, W, H);
}

extern "C" int lipmpc_grid_field_tiled_batch(int device, int64_t F, int32_t W, int32_t H, int32_t grid_shared, const double* origin,
                                             const double* cell, const uint8_t* occ, const double* goal, int32_t r_inflate,
                                             uint32_t* field, int32_t* field_status, void* work, int64_t work_bytes, int32_t max_rounds,
                                             int32_t resume, int32_t* settled, void* hip_stream) {
  return goal_field(device, F, W, H, grid_shared, origin, cell, occ, false, nullptr, goal, r_inflate, field, field_status, work, work_bytes,
                    max_rounds, resume, settled, hip_stream);
}

extern "C" int lipmpc_grid_frontier_field_tiled_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence, int32_t t_free,
                                                      int32_t t_occ, int32_t r_inflate, int32_t min_unknown, uint8_t* frontier,
                                                      uint32_t* field, int32_t* n_frontier, void* work, int64_t work_bytes,
                                                      int32_t max_rounds, int32_t resume, int32_t* settled, void* hip_stream) {
  return frontier_field(device, F, W, H, evidence, false, nullptr, t_free, t_occ, r_inflate, min_unknown, frontier, field, n_frontier, work,
                        work_bytes, max_rounds, resume, settled, hip_stream);
}

extern "C" int lipmpc_grid_path_tiled_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin, const double* cell,
                                            const uint8_t* occ, int32_t grid_shared, const uint32_t* field, const int32_t* field_status,
                                            const int32_t* settled, const double* goal, const double* start, int32_t r_inflate,
                                            int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub, int32_t* status,
                                            double* path_cost, void* hip_stream) {
  if (const int rc = tiled_path_refusal(B, F, W, H, origin, cell, r_inflate, max_seg, S_max)) return rc;
  if (B == 0) return LIPMPC_OK;
  // LATE: B == 0 passes with any of them null
  if (any_null(occ, field, field_status, settled, goal, start, sub_goals, n_sub, status, path_cost)) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(tiled_goal_descent_kernel, path_grid(B), dim3(PATH_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H,
                     grid_shared ? (int64_t)0 : (int64_t)W * H, origin[0], origin[1], cell[0], cell[1], occ, field, field_status, settled,
                     goal, start, r_inflate, max_seg, S_max, sub_goals, n_sub, status, path_cost);
  return launched();
}

extern "C" int lipmpc_grid_frontier_path_tiled_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                                     const double* cell, const int32_t* evidence, int32_t t_occ, const uint32_t* field,
                                                     const int32_t* n_frontier, const int32_t* settled, const double* start,
                                                     int32_t r_inflate, int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub,
                                                     int32_t* status, double* path_cost, int32_t* target_cell, void* hip_stream) {
  if (bad_threshold(t_occ)) return LIPMPC_E_ARG;
  if (const int rc = tiled_path_refusal(B, F, W, H, origin, cell, r_inflate, max_seg, S_max)) return rc;
  if (B == 0) return LIPMPC_OK;
  // LATE: B == 0 passes with any of them null
  if (any_null(evidence, field, n_frontier, settled, start, sub_goals, n_sub, status, path_cost, target_cell)) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(tiled_frontier_descent_kernel, path_grid(B), dim3(PATH_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H,
                     origin[0], origin[1], cell[0], cell[1], evidence, t_occ, field, n_frontier, settled, start, r_inflate, max_seg, S_max,
                     sub_goals, n_sub, status, path_cost, target_cell);
  return launched();
}

// =====================================================================================================================
// THE INFORMED AND THE COORDINATED EXPLORER ON LARGE MAPS (lipmpc_grid_frontier_gain_tiled_batch,
// lipmpc_grid_frontier_utility_field_tiled_batch, lipmpc_grid_frontier_utility_path_tiled_batch,
// lipmpc_grid_frontier_assign_tiled_batch): the gain by one workgroup per tile against bitmaps of the tile grown by r_view, the
// utility field and every claim round's field by the rounds above.
//
// WHY "UNBLOCKED" IS THE ONE-WORKGROUP CALLS' "field != INF".  The one-workgroup utility call takes passable(c) <=> the settled
// nearest-frontier field is finite at c; the tiled one takes the blocked bit, and needs no settled field.  (1) A frontier cell is
// unblocked and holds 0 in that field, so it is passable under both rules: the sources are the same.  (2) An unblocked cell that is
// INF in that field reaches no frontier cell by legal moves, hence no source: it is INF in either utility field, and no move
// through it lowers any other cell.  (3) A diagonal's side cell is an axial neighbour of the diagonal's target; if it is
// unblocked it is finite wherever the target is, so judging diagonals on blocked bits or on finite words allows the same moves
// among the cells that reach a source.  Both rules have the same fixed point, which is unique.
namespace {

constexpr int TILE_CELLS = TILE_W * TILE_H;

// LDS of the tiled gain kernel: the solid and unknown bitmaps of the tile grown by r_view on every side, the tile's frontier
// count (a word pair), the tile's frontier cells, one window per wave -- bounded by r_view, whatever the map: 49,304 bytes at 64
__host__ __device__ inline int64_t tile_gain_lds_bytes(int r_view) {
  const int64_t grown = (int64_t)(TILE_W + 2 * r_view) * (TILE_H + 2 * r_view);
  return 4 * (2 * bitmap_words(grown) + 2 + TILE_CELLS + GAIN_WAVES * gain_window_words(r_view));
}

// frontier_gain_kernel by tiles: blockIdx.x = map * tiles + tile.  A tile without a frontier cell writes its zeros and returns;
// any other classifies the evidence of the grown tile (a cell outside the grid counts as solid: it ends a ray as the grid's edge
// does), then marches as that kernel does, on local indices l = (i - i0 + r) * (TILE_H + 2 r) + j - j0 + r.  A ray from a cell
// of the tile stays within r of it, hence inside the grown tile.
__global__ void __launch_bounds__(GAIN_THREADS) tile_gain_kernel(int W, int H, int tiles_j, int tiles, const int32_t* __restrict__ evidence,
                                                                 int t_free, int t_occ, const uint8_t* __restrict__ frontier, int r_view,
                                                                 int32_t* __restrict__ gain) {
  extern __shared__ uint32_t field_lds[];
  const int64_t f = blockIdx.x / tiles;
  const int tile = blockIdx.x - (int)f * tiles, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = tile / tiles_j, tj = tile - ti * tiles_j, i0 = ti * TILE_W, j0 = tj * TILE_H;
  const int r = r_view, lh = TILE_H + 2 * r, grown = (TILE_W + 2 * r) * lh;
  const int words = (int)bitmap_words(grown), padded = (words - 2) * 32, ww = (int)gain_window_words(r);
  uint32_t *solid = field_lds, *unk = field_lds + words, *count = field_lds + 2 * words, *list = count + 2;
  uint32_t* win = list + TILE_CELLS + wave * ww;
  const int64_t ncells = (int64_t)W * H;
  const int32_t* ev = evidence + f * ncells;
  const uint8_t* fr = frontier + f * ncells;
  int32_t* out = gain + f * ncells;

  if (tid == 0) *count = 0;
  __syncthreads();
  // the tile's frontier cells, as local cells li * TILE_H + lj (in whatever order: each cell's gain is its own)
  for (int t = tid; t < TILE_CELLS; t += GAIN_THREADS) {
    const int i = i0 + t / TILE_H, j = j0 + t % TILE_H;
    if (i < W && j < H) {
      if (fr[i * H + j] != 0) list[atomicAdd(count, 1u)] = (uint32_t)t;
      else out[i * H + j] = 0;
    }
  }
  __syncthreads();
  const int n = (int)*count;
  if (n == 0) return;                                   // (one word for the whole workgroup: uniform)
  for (int l0 = tid - lane; l0 < padded; l0 += GAIN_THREADS) {
    const int l = l0 + lane, li = l / lh, lj = l - li * lh;
    const int gi = i0 - r + li, gj = j0 - r + lj;
    const bool in = l < grown && (unsigned)gi < (unsigned)W && (unsigned)gj < (unsigned)H;
    const int e = in ? ev[gi * H + gj] : 0;
    const bool is_solid = !in || e >= t_occ, is_free = e <= -t_free;
    const uint64_t ms = __ballot(is_solid), mu = __ballot(!is_solid && !is_free);
    if (lane == 0) {
      solid[l0 >> 5] = (uint32_t)ms; solid[(l0 >> 5) + 1] = (uint32_t)(ms >> 32);
      unk[l0 >> 5] = (uint32_t)mu; unk[(l0 >> 5) + 1] = (uint32_t)(mu >> 32);
    }
  }
  if (tid < 2) { solid[words - 2 + tid] = 0; unk[words - 2 + tid] = 0; }
  __syncthreads();
  const int r2 = r * r, two_r = 2 * r, side = two_r + 1, n_rays = 8 * r;
  for (int k = wave; k < n; k += GAIN_WAVES) {
    const int t = (int)list[k], si = t / TILE_H + r, sj = t % TILE_H + r;     // the source, in the grown tile
    for (int w = lane; w < ww; w += 64) win[w] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int q = lane; q < n_rays; q += 64) {
      const int edge = q / two_r, u = q - edge * two_r;
      const int di = edge == 0 ? -r : edge == 1 ? u - r : edge == 2 ? r : r - u;
      const int dj = edge == 0 ? u - r : edge == 1 ? r : edge == 2 ? r - u : -r;
      int qi = 0, ri = r, qj = 0, rj = r;
      for (int step = 1; step <= r; ++step) {
        ri += 2 * di; rj += 2 * dj;
        if (ri >= two_r) { ri -= two_r; ++qi; } else if (ri < 0) { ri += two_r; --qi; }
        if (rj >= two_r) { rj -= two_r; ++qj; } else if (rj < 0) { rj += two_r; --qj; }
        if (qi * qi + qj * qj > r2) break;
        const int l = (si + qi) * lh + sj + qj;
        if (bit_of(solid, l)) break;
        if (bit_of(unk, l)) {
          const int b = (qi + r) * side + qj + r;
          atomicOr(win + (b >> 5), 1u << (b & 31));
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int seen = 0;
    for (int w = lane; w < ww; w += 64) seen += __popc(win[w]);
    for (int o = 32; o; o >>= 1) seen += __shfl_xor(seen, o);
    if (lane == 0) out[(i0 + t / TILE_H) * H + j0 + t % TILE_H] = seen;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the window is read before the next cell clears it)
    __builtin_amdgcn_wave_barrier();
  }
}

// set-up of the utility field: the sources by the blocked bitmap, their seeds and INF elsewhere, their count by integer atomics
// (n_sources was cleared a kernel earlier), the flags round every source
__global__ void __launch_bounds__(SETUP_THREADS) tile_utility_seed_kernel(int W, int H, int chunks, const uint32_t* __restrict__ blk,
                                                                          const uint8_t* __restrict__ frontier,
                                                                          const int32_t* __restrict__ gain, int w_gain, int g_cap,
                                                                          int min_gain, uint32_t* __restrict__ ufield,
                                                                          int32_t* __restrict__ n_sources, uint32_t* __restrict__ flags,
                                                                          int64_t tiles) {
  const int64_t f = blockIdx.x / chunks;
  const int chunk = blockIdx.x - (int)f * chunks, lane = threadIdx.x & 63;
  const int ncells = W * H, words = (int)bitmap_words(ncells);
  const int c = chunk * SETUP_THREADS + threadIdx.x;
  bool src = false;
  if (c < ncells) {
    const int64_t at = f * ncells + c;
    int g = 0;
    if (frontier[at] != 0 && !bit_of(blk + f * words, c)) {
      g = gain[at];
      src = g >= min_gain;
    }
    ufield[at] = src ? gain_seed(g, w_gain, g_cap) : INF;
    if (src) {
      const int i = c / H;
      flag_round_seed(flags + f * tiles, W, H, tiles_along(H, TILE_H), i, c - i * H);
    }
  }
  const int mine = __popcll(__ballot(src));
  if (lane == 0 && mine) atomicAdd(n_sources + f, mine);              // (integers: the sum is the same in any order)
}

// frontier_utility_path_kernel with one more rule in front: a robot whose utility field is not settled gets
// LIPMPC_RRT_FIELD_UNSETTLED before any other rule.  The rest is THAT KERNEL'S BODY, COPIED word for word (as walk_in() is a copy of
// walk()): sharing it through a device function moved instructions in that kernel, which stays as it was compiled.  A fix to one
// of the two bodies belongs in the other.
__global__ void __launch_bounds__(PATH_THREADS) tile_utility_descent_kernel(
    int64_t B, int one_field, int W, int H, double ox, double oy, double dx, double dy, const int32_t* __restrict__ evidence, int t_occ,
    const uint8_t* __restrict__ frontier, const int32_t* __restrict__ gain, const uint32_t* __restrict__ ufield,
    const int32_t* __restrict__ n_sources, const int32_t* __restrict__ settled, int w_gain, int g_cap, int min_gain,
    const double* __restrict__ start, int r_inflate, int max_seg, int S_max, double* __restrict__ sub_goals, int32_t* __restrict__ n_sub,
    int32_t* __restrict__ status, double* __restrict__ path_cost, int32_t* __restrict__ target_cell, int32_t* __restrict__ target_gain) {
  const int64_t b = (int64_t)blockIdx.x * PATH_THREADS + threadIdx.x;
  if (b >= B) return;
  const int64_t f = one_field ? 0 : b;
  const int ncells = W * H;
  const uint32_t* fld = ufield + f * (int64_t)ncells;
  const uint8_t* fr = frontier + f * (int64_t)ncells;
  const int32_t* gn = gain + f * (int64_t)ncells;
  auto done = [&](int st_, int n, double cost, int target) {
    status[b] = st_; n_sub[b] = n; path_cost[b] = cost; target_cell[b] = target; target_gain[b] = target >= 0 ? gn[target] : -1;
  };
  // (a source is passable: its field is finite, which the comparison with a seed says too)
  auto terminal = [&](int c) {
    if (fr[c] == 0) return false;
    const int g = gn[c];
    return g >= min_gain && fld[c] == gain_seed(g, w_gain, g_cap);
  };
  const double nan = __builtin_nan("");
  if (settled[f] == 0) return done(LIPMPC_RRT_FIELD_UNSETTLED, 0, nan, -1);
  int si = 0, sj = 0;
  if (!cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj)) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan, -1);
  int s = si * H + sj;
  if (evidence[f * (int64_t)ncells + s] >= t_occ) return done(LIPMPC_RRT_START_OCCUPIED, 0, nan, -1);
  if (n_sources[f] == 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);
  if (fld[s] == INF) s = snap(fld, W, H, si, sj, r_inflate);
  if (s < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);
  double* sg = sub_goals + b * (int64_t)S_max * 2;
  int last_cell;
  const int n = walk_to(fld, W, H, s, max_seg, ox, oy, dx, dy, nullptr, last_cell, terminal);
  if (n < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);             // (a `ufield` that is no utility field of this map)
  const double cost = (double)(fld[s] - fld[last_cell]) / 5.0;
  if (n > S_max) return done(LIPMPC_RRT_PATH_OVERFLOW, 0, cost, last_cell);
  walk_to(fld, W, H, s, max_seg, ox, oy, dx, dy, sg, last_cell, terminal);
  centre(last_cell, H, ox, oy, dx, dy, sg + 2 * (n - 1));
  done(LIPMPC_RRT_FOUND, n, cost, last_cell);
}

// ---------------------------------------------------------------------------------------------------------------------
// the coordinated claim by tiles (lipmpc_grid_frontier_assign_tiled_batch): assign_body's rounds cut into kernels, every field_k
// relaxed by tiled_round_kernel.  The workspace: the control words, the impassable and the source bitmap, the two flag arrays, then
// field_k.
// CLAIM HYSTERESIS by tiles (lipmpc_grid_frontier_assign_keep_tiled_batch): per SLOT a mode kernel decides whose the slot is -- the
// next keep candidate that has an anchor, else a greedy round -- and the KEEP forms of the bodies below read the mode.  The
// workspace has KEEP_CTL control words in place of CLAIM_CTL; k is the control word CTL_CLAIMS, not the host's slot index.
// Every kernel of the two calls but the set-up and the mode is a body<KEEP> behind a claim_ and a keep_ wrapper.
constexpr int CLAIM_CTL = 8;                          // words 0, 1: the key (64 bits, 8-byte aligned as `work` is); then:
constexpr int CTL_TARGET = 2, CTL_STOPPED = 3, CTL_CLAIMS = 4, CTL_UNSETTLED = 5, CTL_ROUND_SETTLED = 6, CTL_ANY_SOURCE = 7;
constexpr int KEEP_CTL = 16;
constexpr int CTL_MODE = 8, CTL_ROBOT = 9, CTL_ANCHOR = 10, CTL_CURSOR = 11, CTL_KEPT = 12;      // MODE: 1 = a keep slot, 0 = a greedy round

struct ClaimLayout {
  int64_t bm_words, tiles, blocked, sources, flags0, flags1, field, words;
};
inline ClaimLayout claim_layout(int64_t W, int64_t H, int64_t ctl_words) {
  ClaimLayout l;
  l.bm_words = bitmap_words(W * H);
  l.tiles = (int64_t)tiles_along((int)W, TILE_W) * tiles_along((int)H, TILE_H);
  l.blocked = ctl_words;
  l.sources = l.blocked + l.bm_words;
  l.flags0 = l.sources + l.bm_words;
  l.flags1 = l.flags0 + l.tiles;
  l.field = l.flags1 + l.tiles;
  l.words = l.field + W * H;
  return l;
}
inline int64_t claim_bytes(int64_t W, int64_t H, int64_t ctl_words) { return 4 * claim_layout(W, H, ctl_words).words + 256; }

// once per call, over cells: impassable = the given field is INF, sources = the given frontier on passable cells, both by
// ballots; both flag arrays cleared; the control words.  With max_claims == 0 or an unsettled given field the call is stopped
// from the start.
__global__ void __launch_bounds__(SETUP_THREADS) claim_setup_kernel(int ncells, int64_t tiles, int max_claims,
                                                                    const uint8_t* __restrict__ frontier,
                                                                    const uint32_t* __restrict__ field,
                                                                    const int32_t* __restrict__ settled, uint32_t* __restrict__ ctl,
                                                                    uint32_t* __restrict__ blk, uint32_t* __restrict__ src,
                                                                    uint32_t* __restrict__ flags) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  const int c = blockIdx.x * SETUP_THREADS + tid, c0 = c - lane;
  if (c0 < padded) {
    const bool pass = c < ncells && field[c] != INF;
    const uint64_t mb = __ballot(c < ncells && !pass), ms = __ballot(pass && frontier[c] != 0);
    if (lane == 0) {
      blk[c0 >> 5] = (uint32_t)mb; blk[(c0 >> 5) + 1] = (uint32_t)(mb >> 32);
      src[c0 >> 5] = (uint32_t)ms; src[(c0 >> 5) + 1] = (uint32_t)(ms >> 32);
    }
  }
  if (blockIdx.x == 0) {
    if (tid < 2) { blk[words - 2 + tid] = 0; src[words - 2 + tid] = 0; }
    if (tid == 2) {
      const uint32_t unsettled = settled[0] == 0;
      ctl[0] = ctl[1] = ctl[CTL_TARGET] = INF;
      ctl[CTL_STOPPED] = unsettled | (uint32_t)(max_claims == 0);
      ctl[CTL_CLAIMS] = 0;
      ctl[CTL_UNSETTLED] = unsettled;
      ctl[CTL_ROUND_SETTLED] = 1;
      ctl[CTL_ANY_SOURCE] = 0;
    }
  }
  const int64_t total = 2 * tiles, step = (int64_t)gridDim.x * SETUP_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * SETUP_THREADS + tid; k < total; k += step) flags[k] = 0;
}

// once per call, over robots: U_0 as assign_body encodes it, claim_round[b] = -2 - (start cell), -1 for everyone else.  KEEP:
// nobody has kept anything, and the keep control words.
template <bool KEEP>
__device__ __forceinline__ void claim_robots_body(int64_t B, int W, int H, double ox, double oy, double dx, double dy,
                                                  const double* __restrict__ start, const int8_t* __restrict__ may_claim, int max_claims,
                                                  const int32_t* __restrict__ status, int32_t* __restrict__ claim_round,
                                                  int8_t* __restrict__ kept, uint32_t* __restrict__ ctl) {
  const int64_t b = (int64_t)blockIdx.x * SETUP_THREADS + threadIdx.x;
  if constexpr (KEEP) {
    if (b == 0) { ctl[CTL_MODE] = 0; ctl[CTL_ROBOT] = 0; ctl[CTL_ANCHOR] = INF; ctl[CTL_CURSOR] = 0; ctl[CTL_KEPT] = 0; }
  }
  if (b >= B) return;
  const int sb = status[b];
  int si = 0, sj = 0, v = -1;
  if (max_claims > 0 && (sb == LIPMPC_RRT_FOUND || sb == LIPMPC_RRT_PATH_OVERFLOW) && (!may_claim || may_claim[b]) &&
      cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj))
    v = -2 - (si * H + sj);
  claim_round[b] = v;
  if constexpr (KEEP) kept[b] = 0;
}

__global__ void __launch_bounds__(SETUP_THREADS) claim_robots_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, const double* __restrict__ start,
    const int8_t* __restrict__ may_claim, int max_claims, const int32_t* __restrict__ status, int32_t* __restrict__ claim_round) {
  claim_robots_body<false>(B, W, H, ox, oy, dx, dy, start, may_claim, max_claims, status, claim_round, nullptr, nullptr);
}

__global__ void __launch_bounds__(SETUP_THREADS) keep_robots_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, const double* __restrict__ start,
    const int8_t* __restrict__ may_claim, int max_claims, const int32_t* __restrict__ status, int32_t* __restrict__ claim_round,
    int8_t* __restrict__ kept, uint32_t* __restrict__ ctl) {
  claim_robots_body<true>(B, W, H, ox, oy, dx, dy, start, may_claim, max_claims, status, claim_round, kept, ctl);
}

// the mode of the next slot, ONE workgroup: from the cursor on, the first robot of U with a previous target that has an anchor in
// what is left of the sources (assign_keep_body's search, chunk by chunk); none: every slot from here on is a greedy round
__global__ void __launch_bounds__(FIELD_THREADS) keep_mode_kernel(int64_t B, int W, int H, int r_keep, uint32_t* ctl,
                                                                  const uint32_t* __restrict__ src,
                                                                  const int32_t* __restrict__ claim_round,
                                                                  const int32_t* __restrict__ prev_target) {
  __shared__ uint32_t next;
  __shared__ unsigned long long key;
  const int tid = threadIdx.x, lane = tid & 63, ncells = W * H;
  const bool stopped = ctl[CTL_STOPPED] != 0;
  const int64_t from = ctl[CTL_CURSOR];
  if (tid == 0) { next = INF; key = ~0ull; }
  __syncthreads();                                      // (everybody has read the control words)
  if (stopped) return;
  for (int64_t base = from; base < B; base += FIELD_THREADS) {
    const int64_t mb = base + tid;
    const bool candidate = mb < B && claim_round[mb] <= -2 && is_cell(prev_target[mb], ncells);
    for (int cursor = 0;;) {
      if (candidate && tid >= cursor) atomicMin(&next, (uint32_t)tid);
      __syncthreads();
      const uint32_t nx = next;
      __syncthreads();                                  // everybody has read it
      if (nx == INF) break;
      if (tid == 0) next = INF;
      cursor = (int)nx + 1;
      const int64_t wb = base + nx;
      const unsigned long long mine = anchor_key(src, prev_target[wb], r_keep, W, H);
      if (lane == 0 && mine != ~0ull) atomicMin(&key, mine);
      __syncthreads();
      const unsigned long long found = key;
      if (found == ~0ull) continue;                     // nothing is left of the target: no slot is spent (the key is still ~0)
      if (tid == 0) {
        ctl[CTL_MODE] = 1; ctl[CTL_ROBOT] = (uint32_t)wb; ctl[CTL_ANCHOR] = (uint32_t)(found & 0xFFFFFFFFull);
        ctl[CTL_CURSOR] = (uint32_t)(wb + 1);
      }
      return;
    }
  }
  if (tid == 0) { ctl[CTL_MODE] = 0; ctl[CTL_ANCHOR] = INF; ctl[CTL_CURSOR] = (uint32_t)B; }
}

// the claim seed, blockIdx.x = tile: field_k = 0 on what is left of the sources and INF elsewhere on the tile's cells; the tile's
// flag of the first round = some source among its cells or in its halo (what flag_round_seed sets), its flag of the second
// array 0 -- each flag word has one writer, so nothing is cleared under another workgroup's hands.  KEEP: a keep slot's only
// source is the anchor.
template <bool KEEP>
__device__ __forceinline__ void claim_seed_body(int W, int H, int tiles_j, uint32_t* __restrict__ ctl, const uint32_t* __restrict__ src,
                                                uint32_t* __restrict__ field_k, uint32_t* __restrict__ flags0,
                                                uint32_t* __restrict__ flags1) {
  if (ld_agent(ctl + CTL_STOPPED)) return;              // (both flag arrays are clear: whoever stopped the call cleared them)
  bool keep = false;
  int anchor = 0;
  if constexpr (KEEP) {
    keep = ld_agent(ctl + CTL_MODE) != 0;
    anchor = (int)ld_agent(ctl + CTL_ANCHOR);
  }
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int ti = tile / tiles_j, tj = tile - ti * tiles_j, i0 = ti * TILE_W, j0 = tj * TILE_H;
  int own = 0, near = 0;
  for (int l = tid; l < HALO_CELLS; l += TILE_THREADS) {
    const int li = l / HALO_H, lj = l - li * HALO_H, i = i0 + li - 1, j = j0 + lj - 1;
    if ((unsigned)i >= (unsigned)W || (unsigned)j >= (unsigned)H) continue;
    const bool s = keep ? i * H + j == anchor : bit_of(src, i * H + j);
    const bool inner = li >= 1 && li <= TILE_W && lj >= 1 && lj <= TILE_H;
    if (inner) field_k[i * H + j] = s ? 0u : INF;
    own |= s & inner;
    near |= s;
  }
  near = __syncthreads_or(near);
  if (tid == 0) { flags0[tile] = near != 0; flags1[tile] = 0; }
  if (own) st_agent(ctl + CTL_ANY_SOURCE, 1u);
}

__global__ void __launch_bounds__(TILE_THREADS) claim_seed_kernel(
    int W, int H, int tiles_j, uint32_t* __restrict__ ctl, const uint32_t* __restrict__ src, uint32_t* __restrict__ field_k,
    uint32_t* __restrict__ flags0, uint32_t* __restrict__ flags1) {
  claim_seed_body<false>(W, H, tiles_j, ctl, src, field_k, flags0, flags1);
}

__global__ void __launch_bounds__(TILE_THREADS) keep_seed_kernel(
    int W, int H, int tiles_j, uint32_t* __restrict__ ctl, const uint32_t* __restrict__ src, uint32_t* __restrict__ field_k,
    uint32_t* __restrict__ flags0, uint32_t* __restrict__ flags1) {
  claim_seed_body<true>(W, H, tiles_j, ctl, src, field_k, flags0, flags1);
}

// the pick, over robots: the least (cost << 32 | b) among the candidates of U_k, by a wave reduction and a 64-bit atomicMin.
// Every workgroup finds the same answer to "are the rounds over" from words that earlier kernels wrote.  KEEP: in a keep slot the
// slot's robot is the only candidate.
template <bool KEEP>
__device__ __forceinline__ void claim_pick_body(int64_t B, int W, int H, int r_inflate, uint32_t* ctl, const uint32_t* field_k,
                                                const int32_t* __restrict__ claim_round) {
  if (ld_agent(ctl + CTL_STOPPED)) return;
  const bool no_source = ld_agent(ctl + CTL_ANY_SOURCE) == 0, unsettled = ld_agent(ctl + CTL_ROUND_SETTLED) == 0;
  if (no_source || unsettled) return;                   // (the claim kernel stops the call: it reads the same two words)
  bool keep = false;
  int64_t only = 0;
  if constexpr (KEEP) {
    keep = ld_agent(ctl + CTL_MODE) != 0;
    only = ld_agent(ctl + CTL_ROBOT);
  }
  const int64_t b = (int64_t)blockIdx.x * SETUP_THREADS + threadIdx.x;
  unsigned long long mine = ~0ull;
  if (b < B && (!keep || b == only)) {
    const int v = claim_round[b];
    if (v <= -2) {
      const int s = claim_cell(field_k, W, H, -2 - v, r_inflate);
      if (s >= 0) mine = ((unsigned long long)ld(field_k + s) << 32) | (unsigned long long)b;
    }
  }
  for (int o = 32; o; o >>= 1) mine = min(mine, (unsigned long long)__shfl_xor(mine, o));
  if ((threadIdx.x & 63) == 0 && mine != ~0ull) atomicMin((unsigned long long*)ctl, mine);
}

__global__ void __launch_bounds__(SETUP_THREADS) claim_pick_kernel(
    int64_t B, int W, int H, int r_inflate, uint32_t* ctl, const uint32_t* field_k, const int32_t* __restrict__ claim_round) {
  claim_pick_body<false>(B, W, H, r_inflate, ctl, field_k, claim_round);
}

__global__ void __launch_bounds__(SETUP_THREADS) keep_pick_kernel(
    int64_t B, int W, int H, int r_inflate, uint32_t* ctl, const uint32_t* field_k, const int32_t* __restrict__ claim_round) {
  claim_pick_body<true>(B, W, H, r_inflate, ctl, field_k, claim_round);
}

// the claim, ONE workgroup: one lane walks the winner's path down field_k and writes its rows and claim_round; then everybody
// clears the disc from the source bitmap.  Whatever happened, the kernel leaves both flag arrays clear, the key reset and the
// "any source" word 0 for the next round's seed.  `slot`: k, the round's number, without KEEP.
// KEEP: k is the control word; a keeper has to pass the test before its rows are written; a keep slot whose robot has no entry or
// fails the test ends without a winner and without stopping the call.
template <bool KEEP>
__device__ __forceinline__ void claim_take_body(int64_t B, int W, int H, double ox, double oy, double dx, double dy, int r_inflate,
                                                int r_claim, int keep_ratio16, int keep_slack, int max_seg, int S_max, int slot, int tiles,
                                                uint32_t* ctl, uint32_t* src, const uint32_t* field_k, const uint32_t* __restrict__ field,
                                                uint32_t* flags, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                                int32_t* target_cell, int32_t* claim_round, int8_t* kept) {
  const int tid = threadIdx.x;
  const bool stopped = ctl[CTL_STOPPED] != 0, no_source = ctl[CTL_ANY_SOURCE] == 0, unsettled = ctl[CTL_ROUND_SETTLED] == 0;
  const bool keep = KEEP && ctl[CTL_MODE] != 0;
  const int k = KEEP ? (int)ctl[CTL_CLAIMS] : slot;
  const unsigned long long win = *(const unsigned long long*)ctl;
  __syncthreads();                                      // (everybody has read the control words)
  for (int t = tid; t < 2 * tiles; t += FIELD_THREADS) flags[t] = 0;
  if (tid == 0) {
    ctl[0] = ctl[1] = INF; ctl[CTL_ANY_SOURCE] = 0; ctl[CTL_ROUND_SETTLED] = 1;
    if constexpr (KEEP) ctl[CTL_TARGET] = INF;          // (without KEEP lane 0 writes the word below, whatever happens)
  }
  if (stopped) return;
  if (no_source || unsettled || (win == ~0ull && !keep)) {      // no source left, a field that did not settle, no candidate
    if (tid == 0) { ctl[CTL_STOPPED] = 1; if (!no_source && unsettled) ctl[CTL_UNSETTLED] = 1; }
    return;
  }
  if (win == ~0ull) return;                             // a keep slot whose anchor is out of the robot's reach: spent, nothing else
  const int64_t wb = (int64_t)(win & 0xFFFFFFFFull);
  if constexpr (KEEP) __syncthreads();                  // (lane 0's reset of the target word comes before its new value)
  if (tid == 0) {
    // one lane walks the winner's path, twice: count, then -- if the sub-goals fit -- write (rows past n_sub stay untouched)
    const int cell = -2 - claim_round[wb];
    const int s = claim_cell(field_k, W, H, cell, r_inflate);
    bool ok = s >= 0;                                   // (the pick found the winner's entry in the same words)
    if (keep) ok = keep_passes(field_k, field, W, H, cell, s, r_inflate, (uint32_t)keep_ratio16, (uint32_t)keep_slack);
    double* sg = sub_goals + wb * (int64_t)S_max * 2;
    int last_cell = s, n = 0;
    for (int pass = 0; ok && pass < 2 && n >= 0 && n <= S_max; ++pass)
      n = walk_in(field_k, W, H, s, max_seg, ox, oy, dx, dy, pass ? sg : nullptr, last_cell);
    if (n > 0) {
      if (n <= S_max) centre(last_cell, H, ox, oy, dx, dy, sg + 2 * (n - 1));
      status[wb] = n <= S_max ? LIPMPC_RRT_FOUND : LIPMPC_RRT_PATH_OVERFLOW;
      n_sub[wb] = n <= S_max ? n : 0;
      path_cost[wb] = (double)ld(field_k + s) / 5.0;
      target_cell[wb] = last_cell;
      claim_round[wb] = k;
      ctl[CTL_CLAIMS] = (uint32_t)(k + 1);
      if (keep) { kept[wb] = 1; ctl[CTL_KEPT] += 1; }
    }
    if (!KEEP || n > 0) ctl[CTL_TARGET] = n > 0 ? (uint32_t)last_cell : INF;
  }
  __syncthreads();
  const uint32_t t = ctl[CTL_TARGET];
  if (t == INF) {                                       // a keeper that failed the test stays in U; (a winner always has a descent:
    if (tid == 0 && !keep) ctl[CTL_STOPPED] = 1;        // a greedy round without one stops the call, as "U is used up" does)
    return;
  }
  int eligible = 0;
  for (int64_t b = tid; b < B; b += FIELD_THREADS) eligible |= claim_round[b] <= -2;
  const int more = __syncthreads_or(eligible);
  if (!more) {                                          // U is used up
    if (tid == 0) ctl[CTL_STOPPED] = 1;
    return;
  }
  // S_{k+1}: the sources outside the winner's disc, clipped to the grid
  const int ti = (int)t / H, tj = (int)t - ti * H, r2 = r_claim * r_claim;
  const int i_lo = max(ti - r_claim, 0), i_hi = min(ti + r_claim, W - 1);
  for (int c = i_lo * H + tid; c < (i_hi + 1) * H; c += FIELD_THREADS) {
    const int i = c / H, j = c - i * H;
    if (bit_of(src, c) && (i - ti) * (i - ti) + (j - tj) * (j - tj) <= r2) atomicAnd(src + (c >> 5), ~(1u << (c & 31)));
  }
}

__global__ void __launch_bounds__(FIELD_THREADS) claim_take_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, int r_inflate, int r_claim, int max_seg, int S_max, int k,
    int tiles, uint32_t* ctl, uint32_t* src, const uint32_t* field_k, uint32_t* flags, double* sub_goals, int32_t* n_sub, int32_t* status,
    double* path_cost, int32_t* target_cell, int32_t* claim_round) {
  claim_take_body<false>(B, W, H, ox, oy, dx, dy, r_inflate, r_claim, 0, 0, max_seg, S_max, k, tiles, ctl, src, field_k, nullptr, flags,
                         sub_goals, n_sub, status, path_cost, target_cell, claim_round, nullptr);
}

__global__ void __launch_bounds__(FIELD_THREADS) keep_take_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, int r_inflate, int r_claim, int keep_ratio16, int keep_slack,
    int max_seg, int S_max, int tiles, uint32_t* ctl, uint32_t* src, const uint32_t* field_k, const uint32_t* __restrict__ field,
    uint32_t* flags, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell, int32_t* claim_round,
    int8_t* kept) {
  claim_take_body<true>(B, W, H, ox, oy, dx, dy, r_inflate, r_claim, keep_ratio16, keep_slack, max_seg, S_max, 0, tiles, ctl, src, field_k,
                        field, flags, sub_goals, n_sub, status, path_cost, target_cell, claim_round, kept);
}

// the last kernel, over robots: the followers (still in U), n_claims and claims_settled; KEEP: and n_kept
template <bool KEEP>
__device__ __forceinline__ void claim_finish_body(int64_t B, const uint32_t* __restrict__ ctl, int32_t* claim_round,
                                                  int32_t* __restrict__ n_claims, int32_t* __restrict__ n_kept,
                                                  int32_t* __restrict__ claims_settled) {
  const int64_t b = (int64_t)blockIdx.x * SETUP_THREADS + threadIdx.x;
  if (b < B && claim_round[b] < -1) claim_round[b] = -1;
  if (b == 0) {
    n_claims[0] = (int32_t)ctl[CTL_CLAIMS];
    if constexpr (KEEP) n_kept[0] = (int32_t)ctl[CTL_KEPT];
    claims_settled[0] = ctl[CTL_UNSETTLED] == 0;
  }
}

__global__ void __launch_bounds__(SETUP_THREADS) claim_finish_kernel(
    int64_t B, const uint32_t* __restrict__ ctl, int32_t* claim_round, int32_t* __restrict__ n_claims,
    int32_t* __restrict__ claims_settled) {
  claim_finish_body<false>(B, ctl, claim_round, n_claims, nullptr, claims_settled);
}

__global__ void __launch_bounds__(SETUP_THREADS) keep_finish_kernel(
    int64_t B, const uint32_t* __restrict__ ctl, int32_t* claim_round, int32_t* __restrict__ n_claims, int32_t* __restrict__ n_kept,
    int32_t* __restrict__ claims_settled) {
  claim_finish_body<true>(B, ctl, claim_round, n_claims, n_kept, claims_settled);
}

// GAIN-SEEDED CLAIMS by tiles (lipmpc_grid_frontier_assign_utility_tiled_batch): the claim call's kernel sequence with three
// kernels of its own -- the set-up (sources need gain >= min_gain), the seed (a source starts at its seed, not at 0) and the take
// (the utility terminal rule, path_cost, target_gain).  The robots, pick and finish kernels and the rounds are the claim call's
// own, launched as they are; the workspace is that call's, CLAIM_CTL control words.
__global__ void __launch_bounds__(SETUP_THREADS) utility_assign_setup_kernel(int ncells, int64_t tiles, int max_claims,
                                                                     const uint8_t* __restrict__ frontier,
                                                                     const uint32_t* __restrict__ field,
                                                                     const int32_t* __restrict__ gain, int min_gain,
                                                                     const int32_t* __restrict__ settled, uint32_t* __restrict__ ctl,
                                                                     uint32_t* __restrict__ blk, uint32_t* __restrict__ src,
                                                                     uint32_t* __restrict__ flags) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  const int c = blockIdx.x * SETUP_THREADS + tid, c0 = c - lane;
  if (c0 < padded) {
    const bool pass = c < ncells && field[c] != INF;
    bool source = false;
    if (pass && frontier[c] != 0) source = gain[c] >= min_gain;
    const uint64_t mb = __ballot(c < ncells && !pass), ms = __ballot(source);
    if (lane == 0) {
      blk[c0 >> 5] = (uint32_t)mb; blk[(c0 >> 5) + 1] = (uint32_t)(mb >> 32);
      src[c0 >> 5] = (uint32_t)ms; src[(c0 >> 5) + 1] = (uint32_t)(ms >> 32);
    }
  }
  if (blockIdx.x == 0) {
    if (tid < 2) { blk[words - 2 + tid] = 0; src[words - 2 + tid] = 0; }
    if (tid == 2) {
      const uint32_t unsettled = settled[0] == 0;
      ctl[0] = ctl[1] = ctl[CTL_TARGET] = INF;
      ctl[CTL_STOPPED] = unsettled | (uint32_t)(max_claims == 0);
      ctl[CTL_CLAIMS] = 0;
      ctl[CTL_UNSETTLED] = unsettled;
      ctl[CTL_ROUND_SETTLED] = 1;
      ctl[CTL_ANY_SOURCE] = 0;
    }
  }
  const int64_t total = 2 * tiles, step = (int64_t)gridDim.x * SETUP_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * SETUP_THREADS + tid; k < total; k += step) flags[k] = 0;
}

// claim_seed_body without KEEP, a source starting at its seed (gain is read at source cells of the tile only)
__global__ void __launch_bounds__(TILE_THREADS) utility_assign_seed_kernel(
    int W, int H, int tiles_j, uint32_t* __restrict__ ctl, const uint32_t* __restrict__ src, const int32_t* __restrict__ gain, int w_gain,
    int g_cap, uint32_t* __restrict__ field_k, uint32_t* __restrict__ flags0, uint32_t* __restrict__ flags1) {
  if (ld_agent(ctl + CTL_STOPPED)) return;              // (both flag arrays are clear: whoever stopped the call cleared them)
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int ti = tile / tiles_j, tj = tile - ti * tiles_j, i0 = ti * TILE_W, j0 = tj * TILE_H;
  int own = 0, near = 0;
  for (int l = tid; l < HALO_CELLS; l += TILE_THREADS) {
    const int li = l / HALO_H, lj = l - li * HALO_H, i = i0 + li - 1, j = j0 + lj - 1;
    if ((unsigned)i >= (unsigned)W || (unsigned)j >= (unsigned)H) continue;
    const bool s = bit_of(src, i * H + j);
    const bool inner = li >= 1 && li <= TILE_W && lj >= 1 && lj <= TILE_H;
    if (inner) field_k[i * H + j] = s ? gain_seed(gain[i * H + j], w_gain, g_cap) : INF;
    own |= s & inner;
    near |= s;
  }
  near = __syncthreads_or(near);
  if (tid == 0) { flags0[tile] = near != 0; flags1[tile] = 0; }
  if (own) st_agent(ctl + CTL_ANY_SOURCE, 1u);
}

// claim_take_body without KEEP, with the utility path's terminal test on the source bitmap (S_k until the disc below is cleared),
// path_cost as the walk's length and target_gain
__global__ void __launch_bounds__(FIELD_THREADS) utility_assign_take_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, int r_inflate, int r_claim, int max_seg, int S_max, int k,
    int tiles, uint32_t* ctl, uint32_t* src, const uint32_t* field_k, const int32_t* __restrict__ gain, int w_gain, int g_cap,
    uint32_t* flags, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell, int32_t* target_gain,
    int32_t* claim_round) {
  // what only the walking lane needs, parked in LDS as the one-workgroup kernels park it: held in scalar registers through the
  // disc loop it would overfill that file
  __shared__ uint32_t parked[32];
  auto park = [&](int slot, unsigned long long v) { parked[2 * slot] = (uint32_t)v; parked[2 * slot + 1] = (uint32_t)(v >> 32); };
  auto unpark = [&](int slot) { return ((unsigned long long)parked[2 * slot + 1] << 32) | parked[2 * slot]; };
  const int tid = threadIdx.x;
  const bool stopped = ctl[CTL_STOPPED] != 0, no_source = ctl[CTL_ANY_SOURCE] == 0, unsettled = ctl[CTL_ROUND_SETTLED] == 0;
  const unsigned long long win = *(const unsigned long long*)ctl;
  if (tid == 0) {
    park(0, __double_as_longlong(ox)); park(1, __double_as_longlong(oy)); park(2, __double_as_longlong(dx));
    park(3, __double_as_longlong(dy));
    park(4, (unsigned long long)sub_goals); park(5, (unsigned long long)n_sub); park(6, (unsigned long long)status);
    park(7, (unsigned long long)path_cost); park(8, (unsigned long long)target_cell); park(9, (unsigned long long)target_gain);
    park(10, (unsigned long long)gain);
    parked[22] = (uint32_t)w_gain; parked[23] = (uint32_t)g_cap; parked[24] = (uint32_t)max_seg; parked[25] = (uint32_t)S_max;
  }
  __syncthreads();                                      // (everybody has read the control words)
  for (int t = tid; t < 2 * tiles; t += FIELD_THREADS) flags[t] = 0;
  if (tid == 0) { ctl[0] = ctl[1] = INF; ctl[CTL_ANY_SOURCE] = 0; ctl[CTL_ROUND_SETTLED] = 1; }
  if (stopped) return;
  if (no_source || unsettled || win == ~0ull) {         // no source left, a field that did not settle, no candidate
    if (tid == 0) { ctl[CTL_STOPPED] = 1; if (!no_source && unsettled) ctl[CTL_UNSETTLED] = 1; }
    return;
  }
  const int64_t wb = (int64_t)(win & 0xFFFFFFFFull);
  if (tid == 0) {
    // one lane walks the winner's path, twice: count, then -- if the sub-goals fit -- write (rows past n_sub stay untouched)
    const int s = claim_cell(field_k, W, H, -2 - claim_round[wb], r_inflate);
    const double wox = __longlong_as_double(unpark(0)), woy = __longlong_as_double(unpark(1));
    const double wdx = __longlong_as_double(unpark(2)), wdy = __longlong_as_double(unpark(3));
    const int32_t* wgain = (const int32_t*)unpark(10);
    const int ww = (int)parked[22], wcap = (int)parked[23], wseg = (int)parked[24], wmax = (int)parked[25];
    auto terminal = [&](int c) { return bit_of(src, c) && ld(field_k + c) == gain_seed(wgain[c], ww, wcap); };
    double* sg = (double*)unpark(4) + wb * (int64_t)wmax * 2;
    int last_cell = s, n = 0;
    for (int pass = 0; s >= 0 && pass < 2 && n >= 0 && n <= wmax; ++pass)
      n = walk_in_to(field_k, W, H, s, wseg, wox, woy, wdx, wdy, pass ? sg : nullptr, last_cell, terminal);
    if (n > 0) {
      if (n <= wmax) centre(last_cell, H, wox, woy, wdx, wdy, sg + 2 * (n - 1));
      ((int32_t*)unpark(6))[wb] = n <= wmax ? LIPMPC_RRT_FOUND : LIPMPC_RRT_PATH_OVERFLOW;
      ((int32_t*)unpark(5))[wb] = n <= wmax ? n : 0;
      ((double*)unpark(7))[wb] = (double)(ld(field_k + s) - ld(field_k + last_cell)) / 5.0;
      ((int32_t*)unpark(8))[wb] = last_cell;
      ((int32_t*)unpark(9))[wb] = wgain[last_cell];
      claim_round[wb] = k;
      ctl[CTL_CLAIMS] = (uint32_t)(k + 1);
    }
    ctl[CTL_TARGET] = n > 0 ? (uint32_t)last_cell : INF;
  }
  __syncthreads();
  const uint32_t t = ctl[CTL_TARGET];
  if (t == INF) {                                       // (a winner always has a descent: a round without one stops the call)
    if (tid == 0) ctl[CTL_STOPPED] = 1;
    return;
  }
  int eligible = 0;
  for (int64_t b = tid; b < B; b += FIELD_THREADS) eligible |= claim_round[b] <= -2;
  const int more = __syncthreads_or(eligible);
  if (!more) {                                          // U is used up
    if (tid == 0) ctl[CTL_STOPPED] = 1;
    return;
  }
  // S_{k+1}: the sources outside the winner's disc, clipped to the grid
  const int ti = (int)t / H, tj = (int)t - ti * H, r2 = r_claim * r_claim;
  const int i_lo = max(ti - r_claim, 0), i_hi = min(ti + r_claim, W - 1);
  for (int c = i_lo * H + tid; c < (i_hi + 1) * H; c += FIELD_THREADS) {
    const int i = c / H, j = c - i * H;
    if (bit_of(src, c) && (i - ti) * (i - ti) + (j - tj) * (j - tj) <= r2) atomicAnd(src + (c >> 5), ~(1u << (c & 31)));
  }
}

// CLAIM HYSTERESIS FOR THE GAIN-SEEDED CLAIMS by tiles (lipmpc_grid_frontier_assign_keep_utility_tiled_batch): the tiled keep
// call's kernel sequence with three kernels of its own -- the set-up (sources need gain >= min_gain; the call is stopped from the
// start when either given field did not settle), the seed (a keep slot seeds the anchor alone at its seed, a greedy slot what is
// left of the sources at theirs) and the take (the utility terminal rule, the keep test against `ufield`, path_cost, target_gain).
// The robots, mode, pick and finish kernels and the rounds are the tiled keep call's own, launched as they are; the workspace is
// that call's, KEEP_CTL control words.
__global__ void __launch_bounds__(SETUP_THREADS) keep_utility_setup_kernel(int ncells, int64_t tiles, int max_claims,
                                                                           const uint8_t* __restrict__ frontier,
                                                                           const uint32_t* __restrict__ field,
                                                                           const int32_t* __restrict__ gain, int min_gain,
                                                                           const int32_t* __restrict__ settled,
                                                                           const int32_t* __restrict__ usettled,
                                                                           uint32_t* __restrict__ ctl, uint32_t* __restrict__ blk,
                                                                           uint32_t* __restrict__ src, uint32_t* __restrict__ flags) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int words = (int)bitmap_words(ncells), padded = (words - 2) * 32;
  const int c = blockIdx.x * SETUP_THREADS + tid, c0 = c - lane;
  if (c0 < padded) {
    const bool pass = c < ncells && field[c] != INF;
    bool source = false;
    if (pass && frontier[c] != 0) source = gain[c] >= min_gain;
    const uint64_t mb = __ballot(c < ncells && !pass), ms = __ballot(source);
    if (lane == 0) {
      blk[c0 >> 5] = (uint32_t)mb; blk[(c0 >> 5) + 1] = (uint32_t)(mb >> 32);
      src[c0 >> 5] = (uint32_t)ms; src[(c0 >> 5) + 1] = (uint32_t)(ms >> 32);
    }
  }
  if (blockIdx.x == 0) {
    if (tid < 2) { blk[words - 2 + tid] = 0; src[words - 2 + tid] = 0; }
    if (tid == 2) {
      const uint32_t unsettled = settled[0] == 0 || usettled[0] == 0;
      ctl[0] = ctl[1] = ctl[CTL_TARGET] = INF;
      ctl[CTL_STOPPED] = unsettled | (uint32_t)(max_claims == 0);
      ctl[CTL_CLAIMS] = 0;
      ctl[CTL_UNSETTLED] = unsettled;
      ctl[CTL_ROUND_SETTLED] = 1;
      ctl[CTL_ANY_SOURCE] = 0;
    }
  }
  const int64_t total = 2 * tiles, step = (int64_t)gridDim.x * SETUP_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * SETUP_THREADS + tid; k < total; k += step) flags[k] = 0;
}

// claim_seed_body<KEEP>, a source starting at its seed (gain is read at source cells of the tile only): the anchor alone in a keep
// slot, what is left of the sources in a greedy one
__global__ void __launch_bounds__(TILE_THREADS) keep_utility_seed_kernel(
    int W, int H, int tiles_j, uint32_t* __restrict__ ctl, const uint32_t* __restrict__ src, const int32_t* __restrict__ gain, int w_gain,
    int g_cap, uint32_t* __restrict__ field_k, uint32_t* __restrict__ flags0, uint32_t* __restrict__ flags1) {
  if (ld_agent(ctl + CTL_STOPPED)) return;              // (both flag arrays are clear: whoever stopped the call cleared them)
  const bool keep = ld_agent(ctl + CTL_MODE) != 0;
  const int anchor = (int)ld_agent(ctl + CTL_ANCHOR);
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int ti = tile / tiles_j, tj = tile - ti * tiles_j, i0 = ti * TILE_W, j0 = tj * TILE_H;
  int own = 0, near = 0;
  for (int l = tid; l < HALO_CELLS; l += TILE_THREADS) {
    const int li = l / HALO_H, lj = l - li * HALO_H, i = i0 + li - 1, j = j0 + lj - 1;
    if ((unsigned)i >= (unsigned)W || (unsigned)j >= (unsigned)H) continue;
    const bool s = keep ? i * H + j == anchor : bit_of(src, i * H + j);
    const bool inner = li >= 1 && li <= TILE_W && lj >= 1 && lj <= TILE_H;
    if (inner) field_k[i * H + j] = s ? gain_seed(gain[i * H + j], w_gain, g_cap) : INF;
    own |= s & inner;
    near |= s;
  }
  near = __syncthreads_or(near);
  if (tid == 0) { flags0[tile] = near != 0; flags1[tile] = 0; }
  if (own) st_agent(ctl + CTL_ANY_SOURCE, 1u);
}

// claim_take_body<KEEP> with utility_assign_take_kernel's walk: in a keep slot the walk ends at the anchor and the robot first has
// to pass the test against the given `ufield`; in a greedy slot the utility terminal test on the source bitmap; path_cost is the
// walk's length, target_gain the stored gain of the target
__global__ void __launch_bounds__(FIELD_THREADS) keep_utility_take_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, int r_inflate, int r_claim, int keep_ratio16, int keep_slack,
    int max_seg, int S_max, int tiles, uint32_t* ctl, uint32_t* src, const uint32_t* field_k, const uint32_t* __restrict__ ufield,
    const int32_t* __restrict__ gain, int w_gain, int g_cap, uint32_t* flags, double* sub_goals, int32_t* n_sub, int32_t* status,
    double* path_cost, int32_t* target_cell, int32_t* target_gain, int32_t* claim_round, int8_t* kept) {
  // what only the walking lane needs, parked in LDS as the one-workgroup kernels park it
  __shared__ uint32_t parked[36];
  auto park = [&](int slot, unsigned long long v) { parked[2 * slot] = (uint32_t)v; parked[2 * slot + 1] = (uint32_t)(v >> 32); };
  auto unpark = [&](int slot) { return ((unsigned long long)parked[2 * slot + 1] << 32) | parked[2 * slot]; };
  const int tid = threadIdx.x;
  const bool stopped = ctl[CTL_STOPPED] != 0, no_source = ctl[CTL_ANY_SOURCE] == 0, unsettled = ctl[CTL_ROUND_SETTLED] == 0;
  const bool keep = ctl[CTL_MODE] != 0;
  const int k = (int)ctl[CTL_CLAIMS];
  const unsigned long long win = *(const unsigned long long*)ctl;
  if (tid == 0) {
    park(0, __double_as_longlong(ox)); park(1, __double_as_longlong(oy)); park(2, __double_as_longlong(dx));
    park(3, __double_as_longlong(dy));
    park(4, (unsigned long long)sub_goals); park(5, (unsigned long long)n_sub); park(6, (unsigned long long)status);
    park(7, (unsigned long long)path_cost); park(8, (unsigned long long)target_cell); park(9, (unsigned long long)target_gain);
    park(10, (unsigned long long)gain); park(11, (unsigned long long)ufield); park(12, (unsigned long long)kept);
    parked[26] = (uint32_t)w_gain; parked[27] = (uint32_t)g_cap; parked[28] = (uint32_t)max_seg; parked[29] = (uint32_t)S_max;
    parked[30] = (uint32_t)keep_ratio16; parked[31] = (uint32_t)keep_slack; parked[32] = ctl[CTL_ANCHOR];
  }
  __syncthreads();                                      // (everybody has read the control words)
  for (int t = tid; t < 2 * tiles; t += FIELD_THREADS) flags[t] = 0;
  if (tid == 0) { ctl[0] = ctl[1] = INF; ctl[CTL_ANY_SOURCE] = 0; ctl[CTL_ROUND_SETTLED] = 1; ctl[CTL_TARGET] = INF; }
  if (stopped) return;
  if (no_source || unsettled || (win == ~0ull && !keep)) {      // no source left, a field that did not settle, no candidate
    if (tid == 0) { ctl[CTL_STOPPED] = 1; if (!no_source && unsettled) ctl[CTL_UNSETTLED] = 1; }
    return;
  }
  if (win == ~0ull) return;                             // a keep slot whose anchor is out of the robot's reach: spent, nothing else
  const int64_t wb = (int64_t)(win & 0xFFFFFFFFull);
  __syncthreads();                                      // (lane 0's reset of the target word comes before its new value)
  if (tid == 0) {
    // one lane walks the winner's path, twice: count, then -- if the sub-goals fit -- write (rows past n_sub stay untouched)
    const int cell = -2 - claim_round[wb];
    const int s = per_lane(claim_cell(field_k, W, H, cell, r_inflate));      // (in vector registers, as in the one-workgroup body)
    bool ok = s >= 0;                                   // (the pick found the winner's entry in the same words)
    if (keep) ok = keep_passes(field_k, (const uint32_t*)unpark(11), W, H, cell, s, r_inflate, parked[30], parked[31]);
    const double wox = __longlong_as_double(unpark(0)), woy = __longlong_as_double(unpark(1));
    const double wdx = __longlong_as_double(unpark(2)), wdy = __longlong_as_double(unpark(3));
    const int32_t* wgain = (const int32_t*)unpark(10);
    const int ww = (int)parked[26], wcap = (int)parked[27], wseg = (int)parked[28], wmax = (int)parked[29];
    const int a = per_lane(keep ? (int)parked[32] : -1);
    auto terminal = [&](int c) { return a >= 0 ? c == a : bit_of(src, c) && ld(field_k + c) == gain_seed(wgain[c], ww, wcap); };
    double* sg = (double*)unpark(4) + wb * (int64_t)wmax * 2;
    int last_cell = s, n = 0;
    for (int pass = 0; ok && pass < 2 && n >= 0 && n <= wmax; ++pass)
      n = walk_in_to(field_k, W, H, s, wseg, wox, woy, wdx, wdy, pass ? sg : nullptr, last_cell, terminal);
    if (n > 0) {
      if (n <= wmax) centre(last_cell, H, wox, woy, wdx, wdy, sg + 2 * (n - 1));
      ((int32_t*)unpark(6))[wb] = n <= wmax ? LIPMPC_RRT_FOUND : LIPMPC_RRT_PATH_OVERFLOW;
      ((int32_t*)unpark(5))[wb] = n <= wmax ? n : 0;
      ((double*)unpark(7))[wb] = (double)(ld(field_k + s) - ld(field_k + last_cell)) / 5.0;
      ((int32_t*)unpark(8))[wb] = last_cell;
      ((int32_t*)unpark(9))[wb] = wgain[last_cell];
      claim_round[wb] = k;
      ctl[CTL_CLAIMS] = (uint32_t)(k + 1);
      if (keep) { ((int8_t*)unpark(12))[wb] = 1; ctl[CTL_KEPT] += 1; }
      ctl[CTL_TARGET] = (uint32_t)last_cell;
    }
  }
  __syncthreads();
  const uint32_t t = ctl[CTL_TARGET];
  if (t == INF) {                                       // a keeper that failed the test stays in U; (a winner always has a descent:
    if (tid == 0 && !keep) ctl[CTL_STOPPED] = 1;        // a greedy round without one stops the call, as "U is used up" does)
    return;
  }
  int eligible = 0;
  for (int64_t b = tid; b < B; b += FIELD_THREADS) eligible |= claim_round[b] <= -2;
  const int more = __syncthreads_or(eligible);
  if (!more) {                                          // U is used up
    if (tid == 0) ctl[CTL_STOPPED] = 1;
    return;
  }
  // S_{k+1}: the sources outside the winner's disc, clipped to the grid
  const int ti = (int)t / H, tj = (int)t - ti * H, r2 = r_claim * r_claim;
  const int i_lo = max(ti - r_claim, 0), i_hi = min(ti + r_claim, W - 1);
  for (int c = i_lo * H + tid; c < (i_hi + 1) * H; c += FIELD_THREADS) {
    const int i = c / H, j = c - i * H;
    if (bit_of(src, c) && (i - ti) * (i - ti) + (j - tj) * (j - tj) <= r2) atomicAnd(src + (c >> 5), ~(1u << (c & 31)));
  }
}

}  // namespace

extern "C" int64_t lipmpc_grid_frontier_gain_tiled_lds_bytes(int32_t r_view) {
  if (bad_view(r_view)) return LIPMPC_E_ARG;
  return tile_gain_lds_bytes(r_view);
}

extern "C" int lipmpc_grid_frontier_gain_tiled_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence, int32_t t_free,
                                                     int32_t t_occ, const uint8_t* frontier, int32_t r_view, int32_t* gain,
                                                     void* hip_stream) {
  if (bad_count(F) || bad_shape(W, H) || bad_threshold(t_free) || bad_threshold(t_occ) || bad_view(r_view) ||
      any_null(evidence, frontier, gain))
    return LIPMPC_E_ARG;
  if (const int rc = tiled_cap_refusal(F, W, H)) return rc;
  if (F == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  const int tiles_j = tiles_along(H, TILE_H), tiles = tiles_along(W, TILE_W) * tiles_j;
  hipLaunchKernelGGL(tile_gain_kernel, dim3((unsigned)(F * tiles)), dim3(GAIN_THREADS), (size_t)tile_gain_lds_bytes(r_view),
                     (hipStream_t)hip_stream, W, H, tiles_j, tiles, evidence, t_free, t_occ, frontier, r_view, gain);
  return launched();
}

extern "C" int lipmpc_grid_frontier_utility_field_tiled_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence,
                                                              int32_t t_free, int32_t t_occ, int32_t r_inflate, const uint8_t* frontier,
                                                              const int32_t* gain, int32_t w_gain, int32_t g_cap, int32_t min_gain,
                                                              uint32_t* ufield, int32_t* n_sources, void* work, int64_t work_bytes,
                                                              int32_t max_rounds, int32_t resume, int32_t* settled, void* hip_stream) {
  if (bad_count(F) || bad_grid(W, H, r_inflate) || bad_threshold(t_free) || bad_threshold(t_occ) || bad_gain(w_gain, g_cap, min_gain) ||
      any_null(evidence, frontier, gain, ufield, n_sources))
    return LIPMPC_E_ARG;
  if (const int rc = tiled_refusal(F, W, H, work, work_bytes, max_rounds, resume, settled)) return rc;
  if (F == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const TiledCall t = tiled_call(F, W, H, false, work);
  const TiledLayout& l = t.l;
  if (!resume) {
    frontier_bitmaps(s, t, F, W, H, evidence, t_free, t_occ, r_inflate, n_sources);
    hipLaunchKernelGGL(tile_utility_seed_kernel, dim3((unsigned)(F * t.chunks)), dim3(SETUP_THREADS), 0, s, W, H, t.chunks, t.w + l.blocked,
                       frontier, gain, w_gain, g_cap, min_gain, ufield, n_sources, t.w + l.flags0, l.tiles);
  }
  return tiled_rounds(s, F, W, H, t.blk_stride, round_buffers(l, t.w), ufield, max_rounds, settled);
}

extern "C" int lipmpc_grid_frontier_utility_path_tiled_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                                             const double* cell, const int32_t* evidence, int32_t t_occ,
                                                             const uint8_t* frontier, const int32_t* gain, const uint32_t* ufield,
                                                             const int32_t* n_sources, const int32_t* settled, int32_t w_gain,
                                                             int32_t g_cap, int32_t min_gain, const double* start, int32_t r_inflate,
                                                             int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub,
                                                             int32_t* status, double* path_cost, int32_t* target_cell,
                                                             int32_t* target_gain, void* hip_stream) {
  // (the pointers EARLY, unlike the other tiled path calls: B == 0 with a null one is E_ARG)
  if (bad_threshold(t_occ) || bad_gain(w_gain, g_cap, min_gain) ||
      any_null(evidence, frontier, gain, ufield, n_sources, settled, start, sub_goals, n_sub, status, path_cost, target_cell, target_gain))
    return LIPMPC_E_ARG;
  if (const int rc = tiled_path_refusal(B, F, W, H, origin, cell, r_inflate, max_seg, S_max)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(tile_utility_descent_kernel, path_grid(B), dim3(PATH_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H,
                     origin[0], origin[1], cell[0], cell[1], evidence, t_occ, frontier, gain, ufield, n_sources, settled, w_gain, g_cap,
                     min_gain, start, r_inflate, max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell, target_gain);
  return launched();
}

// THREE SEQUENCES, each read top to bottom as set-up, robots, per slot (mode,) seed, rounds, pick, take, and finish: claim_tiled (plain
// and keep) and the two gain-seeded forms, whose set-up, seed and take kernels take the gain's arguments as well -- one sequence for
// all four would choose among four argument lists at three of its launches.  They share their refusals and the ClaimCall.
namespace {

// what the keep call adds to the claim call's arguments
struct KeepArgs {
  const int32_t* prev_target;
  int32_t r_keep, keep_ratio16, keep_slack;
  int8_t* kept;
  int32_t* n_kept;
};

// what the claim calls refuse behind their E_ARG scalars and pointers: the placed grid (E_ARG), the caps for one field, then a
// `work` too small for a shape within the caps (E_ARG: beyond them no size is defined)
int claim_shape_refusal(int32_t W, int32_t H, const double* origin, const double* cell, int32_t r_inflate, int64_t work_bytes, int ctl_words) {
  if (bad_placed_grid(W, H, origin, cell, r_inflate)) return LIPMPC_E_ARG;
  if (const int rc = tiled_cap_refusal(1, W, H)) return rc;
  return work_bytes < claim_bytes(W, H, ctl_words) ? LIPMPC_E_ARG : LIPMPC_OK;
}

// the four workspace sizes
int64_t claim_workspace_bytes(int32_t W, int32_t H, int ctl_words) {
  if (bad_shape(W, H)) return LIPMPC_E_ARG;
  if (const int rc = tiled_cap_refusal(1, W, H)) return rc;
  return claim_bytes(W, H, ctl_words);
}

// what a tiled claim call derives from its shape: the workspace's layout, the set-up launch's blocks (a wave per 64 cells of the
// padded map), the tiles, the grids of its launches, the placement and what the rounds read
struct ClaimCall {
  ClaimLayout c;
  int ncells, chunks, tiles, tiles_j;
  dim3 cells, robots, setup, tile_grid, tile_block, one, group;
  double ox, oy, dx, dy;
  uint32_t* w;
  RoundBuffers rounds;
  int32_t* round_settled;
};
ClaimCall claim_call(int64_t B, int W, int H, int ctl_words, const double* origin, const double* cell, void* work) {
  const ClaimLayout c = claim_layout(W, H, ctl_words);
  const int chunks = ((int)(c.bm_words - 2) * 32 + SETUP_THREADS - 1) / SETUP_THREADS, tiles = (int)c.tiles;
  uint32_t* w = (uint32_t*)work;
  return {c, W * H, chunks, tiles, tiles_along(H, TILE_H), dim3((unsigned)chunks), dim3((unsigned)((B + SETUP_THREADS - 1) / SETUP_THREADS)),
          dim3(SETUP_THREADS), dim3((unsigned)tiles), dim3(TILE_THREADS), dim3(1), dim3(FIELD_THREADS), origin[0], origin[1], cell[0], cell[1],
          w, round_buffers(c, w), (int32_t*)(w + CTL_ROUND_SETTLED)};
}

// lipmpc_grid_frontier_assign_tiled_batch and, `keep` not null, lipmpc_grid_frontier_assign_keep_tiled_batch.  3 launches round
// the slots, and per slot (the mode,) the seed, max_rounds rounds and their settle, the pick and the take:
// max_claims * (max_rounds + 4) + 3, with the mode max_claims * (max_rounds + 5) + 3
int claim_tiled(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell, const uint8_t* frontier,
                const uint32_t* field, const int32_t* settled, const double* start, const int8_t* may_claim, int32_t r_inflate,
                int32_t r_claim, int32_t max_claims, int32_t max_seg, int32_t S_max, void* work, int64_t work_bytes, int32_t max_rounds,
                double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell, int32_t* claim_round,
                int32_t* n_claims, int32_t* claims_settled, const KeepArgs* keep, void* hip_stream) {
  if (bad_claim(B, r_claim, max_claims, max_seg, S_max, frontier, field, settled, start, work, sub_goals, n_sub, status, path_cost,
                target_cell, claim_round, n_claims, claims_settled) ||
      bad_claim_rounds(work, max_rounds) || too_many_launches(max_claims, max_rounds) ||
      (keep && (bad_keep(keep->r_keep, keep->keep_ratio16, keep->keep_slack) || any_null(keep->prev_target, keep->kept, keep->n_kept))))
    return LIPMPC_E_ARG;
  const int ctl_words = keep ? KEEP_CTL : CLAIM_CTL;
  if (const int rc = claim_shape_refusal(W, H, origin, cell, r_inflate, work_bytes, ctl_words)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const ClaimCall q = claim_call(B, W, H, ctl_words, origin, cell, work);
  const ClaimLayout& c = q.c;
  uint32_t* w = q.w;
  hipLaunchKernelGGL(claim_setup_kernel, q.cells, q.setup, 0, s, q.ncells, c.tiles, max_claims, frontier, field, settled, w, w + c.blocked,
                     w + c.sources, w + c.flags0);
  if (keep)
    hipLaunchKernelGGL(keep_robots_kernel, q.robots, q.setup, 0, s, B, W, H, q.ox, q.oy, q.dx, q.dy, start, may_claim, max_claims, status,
                       claim_round, keep->kept, w);
  else
    hipLaunchKernelGGL(claim_robots_kernel, q.robots, q.setup, 0, s, B, W, H, q.ox, q.oy, q.dx, q.dy, start, may_claim, max_claims, status,
                       claim_round);
  for (int slot = 0; slot < max_claims; ++slot) {
    if (keep)
      hipLaunchKernelGGL(keep_mode_kernel, q.one, q.group, 0, s, B, W, H, keep->r_keep, w, w + c.sources, claim_round, keep->prev_target);
    hipLaunchKernelGGL(keep ? keep_seed_kernel : claim_seed_kernel, q.tile_grid, q.tile_block, 0, s, W, H, q.tiles_j, w, w + c.sources,
                       w + c.field, w + c.flags0, w + c.flags1);
    if (const int rc = tiled_rounds(s, 1, W, H, 0, q.rounds, w + c.field, max_rounds, q.round_settled)) return rc;
    hipLaunchKernelGGL(keep ? keep_pick_kernel : claim_pick_kernel, q.robots, q.setup, 0, s, B, W, H, r_inflate, w, w + c.field, claim_round);
    if (keep)
      hipLaunchKernelGGL(keep_take_kernel, q.one, q.group, 0, s, B, W, H, q.ox, q.oy, q.dx, q.dy, r_inflate, r_claim, keep->keep_ratio16,
                         keep->keep_slack, max_seg, S_max, q.tiles, w, w + c.sources, w + c.field, field, w + c.flags0, sub_goals, n_sub,
                         status, path_cost, target_cell, claim_round, keep->kept);
    else
      hipLaunchKernelGGL(claim_take_kernel, q.one, q.group, 0, s, B, W, H, q.ox, q.oy, q.dx, q.dy, r_inflate, r_claim, max_seg, S_max, slot,
                         q.tiles, w, w + c.sources, w + c.field, w + c.flags0, sub_goals, n_sub, status, path_cost, target_cell, claim_round);
  }
  if (keep)
    hipLaunchKernelGGL(keep_finish_kernel, q.robots, q.setup, 0, s, B, w, claim_round, n_claims, keep->n_kept, claims_settled);
  else
    hipLaunchKernelGGL(claim_finish_kernel, q.robots, q.setup, 0, s, B, w, claim_round, n_claims, claims_settled);
  return launched();
}

}  // namespace

extern "C" int64_t lipmpc_grid_frontier_assign_tiled_workspace_bytes(int32_t W, int32_t H) { return claim_workspace_bytes(W, H, CLAIM_CTL); }

extern "C" int lipmpc_grid_frontier_assign_tiled_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell,
                                                       const uint8_t* frontier, const uint32_t* field, const int32_t* settled,
                                                       const double* start, const int8_t* may_claim, int32_t r_inflate, int32_t r_claim,
                                                       int32_t max_claims, int32_t max_seg, int32_t S_max, void* work, int64_t work_bytes,
                                                       int32_t max_rounds, double* sub_goals, int32_t* n_sub, int32_t* status,
                                                       double* path_cost, int32_t* target_cell, int32_t* claim_round, int32_t* n_claims,
                                                       int32_t* claims_settled, void* hip_stream) {
  return claim_tiled(device, B, W, H, origin, cell, frontier, field, settled, start, may_claim, r_inflate, r_claim, max_claims, max_seg,
                     S_max, work, work_bytes, max_rounds, sub_goals, n_sub, status, path_cost, target_cell, claim_round, n_claims,
                     claims_settled, nullptr, hip_stream);
}

extern "C" int64_t lipmpc_grid_frontier_assign_keep_tiled_workspace_bytes(int32_t W, int32_t H) { return claim_workspace_bytes(W, H, KEEP_CTL); }

extern "C" int lipmpc_grid_frontier_assign_keep_tiled_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin,
                                                            const double* cell, const uint8_t* frontier, const uint32_t* field,
                                                            const int32_t* settled, const double* start, const int8_t* may_claim,
                                                            const int32_t* prev_target, int32_t r_inflate, int32_t r_claim,
                                                            int32_t r_keep, int32_t keep_ratio16, int32_t keep_slack, int32_t max_claims,
                                                            int32_t max_seg, int32_t S_max, void* work, int64_t work_bytes,
                                                            int32_t max_rounds, double* sub_goals, int32_t* n_sub, int32_t* status,
                                                            double* path_cost, int32_t* target_cell, int32_t* claim_round,
                                                            int32_t* n_claims, int8_t* kept, int32_t* n_kept, int32_t* claims_settled,
                                                            void* hip_stream) {
  const KeepArgs keep = {prev_target, r_keep, keep_ratio16, keep_slack, kept, n_kept};
  return claim_tiled(device, B, W, H, origin, cell, frontier, field, settled, start, may_claim, r_inflate, r_claim, max_claims, max_seg,
                     S_max, work, work_bytes, max_rounds, sub_goals, n_sub, status, path_cost, target_cell, claim_round, n_claims,
                     claims_settled, &keep, hip_stream);
}

extern "C" int64_t lipmpc_grid_frontier_assign_utility_tiled_workspace_bytes(int32_t W, int32_t H) {
  return claim_workspace_bytes(W, H, CLAIM_CTL);
}

// claim_tiled's sequence without the keep forms: 3 launches round the rounds, and per round the seed, max_rounds rounds and their
// settle, the pick and the take: max_claims * (max_rounds + 4) + 3
extern "C" int lipmpc_grid_frontier_assign_utility_tiled_batch(int device, int64_t B, int32_t W, int32_t H, const double* origin,
                                                               const double* cell, const uint8_t* frontier, const uint32_t* field,
                                                               const int32_t* settled, const double* start, const int8_t* may_claim,
                                                               int32_t r_inflate, int32_t r_claim, int32_t max_claims, int32_t max_seg,
                                                               int32_t S_max, void* work, int64_t work_bytes, int32_t max_rounds,
                                                               double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                                               int32_t* target_cell, int32_t* claim_round, int32_t* n_claims,
                                                               int32_t* claims_settled, const int32_t* gain, int32_t w_gain,
                                                               int32_t g_cap, int32_t min_gain, int32_t* target_gain, void* hip_stream) {
  if (bad_claim(B, r_claim, max_claims, max_seg, S_max, frontier, field, settled, start, work, sub_goals, n_sub, status, path_cost,
                target_cell, claim_round, n_claims, claims_settled, gain, target_gain) ||
      bad_claim_rounds(work, max_rounds) || too_many_launches(max_claims, max_rounds) || bad_gain(w_gain, g_cap, min_gain))
    return LIPMPC_E_ARG;
  if (const int rc = claim_shape_refusal(W, H, origin, cell, r_inflate, work_bytes, CLAIM_CTL)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const ClaimCall q = claim_call(B, W, H, CLAIM_CTL, origin, cell, work);
  const ClaimLayout& c = q.c;
  uint32_t* w = q.w;
  hipLaunchKernelGGL(utility_assign_setup_kernel, q.cells, q.setup, 0, s, q.ncells, c.tiles, max_claims, frontier, field, gain, min_gain,
                     settled, w, w + c.blocked, w + c.sources, w + c.flags0);
  hipLaunchKernelGGL(claim_robots_kernel, q.robots, q.setup, 0, s, B, W, H, q.ox, q.oy, q.dx, q.dy, start, may_claim, max_claims, status,
                     claim_round);
  for (int k = 0; k < max_claims; ++k) {
    hipLaunchKernelGGL(utility_assign_seed_kernel, q.tile_grid, q.tile_block, 0, s, W, H, q.tiles_j, w, w + c.sources, gain, w_gain, g_cap,
                       w + c.field, w + c.flags0, w + c.flags1);
    if (const int rc = tiled_rounds(s, 1, W, H, 0, q.rounds, w + c.field, max_rounds, q.round_settled)) return rc;
    hipLaunchKernelGGL(claim_pick_kernel, q.robots, q.setup, 0, s, B, W, H, r_inflate, w, w + c.field, claim_round);
    hipLaunchKernelGGL(utility_assign_take_kernel, q.one, q.group, 0, s, B, W, H, q.ox, q.oy, q.dx, q.dy, r_inflate, r_claim, max_seg, S_max,
                       k, q.tiles, w, w + c.sources, w + c.field, gain, w_gain, g_cap, w + c.flags0, sub_goals, n_sub, status, path_cost,
                       target_cell, target_gain, claim_round);
  }
  hipLaunchKernelGGL(claim_finish_kernel, q.robots, q.setup, 0, s, B, w, claim_round, n_claims, claims_settled);
  return launched();
}

extern "C" int64_t lipmpc_grid_frontier_assign_keep_utility_tiled_workspace_bytes(int32_t W, int32_t H) {
  return claim_workspace_bytes(W, H, KEEP_CTL);
}

// claim_tiled's sequence with the keep forms: 3 launches round the slots, and per slot the mode, the seed, max_rounds rounds and
// their settle, the pick and the take: max_claims * (max_rounds + 5) + 3
extern "C" int lipmpc_grid_frontier_assign_keep_utility_tiled_batch(
    int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell, const uint8_t* frontier, const uint32_t* field,
    const int32_t* settled, const double* start, const int8_t* may_claim, const int32_t* prev_target, int32_t r_inflate, int32_t r_claim,
    int32_t r_keep, int32_t keep_ratio16, int32_t keep_slack, int32_t max_claims, int32_t max_seg, int32_t S_max, void* work,
    int64_t work_bytes, int32_t max_rounds, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, int32_t* target_cell,
    int32_t* claim_round, int32_t* n_claims, int8_t* kept, int32_t* n_kept, int32_t* claims_settled, const int32_t* gain,
    const uint32_t* ufield, const int32_t* usettled, int32_t w_gain, int32_t g_cap, int32_t min_gain, int32_t* target_gain,
    void* hip_stream) {
  if (bad_claim(B, r_claim, max_claims, max_seg, S_max, frontier, field, settled, start, prev_target, work, sub_goals, n_sub, status,
                path_cost, target_cell, claim_round, n_claims, kept, n_kept, claims_settled, gain, ufield, usettled, target_gain) ||
      bad_claim_rounds(work, max_rounds) || too_many_launches(max_claims, max_rounds) || bad_keep(r_keep, keep_ratio16, keep_slack) ||
      bad_gain(w_gain, g_cap, min_gain))
    return LIPMPC_E_ARG;
  if (const int rc = claim_shape_refusal(W, H, origin, cell, r_inflate, work_bytes, KEEP_CTL)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const ClaimCall q = claim_call(B, W, H, KEEP_CTL, origin, cell, work);
  const ClaimLayout& c = q.c;
  uint32_t* w = q.w;
  hipLaunchKernelGGL(keep_utility_setup_kernel, q.cells, q.setup, 0, s, q.ncells, c.tiles, max_claims, frontier, field, gain, min_gain, settled,
                     usettled, w, w + c.blocked, w + c.sources, w + c.flags0);
  hipLaunchKernelGGL(keep_robots_kernel, q.robots, q.setup, 0, s, B, W, H, q.ox, q.oy, q.dx, q.dy, start, may_claim, max_claims, status,
                     claim_round, kept, w);
  for (int slot = 0; slot < max_claims; ++slot) {
    hipLaunchKernelGGL(keep_mode_kernel, q.one, q.group, 0, s, B, W, H, r_keep, w, w + c.sources, claim_round, prev_target);
    hipLaunchKernelGGL(keep_utility_seed_kernel, q.tile_grid, q.tile_block, 0, s, W, H, q.tiles_j, w, w + c.sources, gain, w_gain, g_cap,
                       w + c.field, w + c.flags0, w + c.flags1);
    if (const int rc = tiled_rounds(s, 1, W, H, 0, q.rounds, w + c.field, max_rounds, q.round_settled)) return rc;
    hipLaunchKernelGGL(keep_pick_kernel, q.robots, q.setup, 0, s, B, W, H, r_inflate, w, w + c.field, claim_round);
    hipLaunchKernelGGL(keep_utility_take_kernel, q.one, q.group, 0, s, B, W, H, q.ox, q.oy, q.dx, q.dy, r_inflate, r_claim, keep_ratio16,
                       keep_slack, max_seg, S_max, q.tiles, w, w + c.sources, w + c.field, ufield, gain, w_gain, g_cap, w + c.flags0, sub_goals,
                       n_sub, status, path_cost, target_cell, target_gain, claim_round, kept);
  }
  hipLaunchKernelGGL(keep_finish_kernel, q.robots, q.setup, 0, s, B, w, claim_round, n_claims, n_kept, claims_settled);
  return launched();
}

// =====================================================================================================================
// SOFT CLEARANCE (lipmpc_grid_clearance_cost_batch, lipmpc_grid_field_weighted_batch, lipmpc_grid_frontier_field_weighted_batch and
// their path calls): a byte per cell that a path pays when it LEAVES the cell, on top of the step.  The cost layer decays with the
// distance to the nearest solid cell; the weighted fields are the tiled fields above with that byte added in the sweep, relaxed by
// the same rounds -- set-up, seeds, flags and the settle kernel are the tiled calls' own, and the round is round_body's WEIGHTED form.
//
// WHY THE WEIGHTED ROUNDS GIVE WEIGHTED DIJKSTRA'S FIELD, and why nothing wraps: in round_body, beside the line where the cost enters.
namespace {

constexpr int R_CLEAR_MAX = 31;                       // a disc row is at most 63 consecutive bits: one 64-bit window
constexpr int SOFT_ROWS = TILE_W + 2 * R_CLEAR_MAX;   // 94 rows of 128 bits: the tile grown by r_clear
static_assert(LIPMPC_COST_MAX == 248 && (7 + LIPMPC_COST_MAX) * (uint64_t)TILED_MAX_CELLS < INF, "a finite weighted value stays below INF");

// THE COST LAYER.  blockIdx.x = map * tiles + tile; a thread owns the round kernel's eight cells.  The solid bits of the tile grown
// by r_clear go into LDS by ballot (row rr = i - (i0 - r), bit b = j - (j0 - r); a cell outside the grid is not solid); per cell
// and row the nearest set bit left and right of the centre of the 2 r + 1 bit window, rows by increasing |di| until di^2 >= the
// best d2.  KIND 0: occ bytes; KIND 1: evidence >= t_occ.
template <int KIND>
__global__ void __launch_bounds__(TILE_THREADS) soft_cost_kernel(int W, int H, int tiles_j, int tiles, const uint8_t* __restrict__ occ,
                                                                 const int32_t* __restrict__ evidence, int t_occ, int r, int w_clear,
                                                                 uint8_t* __restrict__ cost) {
  __shared__ uint64_t bm[SOFT_ROWS * 2];
  const int64_t m = blockIdx.x / tiles;
  const int tile = blockIdx.x - (int)m * tiles, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = tile / tiles_j, tj = tile - ti * tiles_j, i0 = ti * TILE_W, j0 = tj * TILE_H;
  const int64_t base = m * (int64_t)W * H;
  const int rows = TILE_W + 2 * r;
  int any = 0;
  for (int h = wave; h < 2 * rows; h += TILE_THREADS / 64) {          // (h is uniform in a wave: every lane takes part in the ballot)
    const int gi = i0 - r + (h >> 1), gj = j0 - r + (h & 1) * 64 + lane;
    bool solid = false;
    if ((unsigned)gi < (unsigned)W && (unsigned)gj < (unsigned)H) {
      const int64_t g = base + (int64_t)gi * H + gj;
      solid = KIND == 0 ? occ[g] != 0 : evidence[g] >= t_occ;
    }
    const uint64_t mb = __ballot(solid);
    if (lane == 0) bm[h] = mb;
    any |= mb != 0;
  }
  any = __syncthreads_or(any);
  const int r2 = r * r, lj = lane, gj = j0 + lj;
  const uint64_t mask = (2ull << (2 * r)) - 1, left = (1ull << r) - 1;          // 2 r + 1 <= 63 bits; the r bits below the centre
#pragma unroll 1
  for (int k = 0; k < TILE_OWN; ++k) {
    const int li = k * TILE_ROWS + wave, gi = i0 + li;
    if (gi >= W || gj >= H) continue;
    int best = r2 + 1;
    if (any) {
#pragma unroll 1
      for (int a = 0; a <= r && a * a < best; ++a) {
#pragma unroll 1
        for (int sgn = 0; sgn < (a ? 2 : 1); ++sgn) {
          const uint64_t* row = bm + 2 * (li + r + (sgn ? -a : a));
          const uint64_t win = ((row[0] >> lj) | (lj ? row[1] << (64 - lj) : 0ull)) & mask;     // bit t = column gj - r + t
          const uint64_t hi = win >> r, lo = win & left;
          if (hi) { const int d = __builtin_ctzll(hi); best = min(best, a * a + d * d); }
          if (lo) { const int d = r - (63 - __builtin_clzll(lo)); best = min(best, a * a + d * d); }
        }
      }
    }
    cost[base + (int64_t)gi * H + gj] = best <= r2 ? (uint8_t)((uint32_t)(w_clear * (r2 - best)) / (uint32_t)r2) : (uint8_t)0;
  }
}

// the weighted descent's next cell: the first neighbour in the contract's order with a legal move and
// field[n] + step + k(c) == field[c]; -1 if none
__device__ inline int soft_descend(const uint32_t* __restrict__ fld, const uint8_t* __restrict__ kc, int W, int H, int c) {
  const int i = c / H, j = c - i * H;
  const uint32_t fc = fld[c], k = soft_k(kc, c);
  for (int di = -1; di <= 1; ++di)
    for (int dj = -1; dj <= 1; ++dj) {
      if ((di == 0 && dj == 0) || (unsigned)(i + di) >= (unsigned)W || (unsigned)(j + dj) >= (unsigned)H) continue;
      const int n = c + di * H + dj;
      const uint32_t v = fld[n];
      if (v == INF) continue;
      const bool diag = di != 0 && dj != 0;
      if (diag && (fld[c + di * H] == INF || fld[c + dj] == INF)) continue;
      if (v < fc && fc - v == (diag ? DIAGONAL : AXIAL) + k) return n;
    }
  return -1;
}

// los() that also sums k over the cells it visits, both ends included; false (the sum meaningless) where the sight breaks
__device__ inline bool soft_los(const uint32_t* __restrict__ fld, const uint8_t* __restrict__ kc, int H, int a, int b, uint32_t& sum) {
  if (b < a) { const int t = a; a = b; b = t; }
  const int ai = a / H, aj = a - ai * H, bi = b / H, bj = b - bi * H;
  const int di = bi - ai, dj = bj - aj;
  const int m = max(abs(di), abs(dj)), two_m = 2 * m;
  sum = 0;
  if (m == 0) { sum = soft_k(kc, a); return fld[a] != INF; }
  int qi = 0, ri = m, qj = 0, rj = m;
  for (int k = 0; k <= m; ++k) {
    const int c = (ai + qi) * H + aj + qj;
    if (fld[c] == INF) return false;
    sum += soft_k(kc, c);
    ri += 2 * di; rj += 2 * dj;
    if (ri >= two_m) { ri -= two_m; ++qi; } else if (ri < 0) { ri += two_m; --qi; }
    if (rj >= two_m) { rj -= two_m; ++qj; } else if (rj < 0) { rj += two_m; --qj; }
  }
  return true;
}

// walk() down a weighted field.  `pen`: the sum of k over the descended cells from the anchor (inclusive) to cur (exclusive), so
// that (fld[a] - fld[cur]) - pen is the length in steps alone, which is what max_seg caps; a sub-goal is also set where the
// straight segment would pay more penalty than the descended path did.  With k = 0 everywhere this is walk(), test for test.
__device__ inline int soft_walk(const uint32_t* __restrict__ fld, const uint8_t* __restrict__ kc, int W, int H, int s, int max_seg,
                                double ox, double oy, double dx, double dy, double* sg, int& last_cell) {
  int count = 0;
  auto emit = [&](int c) {
    if (sg) centre(c, H, ox, oy, dx, dy, sg + 2 * count);
    ++count;
  };
  last_cell = s;
  if (fld[s] != 0) {
    int a = s, prev = s, cur = soft_descend(fld, kc, W, H, s);
    uint32_t pen = soft_k(kc, s);
    while (cur >= 0) {
      const bool last = fld[cur] == 0;
      uint32_t seg = 0;
      const bool sight = soft_los(fld, kc, H, a, cur, seg);
      if (!sight || seg - soft_k(kc, cur) > pen || (fld[a] - fld[cur]) - pen >= (uint32_t)max_seg) {
        if (prev != a) { emit(prev); a = prev; pen = soft_k(kc, prev); continue; }          // cur is looked at again from the new anchor
        if (last) break;
        emit(cur); a = cur; pen = 0;
      }
      if (last) break;
      prev = cur;
      pen += soft_k(kc, cur);
      cur = soft_descend(fld, kc, W, H, cur);
    }
    if (cur < 0) return -1;
    last_cell = cur;
  }
  return count + 1;
}

}  // namespace

extern "C" int lipmpc_grid_clearance_cost_batch(int device, int64_t M, int32_t W, int32_t H, const uint8_t* occ, const int32_t* evidence,
                                                int32_t t_occ, int32_t r_clear, int32_t w_clear, uint8_t* cost, void* hip_stream) {
  if (bad_count(M) || bad_shape(W, H) || r_clear < 1 || r_clear > R_CLEAR_MAX || w_clear < 0 || w_clear > LIPMPC_COST_MAX) return LIPMPC_E_ARG;
  // (the map is occ or evidence, never both; t_occ is read with evidence alone)
  if ((occ != nullptr) == (evidence != nullptr) || !cost || (evidence && bad_threshold(t_occ))) return LIPMPC_E_ARG;
  if (const int rc = tiled_cap_refusal(M, W, H)) return rc;
  if (M == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  const int tiles_j = tiles_along(H, TILE_H), tiles = tiles_along(W, TILE_W) * tiles_j;
  const dim3 grid((unsigned)(M * tiles)), block(TILE_THREADS);
  hipLaunchKernelGGL(occ ? soft_cost_kernel<0> : soft_cost_kernel<1>, grid, block, 0, (hipStream_t)hip_stream, W, H, tiles_j, tiles, occ,
                     evidence, t_occ, r_clear, w_clear, cost);
  return launched();
}

extern "C" int lipmpc_grid_field_weighted_batch(int device, int64_t F, int32_t W, int32_t H, int32_t grid_shared, const double* origin,
                                                const double* cell, const uint8_t* occ, const uint8_t* cost, const double* goal,
                                                int32_t r_inflate, uint32_t* field, int32_t* field_status, void* work, int64_t work_bytes,
                                                int32_t max_rounds, int32_t resume, int32_t* settled, void* hip_stream) {
  return goal_field(device, F, W, H, grid_shared, origin, cell, occ, true, cost, goal, r_inflate, field, field_status, work, work_bytes,
                    max_rounds, resume, settled, hip_stream);
}

extern "C" int lipmpc_grid_frontier_field_weighted_batch(int device, int64_t F, int32_t W, int32_t H, const int32_t* evidence,
                                                         const uint8_t* cost, int32_t t_free, int32_t t_occ, int32_t r_inflate,
                                                         int32_t min_unknown, uint8_t* frontier, uint32_t* field, int32_t* n_frontier,
                                                         void* work, int64_t work_bytes, int32_t max_rounds, int32_t resume,
                                                         int32_t* settled, void* hip_stream) {
  return frontier_field(device, F, W, H, evidence, true, cost, t_free, t_occ, r_inflate, min_unknown, frontier, field, n_frontier, work,
                        work_bytes, max_rounds, resume, settled, hip_stream);
}

extern "C" int lipmpc_grid_path_weighted_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                               const double* cell, const uint8_t* occ, int32_t grid_shared, const uint8_t* cost,
                                               const uint32_t* field, const int32_t* field_status, const int32_t* settled,
                                               const double* goal, const double* start, int32_t r_inflate, int32_t max_seg, int32_t S_max,
                                               double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost, void* hip_stream) {
  if (const int rc = tiled_path_refusal(B, F, W, H, origin, cell, r_inflate, max_seg, S_max)) return rc;
  if (B == 0) return LIPMPC_OK;
  // LATE: B == 0 passes with any of them null
  if (any_null(occ, cost, field, field_status, settled, goal, start, sub_goals, n_sub, status, path_cost)) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(soft_goal_descent_kernel, path_grid(B), dim3(PATH_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H,
                     grid_shared ? (int64_t)0 : (int64_t)W * H, origin[0], origin[1], cell[0], cell[1], occ, cost, field, field_status,
                     settled, goal, start, r_inflate, max_seg, S_max, sub_goals, n_sub, status, path_cost);
  return launched();
}

extern "C" int lipmpc_grid_frontier_path_weighted_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                                        const double* cell, const int32_t* evidence, const uint8_t* cost, int32_t t_occ,
                                                        const uint32_t* field, const int32_t* n_frontier, const int32_t* settled,
                                                        const double* start, int32_t r_inflate, int32_t max_seg, int32_t S_max,
                                                        double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                                        int32_t* target_cell, void* hip_stream) {
  if (bad_threshold(t_occ)) return LIPMPC_E_ARG;
  if (const int rc = tiled_path_refusal(B, F, W, H, origin, cell, r_inflate, max_seg, S_max)) return rc;
  if (B == 0) return LIPMPC_OK;
  // LATE: B == 0 passes with any of them null
  if (any_null(evidence, cost, field, n_frontier, settled, start, sub_goals, n_sub, status, path_cost, target_cell)) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(soft_frontier_descent_kernel, path_grid(B), dim3(PATH_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H,
                     origin[0], origin[1], cell[0], cell[1], evidence, cost, t_occ, field, n_frontier, settled, start, r_inflate, max_seg,
                     S_max, sub_goals, n_sub, status, path_cost, target_cell);
  return launched();
}

// =====================================================================================================================
// WAVE-PER-ROBOT PATH CALLS (lipmpc_grid_path_wave_batch, lipmpc_grid_frontier_path_wave_batch,
// lipmpc_grid_frontier_utility_path_wave_batch): the path kernels above with a wavefront walking each robot's path; a section of its
// own that shares this file's helpers and constants
#include "lipmpc_field_wave.inc"
#include "lipmpc_field_robots.inc"
