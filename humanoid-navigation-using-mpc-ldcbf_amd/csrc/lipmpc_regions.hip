// lipmpc_regions.hip -- frontier REGIONS (lipmpc_grid_frontier_regions_batch, include/lipmpc.h): the maximal 8-connected groups of
// frontier cells of a mask, each cell's region root and size, and a table of the kept regions with centroid and representative.
// Connected-component labelling by a lock-free union-find whose parent words live in the `label` output itself:
//   regions_tile_kernel    one workgroup per (map, 32 x 64 tile): the tile's components in LDS; label = the tile component's least cell
//   regions_border_kernel  a lane per cell: the unions across tile borders, atomicMin on the parent words in global memory
//   regions_flatten_kernel a lane per cell: label = the root; the root's `size` word counts its cells
//   regions_count_kernel   a workgroup per 2048 consecutive cells: its roots and its kept roots; the statistics' start values
//   regions_scan_kernel    a workgroup per map: the chunks' kept counts into offsets; n_regions
//   regions_rank_kernel    a workgroup per chunk: a kept root's rank = the chunk's offset + the kept roots before it; table (root,
//                          size); every other cell takes its root's size
//   regions_sum_kernel     a lane per cell: the sums of i and j of every tabled region, 64-bit
//   regions_key_kernel     a lane per cell: the least key ((i - ci)^2 + (j - cj)^2, cell) of every tabled region
//   regions_table_kernel   a lane per table row: centroid and representative into the table, the representative's byte of `rep`
// NINE launches, whatever the map holds and whatever its size (without a table, R_max == 0, the first six).  Kernel boundaries are the only ordering between the passes: no
// thread ever waits for another thread's store.
//
// WHY THE UNION-FIND IS RIGHT AND ENDS.  The parent word p[c] of a frontier cell starts as c and is only ever lowered by
// atomicMin to a cell of the SAME region, so at all times p[c] <= c, and a chain c, p[c], p[p[c]], ... falls strictly until it
// reaches a cell with p[r] == r: find() takes at most as many steps as there are cells.  unite(a, b) of two adjacent cells
// repeats:  a, b = the ends of their chains; equal: done; let a > b; old = atomicMin(&p[a], b); old == a: a was a root and now
// hangs under b, done; otherwise somebody lowered p[a] first, and whichever of old and b is now NOT a's parent still has to be
// joined to the other: go on with (old, b), where old < a.  Every round ends the call or goes on with a strictly smaller pair
// (their sum falls: the chain ends never exceed the cells they came from, and old < a), so the rounds are bounded by twice the
// cell count.  No link is ever lost without the thread that replaced it joining its two ends again, so when every unite() of the
// adjacent pairs has returned, two cells are in one tree iff they are in one region; parents are smaller than children, so a
// tree's root is its region's least cell whatever order the races fell in.  The adjacent pairs united are, for each frontier cell
// c: W and N if N is a frontier cell, else W, NW and NE -- (c, NW) and (c, NE) with N set follow from (c, N) and N's own W / NE's
// own W pair.  Everything downstream is an integer add or a min over totally ordered keys: two calls give identical bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lipmpc.h"

namespace {

constexpr int TILE_W = 32, TILE_H = 64, TILE_CELLS = TILE_W * TILE_H;   // the tiled field's tiles
constexpr int THREADS = 256, PER_THREAD = TILE_CELLS / THREADS;
constexpr int CHUNK = 2048, CHUNK_PER_THREAD = CHUNK / THREADS;        // consecutive cells of the ranking passes
constexpr int MAX_SIDE = 4096;
constexpr int64_t MAX_TOTAL = (int64_t)1 << 31;
constexpr int MIN_SIZE_MAX = 1 << 24, R_MAX_MAX = 1 << 20;
constexpr uint64_t NO_KEY = ~0ull;

struct Stat {                      // per table rank
  unsigned long long sum_i, sum_j; // over the region's cells
  unsigned long long key;          // the least (d^2 << 32 | cell)
  unsigned long long pad;
};
static_assert(sizeof(Stat) == 32, "the workspace formula");

__host__ __device__ inline int64_t chunks_of(int64_t ncells) { return (ncells + CHUNK - 1) / CHUNK; }

// the workspace: [F * R_max] Stat, [F * ncells] int32 rank of the root cell, [F * chunks] int32 pairs (roots, kept roots -> offset)
inline int64_t work_bytes_of(int64_t F, int64_t ncells, int64_t R_max) {
  return 64 + (int64_t)sizeof(Stat) * F * R_max + 8 * ((F * ncells + 1) / 2) + 8 * F * chunks_of(ncells);      // a multiple of 8
}

template <typename P> __device__ inline int ld(P p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the end of c's chain.  p[x] < x for every cell that is not a root, so the chain falls strictly: at most `bound` (the cell count)
// steps, and the loop ends at the first root it meets.
template <typename P> __device__ inline int find(P p, int c, int bound) {
  for (int n = 0; n < bound; ++n) {
    const int q = ld(p + c);
    if (q == c) break;
    c = q;
  }
  return c;
}

// see WHY THE UNION-FIND IS RIGHT AND ENDS: every round returns or goes on with a strictly smaller pair of labels, so 2 * bound rounds
// are never all used.
template <typename P> __device__ inline void unite(P p, int a, int b, int bound) {
  for (int n = 0; n < 2 * bound; ++n) {
    a = find(p, a, bound);
    b = find(p, b, bound);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(p + a, b);
    if (old == a) return;
    a = old;
  }
}

// the neighbours of (i, j) a cell is united with, as offsets (di, dj), given which of W, NW, N, NE are frontier cells
__device__ inline int pairs_of(bool w, bool nw, bool n, bool ne) { return (w ? 1 : 0) | (n ? 4 : ((nw ? 2 : 0) | (ne ? 8 : 0))); }

__global__ __launch_bounds__(THREADS) void regions_tile_kernel(int W, int H, int tiles_i, int tiles_j, const uint8_t* __restrict__ frontier,
                                                               int32_t* __restrict__ label, int32_t* __restrict__ size,
                                                               uint8_t* __restrict__ rep) {
  __shared__ int par[TILE_CELLS];
  const int64_t tiles = (int64_t)tiles_i * tiles_j, blk = blockIdx.x;
  const int64_t f = blk / tiles;
  const int t = (int)(blk - f * tiles);
  const int i0 = (t / tiles_j) * TILE_W, j0 = (t % tiles_j) * TILE_H;
  const int64_t base = f * (int64_t)W * H;
  for (int k = 0; k < PER_THREAD; ++k) {
    const int l = threadIdx.x + k * THREADS, i = i0 + l / TILE_H, j = j0 + l % TILE_H;
    par[l] = (i < W && j < H && frontier[base + (int64_t)i * H + j] != 0) ? l : -1;
  }
  __syncthreads();
  for (int k = 0; k < PER_THREAD; ++k) {
    const int l = threadIdx.x + k * THREADS, li = l / TILE_H, lj = l % TILE_H;
    if (ld(par + l) < 0) continue;
    const bool w = lj > 0 && ld(par + l - 1) >= 0, n = li > 0 && ld(par + l - TILE_H) >= 0;
    const bool nw = li > 0 && lj > 0 && ld(par + l - TILE_H - 1) >= 0, ne = li > 0 && lj + 1 < TILE_H && ld(par + l - TILE_H + 1) >= 0;
    const int m = pairs_of(w, nw, n, ne);
    if (m & 1) unite(par, l, l - 1, TILE_CELLS);
    if (m & 2) unite(par, l, l - TILE_H - 1, TILE_CELLS);
    if (m & 4) unite(par, l, l - TILE_H, TILE_CELLS);
    if (m & 8) unite(par, l, l - TILE_H + 1, TILE_CELLS);
  }
  __syncthreads();
  for (int k = 0; k < PER_THREAD; ++k) {
    const int l = threadIdx.x + k * THREADS, i = i0 + l / TILE_H, j = j0 + l % TILE_H;
    if (i >= W || j >= H) continue;
    const int64_t c = base + (int64_t)i * H + j;
    int lab = -1;
    if (par[l] >= 0) {
      const int r = find(par, l, TILE_CELLS);
      lab = (i0 + r / TILE_H) * H + j0 + r % TILE_H;
    }
    label[c] = lab;
    size[c] = 0;
    if (rep) rep[c] = 0;
  }
}

__global__ __launch_bounds__(THREADS) void regions_border_kernel(int W, int H, int64_t total, int32_t* label) {
  const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (g >= total) return;
  const int ncells = W * H;
  const int64_t f = g / ncells;
  const int c = (int)(g - f * ncells), i = c / H, j = c - i * H;
  const int li = i % TILE_W, lj = j % TILE_H;
  if (li != 0 && lj != 0 && lj != TILE_H - 1) return;
  int32_t* p = label + f * ncells;
  if (ld(p + c) < 0) return;
  const bool w = j > 0 && ld(p + c - 1) >= 0, n = i > 0 && ld(p + c - H) >= 0;
  const bool nw = i > 0 && j > 0 && ld(p + c - H - 1) >= 0, ne = i > 0 && j + 1 < H && ld(p + c - H + 1) >= 0;
  const int m = pairs_of(w, nw, n, ne);
  // only the pairs that leave the tile: the others were united in LDS
  if ((m & 1) && lj == 0) unite(p, c, c - 1, ncells);
  if ((m & 2) && (li == 0 || lj == 0)) unite(p, c, c - H - 1, ncells);
  if ((m & 4) && li == 0) unite(p, c, c - H, ncells);
  if ((m & 8) && (li == 0 || lj == TILE_H - 1)) unite(p, c, c - H + 1, ncells);
}

// What one wavefront adds into words indexed by a key (a root, a rank).  While every live lane of the wavefront holds ONE key -- the
// common case: neighbours in memory are neighbours on the map -- the lanes' values are summed across the wavefront and carried in
// registers; the carried sums leave as one atomic per word when the key changes and at the end.  Mixed keys: a lane an atomic.
// Integer adds and mins commute, so the bits do not depend on which way a wavefront went.
__device__ inline int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline unsigned long long wave_min(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o);
    v = u < v ? u : v;
  }
  return v;
}
// true: the live lanes share the key `lead`
__device__ inline bool wave_uniform(bool live, long long key, long long& lead) {
  const unsigned long long m = __ballot(live);
  if (m == 0) { lead = -1; return true; }
  lead = __shfl(key, __ffsll((long long)m) - 1);
  return __all(!live || key == lead);
}

__global__ __launch_bounds__(THREADS) void regions_flatten_kernel(int W, int H, int64_t total, int32_t* label, int32_t* size) {
  const int ncells = W * H;
  const int lane = threadIdx.x & 63;
  long long carried = -1;                 // wave-uniform, as count
  int count = 0;
  for (int k = 0; k < CHUNK_PER_THREAD; ++k) {
    const int64_t g = (int64_t)blockIdx.x * CHUNK + k * THREADS + threadIdx.x;
    int root = -1;
    int64_t at = 0;
    if (g < total) {
      const int64_t f = g / ncells;
      at = f * ncells;
      const int q = ld(label + g);
      if (q >= 0) {
        root = find(label + at, q, ncells);
        if (root != q) __hip_atomic_store(label + g, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // an ancestor still: finds through c stay right
      }
    }
    // the key is the root's place in the whole batch, so that two maps' roots never share one
    const bool live = root >= 0;
    const long long key = live ? at + root : -1;
    long long lead;
    if (wave_uniform(live, key, lead)) {
      if (lead < 0) continue;
      const int n = wave_sum(live ? 1 : 0);
      if (lead != carried) {
        if (carried >= 0 && lane == 0) atomicAdd(size + carried, count);
        carried = lead;
        count = 0;
      }
      count += n;
    } else if (live) {
      atomicAdd(size + key, 1);
    }
  }
  if (carried >= 0 && lane == 0) atomicAdd(size + carried, count);
}

__device__ inline int block_sum(int v, int* lds) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}
static_assert(THREADS == 256, "block_sum adds four wavefronts");

__global__ __launch_bounds__(THREADS) void regions_count_kernel(int W, int H, int64_t chunks, int min_size, const int32_t* __restrict__ label,
                                                                const int32_t* __restrict__ size, int32_t* __restrict__ counts,
                                                                Stat* __restrict__ stat, int64_t n_stat) {
  __shared__ int lds[4];
  const int ncells = W * H;
  const int64_t f = blockIdx.x / chunks;
  const int ch = (int)(blockIdx.x - f * chunks);
  int all = 0, kept = 0;
  for (int k = 0; k < CHUNK_PER_THREAD; ++k) {
    const int c = ch * CHUNK + k * THREADS + threadIdx.x;
    if (c < ncells && label[f * ncells + c] == c) {
      ++all;
      kept += size[f * ncells + c] >= min_size ? 1 : 0;
    }
  }
  all = block_sum(all, lds);
  kept = block_sum(kept, lds);
  if (threadIdx.x == 0) {
    counts[2 * (int64_t)blockIdx.x] = all;
    counts[2 * (int64_t)blockIdx.x + 1] = kept;
  }
  // the statistics' start values, by the whole grid (n_stat = F * R_max rows)
  for (int64_t s = (int64_t)blockIdx.x * THREADS + threadIdx.x; s < n_stat; s += (int64_t)gridDim.x * THREADS) {
    stat[s].sum_i = 0;
    stat[s].sum_j = 0;
    stat[s].key = NO_KEY;
    stat[s].pad = 0;
  }
}

// one workgroup per map: counts[f, ch, 1] becomes the number of kept roots in the chunks before ch
__global__ __launch_bounds__(THREADS) void regions_scan_kernel(int64_t chunks, int R_max, int32_t* __restrict__ counts,
                                                               int32_t* __restrict__ n_regions) {
  __shared__ int part[THREADS];
  __shared__ int lds[4];
  int32_t* mine = counts + 2 * (int64_t)blockIdx.x * chunks;
  const int per = (int)((chunks + THREADS - 1) / THREADS);
  const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < chunks ? lo + per : chunks;
  int all = 0, kept = 0;
  for (int64_t ch = lo; ch < hi; ++ch) {
    all += mine[2 * ch];
    kept += mine[2 * ch + 1];
  }
  part[threadIdx.x] = kept;
  all = block_sum(all, lds);
  // an inclusive scan of the 256 partial sums (Hillis-Steele: 8 steps)
  for (int o = 1; o < THREADS; o <<= 1) {
    __syncthreads();
    const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
  }
  __syncthreads();
  int run = part[threadIdx.x] - kept;
  for (int64_t ch = lo; ch < hi; ++ch) {
    const int v = mine[2 * ch + 1];
    mine[2 * ch + 1] = run;
    run += v;
  }
  if (threadIdx.x == 0) {
    const int total = part[THREADS - 1];
    n_regions[3 * (int64_t)blockIdx.x] = all;
    n_regions[3 * (int64_t)blockIdx.x + 1] = total;
    n_regions[3 * (int64_t)blockIdx.x + 2] = total > R_max ? total - R_max : 0;
  }
}

// a thread takes CHUNK_PER_THREAD CONSECUTIVE cells here, so that ranks follow the cells' order
__global__ __launch_bounds__(THREADS) void regions_rank_kernel(int W, int H, int64_t chunks, int min_size, int R_max,
                                                               const int32_t* __restrict__ label, int32_t* size,
                                                               const int32_t* __restrict__ counts, int32_t* __restrict__ rankw,
                                                               int32_t* __restrict__ table) {
  __shared__ int part[THREADS];
  const int ncells = W * H;
  const int64_t f = blockIdx.x / chunks;
  const int ch = (int)(blockIdx.x - f * chunks);
  const int64_t base = f * ncells;
  const int c0 = ch * CHUNK + threadIdx.x * CHUNK_PER_THREAD;
  int lab[CHUNK_PER_THREAD], kept = 0;
  unsigned keep_bits = 0;
#pragma unroll
  for (int k = 0; k < CHUNK_PER_THREAD; ++k) {
    const int c = c0 + k;
    lab[k] = c < ncells ? label[base + c] : -1;
    if (lab[k] == c && size[base + c] >= min_size) {
      keep_bits |= 1u << k;
      ++kept;
    }
  }
  part[threadIdx.x] = kept;
  for (int o = 1; o < THREADS; o <<= 1) {
    __syncthreads();
    const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
  }
  __syncthreads();
  int rank = counts[2 * (int64_t)blockIdx.x + 1] + part[threadIdx.x] - kept;
#pragma unroll
  for (int k = 0; k < CHUNK_PER_THREAD; ++k) {
    const int c = c0 + k;
    if (lab[k] < 0) continue;
    if (lab[k] != c) {
      size[base + c] = size[base + lab[k]];       // a root's word is final since the flatten kernel and is not written here
      continue;
    }
    int r = -1;
    if (keep_bits >> k & 1u) {
      if (rank < R_max) {
        r = rank;
        int32_t* row = table + 5 * (f * R_max + rank);
        row[0] = c;
        row[1] = size[base + c];
      }
      ++rank;
    }
    rankw[base + c] = r;
  }
}

__global__ __launch_bounds__(THREADS) void regions_sum_kernel(int W, int H, int64_t total, int R_max, const int32_t* __restrict__ label,
                                                              const int32_t* __restrict__ rankw, Stat* stat) {
  const int ncells = W * H;
  const int lane = threadIdx.x & 63;
  long long carried = -1;                 // wave-uniform, as the sums; 8 rounds of 64 lanes of at most 4095 stay far inside 32 bits
  int si = 0, sj = 0;
  for (int k = 0; k < CHUNK_PER_THREAD; ++k) {
    const int64_t g = (int64_t)blockIdx.x * CHUNK + k * THREADS + threadIdx.x;
    long long key = -1;
    int i = 0, j = 0;
    if (g < total) {
      const int64_t f = g / ncells;
      const int c = (int)(g - f * ncells);
      const int root = label[g];
      if (root >= 0) {
        const int r = rankw[f * ncells + root];
        if (r >= 0) {
          key = f * R_max + r;
          i = c / H;
          j = c - i * H;
        }
      }
    }
    const bool live = key >= 0;
    long long lead;
    if (wave_uniform(live, key, lead)) {
      if (lead < 0) continue;
      const int ti = wave_sum(i), tj = wave_sum(j);
      if (lead != carried) {
        if (carried >= 0 && lane == 0) {
          atomicAdd(&stat[carried].sum_i, (unsigned long long)si);
          atomicAdd(&stat[carried].sum_j, (unsigned long long)sj);
        }
        carried = lead;
        si = sj = 0;
      }
      si += ti;
      sj += tj;
    } else if (live) {
      atomicAdd(&stat[key].sum_i, (unsigned long long)i);
      atomicAdd(&stat[key].sum_j, (unsigned long long)j);
    }
  }
  if (carried >= 0 && lane == 0) {
    atomicAdd(&stat[carried].sum_i, (unsigned long long)si);
    atomicAdd(&stat[carried].sum_j, (unsigned long long)sj);
  }
}

// the centroid of a tabled region: (2 S + n) / (2 n) on non-negative 64-bit values
__device__ inline void centroid_of(const Stat& s, int n, int& ci, int& cj) {
  const unsigned long long d = 2ull * (unsigned long long)n;
  ci = (int)((2ull * s.sum_i + (unsigned long long)n) / d);
  cj = (int)((2ull * s.sum_j + (unsigned long long)n) / d);
}

__global__ __launch_bounds__(THREADS) void regions_key_kernel(int W, int H, int64_t total, int R_max, const int32_t* __restrict__ label,
                                                              const int32_t* __restrict__ rankw, const int32_t* __restrict__ table, Stat* stat) {
  const int ncells = W * H;
  const int lane = threadIdx.x & 63;
  long long carried = -1;
  unsigned long long best = NO_KEY;
  for (int k = 0; k < CHUNK_PER_THREAD; ++k) {
    const int64_t g = (int64_t)blockIdx.x * CHUNK + k * THREADS + threadIdx.x;
    long long key = -1;
    unsigned long long mine = NO_KEY;
    if (g < total) {
      const int64_t f = g / ncells;
      const int c = (int)(g - f * ncells);
      const int root = label[g];
      if (root >= 0) {
        const int r = rankw[f * ncells + root];
        if (r >= 0) {
          key = f * R_max + r;
          // sum_i and sum_j are final (the kernel before this one) and only the key word is written here
          int ci, cj;
          centroid_of(stat[key], table[5 * key + 1], ci, cj);
          const int i = c / H, j = c - i * H;
          const long long di = i - ci, dj = j - cj;
          mine = ((unsigned long long)(di * di + dj * dj) << 32) | (unsigned)c;
        }
      }
    }
    const bool live = key >= 0;
    long long lead;
    if (wave_uniform(live, key, lead)) {
      if (lead < 0) continue;
      const unsigned long long m = wave_min(mine);
      if (lead != carried) {
        if (carried >= 0 && lane == 0) atomicMin(&stat[carried].key, best);
        carried = lead;
        best = NO_KEY;
      }
      best = m < best ? m : best;
    } else if (live) {
      atomicMin(&stat[key].key, mine);
    }
  }
  if (carried >= 0 && lane == 0) atomicMin(&stat[carried].key, best);
}

__global__ __launch_bounds__(THREADS) void regions_table_kernel(int W, int H, int64_t F, int R_max, const int32_t* __restrict__ n_regions,
                                                                const Stat* __restrict__ stat, int32_t* __restrict__ table,
                                                                uint8_t* __restrict__ rep) {
  // a grid-stride loop over the F * R_max rows: the grid is capped, the trip count follows from the sizes
  for (int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x; g < F * R_max; g += (int64_t)gridDim.x * THREADS) {
    const int64_t f = g / R_max;
    const int r = (int)(g - f * R_max);
    if (r >= n_regions[3 * f + 1]) continue;
    int32_t* row = table + 5 * g;
    int ci, cj;
    centroid_of(stat[g], row[1], ci, cj);
    const int cell = (int)(stat[g].key & 0xffffffffull);
    row[2] = ci * H + cj;
    row[3] = cell;
    row[4] = 0;
    if (rep && (unsigned)cell < (unsigned)(W * H)) rep[f * (int64_t)W * H + cell] = 1;      // (a tabled region always has a key)
  }
}

int check(int64_t F, int32_t W, int32_t H, int32_t R_max) {
  if (F < 0 || W < 2 || H < 2 || R_max < 0 || R_max > R_MAX_MAX) return LIPMPC_E_ARG;
  return LIPMPC_OK;
}
int supported(int64_t F, int32_t W, int32_t H) {
  if (W > MAX_SIDE || H > MAX_SIDE) return LIPMPC_E_UNSUPPORTED;
  if (F > MAX_TOTAL || F * (int64_t)W * H > MAX_TOTAL) return LIPMPC_E_UNSUPPORTED;
  return LIPMPC_OK;
}

}  // namespace

extern "C" int64_t lipmpc_grid_frontier_regions_workspace_bytes(int64_t F, int32_t W, int32_t H, int32_t R_max) {
  if (int rc = check(F, W, H, R_max)) return rc;
  if (int rc = supported(F, W, H)) return rc;
  return work_bytes_of(F, (int64_t)W * H, R_max);
}

extern "C" int lipmpc_grid_frontier_regions_batch(int device, int64_t F, int32_t W, int32_t H, const uint8_t* frontier, int32_t min_size,
                                                  int32_t R_max, void* work, int64_t work_bytes, int32_t* label, int32_t* size,
                                                  uint8_t* rep, int32_t* table, int32_t* n_regions, void* hip_stream) {
  if (int rc = check(F, W, H, R_max)) return rc;
  if (min_size < 1 || min_size > MIN_SIZE_MAX || !frontier || !work || ((uintptr_t)work & 7) || !label || !size || !n_regions ||
      (R_max > 0 && !table))
    return LIPMPC_E_ARG;
  // the size of `work` can only be judged for a supported shape: an unsupported one with every other argument right is UNSUPPORTED
  const int sup = supported(F, W, H);
  if (sup == LIPMPC_OK && work_bytes < work_bytes_of(F, (int64_t)W * H, R_max)) return LIPMPC_E_ARG;
  if (sup != LIPMPC_OK) return sup;
  if (F == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t ncells = (int64_t)W * H, total = F * ncells, chunks = chunks_of(ncells);
  const int tiles_i = (W + TILE_W - 1) / TILE_W, tiles_j = (H + TILE_H - 1) / TILE_H;
  Stat* stat = (Stat*)work;
  int32_t* rankw = (int32_t*)(stat + F * R_max);
  int32_t* counts = rankw + total;
  const dim3 threads(THREADS);
  const dim3 per_cell((unsigned)((total + THREADS - 1) / THREADS)), per_chunk((unsigned)((total + CHUNK - 1) / CHUNK));
  hipLaunchKernelGGL(regions_tile_kernel, dim3((unsigned)(F * tiles_i * tiles_j)), threads, 0, s, W, H, tiles_i, tiles_j, frontier, label,
                     size, rep);
  hipLaunchKernelGGL(regions_border_kernel, per_cell, threads, 0, s, W, H, total, label);
  hipLaunchKernelGGL(regions_flatten_kernel, per_chunk, threads, 0, s, W, H, total, label, size);
  hipLaunchKernelGGL(regions_count_kernel, dim3((unsigned)(F * chunks)), threads, 0, s, W, H, chunks, min_size, label, size, counts, stat,
                     F * R_max);
  hipLaunchKernelGGL(regions_scan_kernel, dim3((unsigned)F), threads, 0, s, chunks, R_max, counts, n_regions);
  hipLaunchKernelGGL(regions_rank_kernel, dim3((unsigned)(F * chunks)), threads, 0, s, W, H, chunks, min_size, R_max, label, size, counts,
                     rankw, table);
  if (R_max > 0) {
    hipLaunchKernelGGL(regions_sum_kernel, per_chunk, threads, 0, s, W, H, total, R_max, label, rankw, stat);
    hipLaunchKernelGGL(regions_key_kernel, per_chunk, threads, 0, s, W, H, total, R_max, label, rankw, table, stat);
    const int64_t row_blocks = (F * R_max + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(regions_table_kernel, dim3((unsigned)(row_blocks < (1 << 20) ? row_blocks : (1 << 20))), threads, 0, s, W, H, F,
                       R_max, n_regions, stat, table, rep);
  }
  return hipGetLastError() == hipSuccess ? LIPMPC_OK : LIPMPC_E_HIP;
}
