// lipmpc_field_robots.inc -- the last section of lipmpc_field.hip: CLAIMS FROM PER-ROBOT FIELDS
// (lipmpc_grid_frontier_assign_robot_fields_batch).  The claim calls above relax the whole map once per claim: field_k, from what is
// left of the sources, tells every robot its cost.  Here every robot of U_0 gets ONE single-source field D_b from its own entry
// cell; the B fields are independent, so they are relaxed together by the rounds of THE TILED FIELD (tiled_round_kernel with F = B
// and one shared blocked bitmap).  The move rules are symmetric, so D_b(c) is also the cost from c to the robot, and
// min over c in S of D_b(c) is what field_k would have told robot b: every claim round, and the whole keep phase, is a reduction
// over words that are already in memory.
// THE SEQUENCE, fixed by the host: set-up (cells), robots (a wave per robot), fill (B fields), max_rounds rounds, their settle
// kernel, the all-settled word, the claim kernel (ONE workgroup: the keep phase and every greedy round in a loop), the walks (a
// wave per winner, all winners at once), the finish: max_rounds + 8 launches whatever max_claims is; a resumed call leaves out
// the first three.
// WHY THE CLAIM KERNEL'S RESULT IS FREE OF ORDER.  Every reduction is a minimum over 64-bit integer keys with a total order --
// (d^2, cell) for an anchor, (cost, cell) for a robot's best source, (cost, robot) for a round's winner -- taken by shuffles and
// 64-bit atomicMin: a minimum does not depend on the order in which its operands arrive.  A robot's cached best (cost, cell) is
// recomputed only when that cell left S; sources only ever leave, so any other cached best is still the minimum over the smaller
// set.  The live-source bitmap is cleared word by word, a word by one thread.
// THE WORKSPACE (32-bit words): CTL control words, best [B] (64 bits each), then entry, in_u, target, round, was_kept, fsettled [B]
// each, the impassable bitmap, the sources S_0 and the live sources S (bitmap_words each), the two flag arrays [B, tiles], then
// the B fields.

namespace {

constexpr int ROBOT_CTL = 16;                         // control words: 8-byte aligned data follows
constexpr int RCTL_ALL = 0, RCTL_CLAIMS = 1, RCTL_KEPT = 2;
constexpr int ROBOT_FIELDS_LAUNCHES = 8;              // beside the rounds, of a cold call

struct RobotLayout {
  int64_t bm_words, tiles, best, entry, in_u, target, round, was_kept, fsettled, blocked, sources, live, flags0, flags1, fields, words;
};
inline RobotLayout robot_layout(int64_t B, int64_t W, int64_t H) {
  RobotLayout l;
  l.bm_words = bitmap_words(W * H);
  l.tiles = (int64_t)tiles_along((int)W, TILE_W) * tiles_along((int)H, TILE_H);
  l.best = ROBOT_CTL;
  l.entry = l.best + 2 * B;
  l.in_u = l.entry + B;
  l.target = l.in_u + B;
  l.round = l.target + B;
  l.was_kept = l.round + B;
  l.fsettled = l.was_kept + B;
  l.blocked = l.fsettled + B;
  l.sources = l.blocked + l.bm_words;
  l.live = l.sources + l.bm_words;
  l.flags0 = l.live + l.bm_words;
  l.flags1 = l.flags0 + B * l.tiles;
  l.fields = l.flags1 + B * l.tiles;
  l.words = l.fields + B * W * H;
  return l;
}
// (of a shape within the caps: B * (W * H + 64) <= 2^31, so nothing wraps)
inline int64_t robot_bytes(int64_t B, int64_t W, int64_t H) { return 4 * robot_layout(B, W, H).words + 256; }

// (a) set-up, over cells: impassable = the given field is INF, S_0 = the given frontier on passable cells, both by ballots; both
// flag arrays of all B fields cleared; the control words
__global__ void __launch_bounds__(SETUP_THREADS) robot_setup_kernel(int ncells, int64_t flag_words, const uint8_t* __restrict__ frontier,
                                                                    const uint32_t* __restrict__ field, uint32_t* __restrict__ ctl,
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
    if (tid >= 2 && tid < 2 + ROBOT_CTL) ctl[tid - 2] = 0;
  }
  const int64_t step = (int64_t)gridDim.x * SETUP_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * SETUP_THREADS + tid; k < flag_words; k += step) flags[k] = 0;
}

// (b) the robots, a wave each: membership of U_0 and the ENTRY -- the start cell if passable, else the snap in the GIVEN field --
// or -1; the flags of the entry's tiles for the first round.  A robot outside U_0 sets no flag: its tiles stay idle.
__global__ void __launch_bounds__(WAVEWALK_THREADS) robot_entry_kernel(int64_t B, int W, int H, double ox, double oy, double dx, double dy,
                                                                       const uint32_t* __restrict__ field, const double* __restrict__ start,
                                                                       const int8_t* __restrict__ may_claim,
                                                                       const int32_t* __restrict__ status, int r_inflate, int tiles,
                                                                       int32_t* __restrict__ entry, uint32_t* flags0) {
  const int64_t b = wave_robot(B);
  if (b < 0) return;
  const int lane = threadIdx.x % WAVE;
  const int sb = uni(status[b]);
  int e = -1, si = 0, sj = 0;
  if ((sb == LIPMPC_RRT_FOUND || sb == LIPMPC_RRT_PATH_OVERFLOW) && (!may_claim || uni((int)may_claim[b]) != 0) &&
      uni((int)cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj))) {
    si = uni(si); sj = uni(sj);
    e = si * H + sj;
    if (uni(field[e]) == INF) e = wave_snap(field, W, H, si, sj, r_inflate, lane);
  }
  if (lane == 0) {
    entry[b] = e;
    if (e >= 0) flag_round_seed(flags0 + b * tiles, W, H, tiles_along(H, TILE_H), e / H, e % H);
  }
}

// (b) the fill, blockIdx.x = robot * chunks + chunk: D_b = 0 at the entry and INF elsewhere
__global__ void __launch_bounds__(SETUP_THREADS) robot_fill_kernel(int ncells, int chunks, const int32_t* __restrict__ entry,
                                                                   uint32_t* __restrict__ fields) {
  const int64_t b = blockIdx.x / chunks;
  const int c = (blockIdx.x - (int)b * chunks) * SETUP_THREADS + threadIdx.x;
  if (c < ncells) fields[b * ncells + c] = c == entry[b] ? 0u : INF;
}

// (d) after the settle kernel: the all-settled word = the given field is settled and so is every robot's
__global__ void __launch_bounds__(SETUP_THREADS) robot_all_settled_kernel(int64_t B, const int32_t* __restrict__ settled,
                                                                          const int32_t* __restrict__ fsettled, uint32_t* __restrict__ ctl) {
  int open = 0;
  for (int64_t b = threadIdx.x; b < B; b += SETUP_THREADS) open |= fsettled[b] == 0;
  open = __syncthreads_or(open);
  if (threadIdx.x == 0) ctl[RCTL_ALL] = settled[0] != 0 && !open;
}

// the least key of the workgroup, in every thread: a butterfly per wave, one 64-bit atomicMin per wave, ONE barrier.  Three slots
// in rotation: the slot of the call after next is reset by thread 0 behind this call's barrier -- everybody has read it (before
// this barrier) and nobody lowers it before the next one.
__device__ __forceinline__ unsigned long long group_min(unsigned long long mine, unsigned long long* slots, int& turn) {
  for (int o = 32; o; o >>= 1) mine = min(mine, (unsigned long long)__shfl_xor(mine, o));
  if ((threadIdx.x & 63) == 0 && mine != ~0ull) atomicMin(slots + turn, mine);
  __syncthreads();
  const unsigned long long least = slots[turn];
  const int before = turn == 0 ? 2 : turn - 1;
  if (threadIdx.x == 0) slots[before] = ~0ull;
  turn = turn == 2 ? 0 : turn + 1;
  return least;
}

// S loses the disc round t, clipped to the grid: a word of the bitmap by one thread, the set bits alone
__device__ __forceinline__ void clear_disc(uint32_t* live, int W, int H, int t, int r_claim) {
  const int ti = t / H, tj = t - ti * H;
  const int i_lo = max(ti - r_claim, 0), i_hi = min(ti + r_claim, W - 1);
  const int64_t r2 = (int64_t)r_claim * r_claim;
  for (int w = ((i_lo * H) >> 5) + threadIdx.x; w <= (((i_hi + 1) * H - 1) >> 5); w += FIELD_THREADS) {
    const uint32_t word = live[w];
    uint32_t left = word;
    for (uint32_t bits = word; bits; bits &= bits - 1) {
      const int c = (w << 5) + __builtin_ctz(bits), i = c / H, j = c - i * H;
      if ((int64_t)(i - ti) * (i - ti) + (int64_t)(j - tj) * (j - tj) <= r2) left &= ~(1u << (c & 31));
    }
    if (left != word) live[w] = left;
  }
}

// the best source of robot b in S: the least (D_b(c) << 32 | c) over the set bits, ~0 for none within reach
__device__ __forceinline__ unsigned long long best_source(const uint32_t* live, const uint32_t* __restrict__ D, int words) {
  unsigned long long mine = ~0ull;
  for (int w = threadIdx.x; w < words; w += FIELD_THREADS)
    for (uint32_t bits = live[w]; bits; bits &= bits - 1) {
      const int c = (w << 5) + __builtin_ctz(bits);
      const uint32_t v = D[c];
      if (v != INF) mine = min(mine, ((unsigned long long)v << 32) | (uint32_t)c);
    }
  return mine;
}

// the bests of the robots of U whose best source is gone (`all`: everybody's), one robot after the other in ascending index, the
// whole workgroup on each
__device__ __forceinline__ void refresh_bests(int64_t B, int H, int words, int64_t ncells, bool all, int t, int r_claim, const uint32_t* live,
                                              const uint32_t* __restrict__ fields, const int32_t* in_u, unsigned long long* best,
                                              unsigned long long* slots, int& turn) {
  const int tid = threadIdx.x, ti = t / H, tj = t - ti * H;
  const int64_t r2 = (int64_t)r_claim * r_claim;
  for (int64_t base = 0; base < B; base += FIELD_THREADS) {
    const int64_t mb = base + tid;
    bool stale = false;
    if (mb < B && in_u[mb] != 0) {
      const uint32_t c = (uint32_t)(best[mb] & 0xFFFFFFFFull);
      const int i = (int)c / H, j = (int)c - i * H;
      stale = all || (c != INF && (int64_t)(i - ti) * (i - ti) + (int64_t)(j - tj) * (j - tj) <= r2);
    }
    for (int cursor = 0;;) {
      const unsigned long long nx = group_min(stale && tid >= cursor ? (unsigned long long)tid : ~0ull, slots, turn);
      if (nx == ~0ull) break;
      cursor = (int)nx + 1;
      const int64_t rb = base + (int64_t)nx;
      const unsigned long long found = group_min(best_source(live, fields + rb * ncells, words), slots, turn);
      if (tid == 0) best[rb] = found;
    }
    __syncthreads();                                    // (thread 0's bests before anybody reads them)
  }
}

// (e) THE CLAIM KERNEL, one workgroup: the keep phase, then the greedy rounds, on the words the rounds left in memory.  It writes
// the winners' target, round and kept word into the workspace; the rows are the walks'.
__global__ void __launch_bounds__(FIELD_THREADS) robot_claim_kernel(int64_t B, int W, int H, int r_claim, int r_keep, int keep_ratio16,
                                                                    int keep_slack, int max_claims, uint32_t* ctl,
                                                                    const uint32_t* __restrict__ field,
                                                                    const uint32_t* __restrict__ fields,
                                                                    const int32_t* __restrict__ prev_target,
                                                                    const int32_t* __restrict__ entry, const uint32_t* __restrict__ src0,
                                                                    uint32_t* live, int32_t* in_u, int32_t* target, int32_t* round,
                                                                    int32_t* was_kept, unsigned long long* best) {
  __shared__ unsigned long long slots[3];
  const int tid = threadIdx.x;
  if (ctl[RCTL_ALL] == 0) return;                       // (one word for the whole workgroup: uniform)
  const int64_t ncells = (int64_t)W * H;
  const int words = (int)bitmap_words(ncells);
  if (tid < 3) slots[tid] = ~0ull;
  for (int w = tid; w < words; w += FIELD_THREADS) live[w] = src0[w];
  for (int64_t b = tid; b < B; b += FIELD_THREADS) {
    in_u[b] = entry[b] >= 0;
    target[b] = -1;
    round[b] = -1;
    was_kept[b] = 0;
    best[b] = ~0ull;
  }
  __syncthreads();
  int turn = 0, k = 0, n_kept = 0;

  // the keep phase: the robots of U_0 with a previous target, in ascending index
  if (prev_target) {
    for (int64_t base = 0; base < B && k < max_claims; base += FIELD_THREADS) {
      const int64_t mb = base + tid;
      const bool candidate = mb < B && in_u[mb] != 0 && is_cell(prev_target[mb], (int)ncells);
      for (int cursor = 0; k < max_claims;) {
        const unsigned long long nx = group_min(candidate && tid >= cursor ? (unsigned long long)tid : ~0ull, slots, turn);
        if (nx == ~0ull) break;
        cursor = (int)nx + 1;
        const int64_t wb = base + (int64_t)nx;
        unsigned long long mine = anchor_key(live, prev_target[wb], r_keep, W, H);
        if ((tid & 63) != 0) mine = ~0ull;              // (anchor_key leaves the wave's least in every lane)
        const unsigned long long found = group_min(mine, slots, turn);
        if (found == ~0ull) continue;                   // nothing is left of the target
        const int a = (int)(found & 0xFFFFFFFFull);
        const unsigned long long cost = fields[wb * ncells + a], near = field[entry[wb]];
        if (cost == INF || 16ull * cost > (unsigned long long)keep_ratio16 * near + 80ull * (unsigned long long)keep_slack) continue;
        if (tid == 0) { target[wb] = a; round[wb] = k; was_kept[wb] = 1; in_u[wb] = 0; }
        clear_disc(live, W, H, a, r_claim);
        ++k;
        ++n_kept;
        __syncthreads();                                // (S as it is now, before the next anchor search)
      }
    }
  }

  // the greedy rounds
  refresh_bests(B, H, words, ncells, true, 0, 0, live, fields, in_u, best, slots, turn);
  while (k < max_claims) {
    unsigned long long mine = ~0ull;
    for (int64_t b = tid; b < B; b += FIELD_THREADS)
      if (in_u[b] != 0 && best[b] != ~0ull) mine = min(mine, (best[b] & 0xFFFFFFFF00000000ull) | (unsigned long long)b);
    const unsigned long long win = group_min(mine, slots, turn);
    if (win == ~0ull) break;                            // U or S is used up, or nobody reaches what is left
    const int64_t wb = (int64_t)(win & 0xFFFFFFFFull);
    const int t = (int)(best[wb] & 0xFFFFFFFFull);
    __syncthreads();                                    // (everybody has read the winner's best and U)
    if (tid == 0) { target[wb] = t; round[wb] = k; in_u[wb] = 0; }
    clear_disc(live, W, H, t, r_claim);
    ++k;
    __syncthreads();
    refresh_bests(B, H, words, ncells, false, t, r_claim, live, fields, in_u, best, slots, turn);
  }
  if (tid == 0) { ctl[RCTL_CLAIMS] = (uint32_t)k; ctl[RCTL_KEPT] = (uint32_t)n_kept; }
}

// (f) the walks, a wave per robot, every winner at once: wave_walk() from the target t DOWN D_b to the entry (the word 0), the
// sight judged on PASSABILITY -- the given field -- while the descent and the cost since the anchor are D_b's.  Count, then -- if
// the sub-goals fit -- walk again and write each mark at its REVERSED row (the chain runs from the target to the robot, the
// sub-goals from the robot to the target).  A descent that breaks off (n < 0) cannot happen on settled fields of this map: D_b(t)
// is finite, so the chain exists; the robot then still claims and is reported as PATH_OVERFLOW with nothing written.
__global__ void __launch_bounds__(WAVEWALK_THREADS) robot_walk_kernel(
    int64_t B, int W, int H, double ox, double oy, double dx, double dy, int max_seg, int S_max, const uint32_t* __restrict__ ctl,
    const uint32_t* __restrict__ field, const uint32_t* __restrict__ fields, const int32_t* __restrict__ target,
    const int32_t* __restrict__ round, const int32_t* __restrict__ was_kept, double* __restrict__ sub_goals, int32_t* __restrict__ n_sub,
    int32_t* __restrict__ status, double* __restrict__ path_cost, int32_t* __restrict__ target_cell, int32_t* __restrict__ claim_round,
    int8_t* __restrict__ kept) {
  const int64_t b = wave_robot(B);
  if (b < 0 || uni(ctl[RCTL_ALL]) == 0) return;
  const int t = uni(target[b]);
  if (t < 0) return;
  const int lane = threadIdx.x % WAVE;
  const uint32_t* D = fields + b * (int64_t)W * H;
  double* sg = sub_goals + b * (int64_t)S_max * 2;
  auto entry = [](int, uint32_t word) { return word == 0; };
  int last_cell;
  const int n = wave_walk(D, nullptr, W, H, t, max_seg, lane, last_cell, entry, [](int, int) {}, field);
  const bool fits = n > 0 && n <= S_max;
  if (fits) {
    wave_walk(D, nullptr, W, H, t, max_seg, lane, last_cell, entry, [&](int c, int mark) {
      if (lane == 0) centre(c, H, ox, oy, dx, dy, sg + 2 * (n - 2 - mark));
    }, field);
    if (lane == 0) centre(t, H, ox, oy, dx, dy, sg + 2 * (n - 1));
  }
  if (lane == 0) {
    status[b] = fits ? LIPMPC_RRT_FOUND : LIPMPC_RRT_PATH_OVERFLOW;
    n_sub[b] = fits ? n : 0;
    path_cost[b] = (double)D[t] / 5.0;
    target_cell[b] = t;
    claim_round[b] = round[b];
    if (kept) kept[b] = (int8_t)was_kept[b];
  }
}

// (g) the finish, over robots: the followers (everybody, where some field did not settle) and the counts
__global__ void __launch_bounds__(SETUP_THREADS) robot_finish_kernel(int64_t B, const uint32_t* __restrict__ ctl,
                                                                     const int32_t* __restrict__ target, int32_t* __restrict__ claim_round,
                                                                     int8_t* __restrict__ kept, int32_t* __restrict__ n_claims,
                                                                     int32_t* __restrict__ n_kept, int32_t* __restrict__ claims_settled) {
  const int64_t b = (int64_t)blockIdx.x * SETUP_THREADS + threadIdx.x;
  const bool all = ctl[RCTL_ALL] != 0;
  if (b < B && (!all || target[b] < 0)) {
    claim_round[b] = -1;
    if (kept) kept[b] = 0;
  }
  if (b == 0) {
    n_claims[0] = all ? (int32_t)ctl[RCTL_CLAIMS] : 0;
    if (n_kept) n_kept[0] = all ? (int32_t)ctl[RCTL_KEPT] : 0;
    claims_settled[0] = all;
  }
}

}  // namespace

extern "C" int64_t lipmpc_grid_frontier_assign_robot_fields_workspace_bytes(int64_t B, int32_t W, int32_t H) {
  if (bad_count(B) || bad_shape(W, H)) return LIPMPC_E_ARG;
  if (const int rc = tiled_cap_refusal(B, W, H)) return rc;
  return robot_bytes(B, W, H);
}

extern "C" int lipmpc_grid_frontier_assign_robot_fields_batch(
    int device, int64_t B, int32_t W, int32_t H, const double* origin, const double* cell, const uint8_t* frontier, const uint32_t* field,
    const int32_t* settled, const double* start, const int8_t* may_claim, const int32_t* prev_target, int32_t r_inflate, int32_t r_claim,
    int32_t r_keep, int32_t keep_ratio16, int32_t keep_slack, int32_t max_claims, int32_t max_seg, int32_t S_max, void* work,
    int64_t work_bytes, int32_t max_rounds, int32_t resume, double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
    int32_t* target_cell, int32_t* claim_round, int32_t* n_claims, int8_t* kept, int32_t* n_kept, int32_t* claims_settled,
    void* hip_stream) {
  // (the keep words are tested even without a previous target; kept and n_kept are needed with one alone.  The launches do not
  // grow with max_claims, so max_claims * max_rounds has no limit here, unlike the claim calls by tiles)
  if (bad_claim(B, r_claim, max_claims, max_seg, S_max, frontier, field, settled, start, work, sub_goals, n_sub, status, path_cost,
                target_cell, claim_round, n_claims, claims_settled) ||
      bad_claim_rounds(work, max_rounds, resume) || bad_keep(r_keep, keep_ratio16, keep_slack) ||
      (prev_target && any_null(kept, n_kept)) || bad_placed_grid(W, H, origin, cell, r_inflate))
    return LIPMPC_E_ARG;
  if (const int rc = tiled_cap_refusal(B, W, H)) return rc;
  if (work_bytes < robot_bytes(B, W, H)) return LIPMPC_E_ARG;
  if (B == 0) return LIPMPC_OK;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const RobotLayout r = robot_layout(B, W, H);
  const int ncells = W * H, padded = (int)(r.bm_words - 2) * 32, chunks = (padded + SETUP_THREADS - 1) / SETUP_THREADS;
  const int tiles = (int)r.tiles;
  const dim3 robots((unsigned)((B + SETUP_THREADS - 1) / SETUP_THREADS)), setup(SETUP_THREADS), one(1);
  const double ox = origin[0], oy = origin[1], dx = cell[0], dy = cell[1];
  uint32_t* w = (uint32_t*)work;
  int32_t* wi = (int32_t*)work;
  unsigned long long* best = (unsigned long long*)(w + r.best);
  if (!resume) {
    hipLaunchKernelGGL(robot_setup_kernel, dim3((unsigned)chunks), setup, 0, s, ncells, 2 * B * r.tiles, frontier, field, w, w + r.blocked,
                       w + r.sources, w + r.flags0);
    hipLaunchKernelGGL(robot_entry_kernel, wave_grid(B), dim3(WAVEWALK_THREADS), 0, s, B, W, H, ox, oy, dx, dy, field, start, may_claim,
                       status, r_inflate, tiles, wi + r.entry, w + r.flags0);
    hipLaunchKernelGGL(robot_fill_kernel, dim3((unsigned)(B * chunks)), setup, 0, s, ncells, chunks, wi + r.entry, w + r.fields);
  }
  if (const int rc = tiled_rounds(s, B, W, H, 0, round_buffers(r, w), w + r.fields, max_rounds, wi + r.fsettled)) return rc;
  hipLaunchKernelGGL(robot_all_settled_kernel, one, setup, 0, s, B, settled, wi + r.fsettled, w);
  hipLaunchKernelGGL(robot_claim_kernel, one, dim3(FIELD_THREADS), 0, s, B, W, H, r_claim, r_keep, keep_ratio16, keep_slack, max_claims, w,
                     field, w + r.fields, prev_target, wi + r.entry, w + r.sources, w + r.live, wi + r.in_u, wi + r.target, wi + r.round,
                     wi + r.was_kept, best);
  hipLaunchKernelGGL(robot_walk_kernel, wave_grid(B), dim3(WAVEWALK_THREADS), 0, s, B, W, H, ox, oy, dx, dy, max_seg, S_max, w, field,
                     w + r.fields, wi + r.target, wi + r.round, wi + r.was_kept, sub_goals, n_sub, status, path_cost, target_cell,
                     claim_round, kept);
  hipLaunchKernelGGL(robot_finish_kernel, robots, setup, 0, s, B, w, wi + r.target, claim_round, kept, n_claims, n_kept, claims_settled);
  return launched();
}
