// lipmpc_field_wave.inc -- the last section of lipmpc_field.hip: WAVE-PER-ROBOT PATH CALLS (lipmpc_grid_path_wave_batch,
// lipmpc_grid_frontier_path_wave_batch, lipmpc_grid_frontier_utility_path_wave_batch).  The one-lane path kernels above walk a
// robot's path in ONE lane: every sight test re-walks its segment cell by cell and every descent step reads up to 24 words one
// after the other.  Here a wavefront of 64 lanes walks one robot's path:
//   wave_snap     the lanes stride over the snap window, then one wave minimum of (d^2, field, index)
//   wave_descend  eight lanes take one neighbour each (and a diagonal's two side cells): one load round, a ballot, the first set
//                 lane in the contract's order (di major, dj minor)
//   wave_sight    lane l tests segment cell k = l + 64 t by the CLOSED FORM of los()'s quotients; a ballot per 64 cells ends the
//                 test at the first chunk that holds an impassable cell; the weighted form sums k over the cells across the wave
//   wave_walk     walk() / soft_walk() / walk_to(), rule for rule, on those three
// The outputs are the one-lane calls', bit for bit: every rule is an integer comparison on the same words, the sums are integer
// sums (the same in any order), and the cell centres are written by centre() itself.
// UNIFORMITY.  Anchor, previous and current cell, their field words, the count, the penalty and every status are the same in all
// 64 lanes: each is read back from a ballot, a readfirstlane or a butterfly that leaves one value in every lane, so all lanes take
// every branch together.  A workgroup is four waves = four robots that never wait for each other: no barrier, no LDS.
// THE CLOSED FORM.  los() walks (qi, ri) with qi * 2m + ri = m + 2k * di and ri in [0, 2m): one carry a step is enough because
// |2 di| <= 2m.  Hence qi(k) = floor((2k * di + m) / (2m)), and the same for j.  After the endpoint swap di >= 0, but dj may be
// negative; dj + m >= 0, so floor((2k * dj + m) / (2m)) = floor((m + 2k * (dj + m)) / (2m)) - k with a numerator that is never
// negative: unsigned division is exact.  At 4096 cells a side k, m <= 4095 and dj + m <= 8190: the numerators stay below 2^27.
// TERMINATION ON ANY FIELD.  wave_descend() takes a neighbour only where v < fc, strictly: the words of the cells a walk descends
// fall strictly, so no cell is descended twice and a walk makes at most W * H descents, whatever `field` holds (a stale field, a
// constant one, another map's).  Between two descents the loop body runs at most twice (the `continue` sets a = prev, after which
// prev != a is false), and a sight test visits m + 1 <= 4096 cells.  No loop's end depends on the field being a cost-to-go field.
// TWO PASSES, as the one-lane bodies: count, then -- if the sub-goals fit -- walk again and write ("more than S_max: nothing
// written" needs the count before the first row).  One lane writes the rows.

namespace {

constexpr int WAVE = 64;
constexpr int WAVEWALK_THREADS = 256, WAVEWALK_ROBOTS = WAVEWALK_THREADS / WAVE;     // robot b = 4 * blockIdx.x + wave

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the penalty of cell c (a uniform index): soft_k() on a cost layer, 0 without one
__device__ __forceinline__ uint32_t wave_k(const uint8_t* __restrict__ kc, int c) { return kc ? uni(soft_k(kc, c)) : 0u; }

// snap(): per lane the least (d^2, field) of its cells, ascending index so only a smaller pair replaces; then the least
// (key, index) over the wave, which every lane ends up holding
__device__ __forceinline__ int wave_snap(const uint32_t* __restrict__ fld, int W, int H, int si, int sj, int r_inflate, int lane) {
  const int n = r_inflate + 1;
  const int i0 = max(si - n, 0), j0 = max(sj - n, 0), wj = min(sj + n, H - 1) - j0 + 1, cells = (min(si + n, W - 1) - i0 + 1) * wj;
  uint64_t best = ~0ull;
  int at = 0x7fffffff;
  for (int x = lane; x < cells; x += WAVE) {
    const int i = i0 + x / wj, j = j0 + x % wj;
    const uint32_t v = fld[i * H + j];
    const uint64_t key = ((uint64_t)(uint32_t)((i - si) * (i - si) + (j - sj) * (j - sj)) << 32) | v;
    if (v != INF && key < best) { best = key; at = i * H + j; }
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const uint64_t ok = __shfl_xor(best, off, WAVE);
    const int oa = __shfl_xor(at, off, WAVE);
    if (ok < best || (ok == best && oa < at)) { best = ok; at = oa; }
  }
  at = uni(at);
  return at == 0x7fffffff ? -1 : at;
}

// descend() / soft_descend() from c (field word fc, penalty kcur): lanes 0..7 are the neighbours in the contract's order; a lane
// that has no neighbour inside the map reads c itself and fails the test.  The next cell and its word, or -1.
__device__ __forceinline__ int wave_descend(const uint32_t* __restrict__ fld, int W, int H, int c, uint32_t fc, uint32_t kcur, int lane,
                                            uint32_t& fnext) {
  const int i = c / H, j = c - i * H;
  const int slot = (lane & 7) + ((lane & 7) >= 4), di = slot / 3 - 1, dj = slot % 3 - 1;     // (the centre, slot 4, is skipped)
  const bool inside = lane < 8 && (unsigned)(i + di) < (unsigned)W && (unsigned)(j + dj) < (unsigned)H;
  const bool diag = di != 0 && dj != 0;
  const uint32_t v = fld[inside ? c + di * H + dj : c];
  const uint32_t side_i = fld[inside && diag ? c + di * H : c], side_j = fld[inside && diag ? c + dj : c];
  const bool ok = inside && v != INF && !(diag && (side_i == INF || side_j == INF)) && v < fc &&
                  fc - v == (diag ? DIAGONAL : AXIAL) + kcur;
  const uint64_t mask = __ballot(ok);
  if (mask == 0) return -1;
  const int w = __builtin_ctzll(mask), ws = w + (w >= 4);
  fnext = uni(__shfl(v, w, WAVE));
  return c + (ws / 3 - 1) * H + (ws % 3 - 1);
}

// los() / soft_los() between a and b by the closed form; `sum`: k over the segment's cells, both ends included (0 without a cost
// layer; meaningless where the sight breaks)
__device__ __forceinline__ bool wave_sight(const uint32_t* __restrict__ fld, const uint8_t* __restrict__ kc, int H, int a, int b, int lane,
                                           uint32_t& sum) {
  if (b < a) { const int t = a; a = b; b = t; }
  const int ai = a / H, aj = a - ai * H, bi = b / H, bj = b - bi * H;
  const int di = bi - ai, dj = bj - aj;
  const int m = max(abs(di), abs(dj));
  sum = 0;
  if (m == 0) { sum = wave_k(kc, a); return uni(fld[a]) != INF; }
  const uint32_t two_m = 2u * (uint32_t)m, ui = 2u * (uint32_t)di, uj = 2u * (uint32_t)(dj + m);
  uint32_t part = 0;
  for (int base = 0; base <= m; base += WAVE) {
    const uint32_t k = (uint32_t)(base + lane);
    const bool in = k <= (uint32_t)m;
    const int qi = (int)((k * ui + (uint32_t)m) / two_m), qj = (int)((k * uj + (uint32_t)m) / two_m) - (int)k;
    const int c = in ? (ai + qi) * H + aj + qj : a;
    const uint32_t v = fld[c];
    if (kc) part += in ? soft_k(kc, c) : 0u;
    if (__ballot(in && v == INF) != 0) return false;
  }
  if (kc) {
    for (int off = WAVE / 2; off > 0; off >>= 1) part += __shfl_xor(part, off, WAVE);
    sum = uni(part);
  }
  return true;
}

// walk() (terminal: the word is 0), soft_walk() (the same, with a cost layer) and walk_to() (terminal: a source that holds its
// own seed), rule for rule.  terminal(cell, its word) and emit(cell, row) are called with uniform arguments.  `sight`: another
// field whose INF words judge the line of sight (the claims from per-robot fields: passability); null: fld itself.
template <typename Terminal, typename Emit>
__device__ __forceinline__ int wave_walk(const uint32_t* __restrict__ fld, const uint8_t* __restrict__ kc, int W, int H, int s, int max_seg,
                                         int lane, int& last_cell, Terminal terminal, Emit emit, const uint32_t* sight = nullptr) {
  const uint32_t* seen = sight ? sight : fld;
  int count = 0;
  last_cell = s;
  const uint32_t fs = uni(fld[s]);
  if (!terminal(s, fs)) {
    int a = s, prev = s;
    uint32_t fa = fs, fprev = fs, kprev = wave_k(kc, s), pen = kprev, fcur = 0;
    int cur = wave_descend(fld, W, H, s, fs, kprev, lane, fcur);
    while (cur >= 0) {
      const bool last = terminal(cur, fcur);
      const uint32_t kcur = wave_k(kc, cur);
      uint32_t seg = 0;
      const bool clear = wave_sight(seen, kc, H, a, cur, lane, seg);
      if (!clear || seg - kcur > pen || (fa - fcur) - pen >= (uint32_t)max_seg) {
        if (prev != a) { emit(prev, count); ++count; a = prev; fa = fprev; pen = kprev; continue; }   // cur is looked at again from the new anchor
        if (last) break;
        emit(cur, count); ++count; a = cur; fa = fcur; pen = 0;
      }
      if (last) break;
      prev = cur; fprev = fcur; kprev = kcur;
      pen += kcur;
      cur = wave_descend(fld, W, H, cur, fcur, kcur, lane, fcur);
    }
    if (cur < 0) return -1;
    last_cell = cur;
  }
  return count + 1;
}

// count, then write: the sub-goals of the walk from s but the last one's row (the caller's), or what to report instead
template <typename Terminal>
__device__ __forceinline__ int wave_paths(const uint32_t* __restrict__ fld, const uint8_t* __restrict__ kc, int W, int H, int s, int max_seg,
                                          int S_max, double ox, double oy, double dx, double dy, double* sg, int lane, int& last_cell,
                                          Terminal terminal) {
  const int n = wave_walk(fld, kc, W, H, s, max_seg, lane, last_cell, terminal, [](int, int) {});
  if (n < 0 || n > S_max) return n;
  wave_walk(fld, kc, W, H, s, max_seg, lane, last_cell, terminal, [&](int c, int row) {
    if (lane == 0) centre(c, H, ox, oy, dx, dy, sg + 2 * row);
  });
  return n;
}

// the robot of this wave, or -1 (the whole wave leaves)
__device__ __forceinline__ int64_t wave_robot(int64_t B) {
  const int64_t b = (int64_t)blockIdx.x * WAVEWALK_ROBOTS + uni((int)(threadIdx.x / WAVE));
  return b < B ? b : -1;
}

// grid_path_body's rules in its order, a wave per robot.  `settled` null: the one-workgroup field's call; `cost` null: unweighted.
__global__ void __launch_bounds__(WAVEWALK_THREADS) wavewalk_goal_kernel(
    int64_t B, int one_field, int W, int H, int64_t occ_stride, double ox, double oy, double dx, double dy, const uint8_t* __restrict__ occ,
    const uint8_t* __restrict__ cost, const uint32_t* __restrict__ field, const int32_t* __restrict__ field_status,
    const int32_t* __restrict__ settled, const double* __restrict__ goal, const double* __restrict__ start, int r_inflate, int max_seg,
    int S_max, double* __restrict__ sub_goals, int32_t* __restrict__ n_sub, int32_t* __restrict__ status, double* __restrict__ path_cost) {
  const int64_t b = wave_robot(B);
  if (b < 0) return;
  const int lane = threadIdx.x % WAVE;
  const int64_t f = one_field ? 0 : b;
  const int ncells = W * H;
  const uint32_t* fld = field + f * (int64_t)ncells;
  const uint8_t* kc = cost ? cost + f * occ_stride : nullptr;          // (the layer is shared exactly when the map is)
  auto done = [&](int st_, int n, double c) {
    if (lane == 0) { status[b] = st_; n_sub[b] = n; path_cost[b] = c; }
  };
  const double nan = __builtin_nan("");
  if (settled && uni(settled[f]) == 0) return done(LIPMPC_RRT_FIELD_UNSETTLED, 0, nan);
  const int fs = uni(field_status[f]);
  if (fs == LIPMPC_FIELD_GOAL_OUTSIDE) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan);
  if (fs == LIPMPC_FIELD_GOAL_BLOCKED) return done(LIPMPC_RRT_GOAL_OCCUPIED, 0, nan);
  int si = 0, sj = 0;
  if (!uni((int)cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj))) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan);
  si = uni(si); sj = uni(sj);
  int s = si * H + sj;
  if (uni((int)occ[f * occ_stride + s]) != 0) return done(LIPMPC_RRT_START_OCCUPIED, 0, nan);
  if (uni(fld[s]) == INF) s = wave_snap(fld, W, H, si, sj, r_inflate, lane);
  if (s < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan);
  double* sg = sub_goals + b * (int64_t)S_max * 2;
  int last_cell;
  const int n = wave_paths(fld, kc, W, H, s, max_seg, S_max, ox, oy, dx, dy, sg, lane, last_cell,
                           [](int, uint32_t word) { return word == 0; });
  if (n < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan);                  // (a `field` that is no cost-to-go field of this map and layer)
  const double total = (double)fld[s] / 5.0;                           // penalties included
  if (n > S_max) return done(LIPMPC_RRT_PATH_OVERFLOW, 0, total);
  if (lane == 0) {
    sg[2 * (n - 1)] = goal[2 * f];                                     // the goal itself, not its cell's centre
    sg[2 * (n - 1) + 1] = goal[2 * f + 1];
  }
  done(LIPMPC_RRT_FOUND, n, total);
}

// frontier_path_body's rules in its order, a wave per robot; `settled` and `cost` as above (a layer per field)
__global__ void __launch_bounds__(WAVEWALK_THREADS) wavewalk_frontier_kernel(
    int64_t B, int one_field, int W, int H, double ox, double oy, double dx, double dy, const int32_t* __restrict__ evidence,
    const uint8_t* __restrict__ cost, int t_occ, const uint32_t* __restrict__ field, const int32_t* __restrict__ n_frontier,
    const int32_t* __restrict__ settled, const double* __restrict__ start, int r_inflate, int max_seg, int S_max,
    double* __restrict__ sub_goals, int32_t* __restrict__ n_sub, int32_t* __restrict__ status, double* __restrict__ path_cost,
    int32_t* __restrict__ target_cell) {
  const int64_t b = wave_robot(B);
  if (b < 0) return;
  const int lane = threadIdx.x % WAVE;
  const int64_t f = one_field ? 0 : b;
  const int ncells = W * H;
  const uint32_t* fld = field + f * (int64_t)ncells;
  const uint8_t* kc = cost ? cost + f * (int64_t)ncells : nullptr;
  auto done = [&](int st_, int n, double c, int target) {
    if (lane == 0) { status[b] = st_; n_sub[b] = n; path_cost[b] = c; target_cell[b] = target; }
  };
  const double nan = __builtin_nan("");
  if (settled && uni(settled[f]) == 0) return done(LIPMPC_RRT_FIELD_UNSETTLED, 0, nan, -1);
  int si = 0, sj = 0;
  if (!uni((int)cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj))) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan, -1);
  si = uni(si); sj = uni(sj);
  int s = si * H + sj;
  if (uni(evidence[f * (int64_t)ncells + s]) >= t_occ) return done(LIPMPC_RRT_START_OCCUPIED, 0, nan, -1);
  if (uni(n_frontier[f]) == 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);
  if (uni(fld[s]) == INF) s = wave_snap(fld, W, H, si, sj, r_inflate, lane);
  if (s < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);
  double* sg = sub_goals + b * (int64_t)S_max * 2;
  int last_cell;
  const int n = wave_paths(fld, kc, W, H, s, max_seg, S_max, ox, oy, dx, dy, sg, lane, last_cell,
                           [](int, uint32_t word) { return word == 0; });
  if (n < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);              // (a `field` that is no frontier field of this map and layer)
  const double total = (double)fld[s] / 5.0;                           // penalties included
  if (n > S_max) return done(LIPMPC_RRT_PATH_OVERFLOW, 0, total, last_cell);
  if (lane == 0) centre(last_cell, H, ox, oy, dx, dy, sg + 2 * (n - 1));
  done(LIPMPC_RRT_FOUND, n, total, last_cell);
}

// frontier_utility_path_kernel's rules (tile_utility_descent_kernel's with `settled`) in their order, a wave per robot
__global__ void __launch_bounds__(WAVEWALK_THREADS) wavewalk_utility_kernel(
    int64_t B, int one_field, int W, int H, double ox, double oy, double dx, double dy, const int32_t* __restrict__ evidence, int t_occ,
    const uint8_t* __restrict__ frontier, const int32_t* __restrict__ gain, const uint32_t* __restrict__ ufield,
    const int32_t* __restrict__ n_sources, const int32_t* __restrict__ settled, int w_gain, int g_cap, int min_gain,
    const double* __restrict__ start, int r_inflate, int max_seg, int S_max, double* __restrict__ sub_goals, int32_t* __restrict__ n_sub,
    int32_t* __restrict__ status, double* __restrict__ path_cost, int32_t* __restrict__ target_cell, int32_t* __restrict__ target_gain) {
  const int64_t b = wave_robot(B);
  if (b < 0) return;
  const int lane = threadIdx.x % WAVE;
  const int64_t f = one_field ? 0 : b;
  const int ncells = W * H;
  const uint32_t* fld = ufield + f * (int64_t)ncells;
  const uint8_t* fr = frontier + f * (int64_t)ncells;
  const int32_t* gn = gain + f * (int64_t)ncells;
  auto done = [&](int st_, int n, double cost, int target) {
    if (lane == 0) {
      status[b] = st_; n_sub[b] = n; path_cost[b] = cost; target_cell[b] = target; target_gain[b] = target >= 0 ? gn[target] : -1;
    }
  };
  // (a source is passable: its field is finite, which the comparison with a seed says too)
  auto terminal = [&](int c, uint32_t word) {
    if (uni((int)fr[c]) == 0) return false;
    const int g = uni(gn[c]);
    return g >= min_gain && word == gain_seed(g, w_gain, g_cap);
  };
  const double nan = __builtin_nan("");
  if (settled && uni(settled[f]) == 0) return done(LIPMPC_RRT_FIELD_UNSETTLED, 0, nan, -1);
  int si = 0, sj = 0;
  if (!uni((int)cell_of(start[2 * b], start[2 * b + 1], ox, oy, dx, dy, W, H, si, sj))) return done(LIPMPC_RRT_OUTSIDE_GRID, 0, nan, -1);
  si = uni(si); sj = uni(sj);
  int s = si * H + sj;
  if (uni(evidence[f * (int64_t)ncells + s]) >= t_occ) return done(LIPMPC_RRT_START_OCCUPIED, 0, nan, -1);
  if (uni(n_sources[f]) == 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);
  if (uni(fld[s]) == INF) s = wave_snap(fld, W, H, si, sj, r_inflate, lane);
  if (s < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);
  double* sg = sub_goals + b * (int64_t)S_max * 2;
  int last_cell;
  const int n = wave_paths(fld, nullptr, W, H, s, max_seg, S_max, ox, oy, dx, dy, sg, lane, last_cell, terminal);
  if (n < 0) return done(LIPMPC_RRT_NO_PATH, 0, nan, -1);              // (a `ufield` that is no utility field of this map)
  const double cost = (double)(fld[s] - fld[last_cell]) / 5.0;
  if (n > S_max) return done(LIPMPC_RRT_PATH_OVERFLOW, 0, cost, last_cell);
  if (lane == 0) centre(last_cell, H, ox, oy, dx, dy, sg + 2 * (n - 1));
  done(LIPMPC_RRT_FOUND, n, cost, last_cell);
}

inline dim3 wave_grid(int64_t B) { return dim3((unsigned)((B + WAVEWALK_ROBOTS - 1) / WAVEWALK_ROBOTS)); }

}  // namespace

extern "C" int lipmpc_grid_path_wave_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin, const double* cell,
                                           const uint8_t* occ, int32_t grid_shared, const uint8_t* cost, const uint32_t* field,
                                           const int32_t* field_status, const int32_t* settled, const double* goal, const double* start,
                                           int32_t r_inflate, int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub,
                                           int32_t* status, double* path_cost, void* hip_stream) {
  if (cost && !settled) return LIPMPC_E_ARG;                           // (a weighted field has the word)
  if (const int rc = tiled_path_refusal(B, F, W, H, origin, cell, r_inflate, max_seg, S_max)) return rc;
  if (B == 0) return LIPMPC_OK;
  // LATE, as in the three wave calls: B == 0 passes with any of them null (`settled` may be null, without `cost`)
  if (any_null(occ, field, field_status, goal, start, sub_goals, n_sub, status, path_cost)) return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(wavewalk_goal_kernel, wave_grid(B), dim3(WAVEWALK_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H,
                     grid_shared ? (int64_t)0 : (int64_t)W * H, origin[0], origin[1], cell[0], cell[1], occ, cost, field, field_status,
                     settled, goal, start, r_inflate, max_seg, S_max, sub_goals, n_sub, status, path_cost);
  return launched();
}

extern "C" int lipmpc_grid_frontier_path_wave_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                                    const double* cell, const int32_t* evidence, const uint8_t* cost, int32_t t_occ,
                                                    const uint32_t* field, const int32_t* n_frontier, const int32_t* settled,
                                                    const double* start, int32_t r_inflate, int32_t max_seg, int32_t S_max,
                                                    double* sub_goals, int32_t* n_sub, int32_t* status, double* path_cost,
                                                    int32_t* target_cell, void* hip_stream) {
  if ((cost && !settled) || bad_threshold(t_occ)) return LIPMPC_E_ARG;
  if (const int rc = tiled_path_refusal(B, F, W, H, origin, cell, r_inflate, max_seg, S_max)) return rc;
  if (B == 0) return LIPMPC_OK;
  if (any_null(evidence, field, n_frontier, start, sub_goals, n_sub, status, path_cost, target_cell)) return LIPMPC_E_ARG;       // LATE
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(wavewalk_frontier_kernel, wave_grid(B), dim3(WAVEWALK_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H,
                     origin[0], origin[1], cell[0], cell[1], evidence, cost, t_occ, field, n_frontier, settled, start, r_inflate, max_seg,
                     S_max, sub_goals, n_sub, status, path_cost, target_cell);
  return launched();
}

extern "C" int lipmpc_grid_frontier_utility_path_wave_batch(int device, int64_t B, int64_t F, int32_t W, int32_t H, const double* origin,
                                                            const double* cell, const int32_t* evidence, int32_t t_occ,
                                                            const uint8_t* frontier, const int32_t* gain, const uint32_t* ufield,
                                                            const int32_t* n_sources, const int32_t* settled, int32_t w_gain,
                                                            int32_t g_cap, int32_t min_gain, const double* start, int32_t r_inflate,
                                                            int32_t max_seg, int32_t S_max, double* sub_goals, int32_t* n_sub,
                                                            int32_t* status, double* path_cost, int32_t* target_cell,
                                                            int32_t* target_gain, void* hip_stream) {
  if (bad_threshold(t_occ) || bad_gain(w_gain, g_cap, min_gain)) return LIPMPC_E_ARG;
  if (const int rc = tiled_path_refusal(B, F, W, H, origin, cell, r_inflate, max_seg, S_max)) return rc;
  if (B == 0) return LIPMPC_OK;
  // LATE, unlike lipmpc_grid_frontier_utility_path_batch and its tiled form (`settled` may be null)
  if (any_null(evidence, frontier, gain, ufield, n_sources, start, sub_goals, n_sub, status, path_cost, target_cell, target_gain))
    return LIPMPC_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return LIPMPC_E_HIP;
  hipLaunchKernelGGL(wavewalk_utility_kernel, wave_grid(B), dim3(WAVEWALK_THREADS), 0, (hipStream_t)hip_stream, B, (int)(F == 1), W, H,
                     origin[0], origin[1], cell[0], cell[1], evidence, t_occ, frontier, gain, ufield, n_sources, settled, w_gain, g_cap,
                     min_gain, start, r_inflate, max_seg, S_max, sub_goals, n_sub, status, path_cost, target_cell, target_gain);
  return launched();
}
