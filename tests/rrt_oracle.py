"""numpy restatement of the on-device RRT* sub-goal planner (csrc/lipmpc_rrt.hip, lipmpc_rrt_plan_batch).

The global planner of the reference's HumanoidMPCWithRRT (HumanoidMPCVariants/HumanoidMPCWithRRT.py:21-135) in four
steps: occupancy grid (:21-90), Euclidean distance transform and clearance cost exp(-d) (:107-112), RRT* with the cost
vcost[v] + C[x] |p_v - x| (:116-128), tree path -> world sub-goals (:129-135).  ``rrtplanner``'s random stream is not
reproducible, so the sampler and every tie of the tree are defined here (and in include/lipmpc.h) instead.

Used by the tests only.  Every compared quantity is an integer or a float64 sum / product / sqrt of exact inputs, so once
the cost grid C is fixed the tree is reproducible bit for bit: ``plan(..., C=...)`` takes the device's C.
"""
import math

import numpy as np

FOUND, NO_PATH, START_OCCUPIED, GOAL_OCCUPIED, GRID_TOO_LARGE, NO_OBSTACLE_GRID, PATH_OVERFLOW = range(7)
STATUS_NAMES = ("FOUND", "NO_PATH", "START_OCCUPIED", "GOAL_OCCUPIED", "GRID_TOO_LARGE", "NO_OBSTACLE_GRID",
                "PATH_OVERFLOW")

WIDTH, N_SAMPLES, R_REWIRE, MARGIN = 250, 1500, 80, 3.0
MAX_CELLS = 1 << 17          # lipmpc_rrt_default_params: the bitmap of the largest grid stays within 16 KiB of LDS
_GOLDEN = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


# -- grid ------------------------------------------------------------------------------------------------------------
def transform(rings, goal, start=(0.0, 0.0), width=WIDTH, margin=MARGIN):
    """Bounds and dims (HumanoidMPCWithRRT.py:32-52, the reference's origin replaced by ``start``)."""
    xs = [float(start[0]), float(goal[0])] + [float(v) for r in rings for v in np.asarray(r, float)[:, 0]]
    ys = [float(start[1]), float(goal[1])] + [float(v) for r in rings for v in np.asarray(r, float)[:, 1]]
    min_x, max_x = min(xs) - margin, max(xs) + margin
    min_y, max_y = min(ys) - margin, max(ys) + margin
    H = math.ceil(width * ((max_y - min_y) / (max_x - min_x)))
    return dict(min_x=min_x, max_x=max_x, min_y=min_y, max_y=max_y, W=int(width), H=int(H))


def to_cell(tf, x, y):
    """world -> cell, np.round (half to even) of ((x - min_x) / (max_x - min_x)) * W, as :57-60."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    i = np.rint(((x - tf["min_x"]) / (tf["max_x"] - tf["min_x"])) * tf["W"])
    j = np.rint(((y - tf["min_y"]) / (tf["max_y"] - tf["min_y"])) * tf["H"])
    return i.astype(np.int64), j.astype(np.int64)


def to_world(tf, i, j):
    """cell -> world, :62-65."""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    x = tf["min_x"] + ((i * (tf["max_x"] - tf["min_x"])) / tf["W"])
    y = tf["min_y"] + ((j * (tf["max_y"] - tf["min_y"])) / tf["H"])
    return x, y


def int_hull(pts):
    """Andrew's monotone chain on integer points: CCW hull without collinear points (1 point if all coincide, 2 if they
    are collinear)."""
    P = sorted(set((int(p[0]), int(p[1])) for p in pts))
    if len(P) <= 2:
        return P
    cr = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lo, up = [], []
    for p in P:
        while len(lo) >= 2 and cr(lo[-2], lo[-1], p) <= 0:
            lo.pop()
        lo.append(p)
    for p in reversed(P):
        while len(up) >= 2 and cr(up[-2], up[-1], p) <= 0:
            up.pop()
        up.append(p)
    h = lo[:-1] + up[:-1]
    return h if len(h) >= 1 else P[:1]


def occupancy(rings, tf):
    """Cell (i, j) of the (W+1) x (H+1) grid is occupied if, for some obstacle, xmin <= i < xmax and ymin <= j < ymax over
    its ROUNDED vertices (the half-open range() of :80-81) and (i, j) lies in the closed convex hull of those rounded
    vertices (exact integer orientation tests: what Delaunay(...).find_simplex >= 0 decides on integer points)."""
    W, H = tf["W"], tf["H"]
    og = np.zeros((W + 1, H + 1), bool)
    for r in rings:
        r = np.asarray(r, float)
        if len(r) == 0:
            continue
        vi, vj = to_cell(tf, r[:, 0], r[:, 1])
        x0, x1, y0, y1 = vi.min(), vi.max(), vj.min(), vj.max()
        if x1 <= x0 or y1 <= y0:
            continue
        I, J = np.meshgrid(np.arange(x0, x1), np.arange(y0, y1), indexing="ij")
        inside = np.ones(I.shape, bool)
        h = int_hull(np.stack([vi, vj], 1))
        for k in range(len(h)):
            a, b = h[k], h[(k + 1) % len(h)]
            inside &= (b[0] - a[0]) * (J - a[1]) - (b[1] - a[1]) * (I - a[0]) >= 0
        og[I[inside], J[inside]] = True
    return og


def edt_d2(og):
    """Exact squared Euclidean distance (integers) of every cell to the nearest occupied cell, 0 on occupied cells:
    the square of scipy.ndimage.distance_transform_edt(1 - og).  None if no cell is occupied."""
    if not og.any():
        return None
    Wp, Hp = og.shape
    big = Wp + Hp + 2
    # 1-D pass along y per column x
    g = np.full(og.shape, big, np.int64)
    run = np.full(Wp, big, np.int64)
    for j in range(Hp):
        run = np.where(og[:, j], 0, np.minimum(run + 1, big))
        g[:, j] = run
    run = np.full(Wp, big, np.int64)
    for j in range(Hp - 1, -1, -1):
        run = np.where(og[:, j], 0, np.minimum(run + 1, big))
        g[:, j] = np.minimum(g[:, j], run)
    # 2-D: min over the columns x' of (x - x')^2 + g[x', y]^2 (brute force over x')
    g2 = g * g
    xs = np.arange(Wp, dtype=np.int64)
    d2 = np.empty(og.shape, np.int64)
    for x in range(Wp):
        d2[x] = np.min(((x - xs) ** 2)[:, None] + g2, axis=0)
    return d2


def cost_grid(d2):
    return np.exp(-np.sqrt(d2.astype(np.float64)))


# -- sampler ---------------------------------------------------------------------------------------------------------
def splitmix_draws(seed, k0, k1):
    """z_k = splitmix64 finaliser of (seed + (k+1) * 0x9E3779B97F4A7C15 mod 2^64), k = k0 .. k1-1."""
    with np.errstate(over="ignore"):
        k = np.arange(k0 + 1, k1 + 1, dtype=np.uint64)
        z = np.uint64(int(seed) & _M64) + k * np.uint64(_GOLDEN)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def draw_cells(seed, k0, k1, ncells):
    z = splitmix_draws(seed, k0, k1)
    return (((z >> np.uint64(32)) * np.uint64(ncells)) >> np.uint64(32)).astype(np.int64)


# -- RRT* ------------------------------------------------------------------------------------------------------------
def segment_cells(a, b):
    """Cells of the segment between two cells: endpoints ordered lexicographically (a < b), m = max(|dx|, |dy|),
    cell k = a + floor((2 k d + m) / (2 m)) per coordinate, k = 0..m."""
    a, b = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    if b < a:
        a, b = b, a
    dx, dy = b[0] - a[0], b[1] - a[1]
    m = max(abs(dx), abs(dy))
    if m == 0:
        return np.array([a[0]]), np.array([a[1]])
    k = np.arange(m + 1, dtype=np.int64)
    return a[0] + (2 * k * dx + m) // (2 * m), a[1] + (2 * k * dy + m) // (2 * m)


def segment_free(og, a, b):
    cx, cy = segment_cells(a, b)
    return not og[cx, cy].any()


def plan(rings, goal, start=None, seed=1, width=WIDTH, n=N_SAMPLES, r_rewire=R_REWIRE, margin=MARGIN,
         max_cells=MAX_CELLS, S_max=None, C=None):
    """One plan by the contract of lipmpc_rrt_plan_batch.  ``C``: the cost grid to plan on (default exp(-sqrt(d2)) in
    numpy).  Returns dict(status, sub_goals [n_sub,2], n_sub, path_cost, tf, og, d2, C, cells [V,2], parent [V],
    cost [V], goal_parent, draws, samples: the valid draws among them, 0 on the early statuses)."""
    start = (0.0, 0.0) if start is None else (float(start[0]), float(start[1]))
    rings = [np.asarray(r, float) for r in rings if len(r)]
    tf = transform(rings, goal, start, width, margin)
    W, H = tf["W"], tf["H"]
    out = dict(status=None, sub_goals=np.zeros((0, 2)), n_sub=0, path_cost=float("nan"), tf=tf, og=None, d2=None, C=None,
               cells=np.zeros((0, 2), np.int64), parent=np.zeros(0, np.int64), cost=np.zeros(0), goal_parent=-1, draws=0,
               samples=0)
    ncells = (W + 1) * (H + 1)
    if ncells > max_cells or H + 1 > 4096:
        out["status"] = GRID_TOO_LARGE
        return out
    og = occupancy(rings, tf)
    d2 = edt_d2(og)
    out.update(og=og, d2=d2)
    if d2 is None:
        out["status"] = NO_OBSTACLE_GRID
        return out
    C = cost_grid(d2) if C is None else np.asarray(C, np.float64).reshape(W + 1, H + 1)
    out["C"] = C
    si, sj = (int(v) for v in to_cell(tf, start[0], start[1]))
    gi, gj = (int(v) for v in to_cell(tf, goal[0], goal[1]))
    if og[si, sj]:
        out["status"] = START_OCCUPIED
        return out
    if og[gi, gj]:
        out["status"] = GOAL_OCCUPIED
        return out
    r2 = int(r_rewire) * int(r_rewire)
    cap = 64 * int(n)
    s_cell, g_cell = si * (H + 1) + sj, gi * (H + 1) + gj
    ogf = og.reshape(-1)
    cells = np.zeros((n + 1, 2), np.int64)
    parent = np.full(n + 1, -1, np.int64)
    cost = np.zeros(n + 1)
    cells[0] = (si, sj)
    nv, samples, k, pool, pool_k = 1, 0, 0, np.zeros(0, np.int64), 0
    while samples < n and k < cap:
        if k - pool_k >= len(pool):
            pool_k, pool = k, draw_cells(seed, k, min(cap, k + 4096), ncells)
        c = int(pool[k - pool_k])
        k += 1
        if ogf[c] or c == s_cell or c == g_cell:
            continue
        samples += 1
        x = (c // (H + 1), c % (H + 1))
        P = cells[:nv]
        dd = (P[:, 0] - x[0]) ** 2 + (P[:, 1] - x[1]) ** 2
        vn = int(np.argmin(dd))                       # first index of the minimum
        if dd[vn] == 0 or not segment_free(og, P[vn], x):
            continue
        near = dd <= r2
        near[vn] = True
        idx = np.nonzero(near)[0]
        Cx = C[x[0], x[1]]
        cand = cost[idx] + Cx * np.sqrt(dd[idx].astype(np.float64))
        best_v, best_c = -1, None
        for t in np.lexsort((idx, cand)):             # by cost, then index
            v = int(idx[t])
            if segment_free(og, P[v], x):
                best_v, best_c = v, float(cand[t])
                break
        xv = nv
        cells[xv] = x
        parent[xv] = best_v
        cost[xv] = best_c
        nv += 1
        # rewire against the costs as they were before this sample
        rew = []
        for u in idx:
            u = int(u)
            if u == best_v:
                continue
            nc = best_c + C[P[u][0], P[u][1]] * math.sqrt(float(dd[u]))
            if nc < cost[u] and segment_free(og, P[u], x):
                rew.append(u)
        if rew:
            parent[rew] = xv
            front = np.zeros(nv, bool)
            front[xv] = True
            while True:
                ch = np.nonzero(front[np.maximum(parent[:nv], 0)] & (parent[:nv] >= 0))[0]
                if len(ch) == 0:
                    break
                p = parent[ch]
                e2 = (cells[ch, 0] - cells[p, 0]) ** 2 + (cells[ch, 1] - cells[p, 1]) ** 2
                cost[ch] = cost[p] + C[cells[ch, 0], cells[ch, 1]] * np.sqrt(e2.astype(np.float64))
                front[:] = False
                front[ch] = True
    out.update(cells=cells[:nv].copy(), parent=parent[:nv].copy(), cost=cost[:nv].copy(), draws=k, samples=samples)
    # goal
    P = cells[:nv]
    dd = (P[:, 0] - gi) ** 2 + (P[:, 1] - gj) ** 2
    idx = np.nonzero(dd <= r2)[0]
    Cg = C[gi, gj]
    cand = cost[idx] + Cg * np.sqrt(dd[idx].astype(np.float64))
    gp, gc = -1, float("nan")
    for t in np.lexsort((idx, cand)):
        v = int(idx[t])
        if segment_free(og, P[v], (gi, gj)):
            gp, gc = v, float(cand[t])
            break
    out["goal_parent"] = gp
    if gp < 0:
        out["status"] = NO_PATH
        return out
    chain = [(gi, gj)]
    v = gp
    while v > 0:
        chain.append(tuple(cells[v]))
        v = int(parent[v])
    chain = np.array(chain[::-1], np.int64)
    out["path_cost"] = gc
    if S_max is not None and len(chain) > S_max:
        out["status"] = PATH_OVERFLOW
        return out
    x, y = to_world(tf, chain[:, 0], chain[:, 1])
    out.update(status=FOUND, sub_goals=np.stack([x, y], 1), n_sub=len(chain), chain=chain)
    return out


def check_tree(res):
    """The invariants of a finished tree: cost(v) == cost(parent) + C[v] |p_v - p_parent| exactly, every edge free,
    every path segment free.  Returns a list of violations (empty = ok)."""
    bad = []
    cells, parent, cost, og, C = res["cells"], res["parent"], res["cost"], res["og"], res["C"]
    for v in range(1, len(cells)):
        p = int(parent[v])
        d2 = int(((cells[v] - cells[p]) ** 2).sum())
        if cost[v] != cost[p] + C[cells[v][0], cells[v][1]] * math.sqrt(float(d2)):
            bad.append(("cost", v))
        if not segment_free(og, cells[p], cells[v]):
            bad.append(("edge", v))
    if res["status"] == FOUND:
        pts = [tuple(cells[0])] + [tuple(c) for c in res["chain"]]
        for a, b in zip(pts[:-1], pts[1:]):
            if not segment_free(og, a, b):
                bad.append(("path", a, b))
    return bad
