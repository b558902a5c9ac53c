"""Numpy / plain-Python restatement of the grid field planner's two contracts -- lipmpc_grid_field_batch and
lipmpc_grid_path_batch, include/lipmpc.h: the cost-to-go field by Dijkstra (heapq, Python ints), the snap, the descent, the
line of sight and the string pulling exactly as the header states them.

TEST INFRASTRUCTURE ONLY, like tests/map_oracle.py: the GPU tests require the device's field, statuses, sub-goals and path costs
to equal this module's bit for bit.
"""
from __future__ import annotations

import heapq
import math

import numpy as np

INF = 0xFFFFFFFF
AXIAL, DIAGONAL = 5, 7
R_INFLATE_MAX = 16
NO_CAP = 0x7FFFFFFF                                           # max_seg = "no spacing cap": no field value reaches it
FIELD_OK, FIELD_GOAL_OUTSIDE, FIELD_GOAL_BLOCKED = 0, 1, 2
FOUND, NO_PATH, START_OCCUPIED, GOAL_OCCUPIED, PATH_OVERFLOW, OUTSIDE_GRID = 0, 1, 2, 3, 6, 7      # the LIPMPC_RRT_* codes in use
MOVES = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))                      # the descent's order
LDS_LIMIT, LDS_SLACK = 160 * 1024, 256
MAX_SIDE, MAX_CELLS = 4096, 1 << 17                           # the caps of every grid call


def bitmap_words(ncells):
    """32-bit words of a bitmap of ncells cells: whole 64-cell ballots, + 2 for a window that starts in the last word."""
    return ((ncells + 63) // 64) * 2 + 2


def field_lds_bytes(ncells):
    """Dynamic LDS the field kernel asks for with the field in LDS: the blocked bitmap, then the field (the solid bitmap borrows
    the field's first words)."""
    return 4 * (bitmap_words(ncells) + ncells)


def field_fits_lds(ncells):
    """THE FIELD KERNEL'S LDS RULE (its own, not the frontier kernel's): the field, 4 bytes a cell, beside the blocked bitmap and
    the workgroup reduction's slack within the 160 KiB of a workgroup."""
    return field_lds_bytes(ncells) + LDS_SLACK <= LDS_LIMIT


def shapes_of(ncells):
    """Every (W, H) of exactly ncells cells that the grid calls accept: both sides in 2..4096."""
    return [(w, ncells // w) for w in range(2, MAX_SIDE + 1) if ncells % w == 0 and 2 <= ncells // w <= MAX_SIDE]


def lds_boundary(fits):
    """(the largest cell count that ``fits`` and its shapes, the first count above it that has a shape at all and its shapes)."""
    n = 4
    while fits(n + 1):
        n += 1
    over = n + 1
    while not shapes_of(over):
        over += 1
    assert fits(n) and not fits(over) and over <= MAX_CELLS
    return (n, shapes_of(n)), (over, shapes_of(over))


def blocked_cells(occ, r_inflate):
    """blocked [W,H]: some solid cell of the grid within (i - i')^2 + (j - j')^2 <= r_inflate^2."""
    solid = np.asarray(occ) != 0
    W, H = solid.shape
    r = int(r_inflate)
    out = np.zeros((W, H), bool)
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            if di * di + dj * dj > r * r:
                continue
            i0, i1, j0, j1 = max(0, di), min(W, W + di), max(0, dj), min(H, H + dj)      # the targets (i' + di, j' + dj) inside the grid
            if i0 < i1 and j0 < j1:
                out[i0:i1, j0:j1] |= solid[i0 - di:i1 - di, j0 - dj:j1 - dj]
    return out


def cell_of(p, origin, cell, W, H):
    """The floor rule (the grid scan's robot cell): (i, j), or None when the cell is outside the grid (NaN included)."""
    with np.errstate(all="ignore"):
        fi = np.floor((np.float64(p[0]) - np.float64(origin[0])) / np.float64(cell[0]))
        fj = np.floor((np.float64(p[1]) - np.float64(origin[1])) / np.float64(cell[1]))
    if not (0 <= fi < W and 0 <= fj < H):
        return None
    return int(fi), int(fj)


def centre(c, origin, cell):
    """ox + (i + 0.5) * dx, as written, in double."""
    return np.array([np.float64(origin[0]) + (np.float64(c[0]) + 0.5) * np.float64(cell[0]),
                     np.float64(origin[1]) + (np.float64(c[1]) + 0.5) * np.float64(cell[1])])


def moves_from(blocked, i, j):
    """The (i', j', cost) an unblocked cell (i, j) may step to: 8-connected, a diagonal only past two unblocked side cells."""
    W, H = blocked.shape
    for di, dj in MOVES:
        a, b = i + di, j + dj
        if not (0 <= a < W and 0 <= b < H) or blocked[a, b]:
            continue
        if di and dj and (blocked[a, j] or blocked[i, b]):
            continue
        yield a, b, DIAGONAL if di and dj else AXIAL


def field(occ, origin, cell, goal, r_inflate=0):
    """(field [W,H] uint32, field_status) of one goal."""
    blocked = blocked_cells(occ, r_inflate)
    W, H = blocked.shape
    out = np.full((W, H), INF, np.uint32)
    g = cell_of(goal, origin, cell, W, H)
    if g is None:
        return out, FIELD_GOAL_OUTSIDE
    if blocked[g]:
        return out, FIELD_GOAL_BLOCKED
    dist = {g: 0}
    heap = [(0, g[0], g[1])]
    while heap:
        d, i, j = heapq.heappop(heap)
        if d > dist[(i, j)]:
            continue
        for a, b, c in moves_from(blocked, i, j):              # (the move rules are symmetric: to the goal = from the goal)
            if d + c < dist.get((a, b), 1 << 62):
                dist[(a, b)] = d + c
                heapq.heappush(heap, (d + c, a, b))
    for (i, j), d in dist.items():
        out[i, j] = d
    return out, FIELD_OK


def los(fld, a, b):
    """The planner's segment rule on passable cells: endpoints in lexicographic order, m = max(|di|, |dj|), cells
    a + floor((2 k d + m) / (2 m)), k = 0..m, every one passable (field != INF)."""
    if tuple(b) < tuple(a):
        a, b = b, a
    di, dj = b[0] - a[0], b[1] - a[1]
    m = max(abs(di), abs(dj))
    if m == 0:
        return fld[a[0], a[1]] != INF
    return all(fld[a[0] + (2 * k * di + m) // (2 * m), a[1] + (2 * k * dj + m) // (2 * m)] != INF for k in range(m + 1))


def snap(fld, c, r_inflate):
    """The start cell, or -- when it is not passable -- the cell with a finite field within Chebyshev distance r_inflate + 1 of
    it that has the least (d^2, field, index); None when there is none."""
    W, H = fld.shape
    if fld[c] != INF:
        return c
    n, best = int(r_inflate) + 1, None
    for i in range(max(0, c[0] - n), min(W, c[0] + n + 1)):
        for j in range(max(0, c[1] - n), min(H, c[1] + n + 1)):
            if fld[i, j] != INF:
                key = ((i - c[0]) ** 2 + (j - c[1]) ** 2, int(fld[i, j]), i * H + j)
                if best is None or key < best[0]:
                    best = key, (i, j)
    return None if best is None else best[1]


def descend(fld, c, strict=True):
    """The path cells from c to the cell whose field is 0: each time the first neighbour in MOVES order with
    field[n] + cost == field[c], side cells of a diagonal judged by ``passable``.  Where no neighbour satisfies that -- ``fld`` is
    no cost-to-go field -- AssertionError, or None with ``strict=False`` (the contract's LIPMPC_RRT_NO_PATH)."""
    W, H = fld.shape
    path = [c]
    while fld[c] != 0:
        i, j = c
        for di, dj in MOVES:
            a, b = i + di, j + dj
            if not (0 <= a < W and 0 <= b < H) or fld[a, b] == INF:
                continue
            if di and dj and (fld[a, j] == INF or fld[i, b] == INF):
                continue
            if int(fld[a, b]) + (DIAGONAL if di and dj else AXIAL) == int(fld[c]):
                c = (a, b)
                break
        else:
            if not strict:
                return None
            raise AssertionError(f"no descent from {c}: not a cost-to-go field")
        path.append(c)
    return path


def string_pull(fld, path, max_seg):
    """The path cells whose centres are sub-goals (the goal cell, whose sub-goal is the given goal, is not among them)."""
    out, a, k, last = [], 0, 1, len(path) - 1
    while k <= last:
        if not los(fld, path[a], path[k]) or int(fld[path[a]]) - int(fld[path[k]]) >= max_seg:
            e = k - 1 if k - 1 > a else k
            if e == last:
                break
            out.append(path[e])
            a, k = e, e + 1
        else:
            k += 1
    return out


def plan(occ, origin, cell, goal, start, r_inflate=0, max_seg=None, S_max=64, fld=None, field_status=None, strict=True):
    """One robot by the contract of lipmpc_grid_path_batch.  ``fld`` / ``field_status``: the field of ``goal`` when the caller
    has it (shared by many starts) -- or any field at all with ``strict=False``, where a descent that finds no neighbour ends
    NO_PATH as the contract says instead of raising.  Returns dict(status, n_sub, sub_goals [n_sub,2], path_cost, cells (the
    descent), snapped)."""
    solid = np.asarray(occ) != 0
    W, H = solid.shape
    if fld is None:
        fld, field_status = field(occ, origin, cell, goal, r_inflate)
    max_seg = NO_CAP if max_seg is None else int(max_seg)
    out = dict(status=None, n_sub=0, sub_goals=np.zeros((0, 2)), path_cost=float("nan"), cells=[], snapped=None)
    c = cell_of(start, origin, cell, W, H)
    if field_status == FIELD_GOAL_OUTSIDE:
        out["status"] = OUTSIDE_GRID
    elif field_status == FIELD_GOAL_BLOCKED:
        out["status"] = GOAL_OCCUPIED
    elif c is None:
        out["status"] = OUTSIDE_GRID
    elif solid[c]:
        out["status"] = START_OCCUPIED
    if out["status"] is not None:
        return out
    s = snap(fld, c, r_inflate)
    if s is None:
        out["status"] = NO_PATH
        return out
    path = descend(fld, s, strict)
    if path is None:
        out.update(status=NO_PATH, snapped=s)
        return out
    pulled = string_pull(fld, path, max_seg)
    out.update(cells=path, snapped=s, path_cost=float(np.float64(int(fld[s])) / 5.0))
    if len(pulled) + 1 > S_max:
        out["status"] = PATH_OVERFLOW
        return out
    sub = np.array([centre(p, origin, cell) for p in pulled] + [[np.float64(goal[0]), np.float64(goal[1])]]).reshape(-1, 2)
    out.update(status=FOUND, n_sub=len(sub), sub_goals=sub)
    return out


def plan_batch(occ, origin, cell, goal, start, r_inflate=0, max_seg=None, S_max=64):
    """lipmpc_grid_field_batch + lipmpc_grid_path_batch in numpy.  ``occ`` [W,H] (shared) or [F,W,H]; ``goal`` [F,2] with F = 1 or
    B (with per-robot maps F = B); ``start`` [B,2].  Returns dict(field [F,W,H], field_status [F], sub_goals (list of [n,2]),
    n_sub, status, path_cost [B], snapped and cells (lists, as ``plan``'s))."""
    occ, goal, start = np.asarray(occ), np.asarray(goal, np.float64), np.asarray(start, np.float64)
    F, B = len(goal), len(start)
    assert F in (1, B) and (occ.ndim == 2 or occ.shape[0] == F)
    fields = [field(occ if occ.ndim == 2 else occ[f], origin, cell, goal[f], r_inflate) for f in range(F)]
    res = []
    for b in range(B):
        f = 0 if F == 1 else b
        res.append(plan(occ if occ.ndim == 2 else occ[f], origin, cell, goal[f], start[b], r_inflate, max_seg, S_max, *fields[f]))
    return dict(field=np.stack([f for f, _ in fields]), field_status=np.array([s for _, s in fields], np.int32),
                sub_goals=[r["sub_goals"] for r in res], n_sub=np.array([r["n_sub"] for r in res], np.int32),
                status=np.array([r["status"] for r in res], np.int32), path_cost=np.array([r["path_cost"] for r in res]),
                snapped=[r["snapped"] for r in res], cells=[r["cells"] for r in res])


def maze():
    """The completeness example: 40 x 40 cells of 0.1 m at (0, 0), five walls two cells thick at i = 6, 12, 18, 24, 30, each with a
    single one-cell gap alternating between j = 2 and j = 37.  Returns dict(occ, origin, cell, start, goal)."""
    occ = np.zeros((40, 40), np.uint8)
    for n, i in enumerate((6, 12, 18, 24, 30)):
        occ[i:i + 2, :] = 1
        occ[i:i + 2, 2 if n % 2 == 0 else 37] = 0
    return dict(occ=occ, origin=(0.0, 0.0), cell=(0.1, 0.1), start=(0.25, 2.05), goal=(3.85, 2.05))


def spiral(n=24):
    """An n x n grid, all solid but a one-cell spiral corridor from the corner (1, 1) to the centre.  Returns (occ, corridor cells
    from the outside in)."""
    occ = np.ones((n, n), np.uint8)
    i, j, di, dj = 1, 1, 1, 0
    cells = [(i, j)]
    occ[i, j] = 0
    free = lambda a, b: 0 <= a < n and 0 <= b < n and occ[a, b] == 0
    while True:
        for _ in range(2):                                       # straight on, else one turn
            a, b = i + di, j + dj
            a2, b2 = a + di, b + dj
            # the next cell must stay inside the border and keep a wall between this lap and the last
            ok = 1 <= a < n - 1 and 1 <= b < n - 1 and not free(a2, b2) and not free(a + dj, b + di) and not free(a - dj, b - di)
            if ok:
                break
            di, dj = -dj, di
        else:
            return occ, cells
        i, j = a, b
        occ[i, j] = 0
        cells.append((i, j))
