"""Numpy / plain-Python restatement of the soft-clearance contracts (include/lipmpc.h, SOFT CLEARANCE): the cost layer of
lipmpc_grid_clearance_cost_batch by brute force over every solid cell, the weighted fields of lipmpc_grid_field_weighted_batch and
lipmpc_grid_frontier_field_weighted_batch by Dijkstra (heapq, Python ints), and the weighted walk of the two weighted path calls:
the descent with the cell cost in its equation and the string pulling with its two penalty sums.

TEST INFRASTRUCTURE ONLY, like tests/field_oracle.py, whose snap, segment rule, cell rule and centres this module uses as they
are: the GPU tests require every output of the device to equal this module's bit for bit.
"""
from __future__ import annotations

import heapq

import numpy as np

import field_oracle as FO
import frontier_oracle as FR

INF, NO_CAP = FO.INF, FO.NO_CAP
COST_MAX, R_CLEAR_MAX = 248, 31
FOUND, NO_PATH, PATH_OVERFLOW = FO.FOUND, FO.NO_PATH, FO.PATH_OVERFLOW


def clearance_cost(solid, r_clear, w_clear):
    """cost [W,H] uint8 of one map (``solid`` [W,H] bool): d2 = the least squared distance to a solid cell of the grid, by brute
    force over the solid cells; 0 where d2 > r_clear^2, else (w_clear * (r_clear^2 - d2)) // r_clear^2."""
    solid = np.asarray(solid, bool)
    W, H = solid.shape
    r, w = int(r_clear), int(w_clear)
    assert 1 <= r <= R_CLEAR_MAX and 0 <= w <= COST_MAX
    i, j = np.arange(W, dtype=np.int64)[:, None], np.arange(H, dtype=np.int64)[None, :]
    d2 = np.full((W, H), 1 << 40, np.int64)
    for si, sj in zip(*np.nonzero(solid)):
        lo_i, hi_i, lo_j, hi_j = max(0, si - r), min(W, si + r + 1), max(0, sj - r), min(H, sj + r + 1)     # (beyond the box d2 > r^2 anyway)
        box = (i[lo_i:hi_i] - si) ** 2 + (j[:, lo_j:hi_j] - sj) ** 2
        d2[lo_i:hi_i, lo_j:hi_j] = np.minimum(d2[lo_i:hi_i, lo_j:hi_j], box)
    return np.where(d2 <= r * r, (w * (r * r - np.minimum(d2, r * r))) // (r * r), 0).astype(np.uint8)


def clearance_cost_evidence(evidence, t_occ, r_clear, w_clear):
    """The evidence form: solid = e >= t_occ (exact for every int32); unknown cells are no sources of cost."""
    return clearance_cost(np.asarray(evidence).astype(np.int64) >= int(t_occ), r_clear, w_clear)


def k_of(cost):
    """k(c) = min(cost[c], 248) as Python-int-safe int64."""
    return np.minimum(np.asarray(cost).astype(np.int64), COST_MAX)


def _dijkstra(blocked, k, sources):
    """The weighted field: f = 0 on the sources, f(c) = k(c) + min over legal moves c -> n of f(n) + step.  Relaxing from a settled
    n to its neighbour c charges k(c): the move rules are symmetric, the cost is that of the cell that is LEFT."""
    W, H = blocked.shape
    out = np.full((W, H), INF, np.uint32)
    dist = {s: 0 for s in sources}
    heap = [(0, i, j) for i, j in dist]
    heapq.heapify(heap)
    while heap:
        d, i, j = heapq.heappop(heap)
        if d > dist[(i, j)]:
            continue
        for a, b, step in FO.moves_from(blocked, i, j):
            nd = d + step + int(k[a, b])
            if nd < dist.get((a, b), 1 << 62):
                dist[(a, b)] = nd
                heapq.heappush(heap, (nd, a, b))
    for (i, j), d in dist.items():
        assert d < INF
        out[i, j] = d
    return out


def field(occ, cost, origin, cell, goal, r_inflate=0):
    """(field [W,H] uint32, field_status) of one goal: tests/field_oracle.py's ``field`` in the weighted metric."""
    blocked = FO.blocked_cells(occ, r_inflate)
    W, H = blocked.shape
    g = FO.cell_of(goal, origin, cell, W, H)
    if g is None:
        return np.full((W, H), INF, np.uint32), FO.FIELD_GOAL_OUTSIDE
    if blocked[g]:
        return np.full((W, H), INF, np.uint32), FO.FIELD_GOAL_BLOCKED
    return _dijkstra(blocked, k_of(cost), [g]), FO.FIELD_OK


def frontier_field(evidence, cost, t_free, t_occ, r_inflate=2, min_unknown=2):
    """(field, frontier uint8, n_frontier) of one map: tests/frontier_oracle.py's ``field`` in the weighted metric."""
    blocked, frontier, _ = FR.masks(evidence, t_free, t_occ, r_inflate, min_unknown)
    sources = [(int(i), int(j)) for i, j in zip(*np.nonzero(frontier))]
    return _dijkstra(blocked, k_of(cost), sources), frontier.astype(np.uint8), int(frontier.sum())


def descent_step(fld, k, c):
    """The weighted descent from c, one step: the first neighbour in MOVES order with a legal move and
    field[n] + step + k(c) == field[c]; None where there is none."""
    W, H = fld.shape
    i, j = c
    for di, dj in FO.MOVES:
        a, b = i + di, j + dj
        if not (0 <= a < W and 0 <= b < H) or fld[a, b] == INF:
            continue
        if di and dj and (fld[a, j] == INF or fld[i, b] == INF):
            continue
        if int(fld[a, b]) + (FO.DIAGONAL if di and dj else FO.AXIAL) + int(k[c]) == int(fld[c]):
            return a, b
    return None


def descend(fld, k, c, strict=True):
    """The path cells from c to the first cell whose field is 0, step by step.  Where a cell has no next one -- ``fld`` is no
    weighted field of ``k`` -- AssertionError, or None with ``strict=False`` (the contract's LIPMPC_RRT_NO_PATH)."""
    path = [c]
    while fld[c] != 0:
        c = descent_step(fld, k, c)
        if c is None:
            if not strict:
                return None
            raise AssertionError(f"no weighted descent from {path[-1]}")
        path.append(c)
    return path


def seg_cells(a, b):
    """The cells the segment rule visits between a and b, both ends included (tests/field_oracle.py's ``los``)."""
    if tuple(b) < tuple(a):
        a, b = b, a
    di, dj = b[0] - a[0], b[1] - a[1]
    m = max(abs(di), abs(dj))
    if m == 0:
        return [tuple(a)]
    return [(a[0] + (2 * t * di + m) // (2 * m), a[1] + (2 * t * dj + m) // (2 * m)) for t in range(m + 1)]


def seg_pen(k, a, cur):
    """The sum of k over the cells the segment rule visits between a and cur, minus k(cur)."""
    return sum(int(k[c]) for c in seg_cells(a, cur)) - int(k[cur])


def string_pull(fld, k, path, max_seg, why=None):
    """The path cells whose centres are sub-goals (the last cell is not among them).  A sub-goal is set where the line of sight
    breaks, where seg_pen(a, cur) > pen, or where the length since the anchor with penalties excluded reaches max_seg.  ``why``:
    a list that receives, per sub-goal, the set of the rules that fired ("los", "pen", "seg")."""
    out, a, t, last = [], 0, 1, len(path) - 1
    while t <= last:
        pen = sum(int(k[path[u]]) for u in range(a, t))
        sight = FO.los(fld, path[a], path[t])
        fired = set() if sight else {"los"}
        if sight and seg_pen(k, path[a], path[t]) > pen:
            fired.add("pen")
        if int(fld[path[a]]) - int(fld[path[t]]) - pen >= max_seg:
            fired.add("seg")
        if fired:
            e = t - 1 if t - 1 > a else t
            if e == last:
                break
            out.append(path[e])
            if why is not None:
                why.append(fired)
            a, t = e, e + 1
        else:
            t += 1
    return out


def _walk(fld, k, c, r_inflate, max_seg, S_max, origin, cell, strict, why=None):
    """snap, descent and string pulling from the start cell c: dict(status or None (= go on), cells, snapped, pulled, path_cost)."""
    s = FO.snap(fld, c, r_inflate)
    if s is None:
        return dict(status=NO_PATH)
    path = descend(fld, k, s, strict)
    if path is None:
        return dict(status=NO_PATH, snapped=s)
    pulled = string_pull(fld, k, path, max_seg, why)
    res = dict(status=None, cells=path, snapped=s, pulled=pulled, path_cost=float(np.float64(int(fld[s])) / 5.0))
    if len(pulled) + 1 > S_max:
        res["status"] = PATH_OVERFLOW
    return res


def plan(occ, cost, origin, cell, goal, start, r_inflate=0, max_seg=None, S_max=64, fld=None, field_status=None, strict=True, why=None):
    """One robot by the contract of lipmpc_grid_path_weighted_batch: tests/field_oracle.py's ``plan`` with the weighted walk."""
    solid = np.asarray(occ) != 0
    W, H = solid.shape
    if fld is None:
        fld, field_status = field(occ, cost, origin, cell, goal, r_inflate)
    max_seg = NO_CAP if max_seg is None else int(max_seg)
    out = dict(status=None, n_sub=0, sub_goals=np.zeros((0, 2)), path_cost=float("nan"), cells=[], snapped=None)
    c = FO.cell_of(start, origin, cell, W, H)
    if field_status == FO.FIELD_GOAL_OUTSIDE:
        out["status"] = FO.OUTSIDE_GRID
    elif field_status == FO.FIELD_GOAL_BLOCKED:
        out["status"] = FO.GOAL_OCCUPIED
    elif c is None:
        out["status"] = FO.OUTSIDE_GRID
    elif solid[c]:
        out["status"] = FO.START_OCCUPIED
    if out["status"] is not None:
        return out
    w = _walk(fld, k_of(cost), c, r_inflate, max_seg, S_max, origin, cell, strict, why)
    out.update({key: w[key] for key in ("cells", "snapped", "path_cost") if key in w})
    if w["status"] is not None:
        out["status"] = w["status"]
        return out
    sub = np.array([FO.centre(p, origin, cell) for p in w["pulled"]] + [[np.float64(goal[0]), np.float64(goal[1])]]).reshape(-1, 2)
    out.update(status=FOUND, n_sub=len(sub), sub_goals=sub)
    return out


def plan_batch(occ, cost, origin, cell, goal, start, r_inflate=0, max_seg=None, S_max=64):
    """The weighted goal field and path call in numpy: tests/field_oracle.py's ``plan_batch``; ``cost`` has ``occ``'s shape."""
    occ, cost, goal, start = np.asarray(occ), np.asarray(cost), np.asarray(goal, np.float64), np.asarray(start, np.float64)
    F, B = len(goal), len(start)
    assert F in (1, B) and (occ.ndim == 2 or occ.shape[0] == F) and cost.shape == occ.shape
    of = lambda a, f: a if a.ndim == 2 else a[f]
    fields = [field(of(occ, f), of(cost, f), origin, cell, goal[f], r_inflate) for f in range(F)]
    res = []
    for b in range(B):
        f = 0 if F == 1 else b
        res.append(plan(of(occ, f), of(cost, f), origin, cell, goal[f], start[b], r_inflate, max_seg, S_max, *fields[f]))
    return dict(field=np.stack([f for f, _ in fields]), field_status=np.array([s for _, s in fields], np.int32),
                sub_goals=[r["sub_goals"] for r in res], n_sub=np.array([r["n_sub"] for r in res], np.int32),
                status=np.array([r["status"] for r in res], np.int32), path_cost=np.array([r["path_cost"] for r in res]),
                snapped=[r["snapped"] for r in res], cells=[r["cells"] for r in res])


def frontier_plan(evidence, cost, t_occ, fld, n_frontier, origin, cell, start, r_inflate=2, max_seg=None, S_max=64, strict=True, why=None):
    """One robot by the contract of lipmpc_grid_frontier_path_weighted_batch: tests/frontier_oracle.py's ``plan``, weighted walk."""
    ev = np.asarray(evidence)
    W, H = ev.shape
    max_seg = NO_CAP if max_seg is None else int(max_seg)
    out = dict(status=None, n_sub=0, sub_goals=np.zeros((0, 2)), path_cost=float("nan"), target_cell=-1, cells=[], snapped=None)
    c = FO.cell_of(start, origin, cell, W, H)
    if c is None:
        out["status"] = FO.OUTSIDE_GRID
    elif int(ev[c]) >= int(t_occ):
        out["status"] = FO.START_OCCUPIED
    elif n_frontier == 0:
        out["status"] = NO_PATH
    if out["status"] is not None:
        return out
    w = _walk(fld, k_of(cost), c, r_inflate, max_seg, S_max, origin, cell, strict, why)
    out.update({key: w[key] for key in ("cells", "snapped", "path_cost") if key in w})
    if "cells" in w:
        last = w["cells"][-1]
        out["target_cell"] = last[0] * H + last[1]
    if w["status"] is not None:
        out["status"] = w["status"]
        return out
    sub = np.array([FO.centre(p, origin, cell) for p in w["pulled"] + [last]]).reshape(-1, 2)
    out.update(status=FOUND, n_sub=len(sub), sub_goals=sub)
    return out


def frontier_plan_batch(evidence, cost, t_free, t_occ, origin, cell, start, r_inflate=2, min_unknown=2, max_seg=None, S_max=64):
    """The weighted frontier field and path call in numpy: tests/frontier_oracle.py's ``plan_batch``; ``cost`` has the maps' shape."""
    ev, cost, start = np.asarray(evidence), np.asarray(cost), np.asarray(start, np.float64)
    ev, cost = (ev if ev.ndim == 3 else ev[None]), (cost if cost.ndim == 3 else cost[None])
    F, B = len(ev), len(start)
    assert F in (1, B) and cost.shape == ev.shape
    fields = [frontier_field(ev[f], cost[f], t_free, t_occ, r_inflate, min_unknown) for f in range(F)]
    res = []
    for b in range(B):
        f = 0 if F == 1 else b
        res.append(frontier_plan(ev[f], cost[f], t_occ, fields[f][0], fields[f][2], origin, cell, start[b], r_inflate, max_seg, S_max))
    H = ev.shape[2]
    tc = np.array([r["target_cell"] for r in res], np.int32)
    target = np.array([FO.centre((t // H, t % H), origin, cell) if t >= 0 else (np.nan, np.nan) for t in tc]).reshape(-1, 2)
    return dict(field=np.stack([f[0] for f in fields]), frontier=np.stack([f[1] for f in fields]),
                n_frontier=np.array([f[2] for f in fields], np.int32), sub_goals=[r["sub_goals"] for r in res],
                n_sub=np.array([r["n_sub"] for r in res], np.int32), status=np.array([r["status"] for r in res], np.int32),
                path_cost=np.array([r["path_cost"] for r in res]), target_cell=tc, target=target, cells=[r["cells"] for r in res])
