"""Numpy / plain-Python restatement of the frontier explorer's two contracts -- lipmpc_grid_frontier_field_batch and
lipmpc_grid_frontier_path_batch, include/lipmpc.h: the three cell classes, the blocked mask, the frontier mask, the cost-to-go to
the nearest frontier cell by multi-source Dijkstra, and the paths by tests/field_oracle.py's snap, descent, line of sight and
string pulling.

TEST INFRASTRUCTURE ONLY, like tests/field_oracle.py: the GPU tests require the device's frontier, n_frontier, field, statuses,
sub-goals, path costs and target cells to equal this module's bit for bit.
"""
from __future__ import annotations

import heapq

import numpy as np

import field_oracle as FO

INF, NO_CAP = FO.INF, FO.NO_CAP
FOUND, NO_PATH, START_OCCUPIED, PATH_OVERFLOW, OUTSIDE_GRID = FO.FOUND, FO.NO_PATH, FO.START_OCCUPIED, FO.PATH_OVERFLOW, FO.OUTSIDE_GRID
THRESHOLD_MAX = 1 << 30
LDS_LIMIT, LDS_SLACK, bitmap_words = FO.LDS_LIMIT, FO.LDS_SLACK, FO.bitmap_words


def field_lds_bytes(ncells):
    """Dynamic LDS the frontier kernel asks for with the field in LDS: three bitmaps, the frontier count's word pair, the field."""
    return 4 * (3 * bitmap_words(ncells) + 2 + ncells)


def field_fits_lds(ncells):
    """THE FRONTIER KERNEL'S LDS RULE (its own, not the grid field planner's): the field, 4 bytes a cell, beside three bitmaps
    (blocked, solid, unknown), the frontier count's word pair and the reduction's slack within the 160 KiB of a workgroup."""
    return field_lds_bytes(ncells) + LDS_SLACK <= LDS_LIMIT


def sizes_at_the_lds_switch(H=193):
    """((W, H) the largest map of H columns whose field is kept in LDS, (W + 1, H) the smallest that is relaxed in the output)."""
    W = 2
    while field_fits_lds((W + 1) * H):
        W += 1
    assert field_fits_lds(W * H) and not field_fits_lds((W + 1) * H) and (W + 1) * H <= 1 << 17
    return (W, H), (W + 1, H)


def classes(evidence, t_free, t_occ):
    """(solid, free, unknown) [W,H] bool: e >= t_occ; e <= -t_free; neither.  Python ints: exact for every int32."""
    ev = np.asarray(evidence)
    assert 1 <= t_free <= THRESHOLD_MAX and 1 <= t_occ <= THRESHOLD_MAX
    e = ev.astype(np.int64)
    solid, free = e >= int(t_occ), e <= -int(t_free)
    return solid, free, ~solid & ~free


def masks(evidence, t_free, t_occ, r_inflate, min_unknown):
    """(blocked, frontier, unknown) [W,H] bool by the contract."""
    solid, free, unknown = classes(evidence, t_free, t_occ)
    W, H = solid.shape
    blocked = ~free | FO.blocked_cells(solid, r_inflate)
    count = np.zeros((W, H), np.int64)
    for di, dj in FO.MOVES:                                   # the 8 neighbours inside the grid
        i0, i1, j0, j1 = max(0, -di), min(W, W - di), max(0, -dj), min(H, H - dj)
        count[i0:i1, j0:j1] += unknown[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return blocked, ~blocked & (count >= int(min_unknown)), unknown


def field(evidence, t_free, t_occ, r_inflate=2, min_unknown=2):
    """(field [W,H] uint32, frontier [W,H] uint8, n_frontier) of one map: multi-source Dijkstra from every frontier cell."""
    blocked, frontier, _ = masks(evidence, t_free, t_occ, r_inflate, min_unknown)
    W, H = blocked.shape
    out = np.full((W, H), INF, np.uint32)
    dist = {(int(i), int(j)): 0 for i, j in zip(*np.nonzero(frontier))}
    heap = [(0, i, j) for i, j in dist]
    heapq.heapify(heap)
    while heap:
        d, i, j = heapq.heappop(heap)
        if d > dist[(i, j)]:
            continue
        for a, b, c in FO.moves_from(blocked, i, j):
            if d + c < dist.get((a, b), 1 << 62):
                dist[(a, b)] = d + c
                heapq.heappush(heap, (d + c, a, b))
    for (i, j), d in dist.items():
        out[i, j] = d
    return out, frontier.astype(np.uint8), int(frontier.sum())


def plan(evidence, t_occ, fld, n_frontier, origin, cell, start, r_inflate=2, max_seg=None, S_max=64, strict=True):
    """One robot by the contract of lipmpc_grid_frontier_path_batch.  ``strict=False``: ``fld`` may be any field, and a descent
    that finds no neighbour ends NO_PATH as the contract says instead of raising.  Returns dict(status, n_sub, sub_goals
    [n_sub,2], path_cost, target_cell, cells (the descent), snapped)."""
    ev = np.asarray(evidence)
    W, H = ev.shape
    max_seg = NO_CAP if max_seg is None else int(max_seg)
    out = dict(status=None, n_sub=0, sub_goals=np.zeros((0, 2)), path_cost=float("nan"), target_cell=-1, cells=[], snapped=None)
    c = FO.cell_of(start, origin, cell, W, H)
    if c is None:
        out["status"] = OUTSIDE_GRID
    elif int(ev[c]) >= int(t_occ):
        out["status"] = START_OCCUPIED
    elif n_frontier == 0:
        out["status"] = NO_PATH
    if out["status"] is not None:
        return out
    s = FO.snap(fld, c, r_inflate)
    if s is None:
        out["status"] = NO_PATH
        return out
    path = FO.descend(fld, s, strict)                         # ends at the first cell whose field is 0
    if path is None:
        out.update(status=NO_PATH, snapped=s)
        return out
    pulled = FO.string_pull(fld, path, max_seg)
    last = path[-1]
    out.update(cells=path, snapped=s, path_cost=float(np.float64(int(fld[s])) / 5.0), target_cell=last[0] * H + last[1])
    if len(pulled) + 1 > S_max:
        out["status"] = PATH_OVERFLOW
        return out
    sub = np.array([FO.centre(p, origin, cell) for p in pulled + [last]]).reshape(-1, 2)
    out.update(status=FOUND, n_sub=len(sub), sub_goals=sub)
    return out


def plan_batch(evidence, t_free, t_occ, origin, cell, start, r_inflate=2, min_unknown=2, max_seg=None, S_max=64):
    """Both calls in numpy.  ``evidence`` [W,H] (shared: F = 1) or [F,W,H] with F = 1 or B; ``start`` [B,2].  Returns dict(field,
    frontier [F,W,H], n_frontier [F], sub_goals (list of [n,2]), n_sub, status, path_cost, target_cell [B], target [B,2] (NaN
    where target_cell is -1), cells (list))."""
    ev, start = np.asarray(evidence), np.asarray(start, np.float64)
    ev = ev if ev.ndim == 3 else ev[None]
    F, B = len(ev), len(start)
    assert F in (1, B)
    fields = [field(ev[f], t_free, t_occ, r_inflate, min_unknown) for f in range(F)]
    res = []
    for b in range(B):
        f = 0 if F == 1 else b
        res.append(plan(ev[f], t_occ, fields[f][0], fields[f][2], origin, cell, start[b], r_inflate, max_seg, S_max))
    H = ev.shape[2]
    tc = np.array([r["target_cell"] for r in res], np.int32)
    target = np.array([FO.centre((t // H, t % H), origin, cell) if t >= 0 else (np.nan, np.nan) for t in tc]).reshape(-1, 2)
    return dict(field=np.stack([f[0] for f in fields]), frontier=np.stack([f[1] for f in fields]),
                n_frontier=np.array([f[2] for f in fields], np.int32), sub_goals=[r["sub_goals"] for r in res],
                n_sub=np.array([r["n_sub"] for r in res], np.int32), status=np.array([r["status"] for r in res], np.int32),
                path_cost=np.array([r["path_cost"] for r in res]), target_cell=tc, target=target, cells=[r["cells"] for r in res])


def room(W=12, H=10, t_free=1, t_occ=3):
    """A fully known room: solid outer walls one cell thick, every inner cell seen free."""
    ev = np.full((W, H), -t_free, np.int32)
    ev[0, :] = ev[-1, :] = ev[:, 0] = ev[:, -1] = t_occ
    return ev
