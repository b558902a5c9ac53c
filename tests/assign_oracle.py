"""Numpy / plain-Python restatement of the coordinated claim -- lipmpc_grid_frontier_assign_batch, include/lipmpc.h: per round a
multi-source Dijkstra from what is left of the frontier, every eligible robot's entry cell and cost, the least (cost, robot) as the
winner, its path by tests/field_oracle.py's snap, descent and string pulling, and the winner's disc taken out of the sources.

TEST INFRASTRUCTURE ONLY, like tests/frontier_oracle.py: the GPU tests require the device's sub-goals, n_sub, status, path costs,
target cells, claim rounds and n_claims to equal this module's bit for bit.
"""
from __future__ import annotations

import heapq

import numpy as np

import field_oracle as FO
import frontier_oracle as FR

INF = FO.INF
FOUND, PATH_OVERFLOW = FR.FOUND, FR.PATH_OVERFLOW
R_CLAIM_MAX = MAX_CLAIMS_MAX = 4096
LDS_LIMIT, LDS_SLACK, bitmap_words = FO.LDS_LIMIT, FO.LDS_SLACK, FO.bitmap_words


def field_lds_bytes(ncells):
    """Dynamic LDS the assign kernel asks for with the round's field in LDS: two bitmaps (impassable, sources), 22 words (the
    winner's key and target, the placement and the output rows' pointers for the lane that walks), the field."""
    return 4 * (2 * bitmap_words(ncells) + 22 + ncells)


def field_fits_lds(ncells):
    """THE ASSIGN KERNEL'S LDS RULE (its own, not the frontier field kernel's): the field, 4 bytes a cell, beside two bitmaps, 22
    words and the reduction's slack within the 160 KiB of a workgroup."""
    return field_lds_bytes(ncells) + LDS_SLACK <= LDS_LIMIT


def sizes_at_the_lds_switch(H=193):
    """((W, H) the largest map of H columns whose round field is kept in LDS, (W + 1, H) the smallest relaxed in ``work``)."""
    W = 2
    while field_fits_lds((W + 1) * H):
        W += 1
    assert field_fits_lds(W * H) and not field_fits_lds((W + 1) * H) and (W + 1) * H <= 1 << 17
    return (W, H), (W + 1, H)


def field_of(passable, sources):
    """field_k [W,H] uint32: the least cost from every passable cell to any cell of ``sources`` (moves between passable cells,
    5 / 7, no corner cut); INF elsewhere."""
    blocked = ~np.asarray(passable, bool)
    W, H = blocked.shape
    out = np.full((W, H), INF, np.uint32)
    dist = {(int(i), int(j)): 0 for i, j in zip(*np.nonzero(np.asarray(sources, bool) & ~blocked))}
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
    return out


def disc(W, H, t, r_claim):
    """[W,H] bool: the cells (i, j) with (i - i_t)^2 + (j - j_t)^2 <= r_claim^2, t = (i_t, j_t)."""
    i, j = np.arange(W, dtype=np.int64)[:, None], np.arange(H, dtype=np.int64)[None, :]
    return (i - t[0]) ** 2 + (j - t[1]) ** 2 <= int(r_claim) ** 2


def assign(frontier, field, origin, cell, start, path, r_inflate, r_claim, max_claims, max_seg=None, S_max=64, may_claim=None,
           passable=None):
    """The call by its contract.  ``frontier`` / ``field`` [W,H]: the frontier field call's outputs; ``path``: the path call's
    outputs as tests/frontier_oracle.py's plan_batch gives them (sub_goals a list of [n,2]; n_sub, status, path_cost, target_cell
    [B]).  ``passable``: another passability mask than field != INF (the tests' check that the two agree).  Returns dict(sub_goals
    (list), n_sub, status, path_cost, target_cell, target [B,2], claim_round [B], n_claims, and per round: winners, costs, targets
    ((i, j)), snapped (the winner's entry cell), n_sources)."""
    frontier, field, start = np.asarray(frontier), np.asarray(field), np.asarray(start, np.float64).reshape(-1, 2)
    W, H = field.shape
    B = len(start)
    assert 0 <= r_claim <= R_CLAIM_MAX and 0 <= max_claims <= MAX_CLAIMS_MAX
    max_seg = FO.NO_CAP if max_seg is None else int(max_seg)
    passable = field != INF if passable is None else np.asarray(passable, bool)
    sources = (frontier != 0) & passable
    may = np.ones(B, bool) if may_claim is None else np.asarray(may_claim) != 0
    out = dict(sub_goals=[np.array(s, np.float64).reshape(-1, 2) for s in path["sub_goals"]], n_sub=np.array(path["n_sub"], np.int32),
               status=np.array(path["status"], np.int32), path_cost=np.array(path["path_cost"], np.float64),
               target_cell=np.array(path["target_cell"], np.int32), claim_round=np.full(B, -1, np.int32))
    left = [b for b in range(B) if may[b] and out["status"][b] in (FOUND, PATH_OVERFLOW)]
    winners, costs, targets, snapped, n_sources = [], [], [], [], []
    k = 0
    while k < max_claims and left and sources.any():
        fld = field_of(passable, sources)
        best = None
        for b in left:
            c = FO.cell_of(start[b], origin, cell, W, H)
            s = None if c is None else FO.snap(fld, c, r_inflate)
            if s is not None and (best is None or (int(fld[s]), b) < best[0]):
                best = (int(fld[s]), b), s
        if best is None:
            break
        (cost, b), s = best
        cells = FO.descend(fld, s)
        pulled = FO.string_pull(fld, cells, max_seg)
        last = cells[-1]
        if len(pulled) + 1 > S_max:                               # (nothing written to sub_goals: the path call's rows stay)
            out["status"][b], out["n_sub"][b] = PATH_OVERFLOW, 0
        else:
            new = np.array([FO.centre(p, origin, cell) for p in pulled + [last]]).reshape(-1, 2)
            out["sub_goals"][b] = new                             # (rows from n_sub on: whatever the path call left there)
            out["status"][b], out["n_sub"][b] = FOUND, len(new)
        out["path_cost"][b] = np.float64(cost) / 5.0
        out["target_cell"][b] = last[0] * H + last[1]
        out["claim_round"][b] = k
        n_sources.append(int(sources.sum()))
        winners.append(b), costs.append(cost), targets.append(last), snapped.append(s)
        sources = sources & ~disc(W, H, last, r_claim)
        left.remove(b)
        k += 1
    tc = out["target_cell"]
    out["target"] = np.array([FO.centre((t // H, t % H), origin, cell) if t >= 0 else (np.nan, np.nan) for t in tc]).reshape(-1, 2)
    out.update(n_claims=len(winners), winners=winners, costs=costs, targets=targets, snapped=snapped, n_sources=n_sources)
    return out


def plan_batch(evidence, t_free, t_occ, origin, cell, start, r_claim, max_claims=64, r_inflate=2, min_unknown=2, max_seg=None, S_max=64,
               may_claim=None, nearest=None):
    """The three calls in numpy on ONE shared map ``evidence`` [W,H]: tests/frontier_oracle.py's plan_batch, then ``assign``.
    ``nearest``: that plan_batch's result when the caller has it.  Returns its dict with the claimed robots' rows replaced, plus
    claim_round, n_claims and the rounds' records; ``nearest``: the plain plan."""
    ev = np.asarray(evidence)
    assert ev.ndim == 2
    if nearest is None:
        nearest = FR.plan_batch(ev, t_free, t_occ, origin, cell, start, r_inflate, min_unknown, max_seg, S_max)
    got = assign(nearest["frontier"][0], nearest["field"][0], origin, cell, start, nearest, r_inflate, r_claim, max_claims, max_seg, S_max,
                 may_claim)
    return dict(nearest, **got, nearest=nearest)
