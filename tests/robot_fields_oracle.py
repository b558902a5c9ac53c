"""Numpy / plain-Python restatement of the claims from per-robot fields -- lipmpc_grid_frontier_assign_robot_fields_batch,
include/lipmpc.h: one single-source Dijkstra (heapq, Python ints) per entry cell, the keep phase and the greedy rounds as reductions
over those fields, the winners' chains down their own field and the string pulling of tests/field_oracle.py along them.

TEST INFRASTRUCTURE ONLY, like tests/assign_keep_oracle.py: the GPU tests require the device's sub-goals, n_sub, status, path costs,
target cells, claim rounds, n_claims, kept and n_kept to equal this module's bit for bit.
"""
from __future__ import annotations

import heapq

import numpy as np

import assign_keep_oracle as K
import assign_oracle as AO
import field_oracle as FO
import frontier_oracle as FR

INF = FO.INF
FOUND, PATH_OVERFLOW = FR.FOUND, FR.PATH_OVERFLOW
MAX_THREADS = 1 << 31                                         # B * (W * H + 64): the threads of one round launch


def field_from(passable, e):
    """D [W,H] uint32: the least cost from the cell e to every passable cell (moves between passable cells, 5 / 7, no corner cut);
    INF elsewhere."""
    blocked = ~np.asarray(passable, bool)
    W, H = blocked.shape
    out = np.full((W, H), INF, np.uint32)
    dist = {tuple(e): 0}
    heap = [(0, int(e[0]), int(e[1]))]
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


def best_source(D, sources):
    """((D(c), c), (i, j)) of the cell of ``sources`` with the least (D(c), cell index); None when none is within reach."""
    H = D.shape[1]
    live = np.flatnonzero(np.asarray(sources, bool) & (D != INF))
    if len(live) == 0:
        return None
    d = D.reshape(-1)[live].astype(np.int64)
    c = int(live[np.lexsort((live, d))[0]])
    return (int(D.reshape(-1)[c]), c), (c // H, c % H)


def rows(D, passable, t, origin, cell, max_seg):
    """(the chain from t down D to the entry, the marked cells in the chain's order, the sub-goals [marks + 1, 2]).  The sight is
    judged on PASSABILITY: a passable cell out of the entry's reach counts as any other (its word here: INF - 1, which no
    comparison of costs ever reads -- the chain's cells are all within reach)."""
    chain = FO.descend(D, t)
    sight = np.where(np.asarray(passable, bool) & (D == INF), np.uint32(INF - 1), D)
    marked = FO.string_pull(sight, chain, max_seg)
    sub = np.array([FO.centre(p, origin, cell) for p in marked[::-1] + [t]]).reshape(-1, 2)
    return chain, marked, sub


def assign(frontier, field, origin, cell, start, path, r_inflate, r_claim, max_claims, prev_target=None, keep=(0, 16, 0), max_seg=None,
           S_max=64, may_claim=None, fields=None):
    """The call by its contract, settled.  The arguments of tests/assign_keep_oracle.py's ``assign_keep`` (``keep`` = (r_keep,
    keep_ratio16, keep_slack); ``prev_target`` None = the NULL of the C call).  ``fields``: a dict entry cell -> D that is filled and
    may be shared between calls on one map.  Returns that oracle's dict (no ``slots``: there are none) plus entries [B] ((i, j) or
    None) and D: per robot of U_0 its field."""
    frontier, field, start = np.asarray(frontier), np.asarray(field), np.asarray(start, np.float64).reshape(-1, 2)
    W, H = field.shape
    B = len(start)
    r_keep, keep_ratio16, keep_slack = keep
    assert 0 <= r_claim <= AO.R_CLAIM_MAX and 0 <= max_claims <= AO.MAX_CLAIMS_MAX and B * (W * H + 64) <= MAX_THREADS
    assert 0 <= r_keep <= K.R_KEEP_MAX and K.KEEP_RATIO_MIN <= keep_ratio16 <= K.KEEP_RATIO_MAX and 0 <= keep_slack <= K.KEEP_SLACK_MAX
    max_seg = FO.NO_CAP if max_seg is None else int(max_seg)
    passable = field != INF
    sources = (frontier != 0) & passable
    may = np.ones(B, bool) if may_claim is None else np.asarray(may_claim) != 0
    fields = {} if fields is None else fields
    out = dict(sub_goals=[np.array(s, np.float64).reshape(-1, 2) for s in path["sub_goals"]], n_sub=np.array(path["n_sub"], np.int32),
               status=np.array(path["status"], np.int32), path_cost=np.array(path["path_cost"], np.float64),
               target_cell=np.array(path["target_cell"], np.int32), claim_round=np.full(B, -1, np.int32), kept=np.zeros(B, np.int8))
    entries, D = [None] * B, {}
    for b in range(B):
        if may[b] and out["status"][b] in (FOUND, PATH_OVERFLOW):
            e = FO.snap(field, FO.cell_of(start[b], origin, cell, W, H), r_inflate)      # (the start cell itself where it is passable)
            assert e is not None
            entries[b] = e
            if e not in fields:
                fields[e] = field_from(passable, e)
            D[b] = fields[e]
    left = sorted(D)
    winners, costs, targets, attempts, chains = [], [], [], [], {}
    k = 0

    def win(b, t, was_kept):
        chain, marked, sub = rows(D[b], passable, t, origin, cell, max_seg)
        assert chain[-1] == entries[b]
        if len(sub) > S_max:                                       # (nothing written to sub_goals: the path call's rows stay)
            out["status"][b], out["n_sub"][b] = PATH_OVERFLOW, 0
        else:
            out["sub_goals"][b] = sub
            out["status"][b], out["n_sub"][b] = FOUND, len(sub)
        out["path_cost"][b] = np.float64(int(D[b][t])) / 5.0
        out["target_cell"][b] = t[0] * H + t[1]
        out["claim_round"][b] = k
        out["kept"][b] = int(was_kept)
        chains[b] = chain
        winners.append(b), costs.append(int(D[b][t])), targets.append(t)
        left.remove(b)

    # the keep phase
    if prev_target is not None:
        prev = np.asarray(prev_target, np.int64)
        for b in list(left):
            if k >= max_claims:
                break
            if not 0 <= prev[b] < W * H:
                continue
            a = K.anchor(sources, (int(prev[b]) // H, int(prev[b]) % H), r_keep)
            if a is None:
                continue
            cost, near = int(D[b][a]), int(field[entries[b]])
            rec = dict(robot=b, anchor=a, cost=None if cost == INF else cost, near=near,
                       kept=cost != INF and K.keeps(cost, near, keep_ratio16, keep_slack))
            attempts.append(rec)
            if not rec["kept"]:
                continue                                              # (it costs nothing: k counts the winners)
            win(b, a, True)
            sources = sources & ~AO.disc(W, H, a, r_claim)
            k += 1
    # the greedy rounds
    while k < max_claims and left and sources.any():
        best = None
        for b in left:
            s = best_source(D[b], sources)
            if s is not None and (best is None or (s[0][0], b) < best[0]):
                best = (s[0][0], b), s[1]
        if best is None:
            break
        (_, b), t = best
        win(b, t, False)
        sources = sources & ~AO.disc(W, H, t, r_claim)
        k += 1
    tc = out["target_cell"]
    out["target"] = np.array([FO.centre((t // H, t % H), origin, cell) if t >= 0 else (np.nan, np.nan) for t in tc]).reshape(-1, 2)
    out.update(n_claims=len(winners), n_kept=int(out["kept"].sum()), winners=winners, costs=costs, targets=targets, attempts=attempts,
               entries=entries, D=D, chains=chains)
    return out


def pair_greedy(frontier, field, D, r_claim, max_claims):
    """The winners, INDEPENDENTLY of ``assign``: every (robot, source cell) pair with a finite cost, sorted once by (cost, robot,
    cell); the first pair whose robot has not won and whose cell is outside every winner's disc wins.  Returns (winners, targets)."""
    field = np.asarray(field)
    W, H = field.shape
    src = np.flatnonzero(((np.asarray(frontier) != 0) & (field != INF)).reshape(-1))
    pairs = sorted((int(D[b].reshape(-1)[c]), b, int(c)) for b in D for c in src if D[b].reshape(-1)[c] != INF)
    winners, targets = [], []
    for _, b, c in pairs:
        if len(winners) >= max_claims:
            break
        i, j = c // H, c % H
        if b in winners or any((i - t[0]) ** 2 + (j - t[1]) ** 2 <= r_claim * r_claim for t in targets):
            continue
        winners.append(b), targets.append((i, j))
    return winners, targets


def plan_batch(evidence, t_free, t_occ, origin, cell, start, r_claim, max_claims=64, prev_target=None, keep=(0, 16, 0), r_inflate=2,
               min_unknown=2, max_seg=None, S_max=64, may_claim=None, nearest=None, fields=None):
    """The three calls in numpy on ONE shared map ``evidence`` [W,H]: tests/frontier_oracle.py's plan_batch, then ``assign``.
    ``nearest``: that plan_batch's result when the caller has it."""
    ev = np.asarray(evidence)
    assert ev.ndim == 2
    if nearest is None:
        nearest = FR.plan_batch(ev, t_free, t_occ, origin, cell, start, r_inflate, min_unknown, max_seg, S_max)
    got = assign(nearest["frontier"][0], nearest["field"][0], origin, cell, start, nearest, r_inflate, r_claim, max_claims, prev_target, keep,
                 max_seg, S_max, may_claim, fields)
    return dict(nearest, **got, nearest=nearest)
