"""Numpy / plain-Python restatement of the gain-seeded claim -- lipmpc_grid_frontier_assign_utility_batch, include/lipmpc.h:
tests/assign_oracle.py's rounds with tests/gain_oracle.py's seeds on what is left of the sources and its terminal test where the
winner walks.  Composed from those two modules, tests/field_oracle.py and tests/frontier_oracle.py; it changes none of them.

TEST INFRASTRUCTURE ONLY: the GPU tests require the device's sub-goals, n_sub, status, path costs, target cells, target gains,
claim rounds and n_claims to equal this module's bit for bit.
"""
from __future__ import annotations

import heapq

import numpy as np

import assign_oracle as AO
import field_oracle as FO
import frontier_oracle as FR
import gain_oracle as G

INF = FO.INF
FOUND, PATH_OVERFLOW = FR.FOUND, FR.PATH_OVERFLOW
LDS_LIMIT, LDS_SLACK, bitmap_words = FO.LDS_LIMIT, FO.LDS_SLACK, FO.bitmap_words
UCLAIM_WORDS = 34


def field_lds_bytes(ncells):
    """Dynamic LDS the kernel asks for with the round's field in LDS: two bitmaps (impassable, S_k), 34 words (the assign
    kernels' 22, three more pointers and six scalars for the lanes that seed, walk and close a round), the field."""
    return 4 * (2 * bitmap_words(ncells) + UCLAIM_WORDS + ncells)


def field_fits_lds(ncells):
    """THE GAIN-SEEDED CLAIM KERNEL'S LDS RULE (its own): two bitmaps + 34 words + W H words + 256 <= 163840."""
    return field_lds_bytes(ncells) + LDS_SLACK <= LDS_LIMIT


def sizes_at_the_lds_switch(H=193):
    """((W, H) the largest map of H columns whose round field is kept in LDS, (W + 1, H) the smallest relaxed in ``work``)."""
    W = 2
    while field_fits_lds((W + 1) * H):
        W += 1
    assert field_fits_lds(W * H) and not field_fits_lds((W + 1) * H) and (W + 1) * H <= 1 << 17
    return (W, H), (W + 1, H)


def ufield_of(passable, sources, gain_, w_gain, g_cap):
    """ufield_k [W,H] uint32: the least, over the cells s of ``sources``, of seed(s) + the cost to s; INF elsewhere."""
    blocked = ~np.asarray(passable, bool)
    W, H = blocked.shape
    out = np.full((W, H), INF, np.uint32)
    dist = {(int(i), int(j)): G.seed(gain_[i, j], w_gain, g_cap) for i, j in zip(*np.nonzero(np.asarray(sources, bool) & ~blocked))}
    heap = [(d, i, j) for (i, j), d in dist.items()]
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


def assign(frontier, field, gain_, w_gain, g_cap, min_gain, origin, cell, start, path, r_inflate, r_claim, max_claims, max_seg=None,
           S_max=64, may_claim=None):
    """The call by its contract.  ``frontier`` / ``field`` [W,H]: the frontier field call's outputs; ``gain_`` [W,H] int32;
    ``path``: the utility path call's outputs as tests/gain_oracle.py's plan_batch gives them (sub_goals a list of [n,2]; n_sub,
    status, path_cost, target_cell, target_gain [B]).  Returns dict(sub_goals (list), n_sub, status, path_cost, target_cell,
    target_gain, target [B,2], claim_round [B], n_claims, and per round: winners, costs, targets ((i, j)), snapped, round_sources)."""
    frontier, field, start = np.asarray(frontier), np.asarray(field), np.asarray(start, np.float64).reshape(-1, 2)
    gain_ = np.asarray(gain_, np.int32)
    W, H = field.shape
    B = len(start)
    assert 0 <= r_claim <= AO.R_CLAIM_MAX and 0 <= max_claims <= AO.MAX_CLAIMS_MAX
    assert 0 <= w_gain <= G.W_GAIN_MAX and 1 <= g_cap <= G.G_CAP_MAX and 0 <= min_gain <= G.G_CAP_MAX
    max_seg = FO.NO_CAP if max_seg is None else int(max_seg)
    passable = field != INF
    sources = G.sources(frontier, field, gain_, min_gain)
    may = np.ones(B, bool) if may_claim is None else np.asarray(may_claim) != 0
    out = dict(sub_goals=[np.array(s, np.float64).reshape(-1, 2) for s in path["sub_goals"]], n_sub=np.array(path["n_sub"], np.int32),
               status=np.array(path["status"], np.int32), path_cost=np.array(path["path_cost"], np.float64),
               target_cell=np.array(path["target_cell"], np.int32), target_gain=np.array(path["target_gain"], np.int32),
               claim_round=np.full(B, -1, np.int32))
    left = [b for b in range(B) if may[b] and out["status"][b] in (FOUND, PATH_OVERFLOW)]
    winners, costs, targets, snapped, n_sources = [], [], [], [], []
    k = 0
    while k < max_claims and left and sources.any():
        fld = ufield_of(passable, sources, gain_, w_gain, g_cap)
        best = None
        for b in left:
            c = FO.cell_of(start[b], origin, cell, W, H)
            s = None if c is None else FO.snap(fld, c, r_inflate)
            if s is not None and (best is None or (int(fld[s]), b) < best[0]):
                best = (int(fld[s]), b), s
        if best is None:
            break
        (cost, b), s = best
        src_k = sources
        cells = G.descend(fld, s, lambda q: bool(src_k[q]) and int(fld[q]) == G.seed(gain_[q], w_gain, g_cap))
        pulled = FO.string_pull(fld, cells, max_seg)
        last = cells[-1]
        if len(pulled) + 1 > S_max:                               # (nothing written to sub_goals: the path call's rows stay)
            out["status"][b], out["n_sub"][b] = PATH_OVERFLOW, 0
        else:
            new = np.array([FO.centre(p, origin, cell) for p in pulled + [last]]).reshape(-1, 2)
            out["sub_goals"][b] = new
            out["status"][b], out["n_sub"][b] = FOUND, len(new)
        out["path_cost"][b] = np.float64(cost - int(fld[last])) / 5.0
        out["target_cell"][b] = last[0] * H + last[1]
        out["target_gain"][b] = gain_[last]
        out["claim_round"][b] = k
        n_sources.append(int(sources.sum()))
        winners.append(b), costs.append(cost), targets.append(last), snapped.append(s)
        sources = sources & ~AO.disc(W, H, last, r_claim)
        left.remove(b)
        k += 1
    tc = out["target_cell"]
    out["target"] = np.array([FO.centre((t // H, t % H), origin, cell) if t >= 0 else (np.nan, np.nan) for t in tc]).reshape(-1, 2)
    out.update(n_claims=len(winners), winners=winners, costs=costs, targets=targets, snapped=snapped, round_sources=n_sources)
    return out


def plan_batch(evidence, t_free, t_occ, origin, cell, start, r_claim, r_view, w_gain, g_cap, min_gain=0, max_claims=64, r_inflate=2,
               min_unknown=2, max_seg=None, S_max=64, may_claim=None, gain=None, informed=None):
    """All five calls in numpy on ONE shared map ``evidence`` [W,H]: tests/gain_oracle.py's plan_batch, then ``assign``.
    ``gain`` [W,H]: a hand-written gain in the place of the gain call's; ``informed``: that plan_batch's result when the caller has
    it.  Returns its dict with the claimed robots' rows replaced, plus claim_round, n_claims and the rounds' records;
    ``informed``: the shared-field plan."""
    ev = np.asarray(evidence)
    assert ev.ndim == 2
    if informed is None:
        informed = G.plan_batch(ev, t_free, t_occ, origin, cell, start, r_view, w_gain, g_cap, min_gain, r_inflate, min_unknown, max_seg,
                                S_max, gain=gain)
    got = assign(informed["frontier"][0], informed["field"][0], informed["gain"][0], w_gain, g_cap, min_gain, origin, cell, start, informed,
                 r_inflate, r_claim, max_claims, max_seg, S_max, may_claim)
    return dict(informed, **got, informed=informed)
