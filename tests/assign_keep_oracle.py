"""Numpy / plain-Python restatement of claim hysteresis -- lipmpc_grid_frontier_assign_keep_batch, include/lipmpc.h: the keep
phase (per robot with a previous target the anchor, a single-source Dijkstra from it, the entry cell, the integer test against the
nearest frontier, the keeper's rows and disc) ahead of the greedy rounds of tests/assign_oracle.py, all within max_claims slots.

TEST INFRASTRUCTURE ONLY, like tests/assign_oracle.py, on which it is built: the GPU tests require the device's sub-goals, n_sub,
status, path costs, target cells, claim rounds, n_claims, kept and n_kept to equal this module's bit for bit.
"""
from __future__ import annotations

import numpy as np

import assign_oracle as AO
import field_oracle as FO
import frontier_oracle as FR

INF = FO.INF
FOUND, PATH_OVERFLOW = FR.FOUND, FR.PATH_OVERFLOW
R_KEEP_MAX, KEEP_RATIO_MIN, KEEP_RATIO_MAX, KEEP_SLACK_MAX = 64, 16, 1024, 4096
LDS_LIMIT, LDS_SLACK, bitmap_words = FO.LDS_LIMIT, FO.LDS_SLACK, FO.bitmap_words
INT32_MAX = 0x7FFFFFFF


def field_lds_bytes(ncells):
    """Dynamic LDS the keep kernel asks for with the slot's field in LDS: the assign kernel's two bitmaps and 22 words, 12 more
    words (three more pointers, four scalars and the entry cell for the lane that walks, the count of U), the field."""
    return 4 * (2 * bitmap_words(ncells) + 34 + ncells)


def field_fits_lds(ncells):
    """THE KEEP KERNEL'S LDS RULE (its own, not the assign kernel's): the field, 4 bytes a cell, beside two bitmaps, 34 words and
    the reduction's slack within the 160 KiB of a workgroup."""
    return field_lds_bytes(ncells) + LDS_SLACK <= LDS_LIMIT


def sizes_at_the_lds_switch(H=193):
    """((W, H) the largest map of H columns whose slot field is kept in LDS, (W + 1, H) the smallest relaxed in ``work``)."""
    W = 2
    while field_fits_lds((W + 1) * H):
        W += 1
    assert field_fits_lds(W * H) and not field_fits_lds((W + 1) * H) and (W + 1) * H <= 1 << 17
    return (W, H), (W + 1, H)


def anchor(sources, p, r_keep):
    """The cell (i, j) of ``sources`` [W,H] within (i - i_p)^2 + (j - j_p)^2 <= r_keep^2 of p = (i_p, j_p) with the least
    (d^2, cell index); None when there is none."""
    W, H = sources.shape
    best = None
    for i in range(max(p[0] - r_keep, 0), min(p[0] + r_keep, W - 1) + 1):
        for j in range(max(p[1] - r_keep, 0), min(p[1] + r_keep, H - 1) + 1):
            d2 = (i - p[0]) ** 2 + (j - p[1]) ** 2
            if d2 <= r_keep * r_keep and sources[i, j] and (best is None or (d2, i * H + j) < best[0]):
                best = (d2, i * H + j), (i, j)
    return None if best is None else best[1]


def keeps(keep_cost, near, keep_ratio16, keep_slack):
    """THE TEST, in Python integers (the device computes it in 64 bits: nothing here reaches 2^63)."""
    return 16 * int(keep_cost) <= int(keep_ratio16) * int(near) + 80 * int(keep_slack)


def _write_rows(out, fld, b, s, k, origin, cell, max_seg, S_max):
    """The winner's rows by the path rule on ``fld``, as tests/assign_oracle.py writes them; returns the target cell (i, j)."""
    H = fld.shape[1]
    cells = FO.descend(fld, s)
    pulled = FO.string_pull(fld, cells, max_seg)
    last = cells[-1]
    if len(pulled) + 1 > S_max:
        out["status"][b], out["n_sub"][b] = PATH_OVERFLOW, 0
    else:
        new = np.array([FO.centre(p, origin, cell) for p in pulled + [last]]).reshape(-1, 2)
        out["sub_goals"][b] = new
        out["status"][b], out["n_sub"][b] = FOUND, len(new)
    out["path_cost"][b] = np.float64(int(fld[s])) / 5.0
    out["target_cell"][b] = last[0] * H + last[1]
    out["claim_round"][b] = k
    return last


def assign_keep(frontier, field, origin, cell, start, path, r_inflate, r_claim, max_claims, prev_target, r_keep, keep_ratio16, keep_slack,
                max_seg=None, S_max=64, may_claim=None):
    """The call by its contract.  The arguments of tests/assign_oracle.py's ``assign`` plus ``prev_target`` [B] (or None = every
    robot has none) and the three keep parameters.  Returns its dict plus kept [B] int8, n_kept, slots (the relaxations made) and
    attempts: per keep attempt dict(robot, anchor, entry (or None), cost, near, kept)."""
    frontier, field, start = np.asarray(frontier), np.asarray(field), np.asarray(start, np.float64).reshape(-1, 2)
    W, H = field.shape
    B = len(start)
    assert 0 <= r_claim <= AO.R_CLAIM_MAX and 0 <= max_claims <= AO.MAX_CLAIMS_MAX
    assert 0 <= r_keep <= R_KEEP_MAX and KEEP_RATIO_MIN <= keep_ratio16 <= KEEP_RATIO_MAX and 0 <= keep_slack <= KEEP_SLACK_MAX
    max_seg = FO.NO_CAP if max_seg is None else int(max_seg)
    prev = np.full(B, -1, np.int64) if prev_target is None else np.asarray(prev_target, np.int64)
    passable = field != INF
    sources = (frontier != 0) & passable
    may = np.ones(B, bool) if may_claim is None else np.asarray(may_claim) != 0
    out = dict(sub_goals=[np.array(s, np.float64).reshape(-1, 2) for s in path["sub_goals"]], n_sub=np.array(path["n_sub"], np.int32),
               status=np.array(path["status"], np.int32), path_cost=np.array(path["path_cost"], np.float64),
               target_cell=np.array(path["target_cell"], np.int32), claim_round=np.full(B, -1, np.int32), kept=np.zeros(B, np.int8))
    left = [b for b in range(B) if may[b] and out["status"][b] in (FOUND, PATH_OVERFLOW)]
    winners, costs, targets, snapped, n_sources, attempts = [], [], [], [], [], []
    k = slots = 0
    # the keep phase
    for b in list(left):
        if slots >= max_claims:
            break
        c = FO.cell_of(start[b], origin, cell, W, H)
        if c is None or not 0 <= prev[b] < W * H:
            continue
        a = anchor(sources, (int(prev[b]) // H, int(prev[b]) % H), r_keep)
        if a is None:
            continue                                                  # nothing is left of the target: no slot is spent
        slots += 1
        only = np.zeros((W, H), bool)
        only[a] = True
        fld = AO.field_of(passable, only)
        s, e = FO.snap(fld, c, r_inflate), FO.snap(field, c, r_inflate)
        rec = dict(robot=b, anchor=a, entry=s, cost=None if s is None else int(fld[s]), near=None if e is None else int(field[e]), kept=False)
        attempts.append(rec)
        if s is None or e is None or not keeps(fld[s], field[e], keep_ratio16, keep_slack):
            continue                                                  # the slot is spent all the same
        n_sources.append(int(sources.sum()))
        last = _write_rows(out, fld, b, s, k, origin, cell, max_seg, S_max)
        assert last == a
        out["kept"][b] = 1
        rec["kept"] = True
        winners.append(b), costs.append(int(fld[s])), targets.append(last), snapped.append(s)
        sources = sources & ~AO.disc(W, H, last, r_claim)
        left.remove(b)
        k += 1
    # the greedy phase: tests/assign_oracle.py's rounds
    while slots < max_claims and left and sources.any():
        fld = AO.field_of(passable, sources)
        best = None
        for b in left:
            c = FO.cell_of(start[b], origin, cell, W, H)
            s = None if c is None else FO.snap(fld, c, r_inflate)
            if s is not None and (best is None or (int(fld[s]), b) < best[0]):
                best = (int(fld[s]), b), s
        if best is None:
            break
        (cost, b), s = best
        n_sources.append(int(sources.sum()))
        last = _write_rows(out, fld, b, s, k, origin, cell, max_seg, S_max)
        winners.append(b), costs.append(cost), targets.append(last), snapped.append(s)
        sources = sources & ~AO.disc(W, H, last, r_claim)
        left.remove(b)
        k += 1
        slots += 1
    tc = out["target_cell"]
    out["target"] = np.array([FO.centre((t // H, t % H), origin, cell) if t >= 0 else (np.nan, np.nan) for t in tc]).reshape(-1, 2)
    out.update(n_claims=len(winners), n_kept=int(out["kept"].sum()), winners=winners, costs=costs, targets=targets, snapped=snapped,
               n_sources=n_sources, slots=slots, attempts=attempts)
    return out


def plan_batch(evidence, t_free, t_occ, origin, cell, start, r_claim, prev_target, r_keep, keep_ratio16, keep_slack, max_claims=64,
               r_inflate=2, min_unknown=2, max_seg=None, S_max=64, may_claim=None, nearest=None):
    """The three calls in numpy on ONE shared map ``evidence`` [W,H]: tests/frontier_oracle.py's plan_batch, then ``assign_keep``.
    ``nearest``: that plan_batch's result when the caller has it."""
    ev = np.asarray(evidence)
    assert ev.ndim == 2
    if nearest is None:
        nearest = FR.plan_batch(ev, t_free, t_occ, origin, cell, start, r_inflate, min_unknown, max_seg, S_max)
    got = assign_keep(nearest["frontier"][0], nearest["field"][0], origin, cell, start, nearest, r_inflate, r_claim, max_claims,
                      prev_target, r_keep, keep_ratio16, keep_slack, max_seg, S_max, may_claim)
    return dict(nearest, **got, nearest=nearest)
