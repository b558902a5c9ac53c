"""Numpy / plain-Python restatement of claim hysteresis for the gain-seeded claims --
lipmpc_grid_frontier_assign_keep_utility_batch, include/lipmpc.h: tests/assign_keep_oracle.py's keep phase (its anchor key, its
integer test, its slots) on tests/assign_utility_oracle.py's sources, seeds and fields, ahead of that module's greedy rounds.  A keep
slot's field is a single source, the anchor, that starts at ITS seed; the test compares it with the given utility field.  Composed
from those two modules, tests/gain_oracle.py, tests/assign_oracle.py, tests/field_oracle.py and tests/frontier_oracle.py; it changes
none of them.

TEST INFRASTRUCTURE ONLY: the GPU tests require the device's sub-goals, n_sub, status, path costs, target cells, target gains,
claim rounds, n_claims, kept and n_kept to equal this module's bit for bit.
"""
from __future__ import annotations

import numpy as np

import assign_keep_oracle as KO
import assign_oracle as AO
import assign_utility_oracle as UO
import field_oracle as FO
import frontier_oracle as FR
import gain_oracle as G

INF = FO.INF
FOUND, PATH_OVERFLOW = FR.FOUND, FR.PATH_OVERFLOW
LDS_LIMIT, LDS_SLACK, bitmap_words = FO.LDS_LIMIT, FO.LDS_SLACK, FO.bitmap_words
KEEPU_WORDS = 48


def field_lds_bytes(ncells):
    """Dynamic LDS the kernel asks for with the slot's field in LDS: two bitmaps (impassable, S), 48 words (the keep kernels' 34
    with ufield in the given field's place, four more pointers -- gain, target_gain, n_claims, n_kept -- and six more scalars --
    w_gain, g_cap, r_claim, r_keep, r_inflate, max_claims), the field."""
    return 4 * (2 * bitmap_words(ncells) + KEEPU_WORDS + ncells)


def field_fits_lds(ncells):
    """THE KERNEL'S LDS RULE (its own): 4 (2 (2 ceil(W H / 64) + 2) + 48 + W H) + 256 <= 163840."""
    return field_lds_bytes(ncells) + LDS_SLACK <= LDS_LIMIT


def sizes_at_the_lds_switch(H=193):
    """((W, H) the largest map of H columns whose slot field is kept in LDS, (W + 1, H) the smallest relaxed in ``work``)."""
    W = 2
    while field_fits_lds((W + 1) * H):
        W += 1
    assert field_fits_lds(W * H) and not field_fits_lds((W + 1) * H) and (W + 1) * H <= 1 << 17
    return (W, H), (W + 1, H)


def _write_rows(out, fld, gain_, b, s, k, is_terminal, origin, cell, max_seg, S_max):
    """The winner's rows by the utility winner's path rule on ``fld``, as tests/assign_utility_oracle.py writes them; returns the
    target cell (i, j)."""
    H = fld.shape[1]
    cells = G.descend(fld, s, is_terminal)
    pulled = FO.string_pull(fld, cells, max_seg)
    last = cells[-1]
    if len(pulled) + 1 > S_max:                                   # (nothing written to sub_goals: the path call's rows stay)
        out["status"][b], out["n_sub"][b] = PATH_OVERFLOW, 0
    else:
        new = np.array([FO.centre(p, origin, cell) for p in pulled + [last]]).reshape(-1, 2)
        out["sub_goals"][b] = new
        out["status"][b], out["n_sub"][b] = FOUND, len(new)
    out["path_cost"][b] = np.float64(int(fld[s]) - int(fld[last])) / 5.0
    out["target_cell"][b] = last[0] * H + last[1]
    out["target_gain"][b] = gain_[last]
    out["claim_round"][b] = k
    return last


def assign_keep_utility(frontier, field, gain_, ufield, w_gain, g_cap, min_gain, origin, cell, start, path, r_inflate, r_claim, max_claims,
                        prev_target, r_keep, keep_ratio16, keep_slack, max_seg=None, S_max=64, may_claim=None):
    """The call by its contract.  The arguments of tests/assign_utility_oracle.py's ``assign`` plus ``ufield`` [W,H] (the utility
    field call's output), ``prev_target`` [B] (or None = every robot has none) and the three keep parameters.  Returns its dict plus
    kept [B] int8, n_kept, slots (the relaxations made) and attempts: per keep attempt dict(robot, anchor, entry (or None), cost,
    near, kept)."""
    frontier, field, start = np.asarray(frontier), np.asarray(field), np.asarray(start, np.float64).reshape(-1, 2)
    gain_, ufield = np.asarray(gain_, np.int32), np.asarray(ufield)
    W, H = field.shape
    B = len(start)
    assert 0 <= r_claim <= AO.R_CLAIM_MAX and 0 <= max_claims <= AO.MAX_CLAIMS_MAX
    assert 0 <= w_gain <= G.W_GAIN_MAX and 1 <= g_cap <= G.G_CAP_MAX and 0 <= min_gain <= G.G_CAP_MAX
    assert 0 <= r_keep <= KO.R_KEEP_MAX and KO.KEEP_RATIO_MIN <= keep_ratio16 <= KO.KEEP_RATIO_MAX and 0 <= keep_slack <= KO.KEEP_SLACK_MAX
    max_seg = FO.NO_CAP if max_seg is None else int(max_seg)
    prev = np.full(B, -1, np.int64) if prev_target is None else np.asarray(prev_target, np.int64)
    passable = field != INF
    sources = G.sources(frontier, field, gain_, min_gain)
    may = np.ones(B, bool) if may_claim is None else np.asarray(may_claim) != 0
    out = dict(sub_goals=[np.array(s, np.float64).reshape(-1, 2) for s in path["sub_goals"]], n_sub=np.array(path["n_sub"], np.int32),
               status=np.array(path["status"], np.int32), path_cost=np.array(path["path_cost"], np.float64),
               target_cell=np.array(path["target_cell"], np.int32), target_gain=np.array(path["target_gain"], np.int32),
               claim_round=np.full(B, -1, np.int32), kept=np.zeros(B, np.int8))
    left = [b for b in range(B) if may[b] and out["status"][b] in (FOUND, PATH_OVERFLOW)]
    winners, costs, targets, snapped, n_sources, attempts = [], [], [], [], [], []
    k = slots = 0
    # the keep phase: tests/assign_keep_oracle.py's, on these sources, with the anchor starting at its seed
    for b in list(left):
        if slots >= max_claims:
            break
        c = FO.cell_of(start[b], origin, cell, W, H)
        if c is None or not 0 <= prev[b] < W * H:
            continue
        a = KO.anchor(sources, (int(prev[b]) // H, int(prev[b]) % H), r_keep)
        if a is None:
            continue                                                  # nothing is left of the target: no slot is spent
        slots += 1
        only = np.zeros((W, H), bool)
        only[a] = True
        fld = UO.ufield_of(passable, only, gain_, w_gain, g_cap)
        s, e = FO.snap(fld, c, r_inflate), FO.snap(ufield, c, r_inflate)
        rec = dict(robot=b, anchor=a, entry=s, cost=None if s is None else int(fld[s]), near=None if e is None else int(ufield[e]), kept=False)
        attempts.append(rec)
        if s is None or e is None or not KO.keeps(fld[s], ufield[e], keep_ratio16, keep_slack):
            continue                                                  # the slot is spent all the same
        n_sources.append(int(sources.sum()))
        last = _write_rows(out, fld, gain_, b, s, k, lambda q: q == a, origin, cell, max_seg, S_max)
        assert last == a
        out["kept"][b] = 1
        rec["kept"] = True
        winners.append(b), costs.append(int(fld[s])), targets.append(last), snapped.append(s)
        sources = sources & ~AO.disc(W, H, last, r_claim)
        left.remove(b)
        k += 1
    # the greedy phase: tests/assign_utility_oracle.py's rounds
    while slots < max_claims and left and sources.any():
        fld = UO.ufield_of(passable, sources, gain_, w_gain, g_cap)
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
        n_sources.append(int(sources.sum()))
        last = _write_rows(out, fld, gain_, b, s, k, lambda q: bool(src_k[q]) and int(fld[q]) == G.seed(gain_[q], w_gain, g_cap), origin, cell,
                           max_seg, S_max)
        winners.append(b), costs.append(cost), targets.append(last), snapped.append(s)
        sources = sources & ~AO.disc(W, H, last, r_claim)
        left.remove(b)
        k += 1
        slots += 1
    tc = out["target_cell"]
    out["target"] = np.array([FO.centre((t // H, t % H), origin, cell) if t >= 0 else (np.nan, np.nan) for t in tc]).reshape(-1, 2)
    out.update(n_claims=len(winners), n_kept=int(out["kept"].sum()), winners=winners, costs=costs, targets=targets, snapped=snapped,
               round_sources=n_sources, slots=slots, attempts=attempts)
    return out


def plan_batch(evidence, t_free, t_occ, origin, cell, start, r_claim, r_view, w_gain, g_cap, prev_target, r_keep, keep_ratio16, keep_slack,
               min_gain=0, max_claims=64, r_inflate=2, min_unknown=2, max_seg=None, S_max=64, may_claim=None, gain=None, informed=None):
    """All five calls in numpy on ONE shared map ``evidence`` [W,H]: tests/gain_oracle.py's plan_batch, then ``assign_keep_utility``.
    ``gain`` [W,H]: a hand-written gain in the place of the gain call's; ``informed``: that plan_batch's result when the caller has
    it.  Returns its dict with the winners' rows replaced, plus claim_round, n_claims, kept, n_kept and the slots' records;
    ``informed``: the shared-field plan."""
    ev = np.asarray(evidence)
    assert ev.ndim == 2
    if informed is None:
        informed = G.plan_batch(ev, t_free, t_occ, origin, cell, start, r_view, w_gain, g_cap, min_gain, r_inflate, min_unknown, max_seg,
                                S_max, gain=gain)
    got = assign_keep_utility(informed["frontier"][0], informed["field"][0], informed["gain"][0], informed["ufield"][0], w_gain, g_cap,
                              min_gain, origin, cell, start, informed, r_inflate, r_claim, max_claims, prev_target, r_keep, keep_ratio16,
                              keep_slack, max_seg, S_max, may_claim)
    return dict(informed, **got, informed=informed)
