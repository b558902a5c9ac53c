"""Numpy / plain-Python restatement of the informed explorer's three contracts -- lipmpc_grid_frontier_gain_batch,
lipmpc_grid_frontier_utility_field_batch and lipmpc_grid_frontier_utility_path_batch, include/lipmpc.h: the gain as the size of a
set of cells, the utility field by seeded multi-source Dijkstra (heapq, Python ints), and the paths by tests/field_oracle.py's
snap, line of sight and string pulling with the terminal test in the descent.

TEST INFRASTRUCTURE ONLY, like tests/frontier_oracle.py: the GPU tests require the device's gain, ufield, n_sources, statuses,
sub-goals, path costs, target cells and target gains to equal this module's bit for bit.
"""
from __future__ import annotations

import heapq

import numpy as np

import field_oracle as FO
import frontier_oracle as FR

INF, NO_CAP = FO.INF, FO.NO_CAP
FOUND, NO_PATH, START_OCCUPIED, PATH_OVERFLOW, OUTSIDE_GRID = FO.FOUND, FO.NO_PATH, FO.START_OCCUPIED, FO.PATH_OVERFLOW, FO.OUTSIDE_GRID
R_VIEW_MAX, W_GAIN_MAX, G_CAP_MAX = 64, 65535, 16384
LDS_LIMIT, LDS_SLACK, bitmap_words = FO.LDS_LIMIT, FO.LDS_SLACK, FO.bitmap_words
OPEN_MAP_GAINS = {1: 4, 2: 12, 3: 28, 5: 80, 8: 196, 13: 528, 30: 2820, 64: 12852}      # the disc's cell count minus one


def ufield_lds_bytes(ncells):
    """Dynamic LDS the utility field kernel asks for with the field in LDS: one bitmap, the source count's word pair, the field."""
    return 4 * (bitmap_words(ncells) + 2 + ncells)


def field_fits_lds(ncells):
    """THE UTILITY FIELD KERNEL'S LDS RULE (its own, not the frontier kernel's): the field, 4 bytes a cell, beside one bitmap
    (impassable), the source count's word pair and the reduction's slack within the 160 KiB of a workgroup."""
    return ufield_lds_bytes(ncells) + LDS_SLACK <= LDS_LIMIT


def sizes_at_the_lds_switch(H=193):
    """((W, H) the largest map of H columns whose utility field is kept in LDS, (W + 1, H) the smallest relaxed in the output)."""
    W = 2
    while field_fits_lds((W + 1) * H):
        W += 1
    assert field_fits_lds(W * H) and not field_fits_lds((W + 1) * H) and (W + 1) * H <= 1 << 17
    return (W, H), (W + 1, H)


def ray_offsets(r):
    """(a, b) [8 r, r] int64: per end cell (max(|di|, |dj|) == r) the offsets floor((2 k d + r) / (2 r)), k = 1..r (numpy's //
    floors toward minus infinity)."""
    r = int(r)
    assert 1 <= r <= R_VIEW_MAX
    ends = [(di, dj) for di in range(-r, r + 1) for dj in range(-r, r + 1) if max(abs(di), abs(dj)) == r]
    assert len(ends) == 8 * r
    d = np.array(ends, np.int64)
    k = np.arange(1, r + 1, dtype=np.int64)[None, :]
    return (2 * k * d[:, :1] + r) // (2 * r), (2 * k * d[:, 1:] + r) // (2 * r)


def gain(evidence, t_free, t_occ, frontier, r_view):
    """gain [W,H] int32 of one map by the contract: 0 off the given frontier, else the number of distinct unknown cells the fan
    visits before each ray ends (outside the disc, outside the grid, or solid)."""
    solid, _, unknown = FR.classes(evidence, t_free, t_occ)
    W, H = solid.shape
    r = int(r_view)
    a, b = ray_offsets(r)
    in_disc = a * a + b * b <= r * r
    out = np.zeros((W, H), np.int32)
    for i, j in zip(*np.nonzero(np.asarray(frontier) != 0)):
        ci, cj = i + a, j + b
        inside = in_disc & (ci >= 0) & (ci < W) & (cj >= 0) & (cj < H)
        cci, ccj = np.clip(ci, 0, W - 1), np.clip(cj, 0, H - 1)
        going = np.logical_and.accumulate(inside & ~solid[cci, ccj], axis=1)       # a ray ends BEFORE the first k that stops it
        seen = going & unknown[cci, ccj]
        out[i, j] = len(set((cci[seen] * H + ccj[seen]).tolist()))
    return out


def seed(g, w_gain, g_cap):
    return (int(w_gain) * (int(g_cap) - min(max(int(g), 0), int(g_cap)))) >> 4


def sources(frontier, field, gain_, min_gain):
    """source(c) <=> frontier[c] != 0 and passable(c) and gain[c] >= min_gain (as stored)."""
    return (np.asarray(frontier) != 0) & (np.asarray(field) != INF) & (np.asarray(gain_).astype(np.int64) >= int(min_gain))


def ufield(frontier, field, gain_, w_gain, g_cap, min_gain):
    """(ufield [W,H] uint32, n_sources) of one map: Dijkstra from every source at once, each starting at its seed."""
    assert 0 <= w_gain <= W_GAIN_MAX and 1 <= g_cap <= G_CAP_MAX and 0 <= min_gain <= G_CAP_MAX
    blocked = np.asarray(field) == INF
    src = sources(frontier, field, gain_, min_gain)
    W, H = blocked.shape
    out = np.full((W, H), INF, np.uint32)
    dist = {(int(i), int(j)): seed(gain_[i, j], w_gain, g_cap) for i, j in zip(*np.nonzero(src))}
    heap = [(d, i, j) for (i, j), d in dist.items()]
    heapq.heapify(heap)
    while heap:
        d, i, j = heapq.heappop(heap)
        if d > dist[(i, j)]:
            continue
        for p, q, c in FO.moves_from(blocked, i, j):
            if d + c < dist.get((p, q), 1 << 62):
                dist[(p, q)] = d + c
                heapq.heappush(heap, (d + c, p, q))
    for (i, j), d in dist.items():
        assert d < 7 * (1 << 17) + (1 << 26)
        out[i, j] = d
    return out, int(src.sum())


def terminal(c, frontier, gain_, ufld, w_gain, g_cap, min_gain):
    """terminal(c) <=> source(c) and ufield[c] == seed(c)  (a finite ufield says passable)."""
    return bool(frontier[c] != 0 and ufld[c] != INF and int(gain_[c]) >= min_gain and int(ufld[c]) == seed(gain_[c], w_gain, g_cap))


def descend(ufld, c, is_terminal, strict=True):
    """The path cells from c to the FIRST terminal cell: the terminal test first, then the first neighbour in MOVES order with
    ufield[n] + cost == ufield[c], side cells of a diagonal judged by ``passable``.  No such neighbour: AssertionError, or None with
    ``strict=False`` (the contract's LIPMPC_RRT_NO_PATH)."""
    W, H = ufld.shape
    path = [c]
    while not is_terminal(c):
        i, j = c
        for di, dj in FO.MOVES:
            a, b = i + di, j + dj
            if not (0 <= a < W and 0 <= b < H) or ufld[a, b] == INF:
                continue
            if di and dj and (ufld[a, j] == INF or ufld[i, b] == INF):
                continue
            if int(ufld[a, b]) + (FO.DIAGONAL if di and dj else FO.AXIAL) == int(ufld[c]):
                c = (a, b)
                break
        else:
            if not strict:
                return None
            raise AssertionError(f"no descent from {c}: not a utility field")
        path.append(c)
    return path


def plan(evidence, t_occ, frontier, gain_, ufld, n_sources, w_gain, g_cap, min_gain, origin, cell, start, r_inflate=2, max_seg=None,
         S_max=64, strict=True):
    """One robot by the contract of lipmpc_grid_frontier_utility_path_batch.  Returns dict(status, n_sub, sub_goals [n_sub,2],
    path_cost, target_cell, target_gain, cells (the descent), snapped)."""
    ev = np.asarray(evidence)
    W, H = ev.shape
    max_seg = NO_CAP if max_seg is None else int(max_seg)
    out = dict(status=None, n_sub=0, sub_goals=np.zeros((0, 2)), path_cost=float("nan"), target_cell=-1, target_gain=-1, cells=[],
               snapped=None)
    c = FO.cell_of(start, origin, cell, W, H)
    if c is None:
        out["status"] = OUTSIDE_GRID
    elif int(ev[c]) >= int(t_occ):
        out["status"] = START_OCCUPIED
    elif n_sources == 0:
        out["status"] = NO_PATH
    if out["status"] is not None:
        return out
    s = FO.snap(ufld, c, r_inflate)
    if s is None:
        out["status"] = NO_PATH
        return out
    path = descend(ufld, s, lambda q: terminal(q, frontier, gain_, ufld, w_gain, g_cap, min_gain), strict)
    if path is None:
        out.update(status=NO_PATH, snapped=s)
        return out
    pulled = FO.string_pull(ufld, path, max_seg)
    last = path[-1]
    out.update(cells=path, snapped=s, path_cost=float(np.float64(int(ufld[s]) - int(ufld[last])) / 5.0), target_cell=last[0] * H + last[1],
               target_gain=int(gain_[last]))
    if len(pulled) + 1 > S_max:
        out["status"] = PATH_OVERFLOW
        return out
    sub = np.array([FO.centre(p, origin, cell) for p in pulled + [last]]).reshape(-1, 2)
    out.update(status=FOUND, n_sub=len(sub), sub_goals=sub)
    return out


def plan_batch(evidence, t_free, t_occ, origin, cell, start, r_view, w_gain, g_cap, min_gain=0, r_inflate=2, min_unknown=2, max_seg=None,
               S_max=64, gain=None, nearest=None, strict=True):
    """All four calls in numpy.  ``evidence`` [W,H] (shared: F = 1) or [F,W,H] with F = 1 or B; ``start`` [B,2].  ``gain`` [F,W,H]: a
    hand-written gain in the place of the gain call's; ``nearest``: frontier_oracle.plan_batch of the same arguments where the
    caller has it.  Returns dict(field, frontier, n_frontier (the nearest-frontier ones), gain, ufield [F,W,H], n_sources [F],
    sub_goals (list of [n,2]), n_sub, status, path_cost, target_cell, target_gain [B], target [B,2], cells (list), nearest)."""
    ev, start = np.asarray(evidence), np.asarray(start, np.float64).reshape(-1, 2)
    ev = ev if ev.ndim == 3 else ev[None]
    F, B = len(ev), len(start)
    assert F in (1, B)
    if nearest is None:
        nearest = FR.plan_batch(ev, t_free, t_occ, origin, cell, start, r_inflate, min_unknown, max_seg, S_max)
    this = globals()["gain"]
    gains = np.stack([this(ev[f], t_free, t_occ, nearest["frontier"][f], r_view) for f in range(F)]) if gain is None else \
        np.asarray(gain, np.int32).reshape(ev.shape)
    uf = [ufield(nearest["frontier"][f], nearest["field"][f], gains[f], w_gain, g_cap, min_gain) for f in range(F)]
    res = []
    for b in range(B):
        f = 0 if F == 1 else b
        res.append(plan(ev[f], t_occ, nearest["frontier"][f], gains[f], uf[f][0], uf[f][1], w_gain, g_cap, min_gain, origin, cell, start[b],
                        r_inflate, max_seg, S_max, strict))
    H = ev.shape[2]
    tc = np.array([r["target_cell"] for r in res], np.int32)
    target = np.array([FO.centre((t // H, t % H), origin, cell) if t >= 0 else (np.nan, np.nan) for t in tc]).reshape(-1, 2)
    return dict(field=nearest["field"], frontier=nearest["frontier"], n_frontier=nearest["n_frontier"], gain=gains,
                ufield=np.stack([u for u, _ in uf]), n_sources=np.array([n for _, n in uf], np.int32),
                sub_goals=[r["sub_goals"] for r in res], n_sub=np.array([r["n_sub"] for r in res], np.int32),
                status=np.array([r["status"] for r in res], np.int32), path_cost=np.array([r["path_cost"] for r in res]),
                target_cell=tc, target_gain=np.array([r["target_gain"] for r in res], np.int32), target=target,
                cells=[r["cells"] for r in res], nearest=nearest)
