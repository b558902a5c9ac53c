"""Numpy restatement (float64, int64) of the scan integration's contract -- lipmpc_map_update_batch, include/lipmpc.h -- and of
the goal-selection rule of UnknownEnvFleet.run_replanning.

TEST INFRASTRUCTURE ONLY, like tests/grid_lidar_oracle.py, whose robot cell and march it repeats with the map's end points: the
header states the arithmetic (end point, hit cell, march, window, one update per cell), this module evaluates exactly those
expressions in the same order, and the GPU tests require the kernel's evidence to equal it integer for integer.
"""
from __future__ import annotations

import math

import numpy as np

import grid_lidar_oracle as G

WINDOW_CELLS = 49152           # cells of the window the kernel keeps (twice) in LDS: larger windows are refused by the library
LDS_BYTES = 2 * WINDOW_CELLS // 8
RRT_FOUND = 0


def default_depth(cell):
    return 0.5 * min(float(cell[0]), float(cell[1]))


def window_half(lidar_range, depth, cell):
    """(nx, ny): only cells within this many columns / rows of the robot's cell are updated."""
    reach = np.float64(lidar_range) + np.float64(depth)
    return int(math.floor(reach / np.float64(cell[0]))) + 2, int(math.floor(reach / np.float64(cell[1]))) + 2


def window_fits(lidar_range, depth, cell):
    nx, ny = window_half(lidar_range, depth, cell)
    return (2 * nx + 1) * (2 * ny + 1) <= WINDOW_CELLS


def robot_marks(position, hits, origin, cell, lidar_range, table, depth, counts=False):
    """One robot's scan as window bitmaps: (passed [ww,wh], hit [ww,wh], (wi0, wj0)) with window cell (li, lj) = grid cell
    (wi0 + li, wj0 + lj), or None when the robot cannot be given a cell.  ``hits`` [R,2], NaN = no reading.  ``counts``: a fourth
    value, dict(ties = steps of live rays taken with t_x == t_y, t0 = live rays whose first crossing has t == 0); the first three
    are the same either way."""
    c0 = G.robot_cell(position, origin, cell)
    if c0 is None:
        return None
    hits = np.asarray(hits, np.float64)
    table = np.asarray(table, np.float64)
    R = len(table)
    x0, y0 = np.float64(position[0]), np.float64(position[1])
    ox, oy, dx, dy = (np.float64(v) for v in (origin[0], origin[1], cell[0], cell[1]))
    rng, depth = np.float64(lidar_range), np.float64(depth)
    nx, ny = window_half(lidar_range, depth, cell)
    ww, wh = 2 * nx + 1, 2 * ny + 1
    passed, hit = np.zeros((ww, wh), bool), np.zeros((ww, wh), bool)
    fi, fj = np.float64(c0[0]), np.float64(c0[1])
    with np.errstate(all="ignore"):
        qx, qy = hits[:, 0], hits[:, 1]
        reading = ~(np.isnan(qx) | np.isnan(qy))
        ddx, ddy = qx - x0, qy - y0
        L = np.sqrt(ddx * ddx + ddy * ddy)
        s = depth / L
        ex = np.where(reading, qx + s * ddx, x0 + rng * table[:, 0])
        ey = np.where(reading, qy + s * ddy, y0 + rng * table[:, 1])
        use = ~reading | ((L != 0.0) & np.isfinite(L) & np.isfinite(ex) & np.isfinite(ey))
        hi, hj = np.floor((ex - ox) / dx) - fi, np.floor((ey - oy) / dy) - fj
        has_hit = reading & use & (np.abs(hi) <= nx) & (np.abs(hj) <= ny)
        hli = np.where(has_hit, hi + nx, -1).astype(np.int64)
        hlj = np.where(has_hit, hj + ny, -1).astype(np.int64)
        rdx, rdy = ex - x0, ey - y0
        ivx, ivy = 1.0 / rdx, 1.0 / rdy
        upx, upy = (rdx > 0).astype(np.int64), (rdy > 0).astype(np.int64)
        ci, cj = np.full(R, c0[0], np.int64), np.full(R, c0[1], np.int64)
        tx = np.where(rdx != 0, ((ox + (ci + upx).astype(np.float64) * dx) - x0) * ivx, np.inf)
        ty = np.where(rdy != 0, ((oy + (cj + upy).astype(np.float64) * dy) - y0) * ivy, np.inf)
        live = use.copy()
        own = live & ~((hli == nx) & (hlj == ny))
        if own.any():
            passed[nx, ny] = True
        n, first = dict(ties=0, t0=0), True
        while live.any():
            xs = tx <= ty                                   # a tie goes to x
            t = np.where(xs, tx, ty)
            n["ties"] += int((live & (tx == ty) & np.isfinite(tx)).sum())
            n["t0"] += int((live & (t == 0.0)).sum()) if first else 0
            first = False
            ci = np.where(live & xs, ci + 2 * upx - 1, ci)
            cj = np.where(live & ~xs, cj + 2 * upy - 1, cj)
            tnx = ((ox + (ci + upx).astype(np.float64) * dx) - x0) * ivx
            tny = ((oy + (cj + upy).astype(np.float64) * dy) - y0) * ivy
            tx = np.where(live & xs, tnx, tx)
            ty = np.where(live & ~xs, tny, ty)
            ri, rj = ci - c0[0] + nx, cj - c0[1] + ny
            go = live & (t <= 1.0) & (ri >= 0) & (ri < ww) & (rj >= 0) & (rj < wh) & ~((ri == hli) & (rj == hlj))
            passed[ri[go], rj[go]] = True
            live = go
        hit[hli[has_hit], hlj[has_hit]] = True
    return (passed, hit, (c0[0] - nx, c0[1] - ny)) + ((n,) if counts else ())


def robot_delta(position, hits, W, H, origin, cell, lidar_range, table, depth, w_hit, w_miss):
    """(delta [W,H] int64, hit [W,H] bool, passed [W,H] bool) of one robot's scan: + w_hit on its hit cells, - w_miss on the
    cells otherwise passed, cells outside the grid ignored."""
    hit_g, pas_g = np.zeros((W, H), bool), np.zeros((W, H), bool)
    m = robot_marks(position, hits, origin, cell, lidar_range, table, depth)
    if m is not None:
        passed, hit, (wi0, wj0) = m
        ww, wh = passed.shape
        i0, i1, j0, j1 = max(wi0, 0), min(wi0 + ww, W), max(wj0, 0), min(wj0 + wh, H)
        if i0 < i1 and j0 < j1:
            hit_g[i0:i1, j0:j1] = hit[i0 - wi0:i1 - wi0, j0 - wj0:j1 - wj0]
            pas_g[i0:i1, j0:j1] = passed[i0 - wi0:i1 - wi0, j0 - wj0:j1 - wj0] & ~hit_g[i0:i1, j0:j1]
    return np.where(hit_g, int(w_hit), 0).astype(np.int64) - np.where(pas_g, int(w_miss), 0), hit_g, pas_g


def update(evidence, positions, hits, origin, cell, lidar_range, table, depth=None, w_hit=3, w_miss=1, mask=None):
    """lipmpc_map_update_batch in numpy: ``evidence`` [W,H] (shared) or [B,W,H], updated in place and returned.
    positions [B,2], hits [B,R,2]."""
    depth = default_depth(cell) if depth is None else depth
    W, H = evidence.shape[-2:]
    for b in range(len(positions)):
        if mask is not None and mask[b] == 0:
            continue
        d = robot_delta(positions[b], hits[b], W, H, origin, cell, lidar_range, table, depth, w_hit, w_miss)[0]
        if evidence.ndim == 2:
            evidence += d.astype(evidence.dtype)
        else:
            evidence[b] += d.astype(evidence.dtype)
    return evidence


def oracle_hits(positions, occ, origin, cell, lidar_range, table, noise=None):
    """hits [B,R,2] as the grid scan writes them (tests/grid_lidar_oracle.py), NaN = no reading."""
    out = np.full((len(positions), len(table), 2), np.nan)
    for b, p in enumerate(positions):
        h, valid = G.grid_hits(p, occ, origin, cell, lidar_range, table)
        if noise is not None:
            h = h + noise[b]
        out[b, valid] = h[valid]
    return out


def select_goals(position, goal, sub_goals, n_sub, status, lookahead):
    """THE GOAL-SELECTION RULE of run_replanning: robot b's working goal is the first sub-goal of its path that is at least
    ``lookahead`` from the robot (sqrt(dx*dx + dy*dy) >= lookahead); the final goal when none is, or when the plan's status is
    anything other than FOUND.  position, goal [B,2]; sub_goals [B,S,2]; n_sub, status [B].  Returns [B,2]."""
    position, goal = np.asarray(position, np.float64), np.asarray(goal, np.float64)
    out = goal.copy()
    for b in range(len(goal)):
        if status[b] != RRT_FOUND:
            continue
        for s in range(int(n_sub[b])):
            dx, dy = sub_goals[b, s, 0] - position[b, 0], sub_goals[b, s, 1] - position[b, 1]
            if np.sqrt(dx * dx + dy * dy) >= lookahead:
                out[b] = sub_goals[b, s]
                break
    return out
