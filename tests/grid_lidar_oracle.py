"""Numpy restatement (float64) of the grid scan's contract -- lipmpc_lidar_grid_c_eta_batch, include/lipmpc.h.

TEST INFRASTRUCTURE ONLY, like tests/rrt_oracle.py: the header states the arithmetic (start cell, boundary crossings, the tie
rule, the stop rule, the placement of the reading), this module evaluates exactly those expressions in the same order, and
the GPU tests require the kernel's hits to equal it bit for bit.  numpy evaluates every operation in IEEE double without
contraction; division and square root are correctly rounded.
"""
from __future__ import annotations

import math

import numpy as np

WINDOW_CELLS = 49152           # cells of the window the kernel stages in LDS: larger windows are refused by the library


def window_half(lidar_range, cell):
    """(nx, ny): a ray is followed at most this many columns / rows from the robot's cell."""
    return int(math.floor(lidar_range / cell[0])) + 2, int(math.floor(lidar_range / cell[1])) + 2


def window_fits(lidar_range, cell):
    nx, ny = window_half(lidar_range, cell)
    return (2 * nx + 1) * (2 * ny + 1) <= WINDOW_CELLS


def robot_cell(position, origin, cell):
    """(ci, cj) or None when the robot cannot be given a cell (index of 2^30 or more in magnitude, NaN)."""
    with np.errstate(invalid="ignore", over="ignore"):
        fi = np.floor((np.float64(position[0]) - np.float64(origin[0])) / np.float64(cell[0]))
        fj = np.floor((np.float64(position[1]) - np.float64(origin[1])) / np.float64(cell[1]))
    if not (abs(fi) < 2.0 ** 30 and abs(fj) < 2.0 ** 30):
        return None
    return int(fi), int(fj)


def in_solid_cell(position, occ, origin, cell):
    c = robot_cell(position, origin, cell)
    W, H = occ.shape
    return c is not None and 0 <= c[0] < W and 0 <= c[1] < H and bool(occ[c[0], c[1]])


def grid_hits(position, occ, origin, cell, lidar_range, table, counts=False):
    """(hits [R,2], valid [R]) of one robot on the grid ``occ`` [W,H] (nonzero = solid): per ray the point where it enters the
    first solid cell -- on the boundary crossed, the other coordinate that of x0 + t d --, kept if strictly closer than
    lidar_range.  A robot in a solid cell has no scan (all invalid).  ``counts``: a third value, dict(ties = steps of live rays
    taken with t_x == t_y, t0 = live rays whose first crossing has t == 0); the first two are the same either way."""
    occ = np.asarray(occ) != 0
    W, H = occ.shape
    R = len(table)
    x0, y0 = np.float64(position[0]), np.float64(position[1])
    ox, oy, dx, dy = (np.float64(v) for v in (origin[0], origin[1], cell[0], cell[1]))
    rng = np.float64(lidar_range)
    hits, valid = np.zeros((R, 2)), np.zeros(R, bool)
    n = dict(ties=0, t0=0)
    c0 = robot_cell(position, origin, cell)
    if c0 is None or in_solid_cell(position, occ, origin, cell):
        return (hits, valid, n) if counts else (hits, valid)
    nx, ny = window_half(lidar_range, cell)
    table = np.asarray(table, np.float64)
    with np.errstate(all="ignore"):
        ex, ey = x0 + rng * table[:, 0], y0 + rng * table[:, 1]
        ddx, ddy = ex - x0, ey - y0
        ivx, ivy = 1.0 / ddx, 1.0 / ddy
        upx, upy = (ddx > 0).astype(np.int64), (ddy > 0).astype(np.int64)
        ci, cj = np.full(R, c0[0], np.int64), np.full(R, c0[1], np.int64)
        tx = np.where(ddx != 0, ((ox + (ci + upx).astype(np.float64) * dx) - x0) * ivx, np.inf)
        ty = np.where(ddy != 0, ((oy + (cj + upy).astype(np.float64) * dy) - y0) * ivy, np.inf)
        live = np.ones(R, bool)
        t_hit = np.zeros(R)
        b_hit, x_hit = np.zeros(R), np.zeros(R, bool)     # the boundary the solid cell was entered through, and its axis
        found = np.zeros(R, bool)
        first = True
        while live.any():
            xs = tx <= ty                                   # a tie goes to x
            t = np.where(xs, tx, ty)
            n["ties"] += int((live & (tx == ty) & np.isfinite(tx)).sum())
            n["t0"] += int((live & (t == 0.0)).sum()) if first else 0
            first = False
            bnd = np.where(xs, ox + (ci + upx).astype(np.float64) * dx, oy + (cj + upy).astype(np.float64) * dy)      # the one being crossed
            ci = np.where(live & xs, ci + 2 * upx - 1, ci)
            cj = np.where(live & ~xs, cj + 2 * upy - 1, cj)
            tnx = ((ox + (ci + upx).astype(np.float64) * dx) - x0) * ivx
            tny = ((oy + (cj + upy).astype(np.float64) * dy) - y0) * ivy
            tx = np.where(live & xs, tnx, tx)
            ty = np.where(live & ~xs, tny, ty)
            go = live & (t <= 1.0) & (np.abs(ci - c0[0]) <= nx) & (np.abs(cj - c0[1]) <= ny)
            ins = go & (ci >= 0) & (ci < W) & (cj >= 0) & (cj < H)
            sol = np.zeros(R, bool)
            sol[ins] = occ[ci[ins], cj[ins]]
            t_hit = np.where(sol, t, t_hit)
            b_hit, x_hit = np.where(sol, bnd, b_hit), np.where(sol, xs, x_hit)
            found |= sol
            live = go & ~sol
        qx, qy = np.where(x_hit, b_hit, x0 + t_hit * ddx), np.where(x_hit, y0 + t_hit * ddy, b_hit)
        dist = np.sqrt((qx - x0) * (qx - x0) + (qy - y0) * (qy - y0))
    valid = found & (dist < rng)
    hits[valid, 0], hits[valid, 1] = qx[valid], qy[valid]
    return (hits, valid, n) if counts else (hits, valid)


def fixture(seed=0, n_robots=60):
    """The cell-aligned fixture of the grid tests: a 200 x 200 grid of 0.05 m cells at (-1, -1) with axis-aligned boxes (kept
    only if the box grown by 2 cells is empty), the same boxes as vertex rings, and robots whose 3 x 3 cells are free.
    Returns dict(occ, origin, cell, rings, pos, lidar_range, resolution)."""
    rng = np.random.default_rng(seed)
    W = H = 200
    cell, ox, oy = 0.05, -1.0, -1.0
    occ = np.zeros((W, H), np.uint8)
    rings = []
    for _ in range(14):
        a, b = (int(v) for v in rng.integers(10, 170, 2))
        w, h = (int(v) for v in rng.integers(4, 30, 2))
        if occ[max(a - 2, 0):a + w + 2, max(b - 2, 0):b + h + 2].any():
            continue
        occ[a:a + w, b:b + h] = 1
        x_lo, x_hi, y_lo, y_hi = ox + a * cell, ox + (a + w) * cell, oy + b * cell, oy + (b + h) * cell
        rings.append(np.array([[x_lo, y_lo], [x_hi, y_lo], [x_hi, y_hi], [x_lo, y_hi]]))
    pos = []
    while len(pos) < n_robots:
        p = rng.uniform(0, 8, 2)
        i, j = int(math.floor((p[0] - ox) / cell)), int(math.floor((p[1] - oy) / cell))
        if not occ[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2].any():
            pos.append(p)
    return dict(occ=occ, origin=(ox, oy), cell=(cell, cell), rings=rings, pos=np.array(pos), lidar_range=1.5, resolution=360)
