"""Numpy restatement (float64, int64) of the correlative scan matcher's contract -- lipmpc_scan_match_batch, include/lipmpc.h.

TEST INFRASTRUCTURE ONLY, like tests/map_oracle.py, whose robot cell, window and end point it repeats: the header states the
rule (end point, rotated end point, cell, used pairs, clamped evidence, score, the five selection keys, the acceptance test), this
module evaluates exactly those expressions in the same order, and the GPU tests require every output of the kernel to equal it
bit for bit.
"""
from __future__ import annotations

import numpy as np

import grid_lidar_oracle as G
import map_oracle as M

WINDOW_CELLS = 49152           # cells of the grown window the kernel keeps in LDS, one byte each: larger ones are refused
N_MAX = 16                     # n_x, n_y, n_yaw
CLAMP_MAX = 127


def rot_table(n_yaw, yaw_step):
    """[2 n_yaw + 1, 2]: (cos, sin) of (k - n_yaw) * yaw_step, as the host makes it (numpy); entry n_yaw is (1, 0)."""
    ang = (np.arange(2 * n_yaw + 1) - n_yaw).astype(np.float64) * np.float64(yaw_step)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1)


def grown_window(lidar_range, depth, cell, n_x, n_y):
    mx, my = M.window_half(lidar_range, depth, cell)
    return 2 * (mx + n_x) + 1, 2 * (my + n_y) + 1


def window_fits(lidar_range, depth, cell, n_x, n_y):
    gw, gh = grown_window(lidar_range, depth, cell, n_x, n_y)
    return gw * gh <= WINDOW_CELLS


def end_points(position, hits, depth):
    """(e [R,2], valid [R]): the map update's pushed end points of the readings and its validity tests."""
    hits = np.asarray(hits, np.float64)
    x0, y0, depth = np.float64(position[0]), np.float64(position[1]), np.float64(depth)
    with np.errstate(all="ignore"):
        qx, qy = hits[:, 0], hits[:, 1]
        reading = ~(np.isnan(qx) | np.isnan(qy))
        ddx, ddy = qx - x0, qy - y0
        L = np.sqrt(ddx * ddx + ddy * ddy)
        s = depth / L
        ex, ey = qx + s * ddx, qy + s * ddy
        valid = reading & (L != 0.0) & np.isfinite(L) & np.isfinite(ex) & np.isfinite(ey)
    return np.stack([ex, ey], axis=1), valid


def used_cells(position, hits, origin, cell, lidar_range, depth, rot=None, n_yaw=0):
    """Per yaw index k the grid cells (i, j) of the USED pairs (r, k): a list of T int64 arrays [n_k,2], in the order of the
    readings, or None when the robot cannot be given a cell."""
    c0 = G.robot_cell(position, origin, cell)
    if c0 is None:
        return None
    e, valid = end_points(position, hits, depth)
    x0, y0 = np.float64(position[0]), np.float64(position[1])
    ox, oy, dx, dy = (np.float64(v) for v in (origin[0], origin[1], cell[0], cell[1]))
    mx, my = M.window_half(lidar_range, depth, cell)
    fi, fj = np.float64(c0[0]), np.float64(c0[1])
    out = []
    for k in range(2 * n_yaw + 1):
        with np.errstate(all="ignore"):
            if k == n_yaw:
                x, y = e[:, 0], e[:, 1]                       # the end point itself, no arithmetic
            else:
                c, s = np.float64(rot[k][0]), np.float64(rot[k][1])
                rx, ry = e[:, 0] - x0, e[:, 1] - y0
                x, y = x0 + (c * rx - s * ry), y0 + (s * rx + c * ry)
            hi, hj = np.floor((x - ox) / dx) - fi, np.floor((y - oy) / dy) - fj
            used = valid & (np.abs(hi) <= mx) & (np.abs(hj) <= my)
        out.append(np.stack([c0[0] + hi[used].astype(np.int64), c0[1] + hj[used].astype(np.int64)], axis=1))
    return out


def scores(cells, evidence, n_x, n_y, clamp):
    """score [T, 2 n_x + 1, 2 n_y + 1] int64 of the used cells of ``used_cells`` on ``evidence`` [W,H]: V = the evidence clamped
    to +-clamp inside the map, 0 outside; score(k, a, b) = sum over the used pairs of V(i + a, j + b)."""
    W, H = evidence.shape
    V = np.clip(evidence.astype(np.int64), -int(clamp), int(clamp))
    out = np.zeros((len(cells), 2 * n_x + 1, 2 * n_y + 1), np.int64)
    for k, ck in enumerate(cells):
        for i, j in ck:
            # rows i - n_x .. i + n_x, columns j - n_y .. j + n_y, the part inside the map
            a0, a1 = max(-n_x, -int(i)), min(n_x, W - 1 - int(i))
            b0, b1 = max(-n_y, -int(j)), min(n_y, H - 1 - int(j))
            if a0 <= a1 and b0 <= b1:
                out[k, a0 + n_x:a1 + n_x + 1, b0 + n_y:b1 + n_y + 1] += V[i + a0:i + a1 + 1, j + b0:j + b1 + 1]
    return out


def select(score, n_x, n_y, n_yaw):
    """(k, a, b) minimising (-score, a * a + b * b, |k - n_yaw|, k, (a + n_x)(2 n_y + 1) + (b + n_y)) lexicographically."""
    k, a, b = (v.ravel() for v in np.meshgrid(np.arange(score.shape[0]), np.arange(-n_x, n_x + 1), np.arange(-n_y, n_y + 1),
                                              indexing="ij"))
    idx = (a + n_x) * (2 * n_y + 1) + (b + n_y)
    first = np.lexsort((idx, k, np.abs(k - n_yaw), a * a + b * b, -score.astype(np.int64).ravel()))[0]      # last key sorts first
    return int(k[first]), int(a[first]), int(b[first])


def match_one(position, hits, evidence, origin, cell, lidar_range, depth, n_x, n_y, clamp, min_score, min_gain, rot=None, n_yaw=0):
    """One robot: dict(offset_cells (a, b), yaw_index, offset (2 doubles), score (best, zero), n_used, matched)."""
    zero = dict(offset_cells=(0, 0), yaw_index=0, offset=(np.float64(0.0), np.float64(0.0)), score=(0, 0), n_used=0, matched=0)
    cells = used_cells(position, hits, origin, cell, lidar_range, depth, rot, n_yaw)
    if cells is None:
        return zero
    sc = scores(cells, np.asarray(evidence), n_x, n_y, clamp)
    k, a, b = select(sc, n_x, n_y, n_yaw)
    s_best, s_zero = int(sc[k, a + n_x, b + n_y]), int(sc[n_yaw, n_x, n_y])
    accepted = s_best >= int(min_score) and s_best - s_zero >= int(min_gain)
    if not accepted:
        k, a, b = n_yaw, 0, 0
    return dict(offset_cells=(a, b), yaw_index=k - n_yaw, offset=(np.float64(a) * np.float64(cell[0]), np.float64(b) * np.float64(cell[1])),
                score=(s_best, s_zero), n_used=len(cells[n_yaw]), matched=int(accepted and (a != 0 or b != 0 or k != n_yaw)))


def match(positions, hits, evidence, origin, cell, lidar_range, depth, n_x, n_y, clamp, min_score, min_gain, n_yaw=0, yaw_step=None,
          mask=None, rot=None):
    """lipmpc_scan_match_batch in numpy: positions [B,2], hits [B,R,2], evidence [W,H] (shared) or [B,W,H].  Returns the outputs
    as arrays of the call's own types: offset_cells [B,2] int32, yaw_index [B] int32, offset [B,2] float64, score [B,2] int32,
    n_used [B] int32, matched [B] int8."""
    B = len(positions)
    if rot is None and n_yaw > 0:
        rot = rot_table(n_yaw, yaw_step)
    evidence = np.asarray(evidence)
    out = dict(offset_cells=np.zeros((B, 2), np.int32), yaw_index=np.zeros(B, np.int32), offset=np.zeros((B, 2), np.float64),
               score=np.zeros((B, 2), np.int32), n_used=np.zeros(B, np.int32), matched=np.zeros(B, np.int8))
    for b in range(B):
        if mask is not None and mask[b] == 0:
            continue
        ev = evidence if evidence.ndim == 2 else evidence[b]
        r = match_one(positions[b], hits[b], ev, origin, cell, lidar_range, depth, n_x, n_y, clamp, min_score, min_gain, rot, n_yaw)
        for name, v in r.items():
            out[name][b] = v
    return out
