"""Numpy restatement of the sector split of the LiDAR front end -- lipmpc_lidar_c_eta_split_batch /
lipmpc_lidar_grid_c_eta_split_batch, include/lipmpc.h.

TEST INFRASTRUCTURE ONLY, like tests/grid_lidar_oracle.py: the header states the rule (gaps, anchor, offsets, extent, piece count,
piece of a reading), this module evaluates it in Python integers, and the GPU tests require the kernel's pieces to equal it bit
for bit.  Rings come from oracle/lidar_oracle.py::hull_ring per piece, exactly as the unsplit chain takes them per cluster.
"""
from __future__ import annotations

import numpy as np

import lidar_oracle as L

MAX_PIECES = 64                # pieces the kernel stages: more set overflow


def cluster_pieces(rays, split_rays, R):
    """(piece of every reading, piece count, anchor) of ONE cluster whose readings lie on the rays ``rays`` (ascending)."""
    rays = [int(r) for r in rays]
    n = len(rays)
    assert n >= 1 and all(a < b for a, b in zip(rays, rays[1:])) and 0 <= rays[0] and rays[-1] < R
    if n == 1:
        gaps = [R]
    else:
        gaps = [(rays[t] - rays[t - 1]) % R for t in range(n)]          # rays[-1] is r_n: the first gap looks back across ray 0
    g_max = max(gaps)
    anchor = min(r for r, g in zip(rays, gaps) if g == g_max)
    offs = [(r - anchor) % R for r in rays]
    extent = max(offs) + 1
    n_p = -(-extent // split_rays)
    return [o * n_p // extent for o in offs], n_p, anchor


def piece_ids(rays, labels, split_rays, R):
    """Piece number of every reading: ``rays`` [n] ascending ray indices of a scan's readings, ``labels`` [n] their DBSCAN labels
    (-1 noise).  -1 for noise, else the piece's number: clusters in label order, inside a cluster by ascending p.  Returns
    (pieces [n], number of pieces).  ``split_rays`` = 0: every cluster is one piece."""
    rays, labels = np.asarray(rays, int), np.asarray(labels, int)
    out = np.full(len(rays), -1, int)
    base = 0
    for k in range(labels.max() + 1 if len(labels) else 0):
        idx = np.nonzero(labels == k)[0]
        if split_rays > 0:
            p, n_p, _ = cluster_pieces(rays[idx], split_rays, R)
        else:
            p, n_p = [0] * len(idx), 1
        out[idx] = base + np.asarray(p, int)
        base += n_p
    return out, base


def split_scan(hits, valid, split_rays, n_obs_max, v_max, eps=L.DBSCAN_EPS, min_samples=L.DBSCAN_MIN_SAMPLES):
    """What a split scan makes of the readings ``hits`` [R,2] / ``valid`` [R]: dict(labels [R], pieces [R] (-2 no reading, -1
    noise), n_pieces, rings (the hull of every piece that has one, piece order), overflow).  When overflow is set because more
    than 64 pieces exist nothing else is defined about the slots (rings = None)."""
    R = len(hits)
    rays = np.nonzero(valid)[0]
    pts = np.asarray(hits)[valid]
    labels = L.dbscan_labels(pts, eps, min_samples) if len(pts) else np.zeros(0, int)
    pc, n_pieces = piece_ids(rays, labels, split_rays, R)
    lab_full, pc_full = np.full(R, -2, int), np.full(R, -2, int)
    lab_full[rays], pc_full[rays] = labels, pc
    if n_pieces > MAX_PIECES:
        return dict(labels=lab_full, pieces=pc_full, n_pieces=n_pieces, rings=None, overflow=1)
    rings, overflow = [], 0
    for k in range(n_pieces):
        ring = L.hull_ring(pts[pc == k])
        if ring is None:
            continue
        if len(rings) >= n_obs_max or len(ring) > v_max:
            overflow = 1                                                 # (the piece is dropped, later ones may still fit)
            continue
        rings.append(ring)
    return dict(labels=lab_full, pieces=pc_full, n_pieces=n_pieces, rings=rings, overflow=overflow)


def rooms_scene(door=(6, 20)):
    """The scene of tests/golden/make_exploration_rooms.py: 64 x 56 cells of 0.1 m, outer walls 2 cells thick, a vertical wall
    with a door (cells ``door`` of the wall) and a horizontal wall with a gap -- three rooms.  Returns (occ [64,56] uint8, origin,
    cell)."""
    occ = np.zeros((64, 56), np.uint8)
    occ[:2, :] = occ[-2:, :] = 1
    occ[:, :2] = occ[:, -2:] = 1
    occ[30:32, :] = 1
    occ[30:32, door[0]:door[1]] = 0
    occ[32:, 27:29] = 1
    occ[42:54, 27:29] = 0
    return occ, (0.0, 0.0), (0.1, 0.1)
