"""Scenes and cases of the scan matcher's tests (tests/test_scan_match_oracle.py on the CPU, tests/test_scan_match_gpu.py on the
device): one small room, the evidence a walk along a line leaves of it, and the displaced scans the oracle puts back."""
from __future__ import annotations

import functools

import numpy as np

import lipmpc
import map_oracle as M

CELL, ORIGIN, RANGE, R = (0.1, 0.1), (0.0, 0.0), 1.5, 90
W, H = 48, 40
DEPTH = M.default_depth(CELL)
N_SEARCH, CLAMP = 5, 8                # the displaced-scan property: shifts of up to (+-4, +-4) cells inside a search of +-5


def room():
    """occ [48,40] uint8: the outer walls and three inner obstacles."""
    occ = np.zeros((W, H), np.uint8)
    occ[0, :] = occ[-1, :] = 1
    occ[:, 0] = occ[:, -1] = 1
    occ[10:14, 9:12] = 1
    occ[22:24, 14:19] = 1
    occ[30:35, 12:14] = 1
    return occ


def table():
    return lipmpc.ray_table(R)


def scan(positions, noise=None):
    """hits [B,R,2] of the room from ``positions`` [B,2] as the grid scan's oracle writes them."""
    return M.oracle_hits(np.asarray(positions, np.float64), room(), ORIGIN, CELL, RANGE, table(), noise)


def mapped_poses():
    """12 poses along a line through the lower half of the room."""
    t = np.linspace(0.0, 1.0, 12)
    return np.stack([0.75 + 2.6 * t, 0.62 + 0.33 * t], axis=1)


@functools.lru_cache(maxsize=None)
def line_evidence():
    """The evidence [48,40] int64 after the 12 noise-free scans of ``mapped_poses`` (w_hit 3, w_miss 1)."""
    pos = mapped_poses()
    ev = M.update(np.zeros((W, H), np.int64), pos, scan(pos), ORIGIN, CELL, RANGE, table(), depth=DEPTH)
    ev.setflags(write=False)
    return ev


def displaced_cases(seed=3, per_pose=20):
    """(true position, (da, db)): 6 query poses within a cell or two of mapped poses, each displaced by ``per_pose`` whole-cell
    shifts of up to (+-4, +-4), (0, 0) among them: 120 cases.  The believed position is true + (da dx, db dy), the readings are
    placed there (true readings + the same shift), and the matcher must answer (-da, -db)."""
    rng = np.random.default_rng(seed)
    base = mapped_poses()[[1, 3, 5, 7, 9, 10]]
    query = base + rng.uniform(-0.12, 0.12, base.shape)
    out = []
    for q in query:
        shifts = [(0, 0)] + [tuple(int(v) for v in rng.integers(-4, 5, 2)) for _ in range(per_pose - 1)]
        out += [(q, s) for s in shifts]
    return out


def displace(position, hits, shift):
    d = np.array([shift[0] * CELL[0], shift[1] * CELL[1]])
    return np.asarray(position) + d, np.asarray(hits) + d
