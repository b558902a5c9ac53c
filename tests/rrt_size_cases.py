"""Inputs of the RRT* planner's size tests, shared by tests/test_rrt_sizes_oracle.py (CPU: do the inputs reach what they are
meant to reach?) and tests/test_rrt_sizes_gpu.py (the device against the oracle on the same inputs).  numpy only.

A RING case is dict(id, params: the keyword arguments of rrt_oracle.plan that RrtStarPlanner takes too (width, n, r_rewire,
margin, max_cells), problems: [dict(rings, goal, start, seed)], expect: {problem index: status}, bar: see below).
A GRID case is dict(id, params (n, r_rewire, max_cells), occ [W,H] uint8, origin, cell, problems: [dict(goal, start, seed)],
expect, bar).  Unit cells and origin (0, 0) unless a case says otherwise.

``bar``: the least number of tree vertices that 3 of the case's 4 seeds must reach on the oracle, or None where the case is
about something else (an early status, a tree of one or two vertices, a sampler that runs dry).  It is 20, except on a map
with fewer than 21 free cells besides the goal, which cannot hold that many vertices: there it is every such cell.
"""
import numpy as np

import rrt_oracle as R

M64 = (1 << 64) - 1
LDS_LIMIT = 160 * 1024


def lds_bytes(n, max_cells):
    """Dynamic LDS of the tree kernel (include/lipmpc.h): 28 (n + 1) + max_cells / 8 + 256, the bitmap in whole 64-bit words."""
    return 28 * (n + 1) + (max_cells + 63) // 64 * 8 + 256


def box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], float)


TWO_BOXES = [box(1, 1, 1.6, 1.5), box(2.5, 0.2, 3, 2.4)]
GOAL = (4.0, 2.0)


def _ring_case(id_, seeds, rings=TWO_BOXES, goal=GOAL, expect=None, bar=20, **params):
    params.setdefault("margin", 0.5)
    params.setdefault("max_cells", R.MAX_CELLS)
    probs = [dict(rings=rings, goal=np.array(goal, float), start=(0.0, 0.0), seed=s) for s in seeds]
    return dict(id=id_, params=params, problems=probs, expect=expect or {}, bar=bar)


def ring_cases():
    cases = []
    for w in (7, 63, 64, 65, 255, 256, 257):            # W + 1 on both sides of the 64-thread blocks and of 256
        seeds = (5, 0, M64, 6) if w == 7 else (5, 6, 7, 8)
        cases.append(_ring_case(f"width{w}", seeds, width=w, n=120, r_rewire=max(2, w // 3), expect={0: R.FOUND}))
    cases.append(_ring_case("tall", (5, 6, 7, 8), rings=[box(0.3, 100, 0.6, 101)], goal=(0.2, 500.0), width=7, n=300,
                            r_rewire=60, expect={0: R.FOUND}))
    cases.append(_ring_case("wide", (5, 6, 7, 8), rings=[box(100, 0.3, 101, 0.6)], goal=(500.0, 0.2), width=2000, n=300,
                            r_rewire=300, expect={0: R.FOUND}))
    for w in (1, 2, 3):                                   # the smallest grids: no cell is occupied, all five launches still run
        cases.append(_ring_case(f"width{w}", (5, 6, 7, 8), width=w, n=120, r_rewire=2, bar=None,
                                expect={b: R.NO_OBSTACLE_GRID for b in range(4)}))
    for n, st in ((1, R.NO_PATH), (2, R.NO_PATH), (255, R.FOUND), (256, R.FOUND), (257, R.FOUND), (513, R.FOUND)):
        cases.append(_ring_case(f"n{n}", (9, 10, 11, 12), width=60, n=n, r_rewire=20, expect={0: st}, bar=20 if n > 2 else None))
    for r, st in ((1, R.NO_PATH), (2, R.NO_PATH), (8192, R.FOUND)):
        cases.append(_ring_case(f"rewire{r}", (9, 10, 11, 12), width=60, n=300, r_rewire=r, expect={0: st}))
    return cases


# the vertex counts the sample-count and radius cases are built around (problem 0, seed 9)
N_CASE_V = {1: 1, 2: 2, 255: 240, 256: 241, 257: 242, 513: 456}
REWIRE_ALL_V = 281


# -- obstacle packing ------------------------------------------------------------------------------------------------
PACK_V_MAX = 64
PACK_N_OBS = 83             # 12 * 83 * 64 + 20 * 83 = 65 404 bytes of LDS in the occupancy kernel: 84 slots would need 66 192


def packing_case():
    """One batch of 4 problems on the two boxes plus, in every problem: a 64-gon whose obs_nv says 70 (clipped to v_max), slots
    with obs_nv = 0 and obs_nv < 0 that hold coordinates far away (they must not be read), a ring of one vertex repeated and
    then three distinct ones, a ring of collinear vertices (hull of 2 points), a ring whose vertices all round to one cell, and
    a last box in the last slot.  Returns (case, obs_xy [4,83,64,2], obs_nv [4,83]); the case's rings are the clipped ones."""
    ang = 2 * np.pi * np.arange(64) / 64
    gon = np.stack([3.6 + 0.35 * np.cos(ang), 0.9 + 0.35 * np.sin(ang)], 1)
    repeated = np.array([[0.5, 2.0]] * 5 + [[0.9, 2.0], [0.9, 2.3], [0.5, 2.0], [0.5, 2.3], [0.9, 2.3]], float)
    dot = np.array([[3.3, 2.2], [3.301, 2.2], [3.3, 2.201]], float)
    last = box(0.2, 1.2, 0.5, 1.5)
    # five points of a slanted line of CELLS (the bounds come from start, goal and the boxes: no other ring moves them)
    tf = R.transform(TWO_BOXES, GOAL, (0.0, 0.0), 60, 0.5)
    collinear = np.stack(R.to_world(tf, 22 + 2 * np.array([0, 3, 1, 4, 2]), 3 + np.array([0, 3, 1, 4, 2])), 1)
    slots = {0: TWO_BOXES[0], 1: TWO_BOXES[1], 5: gon, 17: repeated, 40: collinear, 64: dot, PACK_N_OBS - 1: last}
    xy = np.zeros((4, PACK_N_OBS, PACK_V_MAX, 2))
    nv = np.zeros((4, PACK_N_OBS), np.int32)
    for o, r in slots.items():
        xy[:, o, : len(r)] = r
        nv[:, o] = len(r)
    nv[:, 5] = 70                                         # above v_max: clipped to the 64 vertices that are there
    xy[:, 2] = 1e6; nv[:, 2] = 0                          # empty slots with coordinates that would blow the bounds up
    xy[:, 3] = -1e6; nv[:, 3] = -3
    xy[:, 17, len(repeated):] = 1e6                       # ... and so would the vertices past a ring's own count
    case = _ring_case("packing", (5, 6, 7, 8), rings=[slots[o] for o in sorted(slots)], width=60, n=120, r_rewire=20)
    return case, xy, nv


def batch65_case():
    """B = 65: one problem more than a block of the setup kernels (61 x 42 cells: a cap of 2^12 keeps the buffers small)."""
    return _ring_case("batch65", tuple(range(100, 165)), width=60, n=120, r_rewire=20, bar=None, max_cells=1 << 12)


# -- given grids -----------------------------------------------------------------------------------------------------
def centre(cell, origin=(0.0, 0.0), size=(1.0, 1.0)):
    return (origin[0] + (cell[0] + 0.5) * size[0], origin[1] + (cell[1] + 0.5) * size[1])


def random_map(W, H, share, seed, free=()):
    occ = (np.random.default_rng(seed).random((W, H)) < share).astype(np.uint8)
    for c in free:
        occ[c] = 0
    return occ


def _grid_case(id_, occ, start_cell, goal_cell, seeds, expect=None, bar=20, origin=(0.0, 0.0), cell=(1.0, 1.0), **params):
    params.setdefault("max_cells", 1 << 14)
    free = int((occ == 0).sum()) - 1                      # a tree holds free cells other than the goal, each once
    probs = [dict(goal=centre(goal_cell, origin, cell), start=centre(start_cell, origin, cell), seed=s) for s in seeds]
    return dict(id=id_, params=params, occ=occ, origin=origin, cell=cell, problems=probs, expect=expect or {},
                bar=None if bar is None else min(bar, free))


def _shape_map(W, H):
    """Thin maps: the few occupied cells in row (column) 0, row (column) 1 a free corridor; the others 3 % random."""
    if W == 2 and H == 2:
        occ = np.zeros((2, 2), np.uint8); occ[0, 1] = 1
        return occ, (0, 0), (1, 1)
    if W == 2:
        occ = np.zeros((W, H), np.uint8); occ[0, [H // 3, H // 2, H - 2]] = 1
        return occ, (1, 0), (1, H - 1)
    if H == 2:
        occ = np.zeros((W, H), np.uint8); occ[[W // 3, W // 2, W - 2], 0] = 1
        return occ, (0, 1), (W - 1, 1)
    return random_map(W, H, 0.03, 1000 * W + H, free=((0, 0), (W - 1, H - 1))), (0, 0), (W - 1, H - 1)


GRID_SHAPES = ((2, 2), (2, 300), (300, 2), (31, 33), (63, 65), (65, 63), (64, 64), (2, 4096), (4096, 2))
DRY_SEEDS = (5, 8, 13, 18)


def grid_cases():
    cases = []
    for W, H in GRID_SHAPES:                              # sides on both sides of 64, cell counts that are no multiple of 64
        occ, s, g = _shape_map(W, H)
        seeds = (5, 0, M64, 6) if (W, H) == (31, 33) else (5, 6, 7, 8)
        cases.append(_grid_case(f"shape{W}x{H}", occ, s, g, seeds, n=150, r_rewire=max(30, max(W, H) // 6)))
    for W, H in ((128, 128), (129, 127)):                 # exactly max_cells = 2^14 cells, and just under
        occ = random_map(W, H, 0.05, 7 * W + H, free=((0, 0), (W - 1, H - 1)))
        cases.append(_grid_case(f"cap{W}x{H}", occ, (0, 0), (W - 1, H - 1), (5, 6, 7, 8), n=150, r_rewire=30))
    for W, H in ((129, 128), (4097, 2), (2, 4097)):       # one cell column over the cap; a side over 4096
        occ = np.zeros((W, H), np.uint8); occ[0, 1] = 1
        cases.append(_grid_case(f"refused{W}x{H}", occ, (0, 0), (W - 1, H - 1), (5, 6, 7, 8), n=150, r_rewire=30, bar=None,
                                expect={b: R.GRID_TOO_LARGE for b in range(4)}))
    cases += [dry_case(), dry_case(empty=True)]
    # more than 64 KiB of LDS in the tree kernel: through the bitmap, through the tree, and 4 bytes under the limit
    cases.append(_grid_case("lds_bitmap", random_map(20, 20, 0.08, 21, free=((0, 0), (19, 19))), (0, 0), (19, 19), (5, 6, 7, 8),
                            n=200, r_rewire=30, max_cells=1 << 19, expect={0: R.FOUND}))
    cases.append(_grid_case("lds_tree", random_map(100, 80, 0.05, 22, free=((0, 0), (99, 79))), (0, 0), (99, 79), (5, 6, 7, 8),
                            n=4000, r_rewire=8, max_cells=1 << 14, expect={0: R.FOUND}, bar=1500))
    cases.append(_grid_case("lds_limit", random_map(48, 40, 0.10, 23, free=((0, 0), (47, 39))), (0, 0), (47, 39), (5, 6, 7, 8),
                            n=1160, r_rewire=6, max_cells=1 << 20, expect={0: R.FOUND}, bar=256))
    return cases


def dry_case(empty=False):
    """The 8 x 8 map on which the sampler runs dry: every cell occupied except (0,0), (0,1) and (7,7) -- or, ``empty``, except
    start and goal alone, where no draw is valid at all."""
    occ = np.ones((8, 8), np.uint8)
    occ[0, 0] = occ[7, 7] = 0
    if empty:
        return _grid_case("dry_empty", occ, (0, 0), (7, 7), DRY_SEEDS, n=4, r_rewire=3, bar=None,
                          expect={b: R.NO_PATH for b in range(4)})
    occ[0, 1] = 0
    return _grid_case("dry", occ, (0, 0), (7, 7), DRY_SEEDS, n=40, r_rewire=3, bar=None)


def replay_case():
    """A plan to capture in a graph: the defaults' LDS size class (below 64 KiB), B = 4."""
    return _grid_case("replay", random_map(40, 30, 0.08, 24, free=((0, 0), (39, 29))), (0, 0), (39, 29), (5, 6, 7, 8), n=150,
                      r_rewire=30)


def case_ids(cases):
    return [c["id"] for c in cases]
