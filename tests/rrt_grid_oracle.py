"""numpy restatement of planning on a GIVEN occupancy grid -- lipmpc_rrt_plan_grid_batch, include/lipmpc.h -- on top of
tests/rrt_oracle.py: only the bounds, the dims and the occupancy differ from a ring plan (and the OUTSIDE_GRID status);
the distance transform, the sampler and the tree are rrt_oracle.plan's own code, run on the given grid.

Used by the tests only.
"""
import numpy as np

import rrt_oracle as R

OUTSIDE_GRID = 7
STATUS_NAMES = R.STATUS_NAMES + ("OUTSIDE_GRID",)
MAX_SIDE = 4096


def grid_transform(W, H, origin, cell):
    """The planner's grid of a W x H occupancy grid: its cell CENTRES.  min = origin + cell / 2, max = origin + (W - 1/2) cell,
    W_p = W - 1, H_p = H - 1."""
    ox, oy, dx, dy = (np.float64(v) for v in (origin[0], origin[1], cell[0], cell[1]))
    return dict(min_x=float(ox + dx / 2.0), max_x=float(ox + (np.float64(W) - 0.5) * dx),
                min_y=float(oy + dy / 2.0), max_y=float(oy + (np.float64(H) - 0.5) * dy), W=int(W) - 1, H=int(H) - 1)


def from_planner(tf):
    """(origin, cell) GridMap.from_planner gives the planner grid ``tf`` (of (W+1) x (H+1) cells): the inverse placement."""
    cell = ((tf["max_x"] - tf["min_x"]) / tf["W"], (tf["max_y"] - tf["min_y"]) / tf["H"])
    return (tf["min_x"] - cell[0] / 2, tf["min_y"] - cell[1] / 2), cell


def rounded_cell(tf, x, y):
    """The rounded cell as doubles (NaN for a NaN coordinate) and whether it is a cell of the grid."""
    with np.errstate(invalid="ignore"):
        i = np.rint(((np.float64(x) - tf["min_x"]) / (tf["max_x"] - tf["min_x"])) * tf["W"])
        j = np.rint(((np.float64(y) - tf["min_y"]) / (tf["max_y"] - tf["min_y"])) * tf["H"])
    return i, j, bool(0 <= i <= tf["W"] and 0 <= j <= tf["H"])


def plan_grid(occ, origin, cell, goal, start=None, seed=1, n=R.N_SAMPLES, r_rewire=R.R_REWIRE, max_cells=R.MAX_CELLS,
              S_max=None, C=None):
    """One plan by the contract of lipmpc_rrt_plan_grid_batch on ``occ`` [W,H] (nonzero = occupied).  Returns the dict of
    rrt_oracle.plan."""
    occ = np.asarray(occ) != 0
    W, H = occ.shape
    start = (0.0, 0.0) if start is None else (float(start[0]), float(start[1]))
    tf = grid_transform(W, H, origin, cell)
    out = dict(status=None, sub_goals=np.zeros((0, 2)), n_sub=0, path_cost=float("nan"), tf=tf, og=None, d2=None, C=None,
               cells=np.zeros((0, 2), np.int64), parent=np.zeros(0, np.int64), cost=np.zeros(0), goal_parent=-1, draws=0,
               samples=0)
    if W * H > max_cells or H > MAX_SIDE or W > MAX_SIDE:
        out["status"] = R.GRID_TOO_LARGE
        return out
    if not (rounded_cell(tf, *start)[2] and rounded_cell(tf, goal[0], goal[1])[2]):
        out["status"] = OUTSIDE_GRID
        return out
    saved = R.transform, R.occupancy
    R.transform, R.occupancy = (lambda *a, **k: tf), (lambda rings, tf_: occ)       # the given grid in the place of the rings'
    try:
        return R.plan([], goal, start=start, seed=seed, width=W - 1, n=n, r_rewire=r_rewire, margin=0.0, max_cells=max_cells,
                      S_max=S_max, C=C)
    finally:
        R.transform, R.occupancy = saved
