"""What every device plan of the RRT* planner is held to, given the oracle's plan of the same problem on the device's own cost
grid: shared by tests/test_rrt_gpu.py, tests/test_rrt_grid_gpu.py and tests/test_rrt_sizes_gpu.py.  numpy only."""
import numpy as np

import rrt_grid_oracle as RG
import rrt_oracle as R

C_ULP = 2                    # exp may differ in the last bits between the device and numpy; everything else is bit for bit
NO_GRID = (R.GRID_TOO_LARGE, RG.OUTSIDE_GRID)                     # statuses that end a problem before its grid is built
NO_COST = NO_GRID + (R.NO_OBSTACLE_GRID,)                         # ... and before there is a cost grid to plan on


def ulp_diff(a, b):
    return np.abs(np.ascontiguousarray(a).view(np.int64) - np.ascontiguousarray(b).view(np.int64))


def device_cost(res, b, W1, H1):
    """The device's cost grid of problem b as the oracle takes it, None where the device built none."""
    return None if res["status"][b] in NO_COST else res["cost_grid"][b, : W1 * H1].reshape(W1, H1)


def check_plan(res, b, o, W1, H1, label, names=RG.STATUS_NAMES):
    """Problem b of a plan (host arrays, with_tree and with_grids) against the oracle's plan ``o`` of it on device_cost(...), on a
    grid of W1 x H1 cells: status, n_sub, the tree's header (V, goal's parent, draws, samples), vertex list, parents and costs,
    sub-goals and path cost bit for bit; occ_d2 equal to the oracle's; cost_grid within C_ULP of numpy's exp(-sqrt(d2)); tree
    rows, d2 and cost cells that the plan does not own still the zeros they were allocated with."""
    assert res["status"][b] == o["status"], (label, names[res["status"][b]], names[o["status"]])
    assert res["n_sub"][b] == o["n_sub"], label
    t = res["tree"][b]
    V = int(t[0, 0])
    assert V == len(o["cells"]), (label, V, len(o["cells"]))
    assert t[0, 2] == o["draws"], (label, "draws", t[0, 2], o["draws"])
    assert t[0, 3] == o["samples"], (label, "samples", t[0, 3], o["samples"])
    assert not t[V + 1:].view(np.int64).any(), (label, "tree rows past V + 1")
    if V:
        assert int(t[0, 1]) == o["goal_parent"], label
        assert np.array_equal(t[1: V + 1, :2].astype(np.int64), o["cells"]), label
        assert np.array_equal(t[1: V + 1, 2].astype(np.int64), o["parent"]), label
        assert np.array_equal(t[1: V + 1, 3].view(np.int64), o["cost"].view(np.int64)), label
    else:
        assert t[0, 1] == -1, label
    # the grids: nothing where no grid was built, d2 = -1 and C = NaN where no cell is occupied
    ncells = 0 if o["status"] in NO_GRID else W1 * H1
    d2, C = res["occ_d2"][b], res["cost_grid"][b]
    assert not d2[ncells:].any() and not C[ncells:].view(np.int64).any(), (label, "cells past the grid")
    if ncells and o["d2"] is None:
        assert (d2[:ncells] == -1).all() and np.isnan(C[:ncells]).all(), label
    elif ncells:
        assert np.array_equal(d2[:ncells].reshape(W1, H1), o["d2"]), (label, int(np.sum(d2[:ncells] != o["d2"].reshape(-1))))
        ulp = ulp_diff(C[:ncells], R.cost_grid(o["d2"]).reshape(-1))
        assert ulp.max() <= C_ULP, (label, "C ulp", int(ulp.max()))
    if o["status"] == R.FOUND:
        assert np.array_equal(res["sub_goals"][b, : o["n_sub"]].view(np.int64), o["sub_goals"].view(np.int64)), label
        assert res["path_cost"][b] == o["path_cost"], label
    else:
        assert res["n_sub"][b] == 0, label
    return o


def check_ring_plan(res, b, prob, label, S_max=None, **params):
    """Problem b of a plan_batch result against rrt_oracle.plan(**params) of ``prob`` = dict(rings, goal, start, seed)."""
    W1, H1 = (int(v) for v in res["grid_dims"][b])
    too_large = res["status"][b] == R.GRID_TOO_LARGE              # (grid_dims then holds the refused size)
    C = None if too_large else device_cost(res, b, W1, H1)
    o = R.plan(prob["rings"], prob["goal"], start=prob.get("start"), seed=prob["seed"], S_max=S_max, C=C, **params)
    if o["status"] != R.GRID_TOO_LARGE:
        assert (W1, H1) == (o["tf"]["W"] + 1, o["tf"]["H"] + 1), (label, W1, H1)
    return check_plan(res, b, o, W1, H1, label)


def check_grid_plan(res, b, occ, origin, cell, prob, label, S_max=None, **params):
    """Problem b of a plan_grid_batch result against rrt_grid_oracle.plan_grid(**params) on ``occ`` [W,H]."""
    W, H = occ.shape
    assert tuple(res["grid_dims"][b]) == (W, H), label
    o = RG.plan_grid(occ, origin, cell, prob["goal"], start=prob["start"], seed=prob["seed"], S_max=S_max,
                     C=device_cost(res, b, W, H), **params)
    check_plan(res, b, o, W, H, label)
    if o["status"] == R.FOUND:
        gb = res["grid_bounds"][b]
        assert (gb[0], gb[1], gb[2], gb[3]) == (o["tf"]["min_x"], o["tf"]["max_x"], o["tf"]["min_y"], o["tf"]["max_y"]), label
    return o
