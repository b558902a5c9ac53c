"""CPU: planning on a given grid (tests/rrt_grid_oracle.py, contract of lipmpc_rrt_plan_grid_batch) is the ring plan's inverse:
on GridMap.from_planner of a ring plan's grid it grows the same tree bit for bit."""
import os

import numpy as np
import pytest

import rrt_grid_oracle as RG
import rrt_oracle as R

HERE = os.path.dirname(os.path.abspath(__file__))
N, N_SCENES = 150, 10


def golden_scenes(count=N_SCENES):
    """The first ``count`` sets of tests/golden/rrt_grid_golden.npz (the four RRT-style scenes, then random sets)."""
    d = np.load(os.path.join(HERE, "golden", "rrt_grid_golden.npz"))
    for s, name in enumerate(d["names"][:count]):
        rings = [d["rings"][s, j, : d["nv"][s, j]] for j in range(d["nv"].shape[1]) if d["nv"][s, j] > 0]
        yield str(name), rings, d["goal"][s]


def same_cells(tf_ring, tf_grid, goal, start=(0.0, 0.0)):
    """Do start and goal round to the same cells under the recomputed bounds?"""
    a = [tuple(int(v) for v in R.to_cell(tf_ring, *p)) for p in (start, goal)]
    b = [tuple(int(v) for v in RG.rounded_cell(tf_grid, *p)[:2]) for p in (start, goal)]
    return a == b


def test_grid_plan_equals_ring_plan_on_its_own_grid():
    kept, dropped, found = [], [], 0
    for name, rings, goal in golden_scenes():
        o = R.plan(rings, goal, seed=5, n=N)
        origin, cell = RG.from_planner(o["tf"])
        tf = RG.grid_transform(*o["og"].shape, origin, cell)
        assert (tf["W"], tf["H"]) == (o["tf"]["W"], o["tf"]["H"])
        for k in ("min_x", "max_x", "min_y", "max_y"):                 # the inverse, up to the rounding of the bounds
            assert abs(tf[k] - o["tf"][k]) <= 1e-12 * max(1.0, abs(o["tf"][k])), (name, k)
        if not same_cells(o["tf"], tf, goal):
            dropped.append(name)
            continue
        g = RG.plan_grid(o["og"], origin, cell, goal, seed=5, n=N, C=o["C"])
        assert g["status"] == o["status"] and g["draws"] == o["draws"] and g["goal_parent"] == o["goal_parent"], name
        assert np.array_equal(g["cells"], o["cells"]) and np.array_equal(g["parent"], o["parent"]), name
        assert np.array_equal(g["cost"].view(np.int64), o["cost"].view(np.int64)), name
        assert g["n_sub"] == o["n_sub"], name
        if o["status"] == R.FOUND:
            assert g["path_cost"] == o["path_cost"] and np.max(np.abs(g["sub_goals"] - o["sub_goals"])) <= 1e-9, name
            found += 1
        assert g["d2"] is o["d2"] is None or np.array_equal(g["d2"], o["d2"])
        kept.append(name)
    print("compared:", kept, "dropped (start or goal rounds to another cell under the recomputed bounds):", dropped)
    assert len(kept) >= 3 and found >= 3


def test_from_planner_is_the_placement_of_GridMap():
    """rrt_grid_oracle.from_planner states what lipmpc.GridMap.from_planner computes."""
    torch = pytest.importorskip("torch")
    import lipmpc
    name, rings, goal = next(golden_scenes(1))
    tf = R.transform(rings, goal)
    og = R.occupancy(rings, tf)
    d2 = R.edt_d2(og)
    out = dict(grid_dims=torch.tensor([[tf["W"] + 1, tf["H"] + 1]]), occ_d2=torch.as_tensor(d2.reshape(1, -1)),
               grid_bounds=torch.tensor([[tf["min_x"], tf["max_x"], tf["min_y"], tf["max_y"]]], dtype=torch.float64))
    gm = lipmpc.GridMap.from_planner(out, 0)
    origin, cell = RG.from_planner(tf)
    assert gm.origin == origin and gm.cell == cell and np.array_equal(gm.occ.numpy() != 0, og)


def test_statuses_of_a_given_grid():
    occ = np.zeros((40, 30), np.uint8)
    occ[10:14, 5:25] = 1
    org, cell = (-1.0, -1.0), (0.1, 0.1)
    plan = lambda goal, start, **kw: RG.plan_grid(occ, org, cell, goal, start=start, seed=3, n=120, r_rewire=12, **kw)
    assert plan((2.5, 0.5), (-0.7, 0.5))["status"] == R.FOUND
    assert plan((2.5, 0.5), (-0.7, 0.5), S_max=1)["status"] == R.PATH_OVERFLOW
    assert plan((2.5, 0.5), (0.12, 0.5))["status"] == R.START_OCCUPIED
    assert plan((0.12, 0.5), (-0.7, 0.5))["status"] == R.GOAL_OCCUPIED
    assert plan((3.5, 0.5), (-0.7, 0.5))["status"] == RG.OUTSIDE_GRID          # beyond the last column's centre by more than half a cell
    assert plan((2.5, 0.5), (-0.7, -1.2))["status"] == RG.OUTSIDE_GRID
    assert plan((2.5, float("nan")), (-0.7, 0.5))["status"] == RG.OUTSIDE_GRID
    assert plan((2.5, 0.5), (-0.7, 0.5), max_cells=1199)["status"] == R.GRID_TOO_LARGE
    assert RG.plan_grid(np.zeros((40, 30)), org, cell, (2.5, 0.5), start=(-0.7, 0.5))["status"] == R.NO_OBSTACLE_GRID
    wall = occ.copy()
    wall[10:14, :] = 1                                                          # the wall spans the grid: no way round
    assert RG.plan_grid(wall, org, cell, (2.5, 0.5), start=(-0.7, 0.5), seed=3, n=120, r_rewire=12)["status"] == R.NO_PATH
    # the cell centres are the planner's points: cell (i, j)'s centre maps to (i, j) and back
    tf = RG.grid_transform(40, 30, org, cell)
    i, j, inside = RG.rounded_cell(tf, -1.0 + 7.5 * 0.1, -1.0 + 29.5 * 0.1)
    assert (i, j, inside) == (7, 29, True)
    x, y = R.to_world(tf, 7, 29)
    assert abs(x - (-1.0 + 7.5 * 0.1)) < 1e-12 and abs(y - (-1.0 + 29.5 * 0.1)) < 1e-12
