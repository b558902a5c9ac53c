"""GPU: the RRT* planner on a GIVEN occupancy grid (lipmpc_rrt_plan_grid_batch, RrtStarPlanner.plan_grid_batch) against the
numpy restatement of its contract (tests/rrt_grid_oracle.py) fed the device's cost grid: trees bit for bit, every status."""
import numpy as np
import pytest

import grid_lidar_oracle as G
import rrt_grid_oracle as RG
import rrt_oracle as R
from rrt_checks import check_grid_plan
from test_rrt_grid_oracle import golden_scenes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

N, R_REWIRE, MAX_CELLS = 150, 30, 1 << 14


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(res, b, occ, origin, cell, goal, start, seed, S_max=None, n=N, r_rewire=R_REWIRE, max_cells=MAX_CELLS, label=""):
    """Problem b of a plan_grid_batch result against the oracle on the device's C: everything tests/rrt_checks.py holds a plan to
    (status, n_sub, the tree bit for bit, draws and samples, d2, C, sub-goals, path cost, grid bounds, untouched cells)."""
    return check_grid_plan(res, b, occ, origin, cell, dict(goal=goal, start=start, seed=seed), label, S_max=S_max, n=n,
                           r_rewire=r_rewire, max_cells=max_cells)


def test_gpu_plan_on_from_planner_grids_equals_the_ring_plan():
    """Golden scenes planned from their rings at width 90 (grids within 2^14 cells), then on GridMap.from_planner of that very
    grid: the tree equals the oracle's on the device's C, and the ring plan's own tree (cells, parents, costs) bit for bit."""
    scenes = list(golden_scenes(10))
    planner = lipmpc.RrtStarPlanner(width_grid_size=90, n=N, r_rewire=R_REWIRE, seed=5, max_cells=MAX_CELLS)
    n_obs = max(len(r) for _, r, _ in scenes)
    v_max = max(len(x) for _, r, _ in scenes for x in r)
    xy, nv = lipmpc.pack_rings([r for _, r, _ in scenes], n_obs, v_max)
    goals = np.array([g for _, _, g in scenes], float)
    ring_out = planner.plan_batch(goals, xy, nv, with_tree=True, with_grids=True)
    ring = _np(ring_out)
    compared = found = 0
    for b, (name, rings, goal) in enumerate(scenes):
        if ring["status"][b] == R.GRID_TOO_LARGE:
            continue
        gm = lipmpc.GridMap.from_planner(ring_out, b)
        assert gm.W * gm.H <= MAX_CELLS
        res = _np(planner.plan_grid_batch(goals[b: b + 1], gm, np.zeros((1, 2)), with_tree=True, with_grids=True))
        occ = gm.occ.cpu().numpy()
        o = _check(res, 0, occ, gm.origin, gm.cell, goal, (0.0, 0.0), 5, label=name)
        tf_ring = dict(zip(("min_x", "max_x", "min_y", "max_y"), ring["grid_bounds"][b]), W=gm.W - 1, H=gm.H - 1)
        same = all(tuple(int(v) for v in R.to_cell(tf_ring, *p)) == tuple(int(v) for v in RG.rounded_cell(o["tf"], *p)[:2])
                   for p in ((0.0, 0.0), goal))
        if not same:
            print(name, "dropped: start or goal rounds to another cell under the recomputed bounds")
            continue
        assert res["status"][0] == ring["status"][b], name
        V = int(ring["tree"][b, 0, 0])
        assert np.array_equal(res["tree"][0, : V + 1].view(np.int64), ring["tree"][b, : V + 1].view(np.int64)), name
        if ring["status"][b] == R.FOUND:
            k = ring["n_sub"][b]
            assert res["n_sub"][0] == k and np.max(np.abs(res["sub_goals"][0, :k] - ring["sub_goals"][b, :k])) <= 1e-9, name
            found += 1
        compared += 1
    print(f"{compared} scenes compared, {found} with a path")
    assert compared >= 3 and found >= 2


def test_gpu_plan_on_a_scan_built_map():
    """The map the robots' own scans build (OccupancyMapper over the grid-scan fixture) thresholded into a GridMap: plans on it
    equal the oracle's on the same cells."""
    fx = G.fixture(n_robots=60)
    sensor = lipmpc.LidarSensor.from_grid(lipmpc.GridMap(fx["occ"], fx["origin"], fx["cell"]), lidar_range=1.5, n_obs_max=24, v_max=64)
    st = np.zeros((60, 5)); st[:, 0] = fx["pos"][:, 0]; st[:, 2] = fx["pos"][:, 1]
    st = torch.as_tensor(st, device="cuda")
    mp = lipmpc.OccupancyMapper(120, 120, (-0.5, -0.5), 0.075, 1.5)
    mp.update(st, sensor.sense(st, None, with_debug=True, c_eta=True)["hits"])
    gm = mp.grid_map()
    occ = gm.occ.cpu().numpy()
    assert occ.sum() > 50 and gm.W * gm.H <= MAX_CELLS
    free = np.argwhere(occ == 0)
    rng = np.random.default_rng(3)
    pick = free[rng.choice(len(free), 8, replace=False)]
    pts = np.array(gm.origin) + (pick + 0.5) * np.array(gm.cell)
    start, goal = pts[:4], pts[4:]
    planner = lipmpc.RrtStarPlanner(n=300, r_rewire=40, max_cells=MAX_CELLS)
    res = _np(planner.plan_grid_batch(goal, gm, start, seeds=[11, 12, 13, 14], with_tree=True, with_grids=True))
    for b in range(4):
        _check(res, b, occ, gm.origin, gm.cell, goal[b], start[b], 11 + b, n=300, r_rewire=40, label=b)
    print("statuses", [RG.STATUS_NAMES[s] for s in res["status"]])
    assert (res["status"] == R.FOUND).any()


def _status_grid():
    occ = np.zeros((40, 30), np.uint8)
    occ[10:14, 5:25] = 1
    return occ, (-1.0, -1.0), (0.1, 0.1)


def test_gpu_every_status():
    """One map per problem ([B,W,H]): FOUND, START_OCCUPIED, GOAL_OCCUPIED, OUTSIDE_GRID (start, goal, a NaN), NO_OBSTACLE_GRID
    (an empty map), NO_PATH (a wall across the grid); PATH_OVERFLOW (S_max = 1) and GRID_TOO_LARGE (max_cells below W * H) in
    calls of their own."""
    occ, org, cell = _status_grid()
    wall = occ.copy(); wall[10:14, :] = 1
    cases = [((2.5, 0.5), (-0.7, 0.5), occ, R.FOUND), ((2.5, 0.5), (0.12, 0.5), occ, R.START_OCCUPIED),
             ((0.12, 0.5), (-0.7, 0.5), occ, R.GOAL_OCCUPIED), ((3.5, 0.5), (-0.7, 0.5), occ, RG.OUTSIDE_GRID),
             ((2.5, 0.5), (-0.7, -1.2), occ, RG.OUTSIDE_GRID), ((2.5, float("nan")), (-0.7, 0.5), occ, RG.OUTSIDE_GRID),
             ((2.5, 0.5), (-0.7, 0.5), np.zeros_like(occ), R.NO_OBSTACLE_GRID), ((2.5, 0.5), (-0.7, 0.5), wall, R.NO_PATH)]
    goal, start = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    maps = np.stack([c[2] for c in cases])
    planner = lipmpc.RrtStarPlanner(n=120, r_rewire=12, seed=3, max_cells=MAX_CELLS)
    kw = dict(n=120, r_rewire=12)
    res = _np(planner.plan_grid_batch(goal, lipmpc.GridMap(maps, org, cell), start, with_tree=True, with_grids=True))
    for b, c in enumerate(cases):
        assert res["status"][b] == c[3], (b, RG.STATUS_NAMES[res["status"][b]], RG.STATUS_NAMES[c[3]])
        _check(res, b, c[2], org, cell, c[0], c[1], 3, label=b, **kw)
    assert res["n_sub"][0] > 1 and np.isnan(res["path_cost"][1:]).all()
    over = _np(planner.plan_grid_batch(goal[:1], lipmpc.GridMap(occ, org, cell), start[:1], S_max=1, with_tree=True, with_grids=True))
    assert over["status"][0] == R.PATH_OVERFLOW and over["n_sub"][0] == 0 and over["path_cost"][0] == res["path_cost"][0]
    _check(over, 0, occ, org, cell, goal[0], start[0], 3, S_max=1, label="overflow", **kw)
    small = lipmpc.RrtStarPlanner(n=120, r_rewire=12, seed=3, max_cells=1199)
    big = _np(small.plan_grid_batch(goal[:2], lipmpc.GridMap(occ, org, cell), start[:2], with_tree=True, with_grids=True))
    assert (big["status"] == R.GRID_TOO_LARGE).all() and (big["n_sub"] == 0).all() and not big["occ_d2"].any()
    _check(big, 1, occ, org, cell, goal[1], start[1], 3, max_cells=1199, label="too large", **kw)


def test_gpu_batch_independence():
    """B = 64 on a shared grid equals 64 calls of B = 1, compared on 4 of them."""
    occ, org, cell = _status_grid()
    rng = np.random.default_rng(8)
    free = np.argwhere(occ == 0)
    pts = np.array(org) + (free[rng.choice(len(free), 128, replace=False)] + 0.5) * np.array(cell)
    start, goal, seeds = pts[:64], pts[64:], list(range(100, 164))
    planner = lipmpc.RrtStarPlanner(n=120, r_rewire=12, max_cells=MAX_CELLS)
    gm = lipmpc.GridMap(occ, org, cell)
    res = _np(planner.plan_grid_batch(goal, gm, start, seeds=seeds, with_tree=True))
    assert (res["status"] == R.FOUND).sum() >= 32
    for b in (0, 21, 42, 63):
        one = _np(planner.plan_grid_batch(goal[b: b + 1], gm, start[b: b + 1], seeds=[seeds[b]], with_tree=True))
        for k in ("status", "n_sub", "path_cost", "sub_goals", "tree"):
            assert np.array_equal(one[k][0], res[k][b], equal_nan=True), (b, k)
