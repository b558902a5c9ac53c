"""The numpy restatement of the RRT* planner's contract (tests/rrt_oracle.py) on the CPU: its grids against scipy's
(tests/golden/rrt_grid_golden.npz, made by make_rrt_golden.py the way the reference makes them), its plans on the three
RRT scenes, and the occupancy rule where the reference has no answer (Qhull refuses degenerate rounded vertices)."""
import os

import numpy as np
import pytest

import rrt_oracle as R

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = ("SimulationRRT", "SimulationMaze1", "SimulationMaze2")
# vertex counts (root included) and sub-goal counts of seeds 0..3 at the default parameters: the table of the contract
TABLE = {"SimulationRRT": ([1478, 1477, 1471, 1490], [35, 43, 36, 29]),
         "SimulationMaze1": ([331, 311, 297, 328], [7, 6, 5, 7]),
         "SimulationMaze2": ([366, 347, 317, 353], [13, 8, 12, 12])}


def _scene(name):
    sc = np.load(os.path.join(HERE, "golden", "pdf_scenarios.npz"))
    rings = [sc[name + "/rings"][j][: sc[name + "/nv"][j]] for j in range(len(sc[name + "/nv"]))]
    return rings, np.asarray(sc[name + "/goal"], float)


def _golden():
    d = np.load(os.path.join(HERE, "golden", "rrt_grid_golden.npz"))
    for s, name in enumerate(d["names"]):
        dims = tuple(int(v) for v in d["dims"][s])
        og = np.unpackbits(d["occ_packed"][d["occ_off"][s]: d["occ_off"][s + 1]])[: dims[0] * dims[1]].reshape(dims)
        d2 = np.cumsum(d["d2_dy"][d["d2_off"][s]: d["d2_off"][s + 1]].reshape(dims).astype(np.int64), axis=1)
        rings = [d["rings"][s, j, : d["nv"][s, j]] for j in range(d["nv"].shape[1]) if d["nv"][s, j] > 0]
        yield str(name), rings, d["goal"][s], d["bounds"][s], dims, og.astype(bool), d2


def test_golden_fixture_shape():
    names = [g[0] for g in _golden()]
    assert len(names) == 28 and sum(n.startswith("random") for n in names) == 24
    assert sum(n.endswith("_tiny") for n in names) >= 8
    assert os.path.getsize(os.path.join(HERE, "golden", "rrt_grid_golden.npz")) < 1 << 20


def test_oracle_grid_matches_golden():
    """Bounds, dims, occupancy and d2 equal scipy's bit for bit on every set; on the random sets d2 is also the
    brute-force minimum over the occupied cells."""
    for name, rings, goal, bounds, dims, og, d2 in _golden():
        tf = R.transform(rings, goal)
        assert (tf["min_x"], tf["max_x"], tf["min_y"], tf["max_y"]) == tuple(bounds), name
        assert (tf["W"] + 1, tf["H"] + 1) == dims, name
        mine = R.occupancy(rings, tf)
        assert np.array_equal(mine, og), (name, int(np.sum(mine != og)))
        e = R.edt_d2(mine)
        assert np.array_equal(e, d2), (name, int(np.sum(e != d2)))
        if name.startswith("random"):
            occ = np.argwhere(og)
            I, J = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), indexing="ij")
            brute = np.full(dims, np.iinfo(np.int64).max)
            for a, b in occ:
                brute = np.minimum(brute, (I - a) ** 2 + (J - b) ** 2)
            assert np.array_equal(brute, d2), name


@pytest.mark.parametrize("name", SCENES)
def test_oracle_plans_on_scenes(name):
    """Default parameters, seeds 0..7: a path every time; cost(v) == cost(parent) + edge(v) exactly; every tree edge and
    path segment free; deterministic; seeds 0..3 give the vertex and sub-goal counts of the contract's table."""
    rings, goal = _scene(name)
    for seed in range(8):
        r = R.plan(rings, goal, seed=seed)
        assert r["status"] == R.FOUND, (name, seed)
        assert R.check_tree(r) == [], (name, seed)
        assert np.allclose(r["sub_goals"][-1], R.to_world(r["tf"], *R.to_cell(r["tf"], goal[0], goal[1])))
        if seed < 4:
            assert len(r["cells"]) == TABLE[name][0][seed], (name, seed, len(r["cells"]))
            assert r["n_sub"] == TABLE[name][1][seed], (name, seed, r["n_sub"])
        if seed < 2:
            again = R.plan(rings, goal, seed=seed)
            for k in ("cells", "parent", "cost", "sub_goals"):
                assert np.array_equal(np.asarray(r[k]).view(np.uint8), np.asarray(again[k]).view(np.uint8)), (name, k)


def test_occupancy_rule_on_degenerate_hulls():
    """Where Qhull refuses the rounded vertices the same rule applies: a horizontal or vertical run of cells has an empty
    half-open box (no cell), a diagonal run keeps the cells ON the segment inside the box, coincident vertices give
    nothing, and the hull of a rounded ring that turned reflex is the hull of its points."""
    tf = dict(min_x=0.0, max_x=10.0, min_y=0.0, max_y=10.0, W=10, H=10)
    horiz = np.array([[1.0, 2.0], [3.0, 2.0], [5.0, 2.0]])
    assert not R.occupancy([horiz], tf).any()
    diag = np.array([[1.0, 1.0], [3.0, 3.0], [5.0, 5.0]])
    og = R.occupancy([diag], tf)
    assert sorted(map(tuple, np.argwhere(og).tolist())) == [(1, 1), (2, 2), (3, 3), (4, 4)]
    same = np.array([[2.0, 2.0], [2.2, 2.1], [1.9, 2.0]])
    assert not R.occupancy([same], tf).any()
    # a convex ring whose rounding adds a reflex vertex: the hull of the rounded points is filled, not the ring
    ring = np.array([[0.0, 0.0], [4.0, 0.0], [2.4, 1.2], [0.0, 4.0]])
    og = R.occupancy([ring], tf)
    assert og[2, 1] and og[3, 0] and og[1, 2]
    # closed hull: boundary cells are in, half-open box: the max row / column are out
    sq = np.array([[1.0, 1.0], [4.0, 1.0], [4.0, 4.0], [1.0, 4.0]])
    og = R.occupancy([sq], tf)
    assert og[1, 1] and og[3, 3] and not og[4, 4] and not og[4, 1] and int(og.sum()) == 9


def test_statuses_without_a_tree():
    """GRID_TOO_LARGE (cells over max_cells, or more than 4096 per side), NO_OBSTACLE_GRID, START / GOAL_OCCUPIED,
    NO_PATH and PATH_OVERFLOW follow the contract's order."""
    box = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], float)
    assert R.plan([box(1, 1, 2, 2)], (0.0, 400.0), n=50)["status"] == R.GRID_TOO_LARGE
    assert R.plan([box(1, 1, 2, 2)], (5.0, 5.0), n=50, max_cells=1000)["status"] == R.GRID_TOO_LARGE
    assert R.plan([], (5.0, 5.0), n=50)["status"] == R.NO_OBSTACLE_GRID
    assert R.plan([box(-1, -1, 1, 1)], (5.0, 5.0), n=50)["status"] == R.START_OCCUPIED
    assert R.plan([box(4, 4, 6, 6)], (5.0, 5.0), n=50)["status"] == R.GOAL_OCCUPIED
    walls = [box(3, 3, 5, 3.3), box(3, 4.7, 5, 5), box(3, 3, 3.3, 5), box(4.7, 3, 5, 5)]
    assert R.plan(walls, (4.0, 4.0), n=200)["status"] == R.NO_PATH
    r = R.plan([box(2, 2, 3, 3)], (5.0, 5.0), n=200, S_max=1)
    assert r["status"] == R.PATH_OVERFLOW and np.isfinite(r["path_cost"])


def test_sampler_stream():
    """splitmix64 draws: the first value of seed 0 is the published splitmix64 output 0xE220A8397B1DCDAF, and the cell
    index is the high 32 bits scaled by the cell count."""
    z = R.splitmix_draws(0, 0, 3)
    assert int(z[0]) == 0xE220A8397B1DCDAF
    c = R.draw_cells(0, 0, 3, 1000)
    assert int(c[0]) == (0xE220A839 * 1000) >> 32
