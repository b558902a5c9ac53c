"""GPU: the grid field planner (lipmpc_grid_field_batch, lipmpc_grid_path_batch) against tests/field_oracle.py: the uint32 field,
the int32 n_sub / status / field_status and the doubles of sub_goals[:n_sub] and path_cost, bit for bit, on every map."""
import functools

import numpy as np
import pytest

import field_oracle as Fo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

from grid_checks import CELL, ORIGIN, SENTINEL, bits as _bits, check_field as _check, field_buffers as _buffers, host as _host, \
    run_field as _run  # noqa: E402  (the helpers this file shares with the other grid planner tests)


def _points(rng, W, H, n, origin=ORIGIN, cell=CELL, margin=0.0):
    """n world points over the grid's rectangle (+ a margin, in cells, that puts some outside)."""
    return np.stack([origin[0] + rng.uniform(-margin, W + margin, n) * cell[0], origin[1] + rng.uniform(-margin, H + margin, n) * cell[1]], 1)


def _free_point(rng, blocked, origin=ORIGIN, cell=CELL):
    ij = np.argwhere(~blocked)
    i, j = ij[rng.integers(len(ij))]
    return origin[0] + (i + rng.uniform(0.05, 0.95)) * cell[0], origin[1] + (j + rng.uniform(0.05, 0.95)) * cell[1]


def test_gpu_smallest_grid():
    got, _ = _check(np.zeros((2, 2), np.uint8), ORIGIN, CELL, [Fo.centre((1, 1), ORIGIN, CELL)] * 4,
                    [Fo.centre(c, ORIGIN, CELL) for c in ((0, 0), (0, 1), (1, 0), (1, 1))])
    assert got["field"][0].tolist() == [[7, 5], [5, 0]] and got["n_sub"].tolist() == [1, 1, 1, 1] and (got["status"] == 0).all()


@pytest.mark.parametrize("r", [0, 1, 2])
def test_gpu_one_solid_cell(r):
    occ = np.zeros((5, 7), np.uint8)
    occ[2, 3] = 1
    rng = np.random.default_rng(r)
    start = np.concatenate([_points(rng, 5, 7, 24, margin=0.4), [Fo.centre((2, 3), ORIGIN, CELL)]])
    got, _ = _check(occ, ORIGIN, CELL, [Fo.centre((4, 6), ORIGIN, CELL)], start, r)
    # the disc of radius r around (2, 3) holds 1, 5, 13 cells; at r = 2 it spans column j = 3 over all five rows, so the goal's side is
    # j > 3 and the 15 cells with j < 3 are cut off, 4 of them in the disc: INF on 13 + 11 cells
    blocked = Fo.blocked_cells(occ, r)
    inf = got["field"][0] == Fo.INF
    assert blocked.sum() == (1, 5, 13)[r] and inf[blocked].all() and inf.sum() == (1, 5, 24)[r]
    assert inf[:, :3].all() == (r == 2) and not inf[:, 4:][~blocked[:, 4:]].any()
    assert got["status"][-1] == Fo.START_OCCUPIED


@functools.lru_cache(maxsize=None)
def _random_maps():
    """33 x 17 (no multiple of the wave size), 30 % solid, three seeds; per map a goal in a free cell and 12 starts."""
    maps, goals, starts = [], [], []
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        occ = (rng.random((33, 17)) < 0.3).astype(np.uint8)
        maps.append(occ)
        goals.append(_free_point(rng, occ != 0))
        starts.append(np.concatenate([[_free_point(rng, occ != 0) for _ in range(8)], _points(rng, 33, 17, 4)]))
    return np.stack(maps), np.array(goals), np.array(starts)


def test_gpu_random_maps_one_map_per_robot():
    occ, goals, starts = _random_maps()
    got, want = _check(occ, ORIGIN, CELL, goals, starts[:, 0])            # F = B = 3: robot b on map b to goal b
    assert (want["status"] == Fo.FOUND).any()


@pytest.mark.parametrize("m", [0, 1, 2])
def test_gpu_random_maps_shared(m):
    occ, goals, starts = _random_maps()
    got, want = _check(occ[m], ORIGIN, CELL, goals[m:m + 1], starts[m])   # one field, 12 robots
    assert (want["status"] == Fo.FOUND).sum() >= 4
    _check(occ[m], ORIGIN, CELL, np.tile(goals[m], (12, 1)), starts[m], r=1)      # a shared map, one field per robot, inflated


def test_gpu_spiral_corridor():
    """A one-cell corridor of 263 cells: a relaxation that stops early leaves INF (or too large a value) at the far end."""
    occ, cells = Fo.spiral(24)
    got, want = _check(occ, ORIGIN, CELL, [Fo.centre(cells[-1], ORIGIN, CELL)], [Fo.centre(c, ORIGIN, CELL) for c in (cells[0], cells[100], cells[-1])])
    assert got["field"][0][cells[0]] == 5 * (len(cells) - 1) and got["status"].tolist() == [0, 0, 0] and got["n_sub"][2] == 1
    assert got["path_cost"][0] == len(cells) - 1


def test_gpu_maze_where_rrt_finds_nothing():
    m = Fo.maze()
    got, _ = _check(m["occ"], m["origin"], m["cell"], [m["goal"]], [m["start"]])
    assert got["status"][0] == Fo.FOUND and got["path_cost"][0] * 5 == 997
    got, _ = _check(m["occ"], m["origin"], m["cell"], [m["goal"]], [m["start"]], r=1)
    assert got["status"][0] == Fo.NO_PATH


def _walls(W, H):
    occ = np.zeros((W, H), np.uint8)
    occ[W // 4, : H - 9] = 1
    occ[W // 2, 7:] = 1
    occ[3 * W // 4, : H // 2] = 1
    occ[3 * W // 4, H // 2 + 9:] = 1
    occ[W // 2:, H // 3] = 1
    occ[W // 2 + 5:W // 2 + 12, H // 3] = 0
    return occ


@pytest.mark.parametrize("W,H", [(182, 181), (199, 199), (200, 199)])
def test_gpu_large_maps(W, H):
    """182 x 181: more than 32768 cells, the largest listed map; 199 x 199 is the largest square map whose field still fits the LDS
    (159.5 KiB) and 200 x 199 the first that is relaxed in the output buffer."""
    occ = _walls(W, H)
    rng = np.random.default_rng(5)
    starts = np.concatenate([[Fo.centre((1, 1), ORIGIN, CELL)], _points(rng, W, H, 7)])
    got, want = _check(occ, ORIGIN, CELL, [Fo.centre((W - 2, H - 3), ORIGIN, CELL)], starts, r=2, S_max=200)
    assert want["status"][0] == Fo.FOUND and want["path_cost"][0] > 1.5 * W


def test_gpu_goal_refusals():
    occ = np.zeros((9, 8), np.uint8)
    occ[4, 4] = 1
    start = [Fo.centre((0, 0), ORIGIN, CELL)] * 5
    goals = [(ORIGIN[0] - 0.01, 0.5), (float("nan"), 0.5), (0.0, float("inf")), Fo.centre((4, 4), ORIGIN, CELL), Fo.centre((5, 5), ORIGIN, CELL)]
    got, _ = _check(occ, ORIGIN, CELL, goals, start, r=2)                 # (5, 5): blocked by the inflation only
    assert got["field_status"].tolist() == [1, 1, 1, 2, 2] and (got["field"] == Fo.INF).all()
    assert got["status"].tolist() == [Fo.OUTSIDE_GRID] * 3 + [Fo.GOAL_OCCUPIED] * 2
    got, _ = _check(occ, ORIGIN, CELL, goals[4:], start[:1], r=1)         # the same goal is free under a smaller radius
    assert got["field_status"].tolist() == [0] and got["status"].tolist() == [0]


@functools.lru_cache(maxsize=None)
def _fleet_case():
    """48 x 36, r_inflate = 2: a solid block with a one-cell pocket (inflated, nothing finite around it), a closed room (cut off),
    a wall to walk around; 130 starts: twelve special ones, then random ones over the grid and a margin around it."""
    occ = np.zeros((48, 36), np.uint8)
    occ[4:13, 4:13] = 1
    occ[8, 8] = 0                                              # the pocket
    occ[20:31, 20] = occ[20:31, 30] = 1
    occ[20, 20:31] = occ[30, 20:31] = 1                        # the room: interior 9 x 9, its middle 5 x 5 unblocked
    occ[38, 6:] = 1
    rng = np.random.default_rng(9)
    special = [Fo.centre(c, ORIGIN, CELL) for c in ((5, 5), (8, 8), (25, 25), (3, 8), (13, 8), (37, 20), (45, 30), (24, 26), (26, 24))]
    special += [(float("nan"), 0.3), (ORIGIN[0] - 0.001, 0.3), (ORIGIN[0] + 48 * CELL[0], 0.3)]
    start = np.concatenate([special, _points(rng, 48, 36, 118, margin=1.5)])
    return occ, np.array([Fo.centre((45, 30), ORIGIN, CELL) + (0.01, -0.02)]), start


def test_gpu_one_field_many_robots():
    occ, goal, start = _fleet_case()
    assert len(start) == 130
    got, want = _check(occ, ORIGIN, CELL, goal, start, r=2)
    st = want["status"]
    assert st[:12].tolist() == [Fo.START_OCCUPIED, Fo.NO_PATH, Fo.NO_PATH, Fo.FOUND, Fo.FOUND, Fo.FOUND, Fo.FOUND, Fo.NO_PATH, Fo.NO_PATH] + [Fo.OUTSIDE_GRID] * 3
    assert want["snapped"][3] != (3, 8) and want["snapped"][4] != (13, 8) and want["snapped"][5] != (37, 20)       # inflated cells that snap
    assert want["n_sub"][6] == 1 and np.array_equal(_bits(got["sub_goals"][6, 0]), _bits(goal[0]))               # in the goal's cell: the goal itself
    blocked = Fo.blocked_cells(occ, 2)
    cells = [Fo.cell_of(s, ORIGIN, CELL, 48, 36) for s in start]
    snapped = sum(1 for c, s in zip(cells, want["snapped"]) if s is not None and s != c)
    cut_off = sum(1 for c, s in zip(cells, st) if c is not None and not blocked[c] and s == Fo.NO_PATH)
    print("statuses", np.bincount(st, minlength=8).tolist(), "snapped", snapped, "cut off", cut_off)
    assert snapped >= 8 and cut_off >= 3 and (st == Fo.OUTSIDE_GRID).sum() >= 8 and (st == Fo.START_OCCUPIED).sum() >= 4
    assert (st == Fo.FOUND).sum() >= 60


def test_gpu_path_overflow_writes_nothing_but_the_cost():
    m = Fo.maze()
    got, want = _check(m["occ"], m["origin"], m["cell"], [m["goal"]], [m["start"], m["goal"]], S_max=2)
    assert got["status"].tolist() == [Fo.PATH_OVERFLOW, Fo.FOUND] and got["n_sub"].tolist() == [0, 1]
    assert got["path_cost"][0] * 5 == 997 and (got["sub_goals"][0] == SENTINEL).all()
    n = Fo.plan(m["occ"], m["origin"], m["cell"], m["goal"], m["start"])["n_sub"]
    assert _check(m["occ"], m["origin"], m["cell"], [m["goal"]], [m["start"]], S_max=n)[0]["status"][0] == Fo.FOUND       # exactly enough
    assert _check(m["occ"], m["origin"], m["cell"], [m["goal"]], [m["start"]], S_max=n - 1)[0]["status"][0] == Fo.PATH_OVERFLOW


@pytest.mark.parametrize("max_seg", [5, 35, None])
def test_gpu_spacing_cap(max_seg):
    occ, goal, start = _fleet_case()
    got, want = _check(occ, ORIGIN, CELL, goal, start[:40], r=1, max_seg=max_seg, S_max=80)
    found = want["status"] == Fo.FOUND
    assert found.sum() >= 15
    if max_seg == 5:                                           # every path cell is a sub-goal
        assert all(want["n_sub"][b] == len(want["cells"][b]) - 1 or len(want["cells"][b]) == 1 for b in np.nonzero(found)[0])


def _captured(pl, goal, grid, start, out, S_max):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pl.plan_grid_batch(goal, grid, start, S_max=S_max, out=out)        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pl.plan_grid_batch(goal, grid, start, S_max=S_max, out=out)
    return graph


@pytest.mark.parametrize("case", ["fleet", "large"])
def test_gpu_graph_replay_and_repeat_give_the_same_bits(case):
    """Field + path captured in one graph and replayed twice equal the eager call; two eager calls equal each other."""
    if case == "fleet":
        occ, goal, start = _fleet_case()
    else:
        occ, goal, start = _walls(182, 181), np.array([Fo.centre((180, 178), ORIGIN, CELL)]), _points(np.random.default_rng(6), 182, 181, 16)
    W, H = occ.shape
    eager = [_run(occ, ORIGIN, CELL, goal, start, r=2) for _ in range(2)]
    for k in eager[0]:
        assert np.array_equal(_bits(eager[0][k]), _bits(eager[1][k])), k
    pl = lipmpc.GridFieldPlanner(r_inflate=2)
    grid = lipmpc.GridMap(occ, ORIGIN, CELL).to("cuda")
    d_goal, d_start = torch.as_tensor(goal, device="cuda"), torch.as_tensor(start, device="cuda")
    out = _buffers(len(start), 1, W, H, 64)
    graph = _captured(pl, d_goal, grid, d_start, out, 64)
    for _ in range(2):
        for k in ("n_sub", "status", "field_status"):
            out[k].fill_(-1)
        out["sub_goals"].fill_(SENTINEL)
        out["path_cost"].fill_(SENTINEL)
        out["field"].view(torch.int32).fill_(12345)
        graph.replay()
        torch.cuda.synchronize()
        got = _host(out)
        for k in eager[0]:
            assert np.array_equal(_bits(got[k]), _bits(eager[0][k])), k


def test_gpu_field_alone_and_argument_checks():
    occ, goal, start = _fleet_case()
    pl = lipmpc.GridFieldPlanner(r_inflate=2)
    grid = lipmpc.GridMap(occ, ORIGIN, CELL)
    f = pl.field(goal, grid)
    torch.cuda.synchronize()
    want, st = Fo.field(occ, ORIGIN, CELL, goal[0], 2)
    assert np.array_equal(f["field"].view(torch.int32).cpu().numpy().view(np.uint32)[0], want) and f["status"].tolist() == [st]
    assert tuple(f["field"].shape) == (1, 48, 36) and f["field"].dtype == torch.uint32
    zero = pl.plan_grid_batch(goal, grid, np.zeros((0, 2)))
    assert tuple(zero["sub_goals"].shape) == (0, 64, 2)
    fresh = pl.plan_grid_batch(goal, grid, start[3:4], seeds=[7])              # seeds: accepted and ignored; rows past n_sub are 0
    n = int(fresh["n_sub"][0])
    assert n >= 1 and (fresh["sub_goals"][0, n:] == 0).all() and set(fresh) >= {"sub_goals", "n_sub", "status", "path_cost", "field"}
    with pytest.raises(ValueError):
        pl.plan_grid_batch(np.zeros((2, 2)), grid, start[:5])                   # goal: [1,2] or [B,2]
    with pytest.raises(ValueError):
        lipmpc.GridFieldPlanner(r_inflate=17)
    with pytest.raises(ValueError):
        lipmpc.GridFieldPlanner(max_seg=4)
    with pytest.raises(ValueError):
        pl.plan_grid_batch(goal, lipmpc.GridMap(np.stack([occ, occ]), ORIGIN, CELL), start[:5])      # two maps, one field
