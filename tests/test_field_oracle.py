"""CPU: the numpy restatement of the grid field planner (tests/field_oracle.py) against brute force, and the completeness
example -- a maze in which the RRT* oracle finds no path with any of four seeds and the field planner finds the shortest one."""
import numpy as np

import field_oracle as Fo
import rrt_grid_oracle as RG
import rrt_oracle as R


def _flood(blocked, g):
    """The cells a flood fill by the field's move rules reaches from g."""
    seen, todo = {g}, [g]
    while todo:
        i, j = todo.pop()
        for a, b, _ in Fo.moves_from(blocked, i, j):
            if (a, b) not in seen:
                seen.add((a, b))
                todo.append((a, b))
    return seen


def test_field_is_finite_exactly_where_a_flood_fill_reaches():
    rng = np.random.default_rng(11)
    n_ok = 0
    for _ in range(200):
        W, H, r = int(rng.integers(2, 13)), int(rng.integers(2, 10)), int(rng.integers(0, 3))
        occ = (rng.random((W, H)) < rng.choice([0.05, 0.15, 0.3])).astype(np.uint8)
        origin, cell = (-0.3, 0.2), (0.1, 0.25)
        goal = (origin[0] + rng.uniform(0, W) * cell[0], origin[1] + rng.uniform(0, H) * cell[1])
        fld, st = Fo.field(occ, origin, cell, goal, r)
        blocked = Fo.blocked_cells(occ, r)
        g = Fo.cell_of(goal, origin, cell, W, H)
        assert g is not None
        # the blocked set, cell by cell from its definition
        for i in range(W):
            for j in range(H):
                want = any(occ[a, b] and (i - a) ** 2 + (j - b) ** 2 <= r * r for a in range(W) for b in range(H))
                assert blocked[i, j] == want
        if blocked[g]:
            assert st == Fo.FIELD_GOAL_BLOCKED and (fld == Fo.INF).all()
            continue
        n_ok += 1
        assert st == Fo.FIELD_OK and fld[g] == 0
        reach = _flood(blocked, g)
        assert {(int(i), int(j)) for i, j in zip(*np.nonzero(fld != Fo.INF))} == reach
        for c in reach - {g}:
            assert any(int(fld[a, b]) + cost == int(fld[c]) for a, b, cost in Fo.moves_from(blocked, *c)), c
            assert all(int(fld[a, b]) + cost >= int(fld[c]) for a, b, cost in Fo.moves_from(blocked, *c) if fld[a, b] != Fo.INF), c
            assert len(Fo.descend(fld, c)) >= 2
    assert n_ok >= 100


def test_goal_outside_and_nan():
    occ = np.zeros((5, 7), np.uint8)
    for goal in ((-0.01, 0.3), (0.3, 0.75), (0.55, 0.1), (float("nan"), 0.1), (0.1, float("inf"))):
        fld, st = Fo.field(occ, (0.0, 0.0), (0.1, 0.1), goal)
        assert st == Fo.FIELD_GOAL_OUTSIDE and (fld == Fo.INF).all(), goal
        assert Fo.plan(occ, (0.0, 0.0), (0.1, 0.1), goal, (0.05, 0.05))["status"] == Fo.OUTSIDE_GRID


def test_maze_rrt_finds_nothing_the_field_planner_finds_the_shortest_path():
    """The completeness example of the issue: RRT* at the reference's own n = 1500, r_rewire = 80 returns NO_PATH for seeds 1-4;
    a path of 997 field units (about 199 cells) exists."""
    m = Fo.maze()
    for seed in (1, 2, 3, 4):
        r = RG.plan_grid(m["occ"], m["origin"], m["cell"], m["goal"], start=m["start"], seed=seed, n=1500, r_rewire=80)
        assert r["status"] == R.NO_PATH, (seed, r["status"])
    fld, st = Fo.field(m["occ"], m["origin"], m["cell"], m["goal"])
    p = Fo.plan(m["occ"], m["origin"], m["cell"], m["goal"], m["start"], fld=fld, field_status=st)
    assert p["status"] == Fo.FOUND and p["path_cost"] * 5 == 997 and int(fld[p["snapped"]]) == 997
    assert p["n_sub"] >= 10 and np.array_equal(p["sub_goals"][-1], np.asarray(m["goal"]))
    cells = [Fo.cell_of(m["start"], m["origin"], m["cell"], 40, 40)] + [Fo.cell_of(s, m["origin"], m["cell"], 40, 40) for s in p["sub_goals"]]
    for a, b in zip(cells[:-1], cells[1:]):
        assert Fo.los(fld, a, b), (a, b)
    # the spacing cap: every leg's path cost stays below it (a single step may reach it)
    for cap in (5, 35):
        q = Fo.plan(m["occ"], m["origin"], m["cell"], m["goal"], m["start"], max_seg=cap, S_max=1000, fld=fld, field_status=st)
        cs = [cells[0]] + [Fo.cell_of(s, m["origin"], m["cell"], 40, 40) for s in q["sub_goals"]]
        legs = [int(fld[a]) - int(fld[b]) for a, b in zip(cs[:-1], cs[1:])]
        assert q["status"] == Fo.FOUND and sum(legs) == 997 and all(leg < cap or leg in (5, 7) for leg in legs), (cap, legs)
    assert Fo.plan(m["occ"], m["origin"], m["cell"], m["goal"], m["start"], S_max=3)["status"] == Fo.PATH_OVERFLOW


def test_maze_gaps_close_under_inflation():
    m = Fo.maze()
    p = Fo.plan(m["occ"], m["origin"], m["cell"], m["goal"], m["start"], r_inflate=1)
    assert p["status"] == Fo.NO_PATH and p["n_sub"] == 0 and np.isnan(p["path_cost"])


def test_snap_takes_the_nearest_finite_cell():
    occ = np.zeros((9, 9), np.uint8)
    occ[4, :] = 1
    occ[4, 8] = 0                                              # a wall with a gap at the far end
    origin, cell = (0.0, 0.0), (0.1, 0.1)
    fld, st = Fo.field(occ, origin, cell, (0.85, 0.05), r_inflate=1)
    assert st == Fo.FIELD_OK and fld[5, 0] == Fo.INF and fld[6, 0] != Fo.INF and fld[2, 0] == Fo.INF     # (the gap closed: cut off)
    p = Fo.plan(occ, origin, cell, (0.85, 0.05), (0.55, 0.05), r_inflate=1, fld=fld, field_status=st)     # in the inflated band
    assert p["status"] == Fo.FOUND and p["snapped"] == (6, 0) and p["path_cost"] == 2.0
    assert Fo.plan(occ, origin, cell, (0.85, 0.05), (0.35, 0.05), r_inflate=1)["status"] == Fo.NO_PATH   # inflated, nothing finite in the window
    assert Fo.plan(occ, origin, cell, (0.85, 0.05), (0.15, 0.05), r_inflate=1)["status"] == Fo.NO_PATH   # free, but cut off
    assert Fo.plan(occ, origin, cell, (0.85, 0.05), (0.45, 0.05), r_inflate=1)["status"] == Fo.START_OCCUPIED
    assert Fo.plan(occ, origin, cell, (0.85, 0.05), (0.95, 0.05), r_inflate=1)["status"] == Fo.OUTSIDE_GRID


def test_spiral_path_runs_the_whole_corridor():
    occ, cells = Fo.spiral(24)
    assert len(cells) > 250
    origin, cell = (0.0, 0.0), (0.1, 0.1)
    p = Fo.plan(occ, origin, cell, Fo.centre(cells[-1], origin, cell), Fo.centre(cells[0], origin, cell))
    assert p["status"] == Fo.FOUND and p["cells"] == cells and p["path_cost"] == len(cells) - 1
