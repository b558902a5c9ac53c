"""CPU: the numpy restatement of the scan integration (tests/map_oracle.py, contract of lipmpc_map_update_batch in
include/lipmpc.h) does what the contract is for, on readings of the grid-scan oracle."""
import math

import numpy as np
import pytest

import grid_lidar_oracle as G
import map_oracle as M

CELL, RANGE = (0.05, 0.05), 1.5
ORIGIN = (-0.2, 0.1)


def _table(resolution=360):
    """The scans' ray table with the four axis rays EXACT (cos / sin of pi / 2 are not): 0, 90, 180 and 270 degrees."""
    step = 2 * math.pi / resolution
    t = np.array([[math.cos(i * step), math.sin(i * step)] for i in range(resolution)])
    q = resolution // 4
    t[0], t[q], t[2 * q], t[3 * q] = (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)
    return t


def _room():
    """A cell-aligned box seen from inside: a frame of solid cells, 3 cells thick, 17 cells from the centre cell -- every ray of
    a robot near the centre has a reading, in all four quadrants and on the four axes."""
    occ = np.zeros((64, 64), np.uint8)
    occ[13:52, 13:52] = 1
    occ[16:49, 16:49] = 0
    return occ


ROBOTS = np.array([[ORIGIN[0] + 32 * 0.05 + 0.012, ORIGIN[1] + 32 * 0.05 + 0.037],      # off-centre in its cell
                   [ORIGIN[0] + 30 * 0.05 + 0.031, ORIGIN[1] + 34 * 0.05 + 0.008],
                   [ORIGIN[0] + 32.5 * 0.05, ORIGIN[1] + 32.5 * 0.05]])                   # a cell centre: the axis rays run along cell middles


@pytest.fixture(scope="module")
def room_scan():
    occ, table = _room(), _table()
    return occ, table, M.oracle_hits(ROBOTS, occ, ORIGIN, CELL, RANGE, table)


def test_default_depth_puts_every_hit_inside_the_wall(room_scan):
    occ, table, hits = room_scan
    assert not np.isnan(hits).any()                       # every ray has a reading: all four quadrants, the four axes
    for b, p in enumerate(ROBOTS):
        _, hit, passed = M.robot_delta(p, hits[b], 64, 64, ORIGIN, CELL, RANGE, table, M.default_depth(CELL), 3, 1)
        assert hit.any() and passed.any()
        assert not (hit & (occ == 0)).any(), ("a hit cell is free", b, np.argwhere(hit & (occ == 0)))
        assert not (passed & (occ != 0)).any(), ("a solid cell was passed", b, np.argwhere(passed & (occ != 0)))
        # the faces seen: walls on all four sides were hit
        ii, jj = np.nonzero(hit)
        assert ii.min() == 15 and ii.max() == 49 and jj.min() == 15 and jj.max() == 49


def test_without_depth_a_reading_names_the_free_neighbour(room_scan):
    """Why ``depth`` exists: a reading lies exactly on the wall's face; for a ray travelling toward -x or -y floor() of it is
    the free cell in front of the wall."""
    occ, table, hits = room_scan
    free_hits = 0
    for b, p in enumerate(ROBOTS):
        _, hit, _ = M.robot_delta(p, hits[b], 64, 64, ORIGIN, CELL, RANGE, table, 0.0, 3, 1)
        free_hits += int((hit & (occ == 0)).sum())
    assert free_hits >= 1


def test_hit_wins_over_passed_within_a_scan():
    table = np.array([[1.0, 0.0], [1.0, 0.0]])            # two rays along +x: one with a reading, one without
    p = np.array([1.012, 1.013])
    hits = np.array([[p[0] + 0.5, p[1]], [np.nan, np.nan]])
    passed, hit, (wi0, wj0) = M.robot_marks(p, hits, (0.0, 0.0), CELL, RANGE, table, 0.025)
    k = np.argwhere(hit)
    assert len(k) == 1 and passed[k[0][0], k[0][1]]       # the other ray went through the hit cell
    d, hit_g, pas_g = M.robot_delta(p, hits, 80, 80, (0.0, 0.0), CELL, RANGE, table, 0.025, 5, 2)
    gi, gj = k[0][0] + wi0, k[0][1] + wj0
    assert (gi, gj) == (30, 20) and d[gi, gj] == 5 and not pas_g[gi, gj]
    assert d[20:30, 20].tolist() == [-2] * 10 and d[31:50, 20].tolist() == [-2] * 19       # before it, and behind it by the other ray
    assert d.sum() == 5 - 2 * int(pas_g.sum())


def test_shared_map_is_the_sum_of_the_per_robot_maps(room_scan):
    occ, table, hits = room_scan
    per = M.update(np.zeros((3, 64, 64), np.int64), ROBOTS, hits, ORIGIN, CELL, RANGE, table)
    sh = M.update(np.zeros((64, 64), np.int64), ROBOTS, hits, ORIGIN, CELL, RANGE, table)
    assert np.array_equal(sh, per.sum(0)) and np.abs(per).sum(axis=(1, 2)).min() > 0
    again = M.update(sh.copy(), ROBOTS, hits, ORIGIN, CELL, RANGE, table)
    assert np.array_equal(again, 2 * sh)


def test_masked_and_nan_robots_contribute_nothing(room_scan):
    occ, table, hits = room_scan
    pos = ROBOTS.copy()
    pos[1, 0] = np.nan
    ev = M.update(np.zeros((3, 64, 64), np.int64), pos, hits, ORIGIN, CELL, RANGE, table, mask=np.array([1, 1, 0]))
    assert np.abs(ev[0]).sum() > 0 and not ev[1].any() and not ev[2].any()
    far = np.array([[1e300, 0.0], [np.inf, 0.0], [0.0, -2.0 ** 31 * 0.05]])
    assert not M.update(np.zeros((3, 64, 64), np.int64), far, hits, ORIGIN, CELL, RANGE, table).any()


def test_cells_outside_the_grid_or_the_window_are_untouched():
    table = _table(8)
    p = np.array([0.26, 0.12])                            # near a corner of a small grid: most of the window is outside it
    hits = np.full((8, 2), np.nan)
    hits[0] = (p[0] + 40.0, p[1])                         # a reading far beyond the window: dropped, its ray stops at the window
    W, H = 90, 12
    d, hit_g, pas_g = M.robot_delta(p, hits, W, H, (0.0, 0.0), CELL, RANGE, table, 0.025, 3, 1)
    nx, ny = M.window_half(RANGE, 0.025, CELL)
    assert (nx, ny) == (32, 32) and not hit_g.any()
    ci = 5
    assert d[ci:ci + nx + 1, 2].tolist() == [-1] * (nx + 1) and not d[ci + nx + 1:, :].any()       # the +x ray: to the window's edge, no further
    assert d.min() == -1 and d.max() == 0
    # ray 4 (-x) leaves the grid after 5 cells and ray 6 (-y) after 2: nothing is written for the cells outside
    assert d[:ci, 2].tolist() == [-1] * ci and d[ci, :3].tolist() == [-1] * 3
    # a window that does not meet the grid at all
    assert not M.robot_delta(np.array([-9.0, -9.0]), hits, W, H, (0.0, 0.0), CELL, RANGE, table, 0.025, 3, 1)[0].any()


def test_window_cap():
    assert M.window_fits(1.5, 0.025, CELL) and M.window_fits(5.4, 0.0, CELL) and not M.window_fits(5.5, 0.0, CELL)
    assert not M.window_fits(5.4, 0.1, CELL)               # the depth counts toward the reach
    assert M.LDS_BYTES == 12288


def test_goal_selection_rule():
    pos = np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
    goal = np.array([[5.0, 5.0]] * 4)
    sub = np.zeros((4, 3, 2))
    sub[:, 0], sub[:, 1], sub[:, 2] = (0.3, 0.4), (0.6, 0.8), (3.0, 4.0)
    n_sub = np.array([3, 3, 2, 3])
    status = np.array([0, 0, 0, 1])
    # exactly at the lookahead counts (0.5 >= 0.5); the first far enough; none among the n_sub first -> the goal; not FOUND -> the goal
    assert M.select_goals(pos, goal, sub, n_sub, status, 0.5).tolist() == [[0.3, 0.4], [0.3, 0.4], [0.3, 0.4], [5.0, 5.0]]
    assert M.select_goals(pos, goal, sub, n_sub, status, 0.75).tolist() == [[0.6, 0.8], [0.6, 0.8], [0.6, 0.8], [5.0, 5.0]]
    assert M.select_goals(pos, goal, sub, n_sub, status, 2.0).tolist() == [[3.0, 4.0], [3.0, 4.0], [5.0, 5.0], [5.0, 5.0]]
    assert M.select_goals(pos, goal, sub, n_sub, np.full(4, 5), 0.5).tolist() == goal.tolist()      # NO_OBSTACLE_GRID: straight for the goal
