"""CPU: the inputs of the window tests (tests/window_cases.py) reach what they are meant to reach, shown on the two numpy oracles
alone -- no case of tests/test_lidar_grid_windows_gpu.py or tests/test_map_windows_gpu.py is vacuous.  Every bar here is a
condition the inputs were chosen to meet, not a measurement."""
import math

import numpy as np
import pytest

import grid_lidar_oracle as G
import map_oracle as M
import window_cases as WC

# the intended windows, restated: id -> (scan window, map window with the case's depth)
SAME = {"w9x5": (9, 5), "w23x23": (23, 23), "w35x35": (35, 35), "w63x63": (63, 63), "w65x65": (65, 65), "w11x305": (11, 305),
        "w305x11": (305, 11), "w221x221": (221, 221), "w5x9829": (5, 9829), "w9829x5": (9829, 5), "per_robot_23": (23, 23),
        "per_robot_cap": (5, 9829), "exact4": (37, 37), "exact8": (37, 37), "origin1e6": (65, 65), "cell2p30": (45, 45),
        "g1x1": (23, 23), "g3000x1": (65, 65), "g1x3000": (65, 65), "g20x20": (65, 65), "range0": (5, 5), "synthetic": (65, 65)}
SAME.update({f"res{R}": (35, 35) for R in WC.SCAN_RESOLUTIONS})
CAP = 49152


def _window(reach, cell):
    """The rule, restated: half-sizes floor(reach / cell) + 2 per axis, the window 2 n + 1 cells across."""
    return tuple(2 * (int(math.floor(reach / c)) + 2) + 1 for c in cell)


def _fits(reach, cell):
    ww, wh = _window(reach, cell)
    return ww * wh <= CAP


def test_every_window_is_the_intended_one_and_the_refusal_rule():
    assert set(SAME) == set(WC.CASE_IDS) and G.WINDOW_CELLS == M.WINDOW_CELLS == CAP
    for i, c in WC.all_cases().items():
        assert c["window"] == SAME[i] == _window(c["lidar_range"], c["cell"]), i
        assert c["map_window"] == SAME[i] == _window(np.float64(c["lidar_range"]) + np.float64(c["depth"]), c["cell"]), i
        assert _fits(c["lidar_range"], c["cell"]) and G.window_fits(c["lidar_range"], c["cell"]), i
        assert M.window_fits(c["lidar_range"], c["depth"], c["cell"]), i
        assert c["depth"] > 0.0 and c["noisy"] == (i not in WC.NOISE_FREE_IDS), i
    # the cap: 49 145 cells is the most a 5-wide window can have and fit; 221 x 221 = 48 841: 764 trips, no multiple of 8
    assert 5 * 9829 == 49145 <= CAP < 5 * 9831 and (49145 + 63) // 64 == 768 and (221 * 221 + 63) // 64 == 764 and 764 % 8 != 0
    assert 9 * 5 < WC.TRIP
    r = WC.REFUSED
    assert _window(r["lidar_range"], r["cell"]) == r["window"] == (5, 9831)
    assert not G.window_fits(r["lidar_range"], r["cell"]) and not M.window_fits(r["lidar_range"], 0.0, r["cell"])
    d = WC.REFUSED_BY_DEPTH
    assert _window(d["lidar_range"], d["cell"]) == d["window"] and G.window_fits(d["lidar_range"], d["cell"])
    assert M.window_fits(d["lidar_range"], 0.0, d["cell"]) and M.window_fits(d["lidar_range"], WC.CAP_DEPTH, d["cell"])
    assert _window(d["lidar_range"] + d["depth"], d["cell"]) == d["map_window"] == (5, 9831)
    assert not M.window_fits(d["lidar_range"], d["depth"], d["cell"])
    # which ids run where
    assert set(WC.SCAN_IDS) | set(WC.MAP_IDS) == set(WC.CASE_IDS)
    assert {f"res{R}" for R in WC.MAP_RESOLUTIONS} <= set(WC.MAP_IDS) and {f"res{R}" for R in WC.SCAN_RESOLUTIONS} <= set(WC.SCAN_IDS)


@pytest.mark.parametrize("case_id", WC.SCAN_IDS)
def test_scan_cases_have_readings_and_a_robot_without(case_id):
    """At least one reading per robot on average and a robot with none.  Two exceptions that the arithmetic forces: with ONE ray a
    robot has at most one reading, so with a robot that has none the average is below one -- there every robot but the far one
    has its reading; and a range of zero gives no reading at all (the GPU test requires exactly that)."""
    c = WC.case(case_id)
    n = np.array([int(valid.sum()) for _, valid, _ in WC.scan_oracle(case_id)])
    B = len(c["pos"])
    assert (n == 0).any()
    if case_id == "range0":
        assert not n.any()
    elif c["resolution"] == 1:
        assert n.sum() == B - len(c["far"]) and all(n[b] == 0 for b in c["far"])
    else:
        assert n.sum() >= B, (int(n.sum()), B)
    # far robots have a cell but their window does not meet the grid; unplaced robots have no cell: exactly the intended ones
    nx, ny = G.window_half(c["lidar_range"], c["cell"])
    for b in range(B):
        cell0 = G.robot_cell(c["pos"][b], c["origin"], c["cell"])
        assert (cell0 is None) == (b in c["unplaced"]), b
        if b in c["far"]:
            assert n[b] == 0 and (cell0[0] - nx >= c["W"] or cell0[0] + nx < 0 or cell0[1] - ny >= c["H"] or cell0[1] + ny < 0), b
        if b in c["unplaced"]:
            assert n[b] == 0


def test_the_cell_limit_robots_are_the_intended_ones():
    c = WC.case("cell2p30")
    idx = [G.robot_cell(p, c["origin"], c["cell"]) for p in c["pos"]]
    assert [i is None for i in idx] == [False] * 16 + [True] * 4
    lim = 2 ** 30 - 1
    assert [idx[12][0], idx[13][0], idx[14][1], idx[15][1]] == [lim, -lim, lim, -lim]
    for p, (axis, sign) in zip(c["pos"][16:], ((0, 1), (0, -1), (1, 1), (1, -1))):
        assert math.floor((p[axis] - c["origin"][axis]) / c["cell"][axis]) == sign * 2 ** 30


def _map_inputs(case_id):
    """What the GPU test uploads, with the oracle's scan in the place of the device's (the two are held equal bit for bit)."""
    c = WC.case(case_id)
    return c, WC.map_readings(c, WC.oracle_hits(case_id)), WC.map_mask(c)


@pytest.mark.parametrize("case_id", WC.MAP_IDS)
def test_map_cases_have_hit_and_passed_cells(case_id):
    c, hits, mask = _map_inputs(case_id)
    d = WC.map_deltas(c, hits, mask)
    assert (d == c["w_hit"]).any() and (d == -c["w_miss"]).any(), case_id
    assert d[0].any() and not d[1].any()                     # robot 0 carries the corner reading; robot 1 is the masked one
    if case_id == "synthetic":
        d2 = d[2]
        print(f"synthetic readings: {int((d2 > 0).sum())} hit cells, {int((d2 < 0).sum())} passed cells")
        assert (d2 > 0).sum() >= 2 and (d2 < 0).sum() >= 100


@pytest.mark.parametrize("case_id", WC.EDGE_IDS)
def test_last_row_and_column_of_the_window_hold_something(case_id):
    """A mis-stepped (li, lj) lands on the last row or column: the scan stages solid cells there, the update has a mark there that
    is a cell of the grid."""
    c = WC.case(case_id)
    ww, wh = c["window"]
    staged = np.concatenate([WC.staged_solid(c, b) for b in range(len(c["pos"]))])
    assert (staged[:, 0] == ww - 1).any() and (staged[:, 1] == wh - 1).any() and (staged[:, 0] == 0).any() and (staged[:, 1] == 0).any()
    _, hits, _ = _map_inputs(case_id)
    passed, hit, (wi0, wj0), _ = WC.map_marks(c, hits, 0)
    assert hit[ww - 1, wh - 1] and 0 <= wi0 + ww - 1 < c["W"] and 0 <= wj0 + wh - 1 < c["H"]


@pytest.mark.parametrize("case_id", WC.CAP_IDS)
def test_cap_cases_reach_the_last_trips(case_id):
    """Beyond trip 760 of the 764 / 768: the scan stages solid cells there (a READING cannot lie there unless the long side comes
    first -- the window's last columns are two columns of cells from the robot, further than the range -- so the 9829 x 5 case
    has readings there and the others have staged cells), the update has marks there."""
    c = WC.case(case_id)
    ww, wh = c["window"]
    bits = np.concatenate([s[:, 0] * wh + s[:, 1] for s in (WC.staged_solid(c, b) for b in range(len(c["pos"])))])
    assert (bits >= WC.LAST_TRIPS * WC.TRIP).any(), int(bits.max())
    if case_id == "w9829x5":
        h, valid, _ = WC.scan_oracle(case_id)[0]
        i = np.floor((h[valid, 0] - c["origin"][0]) / c["cell"][0]) - (G.robot_cell(c["pos"][0], c["origin"], c["cell"])[0] - ww // 2)
        assert (i * wh >= WC.LAST_TRIPS * WC.TRIP).any()
    if case_id in WC.MAP_IDS:
        _, hits, _ = _map_inputs(case_id)
        passed, hit, _, _ = WC.map_marks(c, hits, 0)
        assert np.flatnonzero(passed | hit).max() >= WC.LAST_TRIPS * WC.TRIP


@pytest.mark.parametrize("case_id", WC.EXACT_IDS)
def test_exact_positions_meet_ties_and_crossings_at_zero(case_id):
    """Robots on cell boundaries: first crossings at t = 0 at either resolution.  t_x == t_y needs a ray off the axes (with 4 rays
    every ray has d_x = 0 or d_y = 0, one crossing parameter infinite), so the ties are required of the 8-ray case; there the
    scan also has a reading in a cell that is entered only because the tie goes to x."""
    c = WC.case(case_id)
    counts = [n for *_, n in WC.scan_oracle(case_id)]
    assert sum(n["t0"] for n in counts) >= 1
    _, hits, _ = _map_inputs(case_id)
    marks = [WC.map_marks(c, hits, b)[3] for b in range(len(c["pos"]))]
    assert sum(n["t0"] for n in marks) >= 1
    # robot 5: solid cells exactly the range away on its axis rays and nothing before them -- met at t = 1, dropped by `< range`
    p5, (ci, cj), step = c["pos"][5], WC.EXACT_RIM, c["resolution"] // 4
    assert G.robot_cell(p5, c["origin"], c["cell"]) == (ci, cj) and (c["origin"][0] + (ci + 16) * c["cell"][0]) - p5[0] == c["lidar_range"]
    assert p5[0] - (c["origin"][0] + (ci - 16) * c["cell"][0]) == c["lidar_range"] == (c["origin"][1] + (cj + 16) * c["cell"][1]) - p5[1]
    assert c["occ"][ci + 16, cj] and c["occ"][ci - 17, cj] and c["occ"][ci, cj + 16] and c["occ"][ci, cj - 17]
    assert not c["occ"][ci - 16:ci + 16, cj].any() and not c["occ"][ci, cj - 16:cj + 16].any()
    assert not WC.scan_oracle(case_id)[5][1][::step].any()
    if c["resolution"] == 8:
        assert sum(n["ties"] for n in counts) >= 1 and sum(n["ties"] for n in marks) >= 1
        h, valid, _ = WC.scan_oracle(case_id)[2]              # the robot on a corner, the ray at 45 degrees: the cell (3, 2) from its own
        ci, cj = G.robot_cell(c["pos"][2], c["origin"], c["cell"])
        assert valid[1] and h[1, 0] == c["origin"][0] + (ci + 3) * c["cell"][0]


def test_optional_counts_change_no_result():
    c = WC.case("exact8")
    import lidar_oracle as L
    table = L.ray_table(8)
    for b, p in enumerate(c["pos"]):
        a = G.grid_hits(p, c["occ"], c["origin"], c["cell"], c["lidar_range"], table)
        h, v, _ = WC.scan_oracle("exact8")[b]
        assert len(a) == 2 and np.array_equal(a[0], h) and np.array_equal(a[1], v)
    hits = WC.oracle_hits("exact8")
    m3 = M.robot_marks(c["pos"][0], hits[0], c["origin"], c["cell"], c["lidar_range"], table, c["depth"])
    m4 = M.robot_marks(c["pos"][0], hits[0], c["origin"], c["cell"], c["lidar_range"], table, c["depth"], counts=True)
    assert len(m3) == 3 and len(m4) == 4 and all(np.array_equal(x, y) for x, y in zip(m3, m4[:3]))
