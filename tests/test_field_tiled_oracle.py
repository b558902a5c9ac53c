"""CPU: the inputs of the tiled field tests (tests/field_tiled_cases.py) reach what they claim, shown on the oracles
(tests/field_oracle.py, tests/frontier_oracle.py) -- so that a GPU test that passes has crossed the tile borders it is about."""
import numpy as np
import pytest

import field_oracle as Fo
import field_tiled_cases as T
import frontier_oracle as FR

TW, TH = T.TW, T.TH


def _shape(c):
    return c["occ"].shape[-2:]


def test_tile_sides_and_cap():
    assert TW >= 2 and TH >= 2 and T.MAX_CELLS == 1 << 24
    # a tile with its halo, a field word and a blocked bit per cell, fits LDS many times over
    assert (TW + 2) * (TH + 2) * (4 + 1 / 8) <= 160 * 1024 / 4


def test_shapes_are_derived_from_the_tile():
    want = {"2x2": (2, 2), "one_tile": (TW, TH), "over_under": (TW + 1, TH - 1), "under_over": (TH - 1, TW + 1),
            "baffles": (3 * TW + 1, 2 * TH + 5), "363x362": (363, 362)}
    for id_, shape in want.items():
        assert _shape(T.case(id_)) == shape, id_
    assert 363 * 362 > Fo.MAX_CELLS >= 362 * 362               # the first shape the one-workgroup calls refuse
    for id_ in T.IDS:
        c = T.case(id_)
        F = 1 if c["occ"].ndim == 2 else len(c["occ"])
        assert c["ev"].shape == c["occ"].shape and len(c["goal"]) in (1, len(c["start"])) and F in (1, len(c["start"])), id_


@pytest.mark.parametrize("id_", ["one_tile", "over_under", "under_over", "baffles", "130_robots", "363x362"])
def test_strips_are_crossed(id_):
    """Both planners find paths on the strips, and the path from cell (0, 0) is longer than the long side (it winds round baffles)."""
    c = T.case(id_)
    W, H = _shape(c)
    for planner in ("field", "frontier"):
        want = T.oracle(id_, planner)
        assert want["status"][0] == Fo.FOUND and (want["status"] == Fo.FOUND).sum() >= len(c["start"]) // 2, (planner, want["status"])
        assert want["path_cost"][0] > max(W, H)
    tiles = {T.tile_of(cell) for cell in T.oracle(id_, "field")["cells"][0]}
    assert len(tiles) >= min(-(-W // TW) * -(-H // TH), 4)    # the path from (0, 0) visits several tiles where there are several
    if id_ == "130_robots":
        assert len(c["start"]) == 130 and len(set(T.oracle(id_, "field")["status"])) >= 3


def test_two_by_two():
    want = T.oracle("2x2", "field")
    assert want["field"][0].tolist() == [[7, 5], [5, 0]] and want["status"].tolist() == [Fo.FOUND, Fo.FOUND]
    want = T.oracle("2x2", "frontier")
    assert want["n_frontier"].tolist() == [3] and want["field"][0].tolist() == [[0, 0], [0, Fo.INF]]


def test_spiral_changes_tile_20_times():
    c = T.case("spiral")
    for planner in ("field", "frontier"):
        want = T.oracle("spiral", planner)
        path = want["cells"][0]
        assert want["status"][0] == Fo.FOUND and path[0] == c["cells"][0]
        assert T.tile_changes(path) >= 20, T.tile_changes(path)
        assert len(path) >= len(c["cells"]) - 2 and set(path) <= set(c["cells"])      # the corridor itself: there is no other way
    print("spiral:", len(c["cells"]), "corridor cells,", T.tile_changes(T.oracle("spiral", "field")["cells"][0]), "tile changes")


def test_corner_goals_lie_in_four_tiles():
    c = T.case("corner_goals")
    cells = [Fo.cell_of(g, T.ORIGIN, T.CELL, 2 * TW, 2 * TH) for g in c["goal"]]
    assert cells == list(T.CORNER) and len({T.tile_of(g) for g in cells}) == 4
    want = T.oracle("corner_goals", "field")
    assert want["status"].tolist() == [Fo.FOUND] * 4 and all(want["field"][f][cells[f]] == 0 for f in range(4))
    want = T.oracle("corner_goals", "frontier")
    assert want["n_frontier"].tolist() == [8] * 4
    for f in range(4):                                         # every map's frontier lies in all four tiles
        assert len({T.tile_of(tuple(x)) for x in np.argwhere(want["frontier"][f] != 0)}) == 4


def test_corner_cuts_differ_by_one_blocked_bit():
    c = T.case("corner_cuts")
    target, side_a, side_b, mover = T.CORNER
    assert len({T.tile_of(x) for x in T.CORNER}) == 4           # the mover, the target and each side cell in a tile of its own
    for occ_or_ev, blocked in ((c["occ"], lambda m: Fo.blocked_cells(m, 0)),
                               (c["ev"], lambda m: FR.masks(m, T.T_FREE, T.T_OCC, 0, c["mu"])[0])):
        b = [blocked(m) for m in occ_or_ev]
        assert (b[0] != b[1]).sum() == 1 and (b[1] != b[2]).sum() == 1
        assert [bool(x[side_a]) for x in b] == [False, True, True] and [bool(x[side_b]) for x in b] == [False, False, True]
    want = T.oracle("corner_cuts", "field")["field"]
    assert want[0][mover] == 7 and want[1][mover] == 10 and 10 < want[2][mover] < Fo.INF
    want = T.oracle("corner_cuts", "frontier")
    assert want["n_frontier"].tolist() == [1, 1, 1] and all(f[target] == 0 for f in want["field"])
    assert want["field"][0][mover] == 7 and want["field"][1][mover] == 10 and want["field"][2][mover] > 10


def test_disc_spans_a_tile_border_and_a_word_border():
    c = T.case("disc16")
    W, H = _shape(c)
    blocked = Fo.blocked_cells(c["occ"], 16)
    run = np.nonzero(blocked[TW])[0]
    assert run.min() == TH - 16 and run.max() == TH + 16 and (TW * H + TH) % 32 == 0
    assert {T.tile_of(tuple(x)) for x in np.argwhere(blocked)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    want = T.oracle("disc16", "field")
    assert want["status"].tolist() == [Fo.FOUND] * 5 and want["snapped"][1] != (TW, TH - 16) and want["snapped"][3] == (TW, TH - 17)
    assert T.oracle("disc16", "frontier")["n_frontier"][0] >= 1


def test_refusing_cases():
    assert T.oracle("no_frontier", "frontier")["n_frontier"].tolist() == [0]
    assert set(T.oracle("no_frontier", "frontier")["status"]) <= {Fo.NO_PATH, Fo.OUTSIDE_GRID, Fo.START_OCCUPIED}
    want = T.oracle("bad_goals", "field")
    assert want["field_status"].tolist() == [Fo.FIELD_GOAL_OUTSIDE, Fo.FIELD_GOAL_BLOCKED]
    assert want["status"].tolist() == [Fo.OUTSIDE_GRID, Fo.GOAL_OCCUPIED]


def test_three_maps_need_different_rounds():
    """The path from cell (0, 0) changes tile a different number of times on each map."""
    for planner in ("field", "frontier"):
        want = T.oracle("three_maps", planner)
        changes = [T.tile_changes(p) for p in want["cells"]]
        assert want["status"].tolist() == [Fo.FOUND] * 3 and len(set(changes)) == 3, changes


def test_guaranteed_cells_of_the_spiral():
    """What the budget test holds the device to: after one round the guarantee covers the goal's tile's part of the corridor's end
    and nothing beyond; after tile_changes + 1 rounds it covers every finite cell."""
    want = T.oracle("spiral", "field")
    fld, path = want["field"][0], want["cells"][0]
    n = T.tile_changes(path)
    one, all_ = T.guaranteed(fld, 1), T.guaranteed(fld, n + 1)
    assert one[path[-1]] and not one[path[0]] and 0 < one.sum() < (fld != Fo.INF).sum()
    assert np.array_equal(all_, fld != Fo.INF) and not T.guaranteed(fld, n)[path[0]]
