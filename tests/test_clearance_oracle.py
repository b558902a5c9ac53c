"""CPU: do the soft-clearance cases of tests/clearance_cases.py reach what they claim, and does the weighted oracle
(tests/clearance_oracle.py) reduce to the unweighted ones at zero cost?  No GPU, no library call beyond the host-only tile sizes."""
import numpy as np
import pytest

import clearance_cases as K
import clearance_oracle as CO
import field_oracle as Fo
import field_tiled_cases as T
import frontier_oracle as FR

KINDS = ("field", "frontier")


def _same_plans(a, b, keys):
    for k in keys:
        if k in ("sub_goals", "cells"):
            assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


def test_the_cost_layer_by_hand():
    solid = np.zeros((9, 12), bool)
    solid[4, 5] = True
    c = CO.clearance_cost(solid, 3, 90)
    assert c[4, 5] == 90 and c[4, 6] == 80 and c[5, 6] == 70 and c[4, 7] == 50 and c[6, 7] == 10 and c[4, 8] == 0 and c[7, 5] == 0
    assert (c > 0).sum() == 25                              # d2 < 9: the open disc, 25 cells
    assert not CO.clearance_cost(np.zeros((4, 4), bool), 31, 248).any()
    assert (CO.clearance_cost(solid, 31, 0) == 0).all()
    # integer division, and the nearest of two solid cells
    solid[4, 9] = True
    c = CO.clearance_cost(solid, 2, 7)
    assert c[4, 7] == 0 and c[4, 6] == (7 * 3) // 4 and c[4, 8] == (7 * 3) // 4 and c[5, 6] == (7 * 2) // 4
    ev = np.where(solid, 3, -1).astype(np.int32)
    ev[0, 0], ev[0, 1], ev[8, 11] = 2, np.iinfo(np.int32).min, np.iinfo(np.int32).max
    e = CO.clearance_cost_evidence(ev, 3, 2, 7)
    assert e[8, 11] == 7 and e[0, 0] == 0 and e[0, 1] == 0 and e[4, 5] == 7


def test_the_two_door_map_switches_doors():
    """The issue's example: unweighted and at w_clear 16 the path takes the one-cell door, at w_clear 40 the nine-cell door, where
    r_inflate = 1 would have closed the narrow one altogether; both are FOUND."""
    occ = K.two_door_occ()
    start, goal = K.S.centre((2, 4)), K.S.centre((21, 4))
    plain = Fo.plan(occ, K.ORIGIN, K.CELL, goal, start)
    assert plain["status"] == Fo.FOUND and round(plain["path_cost"] * 5) == 95 and len(plain["cells"]) == 20 and K.door_of(plain["cells"]) == K.NARROW
    got = {}
    for r, w in ((4, 16), (4, 40), (4, 248), (8, 40)):
        p = CO.plan(occ, CO.clearance_cost(occ != 0, r, w), K.ORIGIN, K.CELL, goal, start)
        assert p["status"] == CO.FOUND
        got[r, w] = round(p["path_cost"] * 5), len(p["cells"]), K.door_of(p["cells"])
    print(got)
    assert got[4, 16] == (172, 20, K.NARROW)
    assert got[4, 40] == got[4, 248] == (240, 43, 23) and got[8, 40][2] == 24
    hard = Fo.plan(occ, K.ORIGIN, K.CELL, goal, start, r_inflate=1)           # the narrow door does not exist for r_inflate = 1
    assert hard["status"] == Fo.FOUND and K.door_of(hard["cells"]) in K.WIDE
    # the cases the GPU test runs: the two routes differ, neither is NO_PATH
    a, b = K.oracle("two_door_w16", "field"), K.oracle("two_door", "field")
    assert a["status"][0] == b["status"][0] == CO.FOUND and K.door_of(a["cells"][0]) == K.NARROW and K.door_of(b["cells"][0]) in K.WIDE


ZERO = [(i, k) for i in K.ZERO_IDS for k in KINDS if (i, k) != ("no_frontier", "field")]       # (no_frontier is a frontier case)


@pytest.mark.parametrize("id_,kind", ZERO)
def test_zero_layer_is_the_unweighted_oracle_on_the_tiled_cases(id_, kind):
    want, got = T.oracle(id_, kind), K.zero_oracle(id_, kind)
    _same_plans(got, want, [k for k in want if k != "snapped"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("id_", K.IDS)
def test_zero_layer_is_the_unweighted_oracle_on_the_clearance_cases(id_, kind):
    c = K.case(id_)
    got = K.plan(c, kind, np.zeros(c["occ"].shape, np.uint8))
    if kind == "field":
        want = Fo.plan_batch(c["occ"], K.ORIGIN, K.CELL, c["goal"], c["start"], c["r"], c["max_seg"], c["S_max"])
    else:
        want = FR.plan_batch(c["ev"], K.T_FREE, K.T_OCC, K.ORIGIN, K.CELL, c["start"], c["r"], c["mu"], c["max_seg"], c["S_max"])
    _same_plans(got, want, [k for k in want if k != "snapped"])


@pytest.mark.parametrize("kind", KINDS)
def test_random_layer_changes_paths_and_sets_a_sub_goal_by_the_penalty_rule_alone(kind):
    c, got = K.case("random"), K.oracle("random", kind)
    plain = K.plan(c, kind, np.zeros(c["occ"].shape, np.uint8))
    found = np.nonzero(got["status"] == CO.FOUND)[0]
    assert len(found) >= 8 and np.array_equal(got["status"], plain["status"])
    assert any(got["cells"][b] != plain["cells"][b] for b in found)
    assert (got["field"][got["field"] != CO.INF] >= plain["field"][plain["field"] != CO.INF]).all()
    # the rules that set each sub-goal, restated per robot
    k, fired = CO.k_of(c["cost"]), []
    for b in found:
        CO.string_pull(got["field"][0], k, got["cells"][b], c["max_seg"], fired)
    assert {"pen"} in fired and any("los" in f for f in fired), fired[:20]


@pytest.mark.parametrize("kind", KINDS)
def test_serpentine_needs_more_rounds_than_tiles(kind):
    c, got = K.case("serpentine"), K.oracle("serpentine", kind)
    W, H = c["occ"].shape
    tiles = -(-W // K.TW) * -(-H // K.TH)
    rounds = K.rounds_to_settle(got["field"][0], c["cost"])
    print("serpentine", kind, "tiles", tiles, "rounds", rounds)
    assert tiles == 2 and rounds > tiles + 4 and (got["status"] == CO.FOUND).all()
    assert T.tile_changes(got["cells"][0]) >= 8


def test_the_other_cases_reach_what_they_claim():
    # r_clear <= r_inflate: the priced cells are blocked, the field is the unweighted one
    c = K.case("priced_blocked")
    lay = K.layer(c)
    assert lay.max() == 248 and not (lay.astype(bool) & ~Fo.blocked_cells(c["occ"], c["r"])).any()
    assert np.array_equal(K.oracle("priced_blocked", "field")["field"], Fo.plan_batch(c["occ"], K.ORIGIN, K.CELL, c["goal"], c["start"], c["r"], c["max_seg"], c["S_max"])["field"])
    # the clearance strips: the layer reaches unblocked cells and moves the field
    for id_ in ("clear_strip_r0", "clear_strip_r2", "two_tiles"):
        c = K.case(id_)
        assert (K.layer(c).astype(bool) & ~Fo.blocked_cells(c["occ"], c["r"])).any(), id_
        plain = Fo.plan_batch(c["occ"], K.ORIGIN, K.CELL, c["goal"], c["start"], c["r"], c["max_seg"], c["S_max"])
        assert not np.array_equal(K.oracle(id_, "field")["field"], plain["field"]), id_
    # the snap: every start's cell is blocked but not solid, and the walk starts elsewhere
    c, got = K.case("snap"), K.oracle("snap", "field")
    for b, cell in enumerate(c["snap_cells"]):
        assert c["occ"][cell] == 0 and got["field"][0][cell] == CO.INF and got["snapped"][b] != cell and got["status"][b] == CO.FOUND
    # overflow, per-robot maps, 130 starts
    for kind in KINDS:
        assert (K.oracle("overflow", kind)["status"] == CO.PATH_OVERFLOW).sum() >= 8
        got = K.oracle("per_robot", kind)
        assert got["field"].shape[0] == 4 and (got["status"] == CO.FOUND).all() and len({f.tobytes() for f in got["field"]}) == 4
        assert len(K.oracle("130_starts", kind)["status"]) == 130 and (K.oracle("130_starts", kind)["status"] == CO.FOUND).sum() > 100
    # all 248: field values pass every max_seg although lengths do not; three caps, three sub-goal counts
    n = {}
    for id_ in ("all248_seg5", "all248_seg60", "all248_nocap"):
        c, got = K.case(id_), K.oracle(id_, "field")
        b = int(np.nonzero(got["status"] == CO.FOUND)[0][0])
        moves, value = len(got["cells"][b]) - 1, int(got["field"][0][got["snapped"][b]])
        assert moves >= 20 and value > 100 * 60 and 5 * moves <= value - 248 * moves <= 7 * moves
        n[id_] = int(got["n_sub"][b])
        if id_ == "all248_seg5":
            assert n[id_] == len(got["cells"][b]) - 1          # a sub-goal per cell: lengths reach 5 at once
    assert n["all248_seg5"] > n["all248_seg60"] > n["all248_nocap"] >= 1, n
    # two tiles: one round cannot settle it
    c, got = K.case("two_tiles"), K.oracle("two_tiles", "field")
    assert K.rounds_to_settle(got["field"][0], K.layer(c)) >= 3
