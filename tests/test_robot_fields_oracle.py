"""Claims from per-robot fields, the oracle alone (tests/robot_fields_oracle.py; no GPU): the properties the header lists under HENCE,
on every case of tests/robot_fields_checks.py, and each case is what its name says."""
import numpy as np
import pytest

import assign_checks as AC
import assign_oracle as AO
import field_oracle as FO
import frontier_oracle as FR
import robot_fields_checks as RC
import robot_fields_oracle as RF
from assign_checks import CELL, ORIGIN, T_FREE, T_OCC, centres, open_field
from robot_fields_checks import index

OUTPUTS = ("status", "n_sub", "target_cell", "claim_round", "kept")


def _equal(got, want, but=()):
    assert got["n_claims"] == want["n_claims"] and got["winners"] == want["winners"] and got["targets"] == want["targets"]
    for k in OUTPUTS:
        if k not in but:
            assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(AC.bits(got["path_cost"]), AC.bits(want["path_cost"]))
    assert np.array_equal(AC.bits(got["target"]), AC.bits(want["target"]))
    for g, w in zip(got["sub_goals"], want["sub_goals"]):
        assert np.array_equal(AC.bits(g), AC.bits(w))


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_the_hence_list(name):
    c, want = RC.case(name), RC.expected(name)
    near = want["nearest"]
    field, frontier = near["field"][0], near["frontier"][0]
    W, H = field.shape
    r_claim, winners, targets, costs = c["r_claim"], want["winners"], want["targets"], want["costs"]
    assert want["n_claims"] == len(winners) <= c["max_claims"] and len(set(winners)) == len(winners)
    # two winners' targets are more than r_claim apart
    assert RC.spaced(want, r_claim)
    # greedy winners' costs do not decrease; a winner's target is a nearest live source of that winner
    greedy = [n for n, b in enumerate(winners) if not want["kept"][b]]
    assert all(costs[a] <= costs[b] for a, b in zip(greedy[:-1], greedy[1:]))
    live = (frontier != 0) & (field != FO.INF)
    for n, (b, t) in enumerate(zip(winners, targets)):
        assert live[t] and want["claim_round"][b] == n
        if not want["kept"][b]:
            assert costs[n] == int(want["D"][b][live].min()) == int(want["D"][b][t])
        live = live & ~AO.disc(W, H, t, r_claim)
    # followers keep the path call's outputs
    for b in range(len(c["start"])):
        if b not in winners:
            assert want["claim_round"][b] == -1 and want["kept"][b] == 0
            for k in ("status", "n_sub", "target_cell"):
                assert want[k][b] == near[k][b]
    # the round-0 greedy winner and its cost equal lipmpc_grid_frontier_assign_batch's when every start cell of U_0 is passable
    in_u0 = [b for b, e in enumerate(want["entries"]) if e is not None]
    cells = [FO.cell_of(c["start"][b], ORIGIN, CELL, W, H) for b in in_u0]
    if c["prev"] is None and c["max_claims"] > 0 and all(field[x] != FO.INF for x in cells):
        plain = AO.assign(frontier, field, ORIGIN, CELL, c["start"], near, c["r"], r_claim, 1, c["max_seg"], c["S_max"], c["may_claim"])
        assert plain["winners"] == winners[:1] and plain["costs"] == costs[:1]
    # the winners equal an independent brute-force greedy over all (robot, cell) pairs
    if c["prev"] is None and name != "big":
        assert RF.pair_greedy(frontier, field, want["D"], r_claim, c["max_claims"]) == (winners, targets)
    # with prev_target NULL or all "none" the outputs other than kept / n_kept are equal
    if c["prev"] is None:
        none = RC.expected_of(c, near, prev=np.full(len(c["start"]), -1), keep=(5, 16, 0))
        _equal(none, want)
        assert none["n_kept"] == 0 and none["attempts"] == []
    # two calls give the same answer (the fields are recomputed: no cache is shared)
    if name not in ("B300", "big"):
        _equal(RC.expected_of(c, near), want)
    # the rows: the sub-goals run from the robot to the target, which is the last one
    for b, t in zip(winners, targets):
        if want["status"][b] == FR.FOUND:
            assert np.array_equal(want["sub_goals"][b][-1], FO.centre(t, ORIGIN, CELL)) and want["n_sub"][b] == len(want["sub_goals"][b])
            assert want["path_cost"][b] == int(want["D"][b][t]) / 5.0 and want["chains"][b][0] == t


@pytest.mark.parametrize("r_claim,targets,costs", [(5, None, None),
                                                   (15, [(2, 18), (2, 34), (8, 2), (16, 41), (24, 2), (37, 21)], [30, 67, 85, 111, 122, 145])])
def test_the_open_field_equals_the_existing_call(r_claim, targets, costs):
    """Observed, not derived: on the open field with the six side-by-side starts (every start cell passable) the winners, targets and
    costs are lipmpc_grid_frontier_assign_batch's exactly."""
    ev, start = open_field(40, 44), centres(RC.SIX)
    old = AC.expected(ev, start, r_claim, 64)
    new = RF.plan_batch(ev, T_FREE, T_OCC, ORIGIN, CELL, start, r_claim, 64, nearest=old["nearest"])
    assert new["winners"] == old["winners"] and new["targets"] == old["targets"] and new["costs"] == old["costs"]
    for k in ("claim_round", "target_cell"):
        assert np.array_equal(new[k], old[k])
    assert np.array_equal(AC.bits(new["path_cost"]), AC.bits(old["path_cost"]))
    if targets:
        assert sorted(new["targets"]) == targets and sorted(new["costs"]) == costs


def test_each_case_is_what_its_name_says():
    E = RC.expected
    six = E("open6-r5")
    assert six["n_claims"] == 7 and six["claim_round"][6] == -1 and six["entries"][6] is None      # NaN never; the corner robot snaps in
    assert six["nearest"]["field"][0][0, 0] == FO.INF and six["entries"][7] == (2, 2) and six["claim_round"][7] >= 0
    assert E("open6-r0")["n_claims"] == 7 and E("open6-r4096")["n_claims"] == 1
    assert [E(f"open6-claims{n}")["n_claims"] for n in (0, 1, 3)] == [0, 1, 3]
    assert sorted(E("open6-may")["winners"]) == [1, 2, 4, 7] and E("open6-nobody-may")["n_claims"] == 0
    corner = E("tile-corner")
    assert {(e[0] // RC.TW, e[1] // RC.TH) for e in corner["entries"]} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert corner["n_claims"] == 2 and {t[1] // RC.TH for t in corner["targets"]} == {0, 1}      # a disc takes a whole line: two followers
    rooms = E("two-rooms")                                        # the first room's frontier is used up: its third robot follows
    assert rooms["winners"] == [0, 3, 4] and rooms["D"][1][rooms["targets"][1]] == FO.INF
    band = E("band")
    f = band["nearest"]["field"][0]
    assert f[10, 11] == FO.INF and band["entries"][1] == band["entries"][2] != (10, 11)            # snapped, two robots in ONE cell
    assert band["claim_round"][1] >= 0 and (band["claim_round"][2] < 0 or band["claim_round"][1] < band["claim_round"][2])
    on = E("on-frontier")
    assert on["winners"][0] == 0 and on["costs"][0] == 0 and on["n_sub"][0] == 1 and on["targets"][0] == (2, 20)
    marked = E("every-cell-marked")
    for b in marked["winners"]:
        assert marked["n_sub"][b] == len(marked["chains"][b]) - 1 >= 2
    assert E("B65")["n_claims"] < 65 and E("B300")["n_claims"] < 300 and (E("B300")["claim_round"] == -1).sum() > 100      # followers
    assert max(E("big")["target_cell"]) > 1 << 17
    assert E("keep-none")["n_kept"] == 0 and E("keep-all")["n_kept"] == 6 == E("keep-all")["n_claims"]
    rec, = E("keep-receded")["attempts"]
    assert rec["anchor"] == (2, 20) and rec["kept"] and E("keep-vanished")["attempts"] == [] and E("keep-vanished")["n_kept"] == 0
    strict = E("keep-strict-fails")
    assert [(r["robot"], r["kept"]) for r in strict["attempts"]] == [(0, False), (1, True)] and strict["n_claims"] == 3
    assert strict["attempts"][0]["cost"] > strict["attempts"][0]["near"] == strict["attempts"][1]["cost"]      # 16 / 0: equality keeps
    out = E("keep-out-of-range")
    assert [r["robot"] for r in out["attempts"]] == [3] and out["kept"].tolist() == [0, 0, 0, 1]
    cap = E("keep-cap")
    assert cap["kept"].tolist() == [1, 1, 0, 0, 0, 0] and cap["n_claims"] == 2 and len(cap["attempts"]) == 2
    kc = E("keep-tile-corner")
    assert kc["kept"][0] == 1 and kc["targets"][0] == RC.FAR2 and kc["n_claims"] == 4


def test_s_max_at_n_sub_and_one_below():
    c = RC.case("every-cell-marked")
    want = RC.expected("every-cell-marked")
    b = want["winners"][0]
    n = int(want["n_sub"][b])
    fits, over = RC.expected_of(c, S_max=n), RC.expected_of(c, S_max=n - 1)
    assert fits["status"][b] == FR.FOUND and fits["n_sub"][b] == n
    assert over["status"][b] == FR.PATH_OVERFLOW and over["n_sub"][b] == 0 and over["claim_round"][b] == 0 and over["winners"] == want["winners"]
