"""Claim hysteresis, the oracle alone (tests/assign_keep_oracle.py; no GPU): the properties the header lists as consequences of the
rule, on the maps of tests/assign_checks.py."""
import numpy as np
import pytest

import assign_checks as AC
import assign_keep_checks as KC
import assign_keep_oracle as K
import assign_oracle as A
import field_oracle as FO
from assign_checks import CELL, ORIGIN, centres, open_field
from assign_keep_checks import GENEROUS, index

OUTPUTS = ("status", "n_sub", "target_cell", "claim_round")


def _side_by_side(n, i=6, j0=8):
    return centres([(i, j0 + k) for k in range(n)])


def _equal(got, want):
    assert got["n_claims"] == want["n_claims"] and got["winners"] == want["winners"] and got["targets"] == want["targets"]
    for k in OUTPUTS:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(AC.bits(got["path_cost"]), AC.bits(want["path_cost"]))
    assert np.array_equal(AC.bits(got["target"]), AC.bits(want["target"]))
    for g, w in zip(got["sub_goals"], want["sub_goals"]):
        assert np.array_equal(AC.bits(g), AC.bits(w))


@pytest.mark.parametrize("case", ["ring", "rooms", "band", "may", "few"])
def test_no_previous_target_is_the_plain_claim(case):
    ev, start, r_claim, max_claims, kw = {
        "ring": (open_field(40, 44), _side_by_side(6, 8, 18), 7, 64, {}),
        "rooms": (AC.two_rooms(), centres([(5, 6), (6, 6), (20, 6), (21, 6)]), 12, 64, dict(r=0)),
        "band": (AC.block_in_field(), centres([(4, 12), (10, 11)]), 12, 64, {}),
        "may": (open_field(20, 24), _side_by_side(5), 3, 64, dict(may_claim=np.array([0, 1, 0, 1, 1], np.int8))),
        "few": (open_field(20, 24), _side_by_side(5), 3, 2, {}),
    }[case]
    want = AC.expected(ev, start, r_claim, max_claims, **kw)
    for prev in (None, np.full(len(start), -1), np.full(len(start), ev.size), np.full(len(start), K.INT32_MAX)):
        got = KC.expected(ev, start, r_claim, max_claims, prev, (5, 16, 0), near=want["nearest"], **kw)
        _equal(got, want)
        assert got["n_kept"] == 0 and not got["kept"].any() and got["attempts"] == [] and got["slots"] == want["n_claims"]


def _second_plan(r_keep=3, ratio=24, slack=4, r_claim=7, max_claims=64):
    """Six robots before the ring of an open field claim apart, walk two cells towards their targets' side, and plan again with
    the first plan's targets as the previous ones."""
    ev, start = open_field(40, 44), _side_by_side(6, 8, 18)
    first = AC.expected(ev, start, r_claim, max_claims)
    moved = start + np.array([2 * CELL[0], 0.0])
    return ev, moved, first, KC.expected(ev, moved, r_claim, max_claims, first["target_cell"], (r_keep, ratio, slack))


def test_winners_kept_or_claimed_stay_apart_and_rounds_count_them_in_order():
    ev, start, first, want = _second_plan()
    assert 0 < want["n_kept"] < 6 and want["n_claims"] == 6          # some keep, some fail the test and claim anew
    assert KC.spaced(want, 7)
    won = want["claim_round"] >= 0
    assert sorted(want["claim_round"][won].tolist()) == list(range(want["n_claims"]))
    assert [int(want["claim_round"][b]) for b in want["winners"]] == list(range(want["n_claims"]))
    kept = np.nonzero(want["kept"])[0]
    assert want["winners"][:len(kept)] == kept.tolist()              # the keep phase comes first, in ascending index
    assert np.array_equal(want["target_cell"][kept], first["target_cell"][kept])      # nothing receded: r_keep was not needed
    assert want["slots"] == len(want["attempts"]) + want["n_claims"] - want["n_kept"] <= 64


def test_strict_parameters_keep_only_a_target_as_near_as_the_nearest_frontier():
    ev, start, first, want = _second_plan(ratio=16, slack=0)
    for rec in want["attempts"]:
        assert rec["kept"] == (rec["cost"] <= rec["near"])
    assert any(not rec["kept"] for rec in want["attempts"])


def test_anchor_ties_go_to_the_lower_cell_index():
    ev = open_field(20, 24)
    src = AC.expected(ev, _side_by_side(1), 5, 0)["nearest"]["frontier"][0] != 0
    assert src[2, 5] and src[5, 2] and not src[3:5, 3:6].any()
    assert K.anchor(src, (5, 5), 3) == (2, 5) and index((2, 5), 24) < index((5, 2), 24)      # both at d^2 = 9
    assert K.anchor(src, (5, 5), 2) is None
    assert K.anchor(src.T.copy(), (5, 5), 3) == (2, 5)               # (the transposed map: the same answer by the same rule)
    assert K.anchor(src, (2, 5), 0) == (2, 5) and K.anchor(src, (0, 0), 2) is None and K.anchor(src, (0, 0), 3) == (2, 2)


def test_a_failed_attempt_spends_a_slot_and_nothing_else():
    """Robot 0's previous target lies across the field: too far for the strict test.  With max_claims = 3 the call is the plain
    claim with max_claims = 2; with max_claims = 1 the one slot goes to the failed attempt and nobody claims."""
    ev, start = open_field(20, 24), _side_by_side(3)
    prev = np.array([index((17, 12), 24), -1, -1])
    got = KC.expected(ev, start, 3, 3, prev, (0, 16, 0))
    assert [r["kept"] for r in got["attempts"]] == [False] and got["attempts"][0]["cost"] > got["attempts"][0]["near"]
    assert got["slots"] == 3 and got["n_kept"] == 0
    _equal(got, AC.expected(ev, start, 3, 2))
    none = KC.expected(ev, start, 3, 1, prev, (0, 16, 0))
    assert none["slots"] == 1 and none["n_claims"] == 0
    _equal(none, AC.expected(ev, start, 3, 0))


def test_an_anchor_out_of_reach_spends_its_slot():
    ev, start = AC.two_rooms(), centres([(5, 6)])
    got = KC.expected(ev, start, 12, 64, [index((16, 6), 14)], GENEROUS, r=0)
    assert got["attempts"][0]["anchor"] == (16, 6) and got["attempts"][0]["entry"] is None
    assert got["slots"] == 2 and got["n_claims"] == 1 and got["n_kept"] == 0
    _equal(got, AC.expected(ev, start, 12, 64, r=0))


def test_the_keep_kernels_lds_rule_is_its_own():
    (W, H), (W1, H1) = K.sizes_at_the_lds_switch()
    assert K.field_lds_bytes(W * H) - A.field_lds_bytes(W * H) == 4 * 12
    assert K.field_fits_lds(W * H) and not K.field_fits_lds(W1 * H1) and FO.MAX_CELLS >= W1 * H1
