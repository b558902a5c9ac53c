"""Claim hysteresis for the gain-seeded claims, the oracle alone (tests/assign_keep_utility_oracle.py; no GPU): every consequence the
header states for lipmpc_grid_frontier_assign_keep_utility_batch, on the hand-made cases of tests/assign_keep_utility_checks.py, and
one chain of the committed exploration record."""
import importlib
import os
import sys

import numpy as np
import pytest

import assign_keep_checks as KC
import assign_keep_oracle as KO
import assign_keep_utility_checks as C
import assign_keep_utility_oracle as KU
import assign_utility_checks as U
import assign_utility_oracle as AU
import field_oracle as FO
import gain_checks as K
import gain_oracle as G
from assign_checks import open_field
from assign_keep_utility_checks import GENEROUS, index
from gain_checks import bits, centres

SHARED = ("status", "n_sub", "target_cell", "claim_round")


def _side_by_side(n, i=6, j0=8):
    return centres([(i, j0 + k) for k in range(n)])


def _equal(got, want, keys=SHARED):
    assert got["n_claims"] == want["n_claims"] and got["winners"] == want["winners"] and got["targets"] == want["targets"]
    for k in keys:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got["path_cost"]), bits(want["path_cost"]))
    assert np.array_equal(bits(got["target"]), bits(want["target"]))
    for g, w in zip(got["sub_goals"], want["sub_goals"]):
        assert np.array_equal(bits(g), bits(w))


def test_two_pockets_the_keep_rule_keeps_what_the_memoryless_rule_gives_away():
    ev, gain = C.two_pockets()
    assert ev.shape == (40, 44)
    prev = [index(C.POCKET_FAR, 44), -1]
    memoryless = U.expected(ev, C.POCKET_STARTS, C.POCKET_R_CLAIM, *C.POCKET_GAIN, gain=gain)
    want = C.expected(ev, C.POCKET_STARTS, C.POCKET_R_CLAIM, C.POCKET_GAIN, prev, (6, 24, 8), gain=gain, informed=memoryless["informed"])
    C.hence(want, C.POCKET_R_CLAIM, 64)
    assert memoryless["target_cell"][0] == index(C.POCKET_NEAR, 44) and want["target_cell"][0] == index(C.POCKET_FAR, 44)      # they differ
    assert memoryless["winners"] == [1, 0] and want["winners"] == [0, 1] and want["kept"].tolist() == [1, 0]
    rec, = want["attempts"]
    assert rec["anchor"] == C.POCKET_FAR and rec["cost"] > rec["near"] and 16 * rec["cost"] <= 24 * rec["near"] + 80 * 8
    assert want["target_gain"].tolist() == [110, 60]
    # a keeper's path_cost is the walk's length, its seed taken off: (keepfield[s] - seed(a)) / 5
    assert want["path_cost"][0] == (rec["cost"] - G.seed(110, 16, 120)) / 5.0
    strict = C.expected(ev, C.POCKET_STARTS, C.POCKET_R_CLAIM, C.POCKET_GAIN, prev, (6, 16, 0), gain=gain, informed=memoryless["informed"])
    assert strict["n_kept"] == 0 and strict["slots"] == 3 and strict["target_cell"].tolist() == memoryless["target_cell"].tolist()


@pytest.mark.parametrize("slack,kept", [(5, True), (4, False)])
def test_corridor_keep_test_at_equality_and_one_slack_less(slack, kept):
    ev, gain = C.kept_corridor()
    want = C.expected(ev, C.KEPT_START, 2, C.KEPT_GAIN, [index(C.KEPT_A, 16)], (0, 32, slack), gain=gain, **C.KEPT_KW)
    C.hence(want, 2, 64)
    rec, = want["attempts"]
    assert rec["cost"] == 115 and rec["near"] == 45 and 16 * 115 == 32 * 45 + 80 * 5
    assert rec["kept"] is kept and want["kept"].tolist() == [int(kept)] and KO.keeps(115, 45, 32, slack) is kept
    assert want["target_cell"].tolist() == [index(C.KEPT_A if kept else (1, 4), 16)] and want["slots"] == (1 if kept else 2)
    assert want["path_cost"].tolist() == [11.0 if kept else 3.0] and want["target_gain"].tolist() == [40 if kept else 70]


@pytest.mark.parametrize("gain_a", [0, -7])
def test_previous_target_whose_gain_fell_below_min_gain_or_is_negative(gain_a):
    ev, gain = C.kept_corridor(gain_a)
    near = C.expected(ev, C.KEPT_START, 2, C.KEPT_GAIN, [index(C.KEPT_A, 16)], (3, 1024, 4096), gain=gain, **C.KEPT_KW)
    assert near["attempts"] == [] and near["slots"] == near["n_claims"] == 1 and near["n_kept"] == 0           # the anchor is none
    wide = C.expected(ev, C.KEPT_START, 2, C.KEPT_GAIN, [index(C.KEPT_A, 16)], (8, 1024, 4096), gain=gain, **C.KEPT_KW)
    assert wide["attempts"][0]["anchor"] == (1, 4) and wide["kept"].tolist() == [1]                            # the anchor is elsewhere
    zero = C.expected(ev, C.KEPT_START, 2, (2, 16, 100, 0), [index(C.KEPT_A, 16)], (0, 1024, 4096), gain=gain, **C.KEPT_KW)
    assert (zero["attempts"] == []) == (gain_a < 0)            # at min_gain 0 a stored 0 is a source still, a negative gain never
    for w in (near, wide, zero):
        C.hence(w, 2, 64)


def test_a_keepers_disc_removes_the_next_robots_anchor_and_no_slot_is_spent():
    ev, gain = C.two_pockets()
    want = C.expected(ev, C.POCKET_STARTS, C.POCKET_R_CLAIM, C.POCKET_GAIN, [index(C.POCKET_FAR, 44)] * 2, (3, 1024, 4096), gain=gain)
    C.hence(want, C.POCKET_R_CLAIM, 64)
    assert [r["robot"] for r in want["attempts"]] == [0] and want["kept"].tolist() == [1, 0]
    assert want["slots"] == 2 and want["claim_round"].tolist() == [0, 1] and want["target_cell"][1] == index(C.POCKET_NEAR, 44)


@pytest.mark.parametrize("max_claims", [0, 1, 2, 3])
def test_failed_attempts_use_up_max_claims(max_claims):
    ev, start = open_field(20, 24), _side_by_side(3)
    prev = [index((17, 12), 24), index((2, 20), 24), -1]
    gainp = (4, 16, 60, 0)
    want = C.expected(ev, start, 3, gainp, prev, (0, 16, 0), max_claims=max_claims)
    C.hence(want, 3, max_claims)
    assert [r["kept"] for r in want["attempts"]] == [False] * min(max_claims, 2) and want["slots"] == max_claims
    # a failed attempt changes nothing else: what is left is the memoryless call with the slots that remain
    _equal(want, U.expected(ev, start, 3, *gainp, max_claims=max(max_claims - 2, 0), informed=want["informed"]), SHARED + ("target_gain",))


@pytest.mark.parametrize("r_keep", [0, 64])
def test_smallest_and_largest_keep_radius_window_clipped_at_a_grid_edge(r_keep):
    ev, start = open_field(20, 24), _side_by_side(3)
    prev = [index((10, 12), 24), index((2, 8), 24), 0]
    want = C.expected(ev, start, 5, (4, 16, 60, 0), prev, (r_keep, 1024, 4096))
    C.hence(want, 5, 64)
    if r_keep == 0:
        assert [r["robot"] for r in want["attempts"]] == [1] and want["kept"].tolist() == [0, 1, 0]
    else:
        assert [r["anchor"] for r in want["attempts"]] == [(17, 12), (2, 8), (2, 2)] and want["kept"].tolist() == [1, 1, 1]


@pytest.mark.parametrize("case", ["ring", "pockets", "fleet"])
def test_no_previous_target_is_the_gain_seeded_claim(case):
    if case == "ring":
        ev, start, r_claim, gainp, gain = open_field(40, 44), _side_by_side(6, 8, 18), 7, (6, 16, 60, 0), None
    elif case == "pockets":
        (ev, gain), start, r_claim, gainp = C.two_pockets(), C.POCKET_STARTS, C.POCKET_R_CLAIM, C.POCKET_GAIN
    else:
        (ev, start), r_claim, gainp, gain = K.fleet_case(), 6, (5, 16, 60, 0), None
    want = U.expected(ev, start, r_claim, *gainp, gain=gain)
    for prev in (None, np.full(len(start), -1), np.full(len(start), ev.size), np.full(len(start), KO.INT32_MAX), np.full(len(start), -(1 << 31))):
        got = C.expected(ev, start, r_claim, gainp, prev, (5, 16, 0), gain=gain, informed=want["informed"])
        _equal(got, want, SHARED + ("target_gain",))
        assert got["n_kept"] == 0 and not got["kept"].any() and got["attempts"] == [] and got["slots"] == want["n_claims"]


@pytest.mark.parametrize("case", ["second plan", "fleet"])
def test_w_gain_0_is_the_plain_keep_call(case):
    """w_gain 0, min_gain 0, stored gains >= 0: ufield == field, every seed is 0, and every output is the keep call's."""
    if case == "second plan":
        ev, start, r_claim, keep = open_field(40, 44), _side_by_side(6, 8, 18) + np.array([0.2, 0.0]), 7, (3, 24, 4)
        prev = KC.AC.expected(ev, _side_by_side(6, 8, 18), 7, 64)["target_cell"]
    else:
        (ev, start), r_claim, keep, prev = K.fleet_case(), 6, (6, 24, 8), C.fleet_prev()
    plain = KC.expected(ev, start, r_claim, 64, prev, keep)
    got = C.expected(ev, start, r_claim, (10, 0, 100, 0), prev, keep)
    assert np.array_equal(got["ufield"], got["field"]) and (got["gain"] >= 0).all()
    assert 0 < plain["n_kept"] < plain["n_claims"]
    _equal(got, plain)
    assert np.array_equal(got["kept"], plain["kept"]) and got["n_kept"] == plain["n_kept"] and got["slots"] == plain["slots"]
    assert [(r["robot"], r["anchor"], r["cost"], r["near"], r["kept"]) for r in got["attempts"]] == \
        [(r["robot"], r["anchor"], r["cost"], r["near"], r["kept"]) for r in plain["attempts"]]


def test_two_calls_give_identical_bits_and_the_fleet_case_stays_apart():
    ev, start = K.fleet_case()
    a, b = (C.expected(ev, start, 6, (5, 16, 60, 0), C.fleet_prev(), (6, 24, 8)) for _ in range(2))
    _equal(a, b, SHARED + ("target_gain", "kept"))
    C.hence(a, 6, 64)
    assert a["n_kept"] >= 1 and a["n_claims"] > a["n_kept"] and C.spaced(a, 6)


def test_no_addition_wraps():
    """The largest seed is below 2^26 and a finite cost below 7 * 2^24; both sides of the test, at the largest parameters, fit 64
    bits with room to spare -- and a field value stays below the uint32 INF."""
    seed = G.seed(0, G.W_GAIN_MAX, G.G_CAP_MAX)
    assert seed == (65535 * 16384) >> 4 < 1 << 26
    top = (1 << 26) + 7 * (1 << 24)
    assert top < FO.INF and 16 * top < 1 << 62 and KO.KEEP_RATIO_MAX * top + 80 * KO.KEEP_SLACK_MAX < 1 << 62
    assert KO.keeps(top, top, 16, 0) and not KO.keeps(top, top - 1, 16, 0)
    # on a map: the largest seed on every source, previous targets kept through it
    ev, start = open_field(20, 24), _side_by_side(2)
    want = C.expected(ev, start, 5, (4, 65535, 16384, 0), [index((17, 12), 24), -1], (0, 32, 0), gain=np.zeros((20, 24), np.int32))
    assert want["attempts"][0]["cost"] > seed and want["kept"].tolist() == [1, 0]
    C.hence(want, 5, 64)


def test_the_kernels_lds_rule_is_its_own():
    (W, H), (W1, H1) = KU.sizes_at_the_lds_switch()
    assert KU.field_lds_bytes(W * H) - KO.field_lds_bytes(W * H) == 4 * 14 == KU.field_lds_bytes(W * H) - AU.field_lds_bytes(W * H)
    assert KU.field_fits_lds(W * H) and not KU.field_fits_lds(W1 * H1) and FO.MAX_CELLS >= W1 * H1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "lipmpc.h")) as f:
        assert "4 (2 (2 ceil(W H / 64) + 2) + 48 + W H) + 256 <= 163840" in f.read()


def test_one_chain_of_the_record_reproduces_the_committed_counts(golden_dir):
    """field, seed 0, `seeded 0 + keep 6/24/8`: the chain of tests/golden/make_exploration_gain_kept.py run again."""
    sys.path.insert(0, golden_dir)
    try:
        gen = importlib.import_module("make_exploration_gain_kept")
    finally:
        sys.path.remove(golden_dir)
    rec = np.load(os.path.join(golden_dir, "exploration_gain_kept.npz"))
    rule = "seeded 0 + keep 6/24/8"
    assert rec["rules"].tolist() == list(gen.RULES) and rule in gen.RULES and rec["keeps"].tolist() == [list(k) for k in gen.KEEPS]
    row = gen.chain(("field", rule, 0))
    r = gen.RULES.index(rule)
    for key in gen.COUNTS:
        assert row[key] == rec[f"field/{key}"][r, 0], key
    assert row["finished"] and row["n_kept"] > 0
