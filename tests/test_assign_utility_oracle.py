"""CPU: tests/assign_utility_oracle.py, the numpy restatement of the gain-seeded claims, against what the contract implies -- and
the cases of the GPU tests shown to be what they claim."""
import numpy as np
import pytest

import assign_oracle as AO
import assign_utility_checks as U
import assign_utility_oracle as AU
import frontier_oracle as FR
import gain_checks as K
import gain_oracle as G
from gain_checks import CELL, HAND_MADE, ORIGIN, T_FREE, T_OCC, bits

A_CELL, B_CELL = K.CORRIDOR_A, K.CORRIDOR_B


def _equals_plain(got, plain):
    """Every output the two calls share, bit for bit."""
    assert got["n_claims"] == plain["n_claims"] and got["winners"] == plain["winners"] and got["costs"] == plain["costs"]
    for k in ("status", "n_sub", "target_cell", "claim_round"):
        assert np.array_equal(got[k], plain[k]), k
    assert np.array_equal(bits(got["path_cost"]), bits(plain["path_cost"]))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got["sub_goals"], plain["sub_goals"]))


@pytest.mark.parametrize("case", ["fleet", "uwall"])
def test_w_gain_0_is_the_plain_claim(case):
    """w_gain 0 / min_gain 0: seeds 0, sources the frontier, terminal <=> field 0 -- whatever the gain holds."""
    if case == "fleet":
        (ev, start), origin, cell, r_claim = K.fleet_case(), ORIGIN, CELL, 6
    else:
        ev, start, origin, cell, r_claim = K.scanned_maps()[0], U.UWALL_STARTS, K.MAP_ORIGIN, K.MAP_CELL, U.UWALL_R_CLAIM
    plain = AO.plan_batch(ev, T_FREE, T_OCC, origin, cell, start, r_claim, 64)
    got = U.expected(ev, start, r_claim, 10, 0, 100, 0, origin=origin, cell=cell)
    _equals_plain(got, plain)
    rng = np.random.default_rng(3)
    junk = rng.integers(-(1 << 31), 1 << 31, ev.shape, dtype=np.int64).astype(np.int32)
    _equals_plain(U.expected(ev, start, r_claim, 10, 0, 100, 0, origin=origin, cell=cell, gain=np.maximum(junk, 0)), plain)
    U.hence(got, r_claim, 64)


def test_uwall_targets_of_the_record():
    """The figures the issue quotes: three planners, three different target lists; the gain-seeded winners share no target."""
    ev, _ = K.scanned_maps()
    H = ev.shape[1]
    plain = AO.plan_batch(ev, T_FREE, T_OCC, K.MAP_ORIGIN, K.MAP_CELL, U.UWALL_STARTS, U.UWALL_R_CLAIM, 64)
    got = U.uwall(30, 64, 600, 0)
    lists = dict(informed=U.cells_of(got["informed"]["target_cell"], H), plain=U.cells_of(plain["target_cell"], H),
                 seeded=U.cells_of(got["target_cell"], H))
    assert lists["informed"] == [(41, 51), (41, 51), (41, 51), (54, 29), (54, 29), (65, 34)]
    assert lists["plain"] == [(41, 54), (1, 26), (32, 76), (37, 34), (54, 29), (87, 42)]
    assert lists["seeded"] == [(41, 51), (55, 1), (37, 36), (54, 29), (61, 15), (87, 42)]
    assert got["n_claims"] == 6 and got["costs"] == [134, 154, 155, 243, 367, 735]
    assert lists["informed"] != lists["plain"] != lists["seeded"] != lists["informed"] and len(set(lists["seeded"])) == 6
    near = U.cells_of(U.uwall(10, 16, 120, 0)["target_cell"], H)
    assert near[2] == (35, 73) and near[5] == (85, 41) and len(set(near)) == 6


@pytest.mark.parametrize("params", U.UWALL_SETS)
def test_uwall_consequences(params):
    got = U.uwall(*params)
    U.hence(got, U.UWALL_R_CLAIM, 64)
    assert got["n_claims"] >= 2
    if params[3]:                                              # no source and no target below min_gain (on this map 8 prunes none)
        assert got["n_sources"][0] <= got["n_frontier"][0] and (got["target_gain"][got["claim_round"] >= 0] >= params[3]).all()


@pytest.mark.parametrize("gain_a,targets,costs", [(74, [B_CELL, A_CELL], [35, 41]), (75, [A_CELL, B_CELL], [35, 40]),
                                                  (76, [A_CELL, B_CELL], [34, 40])])
def test_corridor_tie_and_domination_inside_a_round(gain_a, targets, costs):
    """Two robots left of A, r_claim 2.  75 TIES the route through A: the winner stops at A (the terminal test comes first) and B
    is left for round 1.  74 leaves A dominated in round 0: the winner walks through it to B -- and once B's disc is gone A holds
    its own seed, so it is round 1's target.  76 makes A strictly better."""
    ev, gain, got = U.corridor(gain_a)
    assert got["n_sources"][0] == 2 and got["winners"] == [1, 0] and got["targets"] == targets and got["costs"] == costs
    assert got["target_gain"].tolist() == [gain[t] for t in reversed(targets)]
    assert got["path_cost"].tolist() == [(costs[1] - G.seed(gain[targets[1]], 16, 100)) / 5.0, (costs[0] - G.seed(gain[targets[0]], 16, 100)) / 5.0]
    U.hence(got, U.CORRIDOR_R_CLAIM, 64)
    one = U.corridor(gain_a, max_claims=1)[2]
    assert one["winners"] == [1] and one["claim_round"].tolist() == [-1, 0]
    assert one["target_cell"][0] == one["informed"]["target_cell"][0]


def test_min_gain_that_prunes_every_source():
    ev, start = K.fleet_case()
    got = U.expected(ev, start, 6, 5, 16, 60, min_gain=16384)
    assert got["n_sources"][0] == 0 and got["n_claims"] == 0 and (got["claim_round"] == -1).all()
    assert not np.isin(got["status"], (FR.FOUND, FR.PATH_OVERFLOW)).any()


def hand_gain(shape, seed=5, lo=-60, hi=160):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.int32)


def test_gains_below_0_and_above_g_cap_are_clamped():
    ev, start = K.fleet_case()
    gain = hand_gain(ev.shape)
    got = U.expected(ev, start, 6, 5, 40, 120, 0, gain=gain)
    fr = got["frontier"][0] != 0
    assert (gain[fr] < 0).any() and (gain[fr] > 120).any()
    clamped = U.expected(ev, start, 6, 5, 40, 120, 0, gain=np.clip(gain, 0, 120))
    for k in ("status", "n_sub", "target_cell", "claim_round"):
        assert np.array_equal(got[k], clamped[k]), k
    assert got["n_claims"] == clamped["n_claims"] >= 3 and got["costs"] == clamped["costs"]
    won = got["claim_round"] >= 0
    assert np.array_equal(got["target_gain"][won], gain.reshape(-1)[got["target_cell"][won]])          # as stored, not clamped
    U.hence(got, 6, 64)
    # min_gain compares the stored value: a negative gain is no source at min_gain 0 ... and the 5 x 7 map has its own case
    assert got["n_sources"][0] == int((fr & (got["field"][0] != G.INF) & (gain >= 0)).sum()) < got["n_frontier"][0]
    hm = U.expected(HAND_MADE, K.centres(((3, 4), (0, 3), (3, 6))), 2, 2, 16, 10, 0, r=0, mu=1, gain=hand_gain(HAND_MADE.shape, 7, -5, 20))
    assert hm["n_claims"] >= 2
    U.hence(hm, 2, 64)


def test_path_overflow_winner_claims():
    got = U.uwall(30, 64, 600, 0, S_max=1)
    full = U.uwall(30, 64, 600, 0)
    over = (got["claim_round"] >= 0) & (got["status"] == FR.PATH_OVERFLOW)
    assert over.any() and (got["n_sub"][over] == 0).all()
    assert np.array_equal(got["target_cell"], full["target_cell"]) and np.array_equal(got["claim_round"], full["claim_round"])
    U.hence(got, U.UWALL_R_CLAIM, 64)


@pytest.mark.parametrize("max_claims", [0, 1, 3])
def test_max_claims(max_claims):
    got = U.uwall(30, 64, 600, 0, max_claims=max_claims)
    full = U.uwall(30, 64, 600, 0)
    assert got["n_claims"] == max_claims and got["winners"] == full["winners"][:max_claims] and got["targets"] == full["targets"][:max_claims]
    U.hence(got, U.UWALL_R_CLAIM, max_claims)
    if max_claims == 0:
        inf = got["informed"]
        assert all(np.array_equal(got[k], inf[k]) for k in ("status", "n_sub", "target_cell", "target_gain"))


def test_may_claim_mask():
    ev, _ = K.scanned_maps()
    may = np.array([0, 1, 1, 0, 1, 1], np.int8)
    got = U.expected(ev, U.UWALL_STARTS, U.UWALL_R_CLAIM, 30, 64, 600, 0, may_claim=may, origin=K.MAP_ORIGIN, cell=K.MAP_CELL)
    assert (got["claim_round"][may == 0] == -1).all() and (got["claim_round"][may != 0] >= 0).all() and got["n_claims"] == 4
    U.hence(got, U.UWALL_R_CLAIM, 64)


def test_lds_rule_of_the_kernel():
    """Two bitmaps + 34 words + W H words + 256 <= 163840, and where it switches at H = 193."""
    assert AU.field_lds_bytes(92 * 80) == 4 * (2 * (2 * -(-92 * 80 // 64) + 2) + 34 + 92 * 80)
    (W, H), (W1, H1) = AU.sizes_at_the_lds_switch()
    assert H == H1 == 193 and W1 == W + 1 and AU.field_lds_bytes(W * H) + 256 <= 163840 < AU.field_lds_bytes(W1 * H) + 256
    assert AU.field_lds_bytes(W * H) - AO.field_lds_bytes(W * H) == 4 * (34 - 22)
