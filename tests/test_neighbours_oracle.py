"""The neighbour-row contract on the CPU: tests/neighbour_oracle.py on hand-computed cases, and the row MODEL pinned by the swap
scenario on the oracle chain (rows -> lipmpc_oracle.plan_step -> advance): four robots that cross at the origin."""
import numpy as np
import pytest

import lipmpc_oracle as O
import neighbour_oracle as NO


def _states(xy):
    st = np.zeros((len(xy), 5))
    st[:, 0], st[:, 2] = np.asarray(xy, float).T
    return st


def test_a_3_4_5_pair():
    """Robots at (0, 0) and (3, 4), radii 0.5 and 1: dist 5, rs 1.5, offset = 1.5 + 0.5 (5 - 1.5) = 3.25."""
    r = NO.neighbour_rows(_states([(0, 0), (3, 4)]), [0.5, 1.0], 6.0, 2, 3)
    assert list(r["n_rows"]) == [1, 1] and list(r["n_near"]) == [1, 1]
    assert r["neighbours"].tolist() == [[1, -1], [0, -1]]
    # robot 0: eta = (0 - 3, 0 - 4) / 5, c = p_1 + 3.25 eta
    assert np.array_equal(r["c_eta"][0, 0], [3 + 3.25 * (-3 / 5), 4 + 3.25 * (-4 / 5), -3 / 5, -4 / 5])
    assert np.array_equal(r["c_eta"][1, 0], [0 + 3.25 * (3 / 5), 0 + 3.25 * (4 / 5), 3 / 5, 4 / 5])
    assert not r["c_eta"][:, 1:].any()
    # the reciprocal model: eta.(p_i - c) = (dist - rs) / 2 for both, and the two boundaries are rs apart
    for i, p in enumerate([(0.0, 0.0), (3.0, 4.0)]):
        c, eta = r["c_eta"][i, 0, :2], r["c_eta"][i, 0, 2:]
        assert abs(eta @ (np.array(p) - c) - 1.75) < 1e-15
    assert abs(np.linalg.norm(r["c_eta"][0, 0, :2] - r["c_eta"][1, 0, :2]) - 1.5) < 1e-15
    # out of range: strictly
    r = NO.neighbour_rows(_states([(0, 0), (3, 4)]), [0.5, 1.0], 5.0, 2, 3)
    assert not r["n_near"].any() and not r["n_rows"].any() and not r["c_eta"].any()


def test_a_tie_is_broken_by_index():
    """Four robots at distance 1 from robot 2, k_rows 2: the two lowest indices get the rows, nearer ones come first."""
    xy = [(1, 0), (0, 1), (0, 0), (-1, 0), (0, -1), (0.5, 0)]
    r = NO.neighbour_rows(_states(xy), 0.1, 1.25, 2, 4)
    assert r["n_near"][2] == 5 and r["n_rows"][2] == 2 and r["neighbours"][2].tolist() == [5, 0]
    r = NO.neighbour_rows(_states(xy[:5]), 0.1, 1.25, 2, 4)
    assert r["n_near"][2] == 4 and r["neighbours"][2].tolist() == [0, 1]
    assert np.array_equal(r["c_eta"][2, 1], [0.0, 1 + (0.2 + 0.5 * (1 - 0.2)) * -1.0, 0.0, -1.0])


def test_share_zero_is_the_static_disc():
    st = _states([(0, 0), (2, 0)])
    half = NO.neighbour_rows(st, 0.25, 3.0, 1, 1, share=0.5)["c_eta"]
    disc = NO.neighbour_rows(st, 0.25, 3.0, 1, 1, share=0.0)["c_eta"]
    assert np.array_equal(disc[0, 0], [2 - 0.5, 0.0, -1.0, 0.0])               # c = p_j + rs eta
    assert np.array_equal(half[0, 0], [2 - 1.25, 0.0, -1.0, 0.0])              # c = p_j + (rs + (dist - rs) / 2) eta
    one = NO.neighbour_rows(st, 0.25, 3.0, 1, 1, share=1.0)["c_eta"]
    assert np.array_equal(one[0, 0], [0.0, 0.0, -1.0, 0.0])                    # the boundary through the robot itself


def test_an_absent_robot_neither_sees_nor_is_seen():
    st = _states([(0, 0), (0.5, 0), (0, 0.5), (0.5, 0.5), (np.nan, 0)])
    rad = [0.1, 0.1, -0.1, np.inf, 0.1]
    grp = [0, 0, 0, 0, 0]
    r = NO.neighbour_rows(st, rad, 2.0, 4, 4, group=grp)
    assert r["n_near"].tolist() == [1, 1, 0, 0, 0] and r["n_rows"].tolist() == [1, 1, 0, 0, 0]
    assert r["neighbours"][0].tolist() == [1, -1, -1, -1] and (r["neighbours"][2:] == -1).all()
    r = NO.neighbour_rows(st, 0.1, 2.0, 4, 4, group=[0, -1, 0, 1, 1])
    assert r["n_near"].tolist() == [1, 0, 1, 0, 0] and r["neighbours"][0, 0] == 2          # (3 alone in group 1: 4 is NaN)


def test_a_full_first_slot_leaves_no_row():
    st = _states([(0, 0), (0.5, 0), (0, 0.5)])
    before = np.full((3, 3, 4), 7.0)
    r = NO.neighbour_rows(st, 0.1, 2.0, 4, 3, first_slot=[3, 2, 0], c_eta=before)
    assert r["n_near"].tolist() == [2, 2, 2] and r["n_rows"].tolist() == [0, 1, 2]
    assert (r["c_eta"][0] == 7.0).all()                                          # nothing below first_slot is touched
    assert (r["c_eta"][1, :2] == 7.0).all() and r["neighbours"][1].tolist() == [0, -1, -1, -1]
    assert (r["c_eta"][2, :2, 2:] != 7.0).all() and not r["c_eta"][2, 2].any()   # two rows, then zeros
    assert (before == 7.0).all()


def test_coincident_robots_give_nan_eta_and_the_step_is_degenerate():
    r = NO.neighbour_rows(_states([(1, 1), (1, 1)]), 0.1, 1.0, 1, 1)
    assert r["n_rows"].tolist() == [1, 1] and np.isnan(r["c_eta"][:, 0]).all()
    s = NO.plan_step_rows([1, 0, 1, 0, 0], (3.0, 1.0), 1, r["c_eta"][0], O.Params(N=3))
    assert s["status"] == O.STATUS_DEGENERATE


@pytest.fixture(scope="module")
def swap():
    st, goal = NO.swap_scenario()
    return {share: NO.swap_run(st, goal, share=share) for share in (0.5, None, 0.0)}


def test_swap_with_reciprocal_rows_keeps_the_discs_apart(swap):
    """share 0.5: all four robots arrive and no two discs (radius 0.25) ever overlap -- the bound is the contract's derivation
    (the k = 0 row is (dist - rs) / 2 >= 0, the two half-spaces of a pair are rs apart), the run gives 0.5316."""
    r = swap[0.5]
    d = NO.min_pair_distance(r["X"])
    print("share 0.5: min distance", d, "steps", r["n_steps"], "objective", r["last_obj"])
    assert (r["last_status"] == O.STATUS_SOLVED).all() and (r["last_obj"] < 0.05).all()
    assert not r["n_crowded"].any()
    assert d >= 0.5 - 1e-9
    # the second condition of the guarantee: sense_range >= r_i + r_j + 2 x the largest CoM move per sample
    move = np.linalg.norm(np.diff(r["X"][:, :, [0, 2]], axis=1), axis=-1).max()
    print("largest CoM move per sample", move)
    assert 1.5 >= 0.5 + 2 * move


def test_swap_without_rows_walks_through_each_other(swap):
    r = swap[None]
    d = NO.min_pair_distance(r["X"])
    print("no rows: min distance", d)
    assert (r["last_obj"] < 0.05).all() and d < 0.5


def test_swap_with_static_discs_ends_infeasible(swap):
    """share 0: the neighbour steps toward the robot and the robot's constant k = 0 row is violated."""
    r = swap[0.0]
    print("share 0: status", r["last_status"], "min distance", NO.min_pair_distance(r["X"]))
    assert (r["last_status"] == O.STATUS_INFEASIBLE).sum() >= 1
