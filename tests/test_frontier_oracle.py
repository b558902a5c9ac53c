"""CPU: the numpy restatement of the frontier explorer (tests/frontier_oracle.py) against its definition -- the masks cell by
cell, the multi-source field against the minimum of single-goal fields of tests/field_oracle.py -- and the two ends of an
exploration: a map with no free cell, and a fully known room."""
import numpy as np

import field_oracle as FO
import frontier_oracle as FR

ORIGIN, CELL = (-0.3, 0.2), (0.1, 0.25)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _hand_made(rng, W, H, t_free, t_occ):
    """Evidence with all three classes: a known-free blob, some walls, the rest undecided (values on both sides of 0)."""
    ev = rng.integers(-t_free + 1, t_occ, (W, H)).astype(np.int32)                 # unknown, every value of the open interval
    free = rng.random((W, H)) < 0.6
    ev[free] = -t_free - rng.integers(0, 3, int(free.sum()))
    solid = rng.random((W, H)) < 0.12
    ev[solid] = t_occ + rng.integers(0, 3, int(solid.sum()))
    return ev


def test_masks_follow_the_definition_cell_by_cell():
    rng = np.random.default_rng(5)
    for _ in range(60):
        W, H, r, mu = int(rng.integers(2, 11)), int(rng.integers(2, 9)), int(rng.integers(0, 3)), int(rng.integers(1, 9))
        t_free, t_occ = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        ev = _hand_made(rng, W, H, t_free, t_occ)
        blocked, frontier, unknown = FR.masks(ev, t_free, t_occ, r, mu)
        for i in range(W):
            for j in range(H):
                e = int(ev[i, j])
                solid, free = e >= t_occ, e <= -t_free
                assert unknown[i, j] == (not solid and not free)
                near = any(int(ev[a, b]) >= t_occ and (i - a) ** 2 + (j - b) ** 2 <= r * r for a in range(W) for b in range(H))
                assert blocked[i, j] == ((not free) or near)
                n_unk = sum(1 for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di or dj) and 0 <= i + di < W and 0 <= j + dj < H
                            and not int(ev[i + di, j + dj]) >= t_occ and not int(ev[i + di, j + dj]) <= -t_free)
                assert frontier[i, j] == ((not blocked[i, j]) and n_unk >= mu)


def test_classes_at_the_thresholds_and_the_ends_of_int32():
    for t_free, t_occ in ((1, 3), (2, 1), (1 << 30, 1 << 30), (7, 1 << 30), (1 << 30, 5)):
        vals = [-t_free - 1, -t_free, -t_free + 1, t_occ - 1, t_occ, I32_MIN, I32_MAX]
        ev = np.array([vals, vals], np.int32)
        solid, free, unknown = FR.classes(ev, t_free, t_occ)
        want_free = [True, True, False, t_occ - 1 <= -t_free, False, True, False]
        want_solid = [False, False, -t_free + 1 >= t_occ, False, True, False, True]
        assert free[0].tolist() == want_free and solid[0].tolist() == want_solid, (t_free, t_occ)
        assert (unknown == (~solid & ~free)).all() and not (solid & free).any()
    # a strip: free | free | unknown | unknown | solid, thresholds (1, 3): the free cell next to the unknown ones is the frontier
    ev = np.array([[-2, -1, 0, 2, 3]] * 2, np.int32)
    blocked, frontier, unknown = FR.masks(ev, 1, 3, 0, 1)
    assert unknown[0].tolist() == [False, False, True, True, False]
    assert blocked[0].tolist() == [False, False, True, True, True] and frontier[0].tolist() == [False, True, False, False, False]


def test_field_is_the_minimum_of_the_single_goal_fields():
    rng = np.random.default_rng(7)
    n_multi = 0
    for _ in range(25):
        W, H, r, mu = int(rng.integers(3, 12)), int(rng.integers(3, 10)), int(rng.integers(0, 3)), int(rng.integers(1, 4))
        ev = _hand_made(rng, W, H, 1, 3)
        fld, frontier, n = FR.field(ev, 1, 3, r, mu)
        blocked, fr_mask, _ = FR.masks(ev, 1, 3, r, mu)
        assert n == int(fr_mask.sum()) and (frontier != 0).tolist() == fr_mask.tolist()
        want = np.full((W, H), FO.INF, np.uint32)
        for i, j in zip(*np.nonzero(fr_mask)):
            one, st = FO.field(blocked, ORIGIN, CELL, FO.centre((i, j), ORIGIN, CELL), 0)
            assert st == FO.FIELD_OK
            want = np.minimum(want, one)
        assert (fld == want).all()
        assert (fld[fr_mask] == 0).all() and (fld[blocked] == FO.INF).all()
        n_multi += n > 1
    assert n_multi >= 10


def test_the_grids_edge_is_no_frontier():
    ev = np.full((6, 5), -1, np.int32)                         # all free, nothing unknown: the edge does not count
    fld, frontier, n = FR.field(ev, 1, 3, 0, 1)
    assert n == 0 and not frontier.any() and (fld == FO.INF).all()


def test_no_free_cell_and_a_fully_known_room_have_no_frontier():
    for ev in (np.zeros((7, 9), np.int32), np.full((7, 9), 3, np.int32), FR.room()):
        for r in (0, 2):
            fld, frontier, n = FR.field(ev, 1, 3, r, 1)
            assert n == 0 and not frontier.any() and (fld == FO.INF).all()
    ev = FR.room()
    out = FR.plan_batch(ev, 1, 3, ORIGIN, CELL, [FO.centre((5, 5), ORIGIN, CELL)], r_inflate=0)
    assert out["status"].tolist() == [FR.NO_PATH] and out["target_cell"].tolist() == [-1] and out["n_sub"].tolist() == [0]


def test_paths_end_at_the_centre_of_the_first_frontier_cell():
    ev = FR.room(14, 11)
    ev[9:13, 3:8] = 0                                          # an unexplored pocket: its rim is the frontier
    ev[1:3, 1:3] = 0                                           # and a corner
    starts = [FO.centre(c, ORIGIN, CELL) for c in ((5, 5), (3, 2), (8, 5), (6, 9))] + [(99.0, 0.0), (np.nan, 0.3), FO.centre((0, 4), ORIGIN, CELL),
                                                                                    FO.centre((9, 5), ORIGIN, CELL), FO.centre((10, 5), ORIGIN, CELL)]
    out = FR.plan_batch(ev, 1, 3, ORIGIN, CELL, starts, r_inflate=0, min_unknown=2)
    H = ev.shape[1]
    assert out["status"].tolist() == [FR.FOUND] * 4 + [FR.OUTSIDE_GRID, FR.OUTSIDE_GRID, FR.START_OCCUPIED, FR.FOUND, FR.NO_PATH]
    assert out["cells"][7][0] == (8, 5) and out["target_cell"][8] == -1         # an unknown start snaps; deep in the pocket nothing is near
    for b in range(4):
        t = int(out["target_cell"][b])
        assert out["frontier"][0, t // H, t % H] == 1 and out["field"][0, t // H, t % H] == 0
        assert (out["sub_goals"][b][-1] == FO.centre((t // H, t % H), ORIGIN, CELL)).all() and (out["target"][b] == out["sub_goals"][b][-1]).all()
        assert out["cells"][b][-1] == (t // H, t % H) and all(out["field"][0][c] > 0 for c in out["cells"][b][:-1])
        assert out["path_cost"][b] == int(out["field"][0][out["cells"][b][0]]) / 5.0
    assert out["n_sub"][2] == 1 and len(out["cells"][2]) == 1                    # (8, 5) is itself a frontier cell
    assert np.isnan(out["target"][4:7]).all() and (out["target_cell"][4:7] == -1).all()
    tight = FR.plan_batch(ev, 1, 3, ORIGIN, CELL, starts[:1], r_inflate=0, max_seg=5, S_max=1)
    assert tight["status"].tolist() == [FR.PATH_OVERFLOW] and tight["target_cell"][0] == out["target_cell"][0] and tight["n_sub"][0] == 0


def test_the_lds_rule_has_a_size_on_each_side():
    (W, H), (W1, H1) = FR.sizes_at_the_lds_switch()
    assert FR.field_fits_lds(W * H) and not FR.field_fits_lds(W1 * H1) and W1 * H1 <= 1 << 17 and max(W1, H1) <= 4096
