"""The scan matcher's rule on the CPU: tests/scan_match_oracle.py, the numpy restatement of lipmpc_scan_match_batch
(include/lipmpc.h), on hand-built cases for every selection key and for the acceptance test, and on the displaced scans of a
small room (tests/scan_match_cases.py)."""
import numpy as np
import pytest

import map_oracle as M
import scan_match_cases as K
import scan_match_oracle as S

CELL, ORIGIN = (0.1, 0.1), (0.0, 0.0)
P0 = (1.05, 1.05)                       # the centre of cell (10, 10)


def _one(evidence, hits, n_x=2, n_y=2, clamp=8, min_score=1, min_gain=0, position=P0, **kw):
    """Hand-built cases: depth 0, so a reading is its own end point."""
    return S.match_one(position, np.asarray(hits, float), evidence, ORIGIN, CELL, 1.5, 0.0, n_x, n_y, clamp, min_score, min_gain, **kw)


def _centre(i, j):
    return ((i + 0.5) * CELL[0], (j + 0.5) * CELL[1])


def test_empty_map_gives_the_zero_candidate():
    """Every candidate scores 0: the second key (a * a + b * b), then the yaw keys, pick the zero candidate."""
    ev = np.zeros((30, 30), np.int64)
    hits = [_centre(15, 10), _centre(10, 16), _centre(4, 10), (np.nan, 1.0)]
    for n_yaw in (0, 3):
        r = _one(ev, hits, n_x=4, n_y=3, n_yaw=n_yaw, rot=S.rot_table(n_yaw, 0.05))
        assert r == dict(offset_cells=(0, 0), yaw_index=0, offset=(0.0, 0.0), score=(0, 0), n_used=3, matched=0), r


def test_corridor_is_ambiguous_along_its_axis():
    """Two walls along x, the scan displaced by (3, -2) cells: every a scores alike, so a = 0 by the second key; b is put back."""
    ev = np.zeros((40, 30), np.int64)
    ev[:, 6] = ev[:, 16] = 9
    ev[:, 7:16] = -3
    true = np.array(_centre(20, 11))
    hits = np.array([_centre(i, 6) for i in range(16, 25)] + [_centre(i, 16) for i in range(16, 25)])
    d = np.array([3 * CELL[0], -2 * CELL[1]])
    r = _one(ev, hits + d, n_x=4, n_y=4, clamp=8, position=true + d)
    assert r["offset_cells"] == (0, 2) and r["matched"] == 1 and r["score"] == (18 * 8, 9 * -3), r      # unshifted: 9 readings on free cells, 9 below the corridor
    sc = S.scores(S.used_cells(true + d, hits + d, ORIGIN, CELL, 1.5, 0.0), ev, 4, 4, 8)[0]
    assert (sc[:, 4 + 2] == 18 * 8).all() and (np.delete(sc, 4 + 2, axis=1) < 18 * 8).all()      # ambiguous in a, and only there


def _yaw_case(rows):
    """One reading 1.0 ahead of the robot (cell (20, 10)), yaw steps of 0.15: k - n_yaw = -2 .. 2 puts it in rows 7, 9, 10, 11 and 13
    of column 20.  Evidence 5 in the given rows."""
    ev = np.zeros((30, 30), np.int64)
    for j in rows:
        ev[20, j] = 5
    rot = S.rot_table(2, 0.15)
    cells = S.used_cells(P0, [(2.05, 1.05)], ORIGIN, CELL, 1.5, 0.0, rot, 2)
    assert [tuple(c[0]) for c in cells] == [(20, 7), (20, 9), (20, 10), (20, 11), (20, 13)], cells
    return _one(ev, [(2.05, 1.05)], n_x=0, n_y=0, n_yaw=2, rot=rot)


def test_yaw_ties_take_the_smaller_turn_then_the_smaller_index():
    r = _yaw_case((11, 13))              # k - n_yaw = 1 and 2 tie on score and shift: the smaller |k - n_yaw|
    assert r["yaw_index"] == 1 and r["score"] == (5, 0) and r["matched"] == 1 and r["offset_cells"] == (0, 0), r
    r = _yaw_case((9, 11))               # -1 and 1 tie on |k - n_yaw| too: the smaller k
    assert r["yaw_index"] == -1 and r["score"] == (5, 0) and r["matched"] == 1, r
    r = _yaw_case((7, 9, 10, 11, 13))    # the unturned scan ties with all: it wins
    assert r["yaw_index"] == 0 and r["score"] == (5, 5) and r["matched"] == 0, r


def test_index_key_breaks_the_last_tie():
    """Four shifts of one cell score alike: the smallest (a + n_x)(2 n_y + 1) + (b + n_y) is a = -1, b = 0; among the two of
    a = 0 it is b = -1."""
    ev = np.zeros((30, 30), np.int64)
    ev[14, 10] = ev[16, 10] = ev[15, 9] = ev[15, 11] = 4
    assert _one(ev, [_centre(15, 10)])["offset_cells"] == (-1, 0)
    ev[14, 10] = ev[16, 10] = 0
    assert _one(ev, [_centre(15, 10)])["offset_cells"] == (0, -1)
    ev[15, 9] = 0
    assert _one(ev, [_centre(15, 10)])["offset_cells"] == (0, 1)


def test_acceptance_either_side_of_both_thresholds():
    ev = np.zeros((30, 30), np.int64)
    ev[16, 10], ev[15, 10] = 6, 2        # best: a = 1 with 6; the zero candidate has 2
    hit = [_centre(15, 10)]
    yes = dict(offset_cells=(1, 0), yaw_index=0, offset=(np.float64(1) * np.float64(0.1), 0.0), score=(6, 2), n_used=1, matched=1)
    no = dict(yes, offset_cells=(0, 0), offset=(0.0, 0.0), matched=0)
    assert _one(ev, hit, min_score=6, min_gain=4) == yes
    assert _one(ev, hit, min_score=7, min_gain=4) == no
    assert _one(ev, hit, min_score=6, min_gain=5) == no
    assert _one(ev, hit, min_score=-100, min_gain=0) == yes


@pytest.mark.parametrize("clamp", [1, 127])
def test_clamp_bounds_what_a_cell_can_say(clamp):
    ev = np.zeros((30, 30), np.int64)
    ev[15, 10], ev[15, 11], ev[14, 10] = -100000, 100000, clamp
    r = _one(ev, [_centre(15, 10), _centre(15, 10)], clamp=clamp)
    assert r["score"] == (2 * clamp, -2 * clamp) and r["offset_cells"] == (-1, 0), r      # 100000 counts as clamp: a tie, the index key


def test_robots_without_a_cell_and_masked_robots_get_zeros():
    ev = K.line_evidence()
    pos = np.array([[1.0, 0.7], [np.nan, 0.7], [1.0, 0.7], [1e300, 0.7]])
    hits = K.scan(np.array([[1.0, 0.7]] * 4))
    out = S.match(pos, hits, ev, K.ORIGIN, K.CELL, K.RANGE, K.DEPTH, 2, 2, 8, 1, 0, mask=np.array([1, 1, 0, 1]))
    assert out["n_used"][0] > 20 and out["score"][0, 0] > 0
    for name, v in out.items():
        assert not v[1:].any(), name
    assert out["offset_cells"].dtype == np.int32 and out["matched"].dtype == np.int8 and out["offset"].dtype == np.float64


@pytest.mark.parametrize("noisy", [False, True])
def test_used_cells_at_the_zero_yaw_are_the_cells_the_update_raises(noisy):
    rng = np.random.default_rng(7)
    pos = np.concatenate([K.mapped_poses()[::3], [[0.31, 0.27], [4.6, 3.8], [-0.4, 1.0]]])
    hits = K.scan(pos, 0.01 * rng.standard_normal((len(pos), K.R, 2)) if noisy else None)
    rot = S.rot_table(2, 0.03)
    n_hit = 0
    for p, h in zip(pos, hits):
        _, hit, (wi0, wj0) = M.robot_marks(p, h, K.ORIGIN, K.CELL, K.RANGE, K.table(), K.DEPTH)
        want = {(wi0 + i, wj0 + j) for i, j in np.argwhere(hit)}
        for n_yaw in (0, 2):
            got = S.used_cells(p, h, K.ORIGIN, K.CELL, K.RANGE, K.DEPTH, rot, n_yaw)[n_yaw]
            assert {tuple(c) for c in got} == want
        n_hit += len(want)
    assert n_hit > 100


@pytest.mark.parametrize("noisy", [False, True])
def test_displaced_scans_are_put_back(noisy):
    """120 scans from 6 poses near the mapped line, displaced by whole cells of up to (+-4, +-4), matched with n = 5 against the
    evidence of the 12 mapped scans: every displacement is put back exactly, none excluded."""
    ev = K.line_evidence()
    rng = np.random.default_rng(1)
    cases = K.displaced_cases()
    assert len(cases) == 120 and max(max(abs(s[0]), abs(s[1])) for _, s in cases) == 4
    for q, s in cases:
        h = K.scan(q[None], 0.01 * rng.standard_normal((1, K.R, 2)) if noisy else None)[0]
        p, hh = K.displace(q, h, s)
        r = S.match_one(p, hh, ev, K.ORIGIN, K.CELL, K.RANGE, K.DEPTH, K.N_SEARCH, K.N_SEARCH, K.CLAMP, 1, 0)
        assert r["offset_cells"] == (-s[0], -s[1]) and r["matched"] == (s != (0, 0)) and r["n_used"] > 20, (q, s, r)


def test_window_cap():
    assert S.window_fits(1.5, 0.05, (0.1, 0.1), 16, 16) and S.grown_window(1.5, 0.05, (0.1, 0.1), 16, 16) == (67, 67)
    assert S.window_fits(5.0, 0.0, (0.05, 0.05), 8, 8) and not S.window_fits(5.0, 0.0, (0.05, 0.05), 9, 9)      # 221 x 221, 223 x 223
    assert M.window_fits(5.4, 0.0, (0.05, 0.05)) and not S.window_fits(5.4, 0.0, (0.05, 0.05), 1, 0)
