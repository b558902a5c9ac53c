"""GPU: claim hysteresis (lipmpc_grid_frontier_assign_keep_batch, through CoordinatedFrontierPlanner.replan) against
tests/assign_keep_oracle.py: every output of tests/test_assign_gpu.py's comparison plus kept and n_kept, bit for bit, on the smallest
shapes at which the kernel can go wrong.  Every buffer starts poisoned.  Each case first asserts on the oracle's record that it is
the case its name says."""
import numpy as np
import pytest

import assign_checks as AC
import assign_keep_checks as KC
import assign_keep_oracle as K
import field_oracle as FO
import frontier_oracle as FR
from assign_checks import CELL, ORIGIN, SENTINEL, T_FREE, T_OCC, bits, centres, open_field
from assign_keep_checks import GENEROUS, index

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402


def _side_by_side(n, i=6, j0=8):
    return centres([(i, j0 + k) for k in range(n)])


@pytest.mark.parametrize("none", [None, -1, "cells", K.INT32_MAX, -(1 << 31)])
def test_gpu_no_previous_target_gives_the_plain_claims_bits(none):
    """None, -1, W * H, INT32_MAX (and INT32_MIN) all mean "none": the existing call's outputs, and nobody kept."""
    ev, start = open_field(40, 44), _side_by_side(6, 8, 18)
    prev = None if none is None else np.full(6, ev.size if none == "cells" else none, np.int64).astype(np.int32)
    plain = AC.run(ev, start, 7, 64)
    got, want = KC.check(ev, start, 7, 64, prev, (5, 16, 0))
    for k in plain:
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    assert want["n_claims"] == 6 and not got["kept"].any() and got["n_kept"].tolist() == [0]


def test_gpu_one_robot_keeps_a_target_that_is_still_a_source():
    ev, start, t = open_field(20, 24), _side_by_side(1), (17, 12)
    got, want = KC.check(ev, start, 5, 64, [index(t, 24)], GENEROUS)
    only = np.zeros((20, 24), bool)
    only[t] = True
    fld = K.AO.field_of(want["field"][0] != FO.INF, only)
    assert want["kept"].tolist() == [1] and want["claim_round"].tolist() == [0] and want["targets"] == [t]
    assert got["target_cell"].tolist() == [index(t, 24)] and got["path_cost"][0] == fld[6, 8] / 5.0 > want["nearest"]["path_cost"][0]
    assert np.array_equal(bits(got["sub_goals"][0, got["n_sub"][0] - 1]), bits(centres([t])[0]))


@pytest.mark.parametrize("r_keep,anchored", [(3, True), (2, False)])
def test_gpu_receding_frontier(r_keep, anchored):
    """The previous target (14, 12) is no source any more; what is left of it is the ring cell (17, 12), at distance exactly 3."""
    ev, start = open_field(20, 24), _side_by_side(2)
    got, want = KC.check(ev, start, 5, 64, [index((14, 12), 24), -1], (r_keep, 1024, 4096))
    assert not want["frontier"][0][14, 12] and want["frontier"][0][17, 12]
    if anchored:
        assert want["attempts"][0]["anchor"] == (17, 12) and want["kept"].tolist() == [1, 0] and want["slots"] == 2
    else:
        assert want["attempts"] == [] and want["n_kept"] == 0 and want["slots"] == want["n_claims"] == 2      # no slot was spent
        assert np.array_equal(want["claim_round"], AC.expected(ev, start, 5, 64)["claim_round"])


def test_gpu_two_anchors_at_equal_distance_go_to_the_lower_cell_index():
    ev, start = open_field(20, 24), _side_by_side(1)
    got, want = KC.check(ev, start, 5, 64, [index((5, 5), 24)], (3, 1024, 4096))
    assert want["frontier"][0][2, 5] and want["frontier"][0][5, 2] and want["attempts"][0]["anchor"] == (2, 5)
    assert got["target_cell"].tolist() == [index((2, 5), 24)] and got["kept"].tolist() == [1]


@pytest.mark.parametrize("keep,target,kept", [((0, 16, 7), (17, 8), 1), ((0, 16, 7), (9, 18), 0), ((0, 16, 6), (17, 8), 0),
                                              ((0, 44, 0), (17, 8), 1), ((0, 44, 0), (9, 18), 0), ((0, 43, 0), (17, 8), 0)])
def test_gpu_keep_test_at_equality_and_one_unit_above(keep, target, kept):
    """From (6, 8) the nearest frontier costs 20, the ring cell (17, 8) 55 and (9, 18) 56 (three diagonal and seven axial moves):
    16 * 55 = 16 * 20 + 80 * 7 = 44 * 20 holds with equality, 16 * 56 is one cost unit above it, and one step less of either
    parameter fails 55 too."""
    ev, start = open_field(20, 21), _side_by_side(1)
    got, want = KC.check(ev, start, 5, 64, [index(target, 21)], keep)
    rec, = want["attempts"]
    assert rec["near"] == 20 and rec["cost"] == (55 if target == (17, 8) else 56) and rec["kept"] == bool(kept)
    over = 16 * rec["cost"] - (keep[1] * 20 + 80 * keep[2])
    assert over == 0 if kept else over == 16 if rec["cost"] == 56 else 0 < over <= 80
    assert got["kept"].tolist() == [kept] and want["n_claims"] == 1 and want["slots"] == 2 - kept
    if not kept:                                               # the robot claimed greedily afterwards: its nearest frontier
        assert got["target_cell"].tolist() == want["nearest"]["target_cell"].tolist()


def test_gpu_two_robots_with_the_same_previous_target():
    """The lower index keeps it; the other's anchor falls in its disc (r_keep < r_claim), so it spends no slot and claims greedily."""
    ev, start, t = open_field(20, 24), _side_by_side(2), (17, 12)
    got, want = KC.check(ev, start, 5, 64, [index(t, 24)] * 2, (3, 1024, 4096))
    assert [r["robot"] for r in want["attempts"]] == [0] and want["kept"].tolist() == [1, 0] and want["claim_round"].tolist() == [0, 1]
    assert want["slots"] == 2 and KC.spaced(want, 5)


def test_gpu_anchor_in_a_sealed_off_room():
    ev, start = AC.two_rooms(), centres([(5, 6), (6, 6)])
    got, want = KC.check(ev, start, 12, 64, [index((16, 6), 14), -1], GENEROUS, r=0)
    rec, = want["attempts"]
    assert rec["anchor"] == (16, 6) and rec["entry"] is None and not rec["kept"]
    assert want["slots"] == 2 and want["n_claims"] == 1 and want["claim_round"].tolist() == [0, -1]      # slot 2 found no frontier left
    got, want = KC.check(ev, start, 3, 64, [index((16, 6), 14), -1], GENEROUS, r=0)
    assert want["slots"] == 3 and want["claim_round"].tolist() == [0, 1] and want["n_kept"] == 0


def test_gpu_max_claims_used_up_inside_the_keep_phase():
    ev, start = open_field(20, 24), _side_by_side(4)
    prev = [index(c, 24) for c in ((17, 12), (2, 20), (10, 21), (10, 2))]
    got, want = KC.check(ev, start, 3, 2, prev, GENEROUS)
    assert want["kept"].tolist() == [1, 1, 0, 0] and want["claim_round"].tolist() == [0, 1, -1, -1] and want["slots"] == 2
    f = want["claim_round"] == -1                              # the rest are followers: the path call's rows
    assert np.array_equal(got["target_cell"][f], want["nearest"]["target_cell"][f])
    got, want = KC.check(ev, start, 3, 2, [index((17, 12), 24), -1, -1, -1], (0, 16, 0))      # a failed attempt, then one round
    assert want["n_kept"] == 0 and want["n_claims"] == 1 and want["slots"] == 2


def test_gpu_a_robot_that_may_not_claim_is_never_kept():
    ev, start = open_field(20, 24), _side_by_side(3)
    prev = [index((17, 12), 24)] * 3
    got, want = KC.check(ev, start, 3, 64, prev, GENEROUS, may_claim=np.array([0, 1, 1], np.int8))
    assert want["kept"].tolist() == [0, 1, 0] and want["claim_round"][0] == -1 and [r["robot"] for r in want["attempts"]] == [1]
    assert got["target_cell"][0] == want["nearest"]["target_cell"][0]


@pytest.mark.parametrize("r_keep", [6, 64])
def test_gpu_anchor_window_clipped_at_each_grid_edge(r_keep):
    """tests/test_assign_gpu.py's map with frontier cells on the outermost rows and columns: previous targets in the four corners
    and beside the four edges, whose windows reach over every end of the grid."""
    W, H = 14, 17
    ev = np.full((W, H), -T_FREE, np.int32)
    for c in ((1, 1), (1, H - 2), (W - 2, 1), (W - 2, H - 2), (1, 8), (W - 2, 8), (7, 1), (7, H - 2)):
        ev[c] = 0
    start = centres([(6, 7), (6, 8), (6, 9), (7, 7), (7, 8), (7, 9), (8, 7), (8, 9)])
    prev = [index(c, H) for c in ((0, 0), (0, H - 1), (W - 1, 0), (W - 1, H - 1), (0, 5), (W - 1, 11), (4, 0), (10, H - 1))]
    got, want = KC.check(ev, start, 3, 64, prev, (r_keep, 1024, 4096), r=0, mu=1)
    assert len(want["attempts"]) >= (8 if r_keep == 6 else 4) and want["n_kept"] == len(want["attempts"]) and KC.spaced(want, 3)
    if r_keep == 6:
        assert want["attempts"][0]["anchor"] == (0, 0) and want["attempts"][3]["anchor"] == (W - 1, H - 1)


@pytest.mark.parametrize("r_keep", [0, 64])
def test_gpu_smallest_and_largest_keep_radius(r_keep):
    """r_keep 0 takes the very cell or nothing; r_keep 64 searches a window larger than the map."""
    ev, start = open_field(20, 24), _side_by_side(2)
    got, want = KC.check(ev, start, 5, 64, [index((10, 12), 24), index((2, 8), 24)], (r_keep, 1024, 4096))
    if r_keep == 0:
        assert [r["robot"] for r in want["attempts"]] == [1] and want["kept"].tolist() == [0, 1]
    else:
        assert want["attempts"][0]["anchor"] == (17, 12)      # seven cells away: the nearest cell of the ring
        assert want["kept"].tolist() == [1, 1]


def test_gpu_start_in_the_inflation_band_snaps_in_the_keep_field():
    """Robot 0 stands beside the solid cell, inside the band r_inflate blocks: (9, 12) and (11, 12) are equally near, and the
    field of the anchor alone -- on the far side -- is lower at (11, 12), where the nearest-frontier field sent it to (9, 12)."""
    ev = AC.block_in_field()
    start = centres([(10, 11)])
    got, want = KC.check(ev, start, 12, 64, [index((21, 12), 24)], GENEROUS)
    rec, = want["attempts"]
    assert FO.snap(want["nearest"]["field"][0], (10, 11), 2) == (9, 12) and rec["entry"] == (11, 12) and rec["kept"]
    assert rec["near"] == int(want["nearest"]["field"][0][9, 12])


def test_gpu_overflow_keeper_still_takes_its_disc():
    ev = AC.block_in_field()
    start = centres([(12, 10), (12, 11)])
    got, want = KC.check(ev, start, 6, 64, [index((21, 12), 24)] * 2, (3, 1024, 4096), max_seg=10, S_max=1)
    assert want["kept"].tolist() == [1, 0] and (want["status"] == FR.PATH_OVERFLOW).all() and (want["n_sub"] == 0).all()
    assert [r["robot"] for r in want["attempts"]] == [0] and KC.spaced(want, 6) and (got["sub_goals"] == SENTINEL).all()


@pytest.mark.parametrize("B", [65, 1025])
def test_gpu_more_robots_than_a_wave_and_than_the_workgroup(B):
    """Keep candidates in the first wave, past it, and (B = 1025) in the second chunk of robots; robot 1 has a target that fails."""
    ev = open_field(24, 20)
    rng = np.random.default_rng(B)
    start = centres([(4, 9)])[0] + rng.uniform(-0.14, 0.14, (B, 2)) * np.array(CELL)
    prev = np.full(B, -1, np.int64)
    mid = 40 if B == 65 else 64
    prev[[3, mid, B - 1]] = [index(c, 20) for c in ((21, 10), (12, 17), (12, 2))]
    prev[1] = index((21, 3), 20)
    got, want = KC.check(ev, start, 6, 8, prev, (0, 48, 12))
    assert [(r["robot"], r["kept"]) for r in want["attempts"]] == [(1, False), (3, True), (mid, True), (B - 1, True)]
    assert want["n_claims"] == 7 and want["slots"] == 8 and want["kept"].sum() == 3 and (want["claim_round"] == -1).sum() == B - 7


def test_gpu_each_side_of_the_keep_kernels_lds_switch():
    """The largest map whose slot field the keep kernel holds in LDS and the first it relaxes in ``work``, by the oracle module's
    restatement of the kernel's own rule (48 bytes more than the assign kernel's: at 193 columns the switch falls between the
    same two widths); 3 slots."""
    for W, H in K.sizes_at_the_lds_switch():
        ev = open_field(W, H, margin=3)
        ev[W // 2, 10:H - 10] = T_OCC
        start = centres([(W // 2 - 6, H // 2), (W // 2 - 6, H // 2 + 1), (W // 2 - 7, H // 2)])
        got, want = KC.check(ev, start, 30, 3, [-1, index((3, 20), H), -1], GENEROUS, S_max=16)
        assert want["kept"].tolist() == [0, 1, 0] and want["n_claims"] == 3 and want["slots"] == 3


def _captured(pl, ev, start, prev, out):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pl.replan(ev, start, origin=ORIGIN, cell=CELL, out=out, prev_target=prev)         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pl.replan(ev, start, origin=ORIGIN, cell=CELL, out=out, prev_target=prev)
    return graph


def test_gpu_graph_replay_and_repeat_give_the_same_bits():
    ev, start = open_field(40, 44), _side_by_side(6, 8, 18)
    prev = AC.expected(ev, start, 7, 64)["target_cell"]
    keep = (3, 24, 4)
    eager = [KC.run(ev, start, 7, 64, prev, keep) for _ in range(2)]
    for k in eager[0]:
        assert np.array_equal(bits(eager[0][k]), bits(eager[1][k])), k
    assert 0 < eager[0]["n_kept"][0] < 6
    pl = KC.planner(7, 64, keep)
    out = KC.buffers(6, 40, 44, 64)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")      # (alive as long as the graph reads them)
    d_prev = torch.as_tensor(prev, device="cuda")
    graph = _captured(pl, d_ev, d_start, d_prev, out)
    for _ in range(2):
        fresh = KC.buffers(6, 40, 44, 64)
        for k in out:
            out[k].copy_(fresh[k])                             # poisoned again, in the memory the graph writes
        graph.replay()
        torch.cuda.synchronize()
        got = AC.host(out)
        for k in eager[0]:
            assert np.array_equal(bits(got[k]), bits(eager[0][k])), k


def test_gpu_planner_arguments():
    ev, start = open_field(20, 24), _side_by_side(3)
    d_ev = torch.as_tensor(ev, device="cuda")
    pl = KC.planner(5, 64, GENEROUS)
    prev = [index((17, 12), 24), -1, -1]
    fresh = pl.replan(d_ev, start, origin=ORIGIN, cell=CELL, prev_target=prev)          # fresh buffers, a list of Python ints
    torch.cuda.synchronize()
    assert set(fresh) >= {"kept", "n_kept", "claim_round", "n_claims", "work"} and fresh["kept"].tolist() == [1, 0, 0]
    assert fresh["n_kept"].tolist() == [1] and fresh["n_claims"].tolist() == [3]
    wide = pl.replan(d_ev, start, origin=ORIGIN, cell=CELL, prev_target=torch.tensor([index((17, 12), 24), 1 << 40, -(1 << 40)]))
    torch.cuda.synchronize()
    assert all(torch.equal(wide[k], fresh[k]) for k in ("kept", "claim_round", "target_cell", "n_sub"))      # int64: out of range = none
    plain = pl.plan(d_ev, start, origin=ORIGIN, cell=CELL)      # plan = replan without previous targets
    torch.cuda.synchronize()
    old = AC.planner(5, 64).plan(d_ev, start, origin=ORIGIN, cell=CELL)
    torch.cuda.synchronize()
    assert plain["kept"].tolist() == [0, 0, 0] and all(torch.equal(plain[k], old[k]) for k in old if k != "work")
    assert "kept" not in old and "n_kept" not in old           # without r_keep: the dict of before
    assert tuple(pl.replan(d_ev, np.zeros((0, 2)), origin=ORIGIN, cell=CELL)["kept"].shape) == (0,)
    with pytest.raises(ValueError):
        AC.planner(5, 64).replan(d_ev, start, origin=ORIGIN, cell=CELL, prev_target=prev)      # a planner without r_keep
    with pytest.raises(ValueError):
        AC.planner(5, 64).replan(d_ev, start, origin=ORIGIN, cell=CELL)
    for bad in ([1, 2], [[1, 2, 3]], [1.0, 2.0, 3.0], [True, False, True]):
        with pytest.raises(ValueError):
            pl.replan(d_ev, start, origin=ORIGIN, cell=CELL, prev_target=bad)
    for bad in (dict(r_keep=3), dict(r_keep=65, keep_ratio16=16, keep_slack=0), dict(keep_slack=3)):
        with pytest.raises(ValueError):
            lipmpc.CoordinatedFrontierPlanner(5, t_free=T_FREE, t_occ=T_OCC, **bad)
