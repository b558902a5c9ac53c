"""GPU: the coordinated claim (lipmpc_grid_frontier_assign_batch, through CoordinatedFrontierPlanner) against
tests/assign_oracle.py: claim_round, n_claims, the int32 n_sub / status / target_cell and the doubles of path_cost, target and the
WHOLE sub-goal buffer, bit for bit, on the smallest shapes at which the kernel can go wrong.  Every buffer starts poisoned."""
import numpy as np
import pytest

import assign_checks as AC
import assign_oracle as A
import field_oracle as FO
import frontier_oracle as FR
from assign_checks import CELL, ORIGIN, POISON_WORK, SENTINEL, T_FREE, T_OCC, bits, centres, open_field

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402


def _side_by_side(n, i=6, j0=8, origin=ORIGIN, cell=CELL):
    """n robots in neighbouring cells of one row: what the nearest-frontier rule sends to one spot."""
    return centres([(i, j0 + k) for k in range(n)], origin, cell)


def test_gpu_smallest_grid_all_unknown():
    got, want = AC.check(np.zeros((2, 2), np.int32), centres(((0, 0), (1, 1))), 1, 4, r=0, mu=1)
    assert want["n_claims"] == 0 and (want["claim_round"] == -1).all() and (want["status"] == FR.NO_PATH).all()
    assert (got["sub_goals"] == SENTINEL).all()


@pytest.mark.parametrize("max_claims", [0, 1])
def test_gpu_no_claim_and_one_claim_leave_the_path_calls_rows(max_claims):
    """max_claims = 0 writes claim_round and n_claims only; the round-0 winner's rows are the path call's own."""
    ev, start = open_field(20, 24), _side_by_side(3)
    got, want = AC.check(ev, start, 5, max_claims)
    near = want["nearest"]
    assert want["n_claims"] == max_claims and sorted(want["claim_round"].tolist()) == [-1, -1, -1 + max_claims]
    for k in ("status", "n_sub", "target_cell"):
        assert np.array_equal(got[k], near[k]), k
    assert np.array_equal(bits(got["path_cost"]), bits(near["path_cost"])) and np.array_equal(bits(got["target"]), bits(near["target"]))
    for b in range(3):
        assert np.array_equal(bits(got["sub_goals"][b, :near["n_sub"][b]]), bits(near["sub_goals"][b]))


def test_gpu_one_robot():
    got, want = AC.check(open_field(20, 24), _side_by_side(1), 5, 64)
    assert want["n_claims"] == 1 and want["claim_round"].tolist() == [0]


@pytest.mark.parametrize("r_claim", [0, 5, 15, 4096])
def test_gpu_one_ring_of_an_open_field(r_claim):
    """Six robots side by side before the one-ring frontier of an open field: the claims spread with the radius."""
    ev, start = open_field(40, 44), _side_by_side(6, i=8, j0=18)
    got, want = AC.check(ev, start, r_claim, 64)
    t = np.array(want["targets"])
    assert want["n_claims"] == (1 if r_claim == 4096 else 6) and np.all(np.diff(want["costs"]) >= 0)
    d2 = ((t[:, None] - t[None]) ** 2).sum(2)[np.triu_indices(len(t), 1)]
    assert (d2 > r_claim * r_claim).all()
    if r_claim == 4096:                                       # one disc takes the whole ring: five followers keep their nearest plan
        assert sorted(want["claim_round"].tolist()) == [-1] * 5 + [0]
        assert np.array_equal(want["target_cell"], want["nearest"]["target_cell"])
    if r_claim == 15:
        assert len({tuple(x) for x in t}) == 6 and d2.min() > 225


def test_gpu_two_robots_in_one_cell_tie_to_the_lower_index():
    c = centres([(6, 8)])[0]
    start = np.array([c + (0.01, 0.01), c - (0.01, 0.01), c])
    got, want = AC.check(open_field(20, 24), start, 4, 64)
    assert want["winners"] == [0, 1, 2] and want["costs"][0] == want["nearest"]["field"][0][6, 8]


def test_gpu_followers_and_spare_claims():
    ev, start = open_field(20, 24), _side_by_side(5)
    got, want = AC.check(ev, start, 3, 2)                      # more robots than claims: three followers
    assert want["n_claims"] == 2 and (want["claim_round"] == -1).sum() == 3
    f = want["claim_round"] == -1
    assert np.array_equal(want["target_cell"][f], want["nearest"]["target_cell"][f])
    got, want = AC.check(ev, start, 3, 4096)                   # more claims allowed than robots
    assert want["n_claims"] == 5 and sorted(want["claim_round"].tolist()) == [0, 1, 2, 3, 4]


def test_gpu_may_claim_with_zeros():
    ev, start = open_field(20, 24), _side_by_side(5)
    may = np.array([0, 1, 0, 1, 1], np.int8)
    got, want = AC.check(ev, start, 3, 64, may_claim=may)
    assert want["n_claims"] == 3 and (want["claim_round"][may == 0] == -1).all() and (want["claim_round"][may == 1] >= 0).all()
    got, want = AC.check(ev, start, 3, 64, may_claim=np.zeros(5, bool))
    assert want["n_claims"] == 0


def test_gpu_robots_that_never_claim():
    """On a solid cell, deep in the unknown, outside the grid, a NaN and an infinite coordinate: status and rows stay the path call's."""
    ev = open_field(20, 24, margin=4)
    ev[10, 10] = T_OCC
    start = np.concatenate([_side_by_side(2), centres([(10, 10), (0, 0)]), [[ORIGIN[0] - 1.0, 0.5], [np.nan, 0.5], [0.5, np.inf]]])
    got, want = AC.check(ev, start, 3, 64, r=1)
    assert want["status"].tolist() == [FR.FOUND, FR.FOUND, FR.START_OCCUPIED, FR.NO_PATH] + [FR.OUTSIDE_GRID] * 3
    assert want["n_claims"] == 2 and (want["claim_round"][2:] == -1).all()


def test_gpu_two_rooms_one_used_up():
    """Room A's frontier is gone after one claim, room B's is not: A's second robot stays a follower while B's robot claims, and a
    robot whose reachable frontier is used up is no candidate although the sources are not empty."""
    ev = AC.two_rooms()
    start = centres([(5, 6), (6, 6), (20, 6), (21, 6)])
    got, want = AC.check(ev, start, 12, 64, r=0)
    assert want["n_claims"] == 3 and want["claim_round"][1] == -1 and want["claim_round"][0] == 0
    assert want["n_sources"][-1] > 0 and (want["claim_round"][2:] >= 0).all()
    assert want["target_cell"][1] == want["nearest"]["target_cell"][1]


def test_gpu_start_in_the_inflation_band_snaps_per_round():
    """Robot 1 stands beside a solid cell, inside the band r_inflate blocks: its entry cell is a snap, taken in the round's own
    field -- (9, 12) and (11, 12) are equally near, the lower field wins -- so it moves to the other side of the block when robot
    0's claim removes the frontier it pointed to."""
    ev = AC.block_in_field()
    start = centres([(4, 12), (10, 11)])
    got, want = AC.check(ev, start, 12, 64)
    c = FO.cell_of(start[1], ORIGIN, CELL, 24, 24)
    assert want["nearest"]["field"][0][c] == FO.INF and FO.snap(want["nearest"]["field"][0], c, 2) == (9, 12)
    assert want["winners"] == [0, 1] and want["snapped"][1] == (11, 12)


@pytest.mark.parametrize("r_claim", [3, 6])
def test_gpu_discs_clipped_at_the_grid(r_claim):
    """A known field with single unknown cells one step from every corner and every edge (min_unknown 1: their neighbours, the
    grid's outermost rows and columns included, are the frontier): every claim's disc reaches over an end of the grid."""
    W, H = 14, 17
    ev = np.full((W, H), -T_FREE, np.int32)
    for c in ((1, 1), (1, H - 2), (W - 2, 1), (W - 2, H - 2), (1, 8), (W - 2, 8), (7, 1), (7, H - 2)):
        ev[c] = 0
    start = centres([(6, 7), (6, 8), (6, 9), (7, 7), (7, 8), (7, 9), (8, 7), (8, 9)])
    got, want = AC.check(ev, start, r_claim, 64, r=0, mu=1)
    t = np.array(want["targets"])
    assert want["n_claims"] == 8 and ((t[:, 0] < r_claim) | (t[:, 0] > W - 1 - r_claim) | (t[:, 1] < r_claim) | (t[:, 1] > H - 1 - r_claim)).all()
    for side in (t[:, 0] < r_claim, t[:, 0] > W - 1 - r_claim, t[:, 1] < r_claim, t[:, 1] > H - 1 - r_claim):
        assert side.any()
    if r_claim == 6:
        assert (t[:, 0] == 0).any() and (t[:, 1] == 1).any()    # targets on the outermost row / one column from the end


@pytest.mark.parametrize("B", [65, 1025])
def test_gpu_more_robots_than_a_wave_and_than_the_workgroup(B):
    """Robot B - 1 is the only one near the far side: it must win its round from the stride's last pass."""
    ev = open_field(24, 20)
    rng = np.random.default_rng(B)
    start = centres([(4, 9)])[0] + rng.uniform(-0.14, 0.14, (B, 2)) * np.array(CELL)
    start[B - 1] = centres([(20, 10)])[0]
    got, want = AC.check(ev, start, 6, 8)
    assert want["n_claims"] == 8 and want["claim_round"][B - 1] >= 0 and (want["claim_round"] == -1).sum() == B - 8


@pytest.mark.parametrize("W,H", [(5, 13), (4, 33), (3, 64), (2, 65), (7, 31)])
def test_gpu_ballot_words_and_row_ends(W, H):
    """65 cells cross a ballot word; H = 33 / 64 end a row one bit after / at a word boundary.  Frontier cells at both row ends."""
    rng = np.random.default_rng(W * 100 + H)
    ev = np.full((W, H), -T_FREE, np.int32)
    ev[:, 0] = np.where(np.arange(W) % 2 == 0, 0, -T_FREE)
    ev[:, H - 1] = np.where(np.arange(W) % 2 == 0, -T_FREE, 0)
    ev[rng.random((W, H)) < 0.05] = 0
    start = centres([(rng.integers(W), rng.integers(1, H - 1)) for _ in range(6)])
    for r_claim in (1, 3):
        got, want = AC.check(ev, start, r_claim, 64, r=0, mu=1)
        assert want["n_claims"] >= 2


def test_gpu_each_side_of_the_lds_switch():
    """The largest map whose round field the kernel keeps in LDS and the first it relaxes in ``work``, by the oracle module's
    restatement of the kernel's own rule; max_claims 2."""
    for W, H in A.sizes_at_the_lds_switch():
        ev = open_field(W, H, margin=3)
        ev[W // 2, 10:H - 10] = T_OCC
        start = centres([(W // 2 - 6, H // 2), (W // 2 - 6, H // 2 + 1), (W // 2 - 7, H // 2)])
        got, want = AC.check(ev, start, 30, 2, S_max=16)
        assert want["n_claims"] == 2 and want["costs"][1] > want["costs"][0] > 100


def test_gpu_overflow_winner_still_claims():
    """S_max 1: a winner whose path needs more sub-goals ends PATH_OVERFLOW, writes no row, and its disc is taken all the same."""
    ev = AC.block_in_field()
    start = centres([(12, 10), (12, 11), (13, 10)])
    got, want = AC.check(ev, start, 6, 64, max_seg=10, S_max=1)
    assert want["n_claims"] == 3 and (want["status"] == FR.PATH_OVERFLOW).all() and (want["n_sub"] == 0).all()
    t = np.array(want["targets"])
    assert (((t[:, None] - t[None]) ** 2).sum(2)[np.triu_indices(3, 1)] > 36).all() and (got["sub_goals"] == SENTINEL).all()


def test_gpu_spacing_cap():
    ev, start = open_field(30, 34), _side_by_side(4, i=14, j0=15)
    got, want = AC.check(ev, start, 8, 64, max_seg=15)
    assert want["n_claims"] == 4 and (want["n_sub"] >= 3).all()
    got5, want5 = AC.check(ev, start, 8, 64, max_seg=5)          # every path cell a sub-goal
    assert (want5["n_sub"] > want["n_sub"]).all()


def test_gpu_work_and_rows_past_n_sub_are_scratch_and_untouched():
    """``work`` is the call's alone (whatever it holds afterwards, the outputs do not depend on what it held before), and a claim
    with a shorter path than the path call's leaves that call's later rows where they are."""
    ev, start = open_field(30, 34), _side_by_side(4, i=14, j0=15)
    want = AC.expected(ev, start, 8, 64, max_seg=10)
    AC.check(ev, start, 8, 64, max_seg=10, want=want)
    assert any(want["claim_round"][b] > 0 for b in range(4))
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")
    pl = AC.planner(8, 64, max_seg=10)
    out = AC.buffers(4, 30, 34, 64)
    out["work"].view(torch.int32).zero_()                      # another poison: zeros look like sources
    pl.plan(d_ev, d_start, origin=ORIGIN, cell=CELL, out=out)
    torch.cuda.synchronize()
    AC.same(AC.host(out), want, 64)


def _captured(pl, ev, start, out, S_max):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pl.plan(ev, start, origin=ORIGIN, cell=CELL, S_max=S_max, out=out)         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pl.plan(ev, start, origin=ORIGIN, cell=CELL, S_max=S_max, out=out)
    return graph


def test_gpu_graph_replay_and_repeat_give_the_same_bits():
    ev, start = open_field(40, 44), _side_by_side(6, i=8, j0=18)
    eager = [AC.run(ev, start, 7, 64) for _ in range(2)]
    for k in eager[0]:
        assert np.array_equal(bits(eager[0][k]), bits(eager[1][k])), k
    pl = AC.planner(7, 64)
    out = AC.buffers(6, 40, 44, 64)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")      # (alive as long as the graph reads them)
    graph = _captured(pl, d_ev, d_start, out, 64)
    for _ in range(2):
        fresh = AC.buffers(6, 40, 44, 64)
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
    pl = AC.planner(5, 64)
    fresh = pl.plan(d_ev, start, origin=ORIGIN, cell=CELL)      # fresh buffers: rows past n_sub are 0
    torch.cuda.synchronize()
    assert set(fresh) >= {"claim_round", "n_claims", "work", "target", "sub_goals"} and fresh["n_claims"].tolist() == [3]
    assert all((fresh["sub_goals"][b, int(fresh["n_sub"][b]):] == 0).all() for b in range(3))
    assert tuple(pl.plan(d_ev, np.zeros((0, 2)), origin=ORIGIN, cell=CELL)["claim_round"].shape) == (0,)
    with pytest.raises(ValueError):
        pl.plan(torch.zeros((3, 20, 24), dtype=torch.int32, device="cuda"), start, origin=ORIGIN, cell=CELL)      # one map per robot
    with pytest.raises(ValueError):
        pl.plan(d_ev, start, origin=ORIGIN, cell=CELL, may_claim=np.ones(2))
    mapper = lipmpc.OccupancyMapper(20, 24, ORIGIN, CELL, lidar_range=1.0, w_hit=T_OCC, w_miss=T_FREE)
    mapper.evidence.copy_(d_ev)
    got = lipmpc.CoordinatedFrontierPlanner(5).plan(mapper, start)           # thresholds and placement from the mapper
    torch.cuda.synchronize()
    for k in ("claim_round", "target_cell", "n_sub"):
        assert torch.equal(got[k], fresh[k]), k
