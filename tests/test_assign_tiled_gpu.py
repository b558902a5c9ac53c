"""GPU: the tiled coordinated claim (lipmpc_grid_frontier_assign_tiled_batch, through TiledCoordinatedFrontierPlanner) against
tests/assign_oracle.py: claim_round, n_claims, the int32 n_sub / status / target_cell and the doubles of path_cost, target and the
WHOLE sub-goal buffer, bit for bit, on maps of several tiles.  Every shape comes from the tile sides TW x TH; every buffer starts
poisoned."""
import numpy as np
import pytest

import assign_checks as AC
import field_tiled_cases as T
import frontier_oracle as FR
from assign_checks import CELL, ORIGIN, SENTINEL, T_FREE, T_OCC, bits, centres, open_field

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

TW, TH = T.TW, T.TH
POISON = -0x01010102                                          # int32 of the bytes FE FE FE FE: not a status, a count or a flag
BIG_W, BIG_H = 2 * TW + 5, 2 * TH + 3                         # 3 x 3 tiles, no side a multiple of the tile's


def _planner(r_claim, max_claims, r=2, mu=2, max_seg=None, rounds=None):
    return lipmpc.TiledCoordinatedFrontierPlanner(r_claim, max_claims, r_inflate=r, min_unknown=mu, t_free=T_FREE, t_occ=T_OCC, max_seg=max_seg,
                                                  rounds=rounds)


def _buffers(B, W, H, S_max):
    table = lipmpc.planner.tiled_assign_outputs(B, W, H, S_max)
    out = {k: torch.empty(shape, dtype=dt, device="cuda") for k, (dt, shape, _) in table.items()}
    out["settled"] = torch.empty((1,), dtype=torch.int32, device="cuda")
    _poison(out)
    return out


def _poison(out):
    for k in ("sub_goals", "path_cost", "target"):
        out[k].fill_(SENTINEL)
    for k in ("n_sub", "status", "target_cell", "claim_round", "n_claims", "n_frontier"):
        out[k].fill_(AC.POISON_I32)
    for k in ("settled", "claims_settled"):
        out[k].fill_(POISON)
    out["frontier"].fill_(9)
    out["field"].view(torch.int32).fill_(AC.POISON_WORK)


def _run(ev, start, r_claim, max_claims, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, rounds=None, pl=None, origin=ORIGIN, cell=CELL):
    ev, start = np.ascontiguousarray(ev, np.int32), np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, 2))
    W, H = ev.shape
    out = _buffers(len(start), W, H, S_max)
    pl = pl or _planner(r_claim, max_claims, r, mu, max_seg, rounds)
    may = None if may_claim is None else torch.as_tensor(np.asarray(may_claim), device="cuda")
    got = pl.plan(torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda"), origin=origin, cell=cell, S_max=S_max, out=out,
                  may_claim=may)
    torch.cuda.synchronize()
    assert got is out and pl.last is out and "work" not in out
    return AC.host(out)


def _check(ev, start, r_claim, max_claims, r=2, mu=2, max_seg=None, S_max=64, may_claim=None, want=None, origin=ORIGIN, cell=CELL):
    if want is None:
        want = AC.expected(ev, start, r_claim, max_claims, r, mu, max_seg, S_max, may_claim, origin=origin, cell=cell)
    got = _run(ev, start, r_claim, max_claims, r, mu, max_seg, S_max, may_claim, origin=origin, cell=cell)
    assert got["settled"].tolist() == [1] and got["claims_settled"].tolist() == [1]
    AC.same(got, want, S_max)
    return got, want


def _side_by_side(n, i, j0):
    return centres([(i, j0 + k) for k in range(n)])


# -- 1. the existing scenes on several tiles ----------------------------------------------------------------------------------
@pytest.mark.parametrize("r_claim", [0, 15, 4096])
def test_one_ring_of_an_open_field_over_nine_tiles(r_claim):
    """Six robots side by side at the corner where four tiles meet: r_claim = 0 takes one cell per claim, 15 spreads the claims with
    discs that cross tile borders, 4096 -- larger than the map -- leaves one claim and five followers."""
    ev, start = open_field(BIG_W, BIG_H), _side_by_side(6, TW - 1, TH - 3)
    got, want = _check(ev, start, r_claim, 64)
    t = np.array(want["targets"])
    assert want["n_claims"] == (1 if r_claim == 4096 else 6) and np.all(np.diff(want["costs"]) >= 0)
    d2 = ((t[:, None] - t[None]) ** 2).sum(2)[np.triu_indices(len(t), 1)]
    assert (d2 > r_claim * r_claim).all()
    if r_claim == 4096:
        assert sorted(want["claim_round"].tolist()) == [-1] * 5 + [0] and np.array_equal(want["target_cell"], want["nearest"]["target_cell"])


def test_two_rooms_one_used_up():
    """Two rooms that no passable cell connects, each over several tiles: a robot whose room's frontier is used up is no candidate
    although sources are left in the other room."""
    W, H = 2 * TW + 6, TH + 6
    ev = AC.two_rooms(W, H)
    start = centres([(5, 6), (6, 6), (20, 6), (21, 6), (W - 5, H - 5)])
    got, want = _check(ev, start, 64, 64, r=0)                 # robot 0's disc takes its whole room's ring and leaves some of the other's
    assert want["n_claims"] == 3 and want["claim_round"].tolist() == [1, -1, -1, 2, 0] and want["n_sources"][-1] > 0
    got, want = _check(ev, start, 12, 64, r=0)
    assert want["n_claims"] >= 4


def test_start_in_the_inflation_band_snaps_in_the_rounds_field():
    at = (TW, TH)                                              # the solid cell where four tiles meet: its band lies in all four
    ev = AC.block_in_field(2 * TW + 4, 2 * TH + 4, at)
    start = centres([(TW - 6, TH + 2), (TW, TH + 1), (TW + 1, TH - 1)])
    got, want = _check(ev, start, 12, 64)
    assert want["n_claims"] == 3 and (want["nearest"]["field"][0][TW, TH + 1] == FR.INF)
    assert any(s != tuple(int(v) for v in np.floor((start[b] - ORIGIN) / CELL)) for b, s in zip(want["winners"], want["snapped"]))


# -- 2. discs across borders and over the grid's edge -------------------------------------------------------------------------------
@pytest.mark.parametrize("r_claim", [3, 6])
def test_discs_clipped_at_the_grid_and_cut_by_tile_borders(r_claim):
    """A known field with single unknown cells one step from every corner and edge and on both sides of the tile borders (min_unknown
    1: their neighbours are the frontier): discs reach over the ends of the grid and over the borders."""
    W, H = TW + 6, TH + 6
    ev = np.full((W, H), -T_FREE, np.int32)
    holes = ((1, 1), (1, H - 2), (W - 2, 1), (W - 2, H - 2), (1, TH), (W - 2, TH - 1), (TW, 1), (TW - 1, H - 2), (TW, TH))
    for c in holes:
        ev[c] = 0
    start = centres([(TW // 2 + k // 3, TH // 2 + k % 3) for k in range(9)])
    got, want = _check(ev, start, r_claim, 64, r=0, mu=1)
    t = np.array(want["targets"])
    assert want["n_claims"] == 9
    assert ((t[:, 0] < r_claim) | (t[:, 0] > W - 1 - r_claim) | (t[:, 1] < r_claim) | (t[:, 1] > H - 1 - r_claim)).sum() >= 6


# -- 3. the allowance, followers, the mask, an overflow winner, many robots ---------------------------------------------------------
@pytest.mark.parametrize("max_claims", [0, 1])
def test_no_claim_and_one_claim(max_claims):
    ev, start = open_field(BIG_W, BIG_H), _side_by_side(3, TW - 1, TH - 1)
    got, want = _check(ev, start, 5, max_claims)
    near = want["nearest"]
    assert want["n_claims"] == max_claims and sorted(want["claim_round"].tolist()) == [-1, -1, -1 + max_claims]
    for k in ("status", "n_sub", "target_cell"):
        assert np.array_equal(got[k], near[k]), k


def test_followers_and_a_mask():
    ev, start = open_field(BIG_W, BIG_H), _side_by_side(5, TW + 1, TH - 2)
    got, want = _check(ev, start, 3, 2)                        # more robots than claims: three followers
    assert want["n_claims"] == 2 and (want["claim_round"] == -1).sum() == 3
    may = np.array([0, 1, 0, 1, 1], np.int8)
    got, want = _check(ev, start, 3, 64, may_claim=may)
    assert want["n_claims"] == 3 and (want["claim_round"][may == 0] == -1).all() and (want["claim_round"][may == 1] >= 0).all()
    got, want = _check(ev, start, 3, 64, may_claim=np.zeros(5, bool))
    assert want["n_claims"] == 0


def test_overflow_winner_still_claims():
    ev = AC.block_in_field(2 * TW + 4, 2 * TH + 4, (TW, TH))
    start = centres([(TW + 2, TH), (TW + 2, TH + 1), (TW + 3, TH)])
    got, want = _check(ev, start, 6, 64, max_seg=10, S_max=1)
    assert want["n_claims"] == 3 and (want["status"] == FR.PATH_OVERFLOW).all() and (want["n_sub"] == 0).all()
    assert (got["sub_goals"] == SENTINEL).all()


def test_more_robots_than_a_workgroup_of_the_pick():
    """300 robots: the pick's minimum comes from several workgroups.  Robot B - 1 is the only one near the far side."""
    B = 300
    ev = open_field(BIG_W, BIG_H)
    rng = np.random.default_rng(B)
    start = centres([(6, 9)])[0] + rng.uniform(-0.14, 0.14, (B, 2)) * np.array(CELL)
    start[B - 1] = centres([(BIG_W - 6, BIG_H - 9)])[0]
    got, want = _check(ev, start, 10, 4)
    assert want["n_claims"] == 4 and want["claim_round"][B - 1] >= 0 and (want["claim_round"] == -1).sum() == B - 4


# -- 4. the plain planner's bits ----------------------------------------------------------------------------------------------------
def test_equal_to_the_one_workgroup_planner():
    ev, start = open_field(BIG_W, BIG_H), _side_by_side(6, TW - 1, TH - 3)
    plain = AC.run(ev, start, 9, 64, max_seg=25)
    mine = _run(ev, start, 9, 64, max_seg=25)
    assert mine["claims_settled"].tolist() == [1] and plain["n_claims"].tolist() == [6]
    for k in plain:
        assert np.array_equal(bits(plain[k]), bits(mine[k])), k


# -- 5. / 6. budgets -------------------------------------------------------------------------------------------------------------------
def _claims_alone(pl, ev, start, out, S_max=64):
    """The settled nearest-frontier plan (rounds=None) now; returns claim(budget): the claim call alone with a per-claim budget."""
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")
    pl.rounds = None
    lipmpc.FrontierPlanner.plan(pl, d_ev, d_start, ORIGIN, CELL, S_max, out)
    return lambda budget: _claim(pl, d_start, ev.shape, out, budget, S_max)


def _claim(pl, d_start, shape, out, budget, S_max):
    org, cs, org_c, cell_c = pl._placement(ORIGIN, CELL)
    pl.rounds = budget
    pl._claims(d_start.shape[0], shape[0], shape[1], d_start, None, org_c, cell_c, S_max, out)
    pl._target(out, org, cs, shape[1])
    torch.cuda.synchronize()
    return AC.host(out)


def test_a_budget_too_small_gives_a_prefix_and_a_repeat_finishes():
    """Robots in one corner of a ring over nine tiles, a large claim radius: every claim moves the nearest source further away, so
    later rounds need more tiled rounds than earlier ones.  With claims_settled == 0 the claims made are the rule's first n_claims
    rounds -- the oracle with max_claims = n_claims -- and the same call again with a budget that suffices reproduces them and goes
    on to the oracle's full answer."""
    ev, start = open_field(BIG_W, BIG_H), _side_by_side(4, 5, 5)
    full = AC.expected(ev, start, 40, 64)
    assert full["n_claims"] == 4
    pl = _planner(40, 64)
    out = _buffers(4, BIG_W, BIG_H, 64)
    claim = _claims_alone(pl, ev, start, out)
    seen = []
    for budget in range(1, 7):                                 # every call on the SAME buffers, as the last one left them
        got = claim(budget)
        n = int(got["n_claims"][0])
        seen.append((budget, n, int(got["claims_settled"][0])))
        if got["claims_settled"][0] == 0:
            assert n < full["n_claims"]
            want = AC.expected(ev, start, 40, n)               # exactly the first n rounds; everyone else keeps the nearest plan
            AC.same(got, want, 64)
            assert sorted(want["claim_round"].tolist()) == [-1] * (4 - n) + list(range(n))
        else:
            AC.same(got, full, 64)
    print("budget, n_claims, claims_settled:", seen)
    assert seen[0][2] == 0                                     # one round cannot settle a field that crosses a tile border
    assert [n for _, n, _ in seen] == sorted(n for _, n, _ in seen)
    # a stop in mid-sequence: some budget settles the first rounds' fields and not a later one's.  The call after it started from
    # that state -- winners' rows and statuses overwritten, n_claims and claim_round of the partial run in the buffers -- and made
    # the same rounds again before it went on (held to the oracle above).
    partial = [k for k, (_, n, ok) in enumerate(seen) if ok == 0 and 0 < n < full["n_claims"]]
    assert partial and seen[partial[-1] + 1][1] > seen[partial[-1]][1], seen
    assert seen[-1][1:] == (full["n_claims"], 1), seen
    # the same on fresh buffers, without the smaller budgets before it: the partial call, the same call again (the same rounds, the
    # same bits), then straight to a budget that settles
    at, n_at = seen[partial[0]][0], seen[partial[0]][1]
    out = _buffers(4, BIG_W, BIG_H, 64)
    claim = _claims_alone(pl, ev, start, out)
    for _ in range(2):
        got = claim(at)
        assert (int(got["n_claims"][0]), int(got["claims_settled"][0])) == (n_at, 0)
        AC.same(got, AC.expected(ev, start, 40, n_at), 64)
    AC.same(claim(seen[-1][0]), full, 64)
    # a monotone path on the open rectangle changes tile at most (tiles along W - 1) + (tiles along H - 1) times: this budget settles
    got = claim(-(-BIG_W // TW) - (-BIG_H // TH))
    assert got["claims_settled"].tolist() == [1]
    AC.same(got, full, 64)
    # and rounds=None doubles the budget by itself
    got = _run(ev, start, 40, 64)
    AC.same(got, full, 64)


def test_no_robots():
    """B = 0: no call is made, and the dict still has every key the class promises."""
    got = _planner(5, 8).plan(torch.as_tensor(open_field(BIG_W, BIG_H), device="cuda"), np.zeros((0, 2)), origin=ORIGIN, cell=CELL)
    assert tuple(got["claim_round"].shape) == (0,) and tuple(got["settled"].shape) == (1,) and tuple(got["claims_settled"].shape) == (1,)
    assert got["claims_settled"].dtype == torch.int32 and "work" not in got


def test_an_unsettled_input_field_gives_no_claims():
    ev, start = open_field(BIG_W, BIG_H), _side_by_side(3, TW - 1, TH - 1)
    want = AC.expected(ev, start, 5, 0)                        # the nearest-frontier plan with no claim
    pl = _planner(5, 64)
    out = _buffers(3, BIG_W, BIG_H, 64)
    claim = _claims_alone(pl, ev, start, out)
    out["settled"].zero_()
    got = claim(64)
    assert got["n_claims"].tolist() == [0] and got["claims_settled"].tolist() == [0] and (got["claim_round"] == -1).all()
    AC.same(got, want, 64)
    # through the class: rounds=1 settles neither field; every robot is parked, nobody claims
    got = _run(ev, start, 5, 64, rounds=1)
    assert got["settled"].tolist() == [0] and got["claims_settled"].tolist() == [0] and got["n_claims"].tolist() == [0]
    assert got["status"].tolist() == [lipmpc.RRT_FIELD_UNSETTLED] * 3 and (got["claim_round"] == -1).all() and (got["sub_goals"] == SENTINEL).all()


# -- 7. graph replay -----------------------------------------------------------------------------------------------------------------
def test_graph_replay_with_fixed_rounds():
    """The open rectangle: every least-cost path is monotone, so tiles along W + tiles along H rounds settle the frontier field and
    every claim round's field (the round guarantee)."""
    ev, start = open_field(BIG_W, BIG_H), _side_by_side(6, TW - 1, TH - 3)
    want = AC.expected(ev, start, 15, 8)
    rounds = -(-BIG_W // TW) - (-BIG_H // TH)
    pl = _planner(15, 8, rounds=rounds)
    out = _buffers(6, BIG_W, BIG_H, 64)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")
    plan = lambda: pl.plan(d_ev, d_start, origin=ORIGIN, cell=CELL, S_max=64, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan()                                                 # warm-up outside the capture: the workspaces grow here
    torch.cuda.current_stream().wait_stream(side)
    works = len(pl._works), len(pl._claim_works)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan()
    assert (len(pl._works), len(pl._claim_works)) == works
    for _ in range(2):
        _poison(out)
        graph.replay()
        torch.cuda.synchronize()
        got = AC.host(out)
        assert got["settled"].tolist() == [1] and got["claims_settled"].tolist() == [1]
        AC.same(got, want, 64)


# -- 8. beyond the old cap -------------------------------------------------------------------------------------------------------------
def test_363_x_362_with_three_robots():
    c, near = T.case("363x362"), T.oracle("363x362", "frontier")
    found = np.nonzero(near["status"] == FR.FOUND)[0][:3]
    assert len(found) == 3
    start = c["start"][found]
    want = AC.expected(c["ev"], start, 1, 2, c["r"], c["mu"], c["max_seg"], c["S_max"], origin=T.ORIGIN, cell=T.CELL)
    assert want["n_claims"] == 2
    with pytest.raises(RuntimeError) as e:
        AC.planner(1, 2, r=c["r"], mu=c["mu"], max_seg=c["max_seg"]).plan(torch.as_tensor(c["ev"], device="cuda"),
                                                                        torch.as_tensor(start, device="cuda"), origin=T.ORIGIN, cell=T.CELL)
    assert e.value.code == -2
    got = _run(c["ev"], start, 1, 2, r=c["r"], mu=c["mu"], max_seg=c["max_seg"], S_max=c["S_max"], origin=T.ORIGIN, cell=T.CELL)
    assert got["settled"].tolist() == [1] and got["claims_settled"].tolist() == [1]
    AC.same(got, want, c["S_max"])
