"""CPU: the numpy restatement of the coordinated claim (tests/assign_oracle.py) against what the contract of
lipmpc_grid_frontier_assign_batch promises, against passability taken from the evidence instead of the field, and against an
independent greedy over (robot, frontier cell) pairs from one single-source Dijkstra per robot."""
import functools
import heapq

import numpy as np
import pytest

import assign_checks as AC
import assign_oracle as A
import field_oracle as FO
import frontier_oracle as FR
import lidar_oracle as L
import map_oracle as M
from assign_checks import CELL, ORIGIN, T_FREE, T_OCC, centres, open_field


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _consequences(want, r_claim, max_claims):
    """What the header lists under "Hence", on one result."""
    near, t = want["nearest"], np.array(want["targets"]).reshape(-1, 2)
    assert want["n_claims"] == len(want["winners"]) <= max_claims and len(set(want["winners"])) == want["n_claims"]
    assert np.all(np.diff(want["costs"]) >= 0)                                       # the winners' costs do not decrease
    if len(t) > 1:
        assert (((t[:, None] - t[None]) ** 2).sum(2)[np.triu_indices(len(t), 1)] > r_claim * r_claim).all()
    for k, b in enumerate(want["winners"]):
        assert want["claim_round"][b] == k and want["status"][b] in (FR.FOUND, FR.PATH_OVERFLOW)
        assert near["status"][b] in (FR.FOUND, FR.PATH_OVERFLOW) and near["frontier"][0][tuple(t[k])] == 1
        assert want["path_cost"][b] == want["costs"][k] / 5.0
    others = want["claim_round"] == -1
    assert others.sum() == len(others) - want["n_claims"]
    for k in ("status", "n_sub", "target_cell"):                                     # everybody else keeps the path call's outputs
        assert np.array_equal(want[k][others], near[k][others]), k
    assert np.array_equal(_bits(want["path_cost"][others]), _bits(near["path_cost"][others]))
    for b in np.nonzero(others)[0]:
        assert np.array_equal(_bits(want["sub_goals"][b]), _bits(near["sub_goals"][b]))
    if want["n_claims"]:                                                             # the round-0 winner's rows are the path call's
        b = want["winners"][0]
        assert all(want[k][b] == near[k][b] for k in ("status", "n_sub", "target_cell")) and want["path_cost"][b] == near["path_cost"][b]
        assert np.array_equal(_bits(want["sub_goals"][b]), _bits(near["sub_goals"][b]))


@pytest.mark.parametrize("r_claim,max_claims", [(0, 64), (5, 64), (15, 64), (4096, 64), (5, 0), (5, 1), (5, 3)])
def test_consequences_on_the_open_field(r_claim, max_claims):
    ev = open_field(40, 44)
    start = np.concatenate([centres([(8, 18 + k) for k in range(6)]), [[np.nan, 0.0]], centres([(0, 0)])])
    want = AC.expected(ev, start, r_claim, max_claims)
    _consequences(want, r_claim, max_claims)
    assert want["n_claims"] == min(max_claims, 1 if r_claim == 4096 else 7)          # (the robot in the unknown corner snaps in; NaN never)
    assert want["claim_round"][6] == -1
    if max_claims == 0:
        assert (want["claim_round"] == -1).all()
    again = AC.expected(ev, start, r_claim, max_claims)                              # a function of the inputs alone
    for k in ("status", "n_sub", "target_cell", "claim_round"):
        assert np.array_equal(want[k], again[k])
    assert np.array_equal(_bits(want["path_cost"]), _bits(again["path_cost"]))


def test_consequences_with_may_claim_overflow_and_a_cap():
    ev = AC.block_in_field()
    start = centres([(12, 10), (12, 11), (13, 10), (4, 12), (10, 11)])
    may = np.array([1, 0, 1, 1, 1])
    want = AC.expected(ev, start, 6, 64, max_seg=10, S_max=2, may_claim=may)
    _consequences(want, 6, 64)
    assert want["claim_round"][1] == -1 and (want["status"] == FR.PATH_OVERFLOW).any() and (want["status"] == FR.FOUND).any()
    rooms = AC.expected(AC.two_rooms(), centres([(5, 6), (6, 6), (20, 6), (21, 6)]), 12, 64, r=0)
    _consequences(rooms, 12, 64)
    assert rooms["n_claims"] == 3 and rooms["n_sources"][-1] > 0


def test_the_lds_rule_is_the_kernels():
    """4 (2 bitmap_words + 22 + cells) + 256 <= 160 KiB, as include/lipmpc.h states it; the switch lies between the frontier field
    kernel's (three bitmaps) and the grid field kernel's (one)."""
    (W, H), (W1, _) = A.sizes_at_the_lds_switch()
    n = W * H
    assert 4 * (2 * (2 * ((n + 63) // 64) + 2) + 22 + n) + 256 <= 163840 < 4 * (2 * (2 * ((n + H + 63) // 64) + 2) + 22 + n + H) + 256
    assert W1 == W + 1 and not FR.field_fits_lds(n) and FO.field_fits_lds(n + H)         # its own rule, neither of the other two
    assert FR.sizes_at_the_lds_switch()[0][0] < W <= FO.lds_boundary(FO.field_fits_lds)[0][0] // H


# -- passable from the field == unblocked from the evidence ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scanned():
    """A map as the mapper leaves it: three scans of a U-shaped wall (tests/test_frontier_gpu.py's)."""
    Wm, Hm, origin, cell, rng_ = 92, 80, (1.0, 0.0), (0.05, 0.05), 1.5
    occ = np.zeros((Wm, Hm), np.uint8)
    for i0, j0, i1, j1 in ((48, 28, 51, 80), (36, 28, 48, 31), (36, 77, 48, 80)):
        occ[i0:i1, j0:j1] = 1
    table = L.ray_table(360)
    pos = np.array(((1.6, 2.72), (2.6, 1.0), (4.3, 3.2)))
    hits = M.oracle_hits(pos, occ, origin, cell, rng_, table)
    per = M.update(np.zeros((3, Wm, Hm), np.int64), pos, hits, origin, cell, rng_, table)
    return per.sum(0).astype(np.int32), pos, origin, cell


def _both_ways(ev, start, r_claim, r, mu, origin=ORIGIN, cell=CELL):
    near = FR.plan_batch(ev, T_FREE, T_OCC, origin, cell, start, r, mu, None, 64)
    blocked, frontier, _ = FR.masks(ev, T_FREE, T_OCC, r, mu)
    assert np.array_equal(frontier.astype(np.uint8), near["frontier"][0])
    assert not (blocked & (near["field"][0] != FO.INF)).any()                        # finite => unblocked; the converse need not hold
    args = (near["frontier"][0], near["field"][0], origin, cell, start, near, r, r_claim, 64)
    return A.assign(*args), A.assign(*args, passable=~blocked), blocked, near


@pytest.mark.parametrize("r_claim", [0, 6, 20])
def test_passable_from_the_field_gives_the_rounds_of_blocked_from_the_evidence(r_claim):
    ev, pos, origin, cell = _scanned()
    start = np.concatenate([pos, pos + (0.05, 0.0), pos - (0.0, 0.1)])
    a, b, blocked, near = _both_ways(ev, start, r_claim, 2, 2, origin, cell)
    assert a["n_claims"] >= 3
    for k in ("winners", "costs", "targets", "snapped", "n_sources", "n_claims"):
        assert a[k] == b[k], k
    for k in ("status", "n_sub", "target_cell", "claim_round"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a["sub_goals"], b["sub_goals"]))
    # hand-made: two rooms, a known pocket in the unknown, a block to snap round, and a sealed room whose one unblocked cell no
    # frontier can reach: unblocked by the evidence, INF in the field -- the one place where the two masks differ
    ev = AC.two_rooms(34, 14)
    ev[30:33, 5:8] = -T_FREE
    ev[20, 4:9] = T_OCC
    ev[3:8, 3:8] = T_OCC
    ev[4:7, 4:7] = -T_FREE
    start = centres([(9, 9), (10, 9), (18, 6), (22, 6), (31, 6), (19, 6), (5, 5)])
    a, b, blocked, near = _both_ways(ev, start, r_claim, 1, 2)
    assert not blocked[5, 5] and near["field"][0][5, 5] == FO.INF and near["status"][6] == FR.NO_PATH
    assert a["n_claims"] >= 2 and a["claim_round"][6] == -1
    for k in ("winners", "costs", "targets", "snapped", "n_sources"):
        assert a[k] == b[k], k
    for k in ("status", "n_sub", "target_cell", "claim_round"):
        assert np.array_equal(a[k], b[k]), k


# -- an independent greedy -----------------------------------------------------------------------------------------------------
def _from(blocked, s):
    """{cell: least cost from s} over the unblocked cells (single source; the move rules are symmetric)."""
    dist, heap = {s: 0}, [(0,) + s]
    while heap:
        d, i, j = heapq.heappop(heap)
        if d > dist[(i, j)]:
            continue
        for a, b, c in FO.moves_from(blocked, i, j):
            if d + c < dist.get((a, b), 1 << 62):
                dist[(a, b)] = d + c
                heapq.heappush(heap, (d + c, a, b))
    return dist


@pytest.mark.parametrize("seed", range(8))
def test_winners_equal_the_global_greedy_over_robot_cell_pairs(seed):
    """On small random maps (r_inflate 0; robots on passable cells, so no snap): round by round the pair (robot, frontier cell
    left) of the least cost, ties to the lower robot, is the oracle's winner at the oracle's cost, and the oracle's target is
    one of the cells that robot reaches at that cost."""
    rng = np.random.default_rng(seed)
    W, H = int(rng.integers(9, 15)), int(rng.integers(9, 15))
    ev = np.full((W, H), -T_FREE, np.int32)
    ev[rng.random((W, H)) < 0.12] = 0
    ev[rng.random((W, H)) < 0.08] = T_OCC
    r_claim = int(rng.integers(0, 5))
    blocked, frontier, _ = FR.masks(ev, T_FREE, T_OCC, 0, 1)
    free = [c for c in zip(*np.nonzero(~blocked))]
    cells = [free[i] for i in rng.choice(len(free), 6, replace=False)]
    start = centres(cells)
    want = AC.expected(ev, start, r_claim, 64, r=0, mu=1)
    dist = [_from(blocked, (int(c[0]), int(c[1]))) for c in cells]
    left = [b for b in range(6) if want["nearest"]["status"][b] == FR.FOUND]
    sources = {(int(i), int(j)) for i, j in zip(*np.nonzero(frontier))}
    for k in range(want["n_claims"] + 1):
        pairs = [(dist[b][c], b) for b in left for c in sources if c in dist[b]]
        if k == want["n_claims"]:
            assert not pairs or not left                                             # the rounds ended for a reason
            break
        cost, b = min(pairs)
        t = tuple(want["targets"][k])
        assert (b, cost) == (want["winners"][k], want["costs"][k]) and t in sources and dist[b][t] == cost
        sources = {c for c in sources if (c[0] - t[0]) ** 2 + (c[1] - t[1]) ** 2 > r_claim * r_claim}
        left.remove(b)
    assert want["n_claims"] >= 1
