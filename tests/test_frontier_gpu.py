"""GPU: the frontier explorer (lipmpc_grid_frontier_field_batch, lipmpc_grid_frontier_path_batch) against tests/frontier_oracle.py:
the uint8 frontier, the int32 n_frontier / n_sub / status / target_cell, the uint32 field and the doubles of sub_goals[:n_sub],
path_cost and target, bit for bit, on every map."""
import functools

import numpy as np
import pytest

import field_oracle as FO
import frontier_oracle as FR
import lidar_oracle as L
import map_oracle as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

from grid_checks import CELL, ORIGIN, SENTINEL, T_FREE, T_OCC, bits as _bits, check_frontier as _check, frontier_buffers as _buffers, \
    frontier_planner as _planner, host as _host, run_frontier as _run  # noqa: E402  (shared with the other grid planner tests)

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _points(rng, W, H, n, origin=ORIGIN, cell=CELL, margin=0.0):
    """n world points over the grid's rectangle (+ a margin, in cells, that puts some outside)."""
    return np.stack([origin[0] + rng.uniform(-margin, W + margin, n) * cell[0], origin[1] + rng.uniform(-margin, H + margin, n) * cell[1]], 1)


def _centres(cells, origin=ORIGIN, cell=CELL):
    return [FO.centre(c, origin, cell) for c in cells]


def _speckled(rng, W, H, p_free=0.6, p_solid=0.1):
    """Evidence of all three classes cell by cell, the values spread over both sides of each threshold."""
    ev = rng.integers(-T_FREE + 1, T_OCC, (W, H)).astype(np.int32)
    free = rng.random((W, H)) < p_free
    ev[free] = -T_FREE - rng.integers(0, 4, int(free.sum()))
    solid = rng.random((W, H)) < p_solid
    ev[solid] = T_OCC + rng.integers(0, 4, int(solid.sum()))
    return ev


def test_gpu_smallest_grid_all_unknown():
    got, _ = _check(np.zeros((2, 2), np.int32), _centres(((0, 0), (1, 1))) + [(np.nan, 0.0)], r=0, mu=1)
    assert got["n_frontier"].tolist() == [0] and (got["field"] == FO.INF).all() and not got["frontier"].any()
    assert got["status"].tolist() == [FR.NO_PATH, FR.NO_PATH, FR.OUTSIDE_GRID] and (got["target_cell"] == -1).all()


HAND_MADE = np.array([[-1, -1, -1, 0, 0, 3, -1],              # 5 x 7: a free region, an unknown pocket, a wall, a free cell behind it
                      [-1, -2, -1, 0, 2, 3, -1],
                      [-1, -1, -1, -1, -1, 3, 0],
                      [3, -1, -5, -1, 0, 0, 0],
                      [3, 3, -1, -1, -1, 1, -3]], np.int32)


@pytest.mark.parametrize("r", [0, 2, 16])
@pytest.mark.parametrize("mu", [1, 2, 8])
def test_gpu_hand_made(r, mu):
    starts = _centres([(i, j) for i in range(5) for j in range(7)]) + [(ORIGIN[0] - 0.01, 0.3), (0.0, np.inf)]
    got, want = _check(HAND_MADE, starts, r=r, mu=mu)
    if (r, mu) == (0, 1):
        assert got["n_frontier"][0] >= 6 and (want["status"] == FR.FOUND).sum() >= 15 and (want["status"] == FR.START_OCCUPIED).sum() == 6
    if r == 16 or mu == 8:
        assert got["n_frontier"][0] == 0 and set(want["status"].tolist()) == {FR.NO_PATH, FR.START_OCCUPIED, FR.OUTSIDE_GRID}


def test_gpu_thresholds_and_the_ends_of_int32():
    for t in ((1, 3), (2, 1), (1 << 30, 1 << 30), (7, 1 << 30)):
        vals = [-t[0] - 1, -t[0], -t[0] + 1, t[1] - 1, t[1], I32_MIN, I32_MAX, 0, -1, 1]
        ev = np.array([vals, vals[::-1], vals], np.int32)
        _check(ev, _centres([(1, j) for j in range(len(vals))]), r=0, mu=1, t=t)
        _check(ev, _centres([(0, 0), (2, 5)]), r=1, mu=2, t=t)


@pytest.mark.parametrize("W,H", [(5, 13), (4, 33), (3, 64), (2, 65), (7, 31)])
def test_gpu_ballot_words_and_row_ends(W, H):
    """65 cells cross a ballot word; with H = 33 and H = 64 a row ends one bit after / exactly at a word boundary: an unknown cell
    at the end of one row and the start of the next is a neighbour of neither's opposite end."""
    rng = np.random.default_rng(W * 100 + H)
    for k in range(3):
        ev = _speckled(rng, W, H, p_free=0.7, p_solid=0.05)
        ev[:, 0] = np.where(np.arange(W) % 2 == k % 2, 0, -1)                      # unknown / free alternating at both row ends
        ev[:, H - 1] = np.where(np.arange(W) % 2 == k % 2, -1, 0)
        got, want = _check(ev, _points(rng, W, H, 12, margin=0.3), r=k, mu=1 + k)
    ev = np.full((W, H), -1, np.int32)                                              # one unknown cell at a row's end: its 3 (or 5) neighbours only
    ev[1, H - 1] = 0
    got, _ = _check(ev, _centres([(0, 0)]), r=0, mu=1)
    assert got["n_frontier"][0] == (5 if W > 2 else 3) and not got["frontier"][0, :, 0].any()
    ev[1, H - 1], ev[1, 0] = -1, 0
    got, _ = _check(ev, _centres([(0, 0)]), r=0, mu=1)
    assert got["n_frontier"][0] == (5 if W > 2 else 3) and not got["frontier"][0, :, H - 1].any()


# -- a map as the mapper leaves it ---------------------------------------------------------------------------------------
MAP_W, MAP_H, MAP_ORIGIN, MAP_CELL, MAP_RANGE = 92, 80, (1.0, 0.0), (0.05, 0.05), 1.5
SCAN_AT = ((1.6, 2.72), (2.6, 1.0), (4.3, 3.2))


@functools.lru_cache(maxsize=None)
def _scanned_maps():
    """(shared [W,H], per robot [3,W,H]) int32: three scans of a U-shaped wall through tests/map_oracle.py."""
    occ = np.zeros((MAP_W, MAP_H), np.uint8)
    for i0, j0, i1, j1 in ((48, 28, 51, 80), (36, 28, 48, 31), (36, 77, 48, 80)):
        occ[i0:i1, j0:j1] = 1
    table = L.ray_table(360)
    pos = np.array(SCAN_AT)
    hits = M.oracle_hits(pos, occ, MAP_ORIGIN, MAP_CELL, MAP_RANGE, table)
    per = M.update(np.zeros((3, MAP_W, MAP_H), np.int64), pos, hits, MAP_ORIGIN, MAP_CELL, MAP_RANGE, table)
    return per.sum(0).astype(np.int32), per.astype(np.int32)


@pytest.mark.parametrize("r,mu,max_seg", [(2, 2, None), (0, 1, 5), (3, 3, 35)])
def test_gpu_scanned_map_shared(r, mu, max_seg):
    shared, _ = _scanned_maps()
    rng = np.random.default_rng(3)
    starts = np.concatenate([np.array(SCAN_AT), _points(rng, MAP_W, MAP_H, 21, MAP_ORIGIN, MAP_CELL, margin=1.0)])
    got, want = _check(shared, starts, r=r, mu=mu, max_seg=max_seg, S_max=96, origin=MAP_ORIGIN, cell=MAP_CELL)
    assert got["n_frontier"][0] > 20 and (want["status"][:3] == FR.FOUND).all() and (want["status"] == FR.NO_PATH).any()
    if max_seg == 5:                                           # every path cell is a sub-goal
        assert all(want["n_sub"][b] == max(len(want["cells"][b]) - 1, 1) for b in np.nonzero(want["status"] == FR.FOUND)[0])


def test_gpu_scanned_maps_one_per_robot():
    _, per = _scanned_maps()
    got, want = _check(per, np.array(SCAN_AT), origin=MAP_ORIGIN, cell=MAP_CELL)        # F = B = 3: robot b on its own map
    assert (want["status"] == FR.FOUND).all() and len(set(want["n_frontier"].tolist())) == 3
    got, want = _check(per, np.array(SCAN_AT)[::-1], origin=MAP_ORIGIN, cell=MAP_CELL)  # each on a map it never saw
    assert (want["status"] != FR.FOUND).any()


def _rooms(W, H):
    """A large known area with walls, an unknown band along the far edge and an unknown block in the middle."""
    ev = np.full((W, H), -2, np.int32)
    ev[W // 4, : H - 9] = ev[W // 2, 7:] = 5
    ev[3 * W // 4, : H // 2] = ev[3 * W // 4, H // 2 + 9:] = 3
    ev[W - 6:, :] = 0
    ev[W // 3:W // 3 + 8, H // 2:H // 2 + 8] = 1
    return ev


def test_gpu_each_side_of_the_lds_switch():
    """The largest map whose field the frontier kernel keeps in LDS and the first it relaxes in the output buffer, by the oracle
    module's restatement of the kernel's own rule (not the grid field planner's 199 x 199 / 200 x 199)."""
    for W, H in FR.sizes_at_the_lds_switch():
        rng = np.random.default_rng(5)
        starts = np.concatenate([_centres([(1, 1)]), _points(rng, W, H, 7)])
        got, want = _check(_rooms(W, H), starts, r=2, mu=2, S_max=200)
        assert want["status"][0] == FR.FOUND and want["path_cost"][0] > 40 and got["n_frontier"][0] > 100


@functools.lru_cache(maxsize=None)
def _fleet_case():
    """48 x 36, r_inflate = 2: a solid block with a one-cell free pocket (inflated, nothing finite around it), a closed room
    (known, cut off from every frontier), an unknown block and an unknown band; 130 starts: special ones, then random ones over
    the grid and a margin around it."""
    ev = np.full((48, 36), -1, np.int32)
    ev[4:13, 4:13] = 3
    ev[8, 8] = -1                                              # the pocket
    ev[20:31, 20] = ev[20:31, 30] = ev[20, 20:31] = ev[30, 20:31] = 4          # the room: walled in
    ev[38, 6:] = 3
    ev[44:, :] = 0                                             # the unknown band
    ev[14:18, 24:30] = 0                                       # the unknown block
    rng = np.random.default_rng(9)
    special = _centres(((5, 5), (8, 8), (25, 25), (3, 8), (43, 20), (15, 26), (47, 10), (24, 26), (13, 26)))
    special += [(float("nan"), 0.3), (ORIGIN[0] - 0.001, 0.3), (ORIGIN[0] + 48 * CELL[0], 0.3)]
    return ev, np.concatenate([special, _points(rng, 48, 36, 118, margin=1.5)])


def test_gpu_one_field_many_robots():
    ev, start = _fleet_case()
    assert len(start) == 130                                   # two full blocks of lanes and a tail
    got, want = _check(ev, start, r=2, mu=2)
    st = want["status"]
    # solid; pocket; walled in; inflated (snaps); ON a frontier cell; unknown next to the frontier (snaps); deep in the unknown; walled in; on a frontier cell
    assert st[:12].tolist() == [FR.START_OCCUPIED, FR.NO_PATH, FR.NO_PATH, FR.FOUND, FR.FOUND, FR.FOUND, FR.NO_PATH, FR.NO_PATH, FR.FOUND] + \
        [FR.OUTSIDE_GRID] * 3
    H = ev.shape[1]
    for b in (4, 8):                                           # a start on a frontier cell: one sub-goal, its own centre
        assert want["n_sub"][b] == 1 and got["target_cell"][b] == FO.cell_of(start[b], ORIGIN, CELL, 48, 36)[0] * H + FO.cell_of(start[b], ORIGIN, CELL, 48, 36)[1]
        assert np.array_equal(_bits(got["sub_goals"][b, 0]), _bits(start[b])) and got["path_cost"][b] == 0.0
    assert want["cells"][3][0] != (3, 8) and want["cells"][5][0] != (15, 26)
    print("statuses", np.bincount(st, minlength=8).tolist(), "n_frontier", got["n_frontier"].tolist())
    assert (st == FR.FOUND).sum() >= 50 and (st == FR.OUTSIDE_GRID).sum() >= 8 and (st == FR.START_OCCUPIED).sum() >= 4
    found = st == FR.FOUND
    assert (got["frontier"][0].reshape(-1)[got["target_cell"][found]] == 1).all()
    assert np.array_equal(_bits(got["target"][found]), _bits(np.array([got["sub_goals"][b, got["n_sub"][b] - 1] for b in np.nonzero(found)[0]])))


def test_gpu_one_map_per_robot_many_robots():
    rng = np.random.default_rng(21)
    ev = np.stack([_speckled(rng, 19, 23, p_free=0.75, p_solid=0.04) for _ in range(70)])     # F = B = 70: a block and a tail
    _check(ev, _points(rng, 19, 23, 70, margin=0.5), r=1, mu=2)


@pytest.mark.parametrize("max_seg", [5, None])
def test_gpu_spacing_cap_and_overflow(max_seg):
    ev, start = _fleet_case()
    got, want = _check(ev, start[:40], r=1, mu=2, max_seg=max_seg, S_max=80)
    assert (want["status"] == FR.FOUND).sum() >= 15
    b = int(np.argmax(np.where(want["status"] == FR.FOUND, want["n_sub"], 0)))
    n = int(want["n_sub"][b])
    assert n >= 2
    tight, tw = _check(ev, start[b:b + 1], r=1, mu=2, max_seg=max_seg, S_max=n - 1)
    assert tight["status"].tolist() == [FR.PATH_OVERFLOW] and tight["n_sub"].tolist() == [0] and (tight["sub_goals"] == SENTINEL).all()
    assert tight["target_cell"][0] == want["target_cell"][b] and tight["path_cost"][0] == want["path_cost"][b]
    assert _check(ev, start[b:b + 1], r=1, mu=2, max_seg=max_seg, S_max=n)[0]["status"][0] == FR.FOUND       # exactly enough


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


@pytest.mark.parametrize("case", ["fleet", "global"])
def test_gpu_graph_replay_and_repeat_give_the_same_bits(case):
    """Field + path captured in one graph and replayed twice equal the eager call; two eager calls equal each other."""
    if case == "fleet":
        ev, start = _fleet_case()
    else:
        W, H = FR.sizes_at_the_lds_switch()[1]
        ev, start = _rooms(W, H), _points(np.random.default_rng(6), W, H, 16)
    W, H = ev.shape
    eager = [_run(ev, start) for _ in range(2)]
    for k in eager[0]:
        assert np.array_equal(_bits(eager[0][k]), _bits(eager[1][k])), k
    pl = _planner(2, 2, None)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")
    out = _buffers(len(start), 1, W, H, 64)
    graph = _captured(pl, d_ev, d_start, out, 64)
    for _ in range(2):
        for k in ("n_sub", "status", "n_frontier", "target_cell"):
            out[k].fill_(-1)
        for k in ("sub_goals", "path_cost", "target"):
            out[k].fill_(SENTINEL)
        out["frontier"].fill_(7)
        out["field"].view(torch.int32).fill_(12345)
        graph.replay()
        torch.cuda.synchronize()
        got = _host(out)
        for k in eager[0]:
            assert np.array_equal(_bits(got[k]), _bits(eager[0][k])), k


def test_gpu_field_alone_mapper_defaults_and_argument_checks():
    ev, start = _fleet_case()
    mapper = lipmpc.OccupancyMapper(48, 36, ORIGIN, CELL, lidar_range=1.0, w_hit=T_OCC, w_miss=T_FREE)
    mapper.evidence.copy_(torch.as_tensor(ev))
    pl = lipmpc.FrontierPlanner()                              # r_inflate 2, min_unknown 2, thresholds from the mapper
    f = pl.field(mapper)
    torch.cuda.synchronize()
    want = FR.field(ev, T_FREE, T_OCC, 2, 2)
    assert np.array_equal(f["field"].view(torch.int32).cpu().numpy().view(np.uint32)[0], want[0])
    assert np.array_equal(f["frontier"].cpu().numpy()[0], want[1]) and f["n_frontier"].tolist() == [want[2]]
    assert tuple(f["field"].shape) == (1, 48, 36) and f["field"].dtype == torch.uint32 and f["frontier"].dtype == torch.uint8
    fresh = pl.plan(mapper, start[3:4])                        # placement from the mapper; rows past n_sub are 0 in a fresh out
    n = int(fresh["n_sub"][0])
    assert n >= 1 and (fresh["sub_goals"][0, n:] == 0).all()
    assert set(fresh) >= {"sub_goals", "n_sub", "status", "path_cost", "target", "target_cell", "n_frontier", "field", "frontier"}
    assert tuple(pl.plan(mapper, np.zeros((0, 2)))["sub_goals"].shape) == (0, 64, 2)
    with pytest.raises(ValueError):
        pl.plan(mapper.evidence, start[:2], origin=ORIGIN, cell=CELL)              # a tensor has no weights
    with pytest.raises(ValueError):
        _planner(2, 2, None).plan(mapper.evidence, start[:2])                      # ... and no placement
    with pytest.raises(ValueError):
        _planner(2, 2, None).plan(torch.zeros((2, 48, 36), dtype=torch.int32, device="cuda"), start[:5], origin=ORIGIN, cell=CELL)
    with pytest.raises(ValueError):
        _planner(2, 2, None).field(torch.zeros((48, 36), dtype=torch.int64, device="cuda"))
