"""GPU: the informed explorer (lipmpc_grid_frontier_gain_batch, lipmpc_grid_frontier_utility_field_batch,
lipmpc_grid_frontier_utility_path_batch) against tests/gain_oracle.py: the int32 gain / n_sources / n_sub / status / target_cell /
target_gain, the uint32 ufield, the nearest-frontier outputs beside them and the doubles of sub_goals[:n_sub], path_cost and target,
bit for bit, on every map -- every run into poisoned buffers (tests/gain_checks.py)."""
import functools

import numpy as np
import pytest

import field_oracle as FO
import frontier_oracle as FR
import gain_checks as K
import gain_oracle as G
from gain_checks import CELL, HAND_MADE, ORIGIN, SENTINEL, T_FREE, T_OCC, bits as _bits, check as _check

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def test_gpu_smallest_grid_all_unknown():
    got, _ = _check(np.zeros((2, 2), np.int32), list(K.centres(((0, 0), (1, 1)))) + [(np.nan, 0.0)], 3, 16, 10, r=0, mu=1)
    assert got["n_frontier"].tolist() == [0] and got["n_sources"].tolist() == [0] and (got["ufield"] == FO.INF).all() and not got["gain"].any()
    assert got["status"].tolist() == [G.NO_PATH, G.NO_PATH, G.OUTSIDE_GRID] and (got["target_gain"] == -1).all()


@pytest.mark.parametrize("r_view", [1, 2, 3, 64])
def test_gpu_hand_made(r_view):
    """5 x 7: the disc is clipped by the grid on every side."""
    starts = list(K.centres([(i, j) for i in range(5) for j in range(7)])) + [(ORIGIN[0] - 0.01, 0.3), (0.0, np.inf)]
    got, want = _check(HAND_MADE, starts, r_view, 16, 8, r=0, mu=1)
    assert got["n_sources"][0] >= 6 and (want["status"] == G.FOUND).sum() >= 15 and got["gain"].max() >= 2
    _check(HAND_MADE, starts, r_view, 40, 5, 3, r=0, mu=2)


@pytest.mark.parametrize("r", [1, 8, 64])
def test_gpu_one_free_cell_sees_the_disc(r):
    """All unknown but one cell: the count of the disc (at r = 64 the whole 129 x 129-bit window)."""
    ev = K.one_free_cell(r)
    got, _ = _check(ev, K.centres([(r + 1, r + 1), (0, 0)]), r, 16, 16384, r=0, mu=1)
    assert got["n_frontier"].tolist() == [1] and got["gain"][0, r + 1, r + 1] == G.OPEN_MAP_GAINS[r] == got["gain"].sum()
    assert got["target_gain"].tolist() == [G.OPEN_MAP_GAINS[r], -1] and got["status"].tolist() == [G.FOUND, G.NO_PATH]   # (the corner snaps nowhere)
    ev[0, :] = T_OCC                                           # a wall along one side: the rays end before it
    _check(ev, K.centres([(r + 1, r + 1)]), r, 16, 16384, r=0, mu=1)


@pytest.mark.parametrize("W,H", [(5, 13), (4, 33), (3, 64), (2, 65), (7, 31)])
@pytest.mark.parametrize("r_view", [3, 9])
def test_gpu_bitmap_words_and_row_ends(W, H, r_view):
    """65 cells cross a ballot word; with H = 33 and H = 64 a row ends one bit after / exactly at a word boundary: a ray that leaves
    a row's end must not see the next row's start."""
    rng = np.random.default_rng(W * 100 + H + r_view)
    for k in range(2):
        ev = K.speckled(rng, W, H, p_free=0.7, p_solid=0.05)
        ev[:, 0] = np.where(np.arange(W) % 2 == k % 2, 0, -1)                      # unknown / free alternating at both row ends
        ev[:, H - 1] = np.where(np.arange(W) % 2 == k % 2, -1, 0)
        got, want = _check(ev, K.points(rng, W, H, 12, margin=0.3), r_view, 16 + 50 * k, 6 + 10 * k, k, r=k, mu=1 + k)
    assert got["gain"].max() >= 3


def test_gpu_thresholds_and_the_ends_of_int32():
    for t in ((1, 3), (2, 1), (1 << 30, 1 << 30), (7, 1 << 30)):
        vals = [-t[0] - 1, -t[0], -t[0] + 1, t[1] - 1, t[1], I32_MIN, I32_MAX, 0, -1, 1]
        ev = np.array([vals, vals[::-1], vals], np.int32)
        got, _ = _check(ev, K.centres([(1, j) for j in range(len(vals))]), 2, 16, 6, r=0, mu=1, t=t)
        assert got["gain"].max() >= 2
        _check(ev, K.centres([(0, 0), (2, 5)]), 4, 30, 9, 1, r=1, mu=2, t=t)


@functools.lru_cache(maxsize=None)
def _scanned_nearest(per_robot):
    shared, per = K.scanned_maps()
    starts = np.array(K.SCAN_AT) if per_robot else _scanned_starts()
    return FR.plan_batch(per if per_robot else shared, T_FREE, T_OCC, K.MAP_ORIGIN, K.MAP_CELL, starts, 2, 2, None, 96)


def _scanned_starts():
    rng = np.random.default_rng(3)
    return np.concatenate([np.array(K.SCAN_AT), np.array(K.SCAN_AT) + (0.3, -0.25),
                           K.points(rng, K.MAP_W, K.MAP_H, 18, K.MAP_ORIGIN, K.MAP_CELL, margin=1.0)])


@pytest.mark.parametrize("r_view,g_cap,lo,hi", [(10, 174, 18, 174), (30, 600, 90, 1195)])
def test_gpu_scanned_map_shared(r_view, g_cap, lo, hi):
    shared, _ = K.scanned_maps()
    want = K.expected(shared, _scanned_starts(), r_view, 16, g_cap, S_max=96, origin=K.MAP_ORIGIN, cell=K.MAP_CELL, nearest=_scanned_nearest(False))
    got, _ = _check(shared, _scanned_starts(), r_view, 16, g_cap, S_max=96, origin=K.MAP_ORIGIN, cell=K.MAP_CELL, want=want)
    g = got["gain"][0][got["frontier"][0] != 0]
    assert got["n_frontier"][0] == 153 and g.min() == lo and g.max() == hi
    assert (want["status"][:6] == G.FOUND).all() and (want["status"] == G.NO_PATH).any()
    if r_view == 10:                                           # g_cap = the largest gain: every start's target is another than its nearest
        assert (got["target_cell"][:6] != want["nearest"]["target_cell"][:6]).all()


@pytest.mark.parametrize("r_view", [10, 30])
def test_gpu_scanned_maps_one_per_robot(r_view):
    _, per = K.scanned_maps()
    kw = dict(S_max=96, origin=K.MAP_ORIGIN, cell=K.MAP_CELL)
    want = K.expected(per, np.array(K.SCAN_AT), r_view, 16, 300, 20, nearest=_scanned_nearest(True), **kw)
    got, _ = _check(per, np.array(K.SCAN_AT), r_view, 16, 300, 20, want=want, **kw)
    assert (want["status"] == G.FOUND).all() and len(set(want["n_sources"].tolist())) == 3        # F = B = 3: robot b on its own map


def test_gpu_one_map_per_robot_many_robots():
    rng = np.random.default_rng(21)
    ev = np.stack([K.speckled(rng, 19, 23, p_free=0.75, p_solid=0.04) for _ in range(70)])     # F = B = 70: a block and a tail
    got, want = _check(ev, K.points(rng, 19, 23, 70, margin=0.5), 5, 24, 20, 2, r=1, mu=2)
    assert (want["status"] == G.FOUND).sum() >= 30 and len(set(want["n_sources"].tolist())) > 10


def test_gpu_each_side_of_the_lds_switch():
    """The largest map whose utility field is kept in LDS and the first that is relaxed in the output buffer, by the oracle module's
    restatement of THIS kernel's rule: hundreds of frontier cells, many more than a workgroup has waves."""
    for W, H in G.sizes_at_the_lds_switch():
        rng = np.random.default_rng(5)
        starts = np.concatenate([K.centres([(1, 1)]), K.points(rng, W, H, 7)])
        got, want = _check(K.rooms(W, H), starts, 4, 16, 30, 4, r=2, mu=2, S_max=200)
        assert want["status"][0] == G.FOUND and want["path_cost"][0] > 40 and got["n_frontier"][0] > 100 and got["n_sources"][0] > 100


def test_gpu_the_cell_cap():
    """32 x 4096 cells, both caps at once (2^17 cells, a side of 4096; a 2 x 65 536 map is refused for its side), at the largest
    view radius: the bitmaps of the whole map beside sixteen full windows, more than 64 KiB of LDS."""
    W, H = 32, 4096
    ev = np.zeros((W, H), np.int32)                            # unknown, but three walled corridors two cells wide, the last along the map's edge
    for i0 in (0, 10, 30):
        ev[max(i0 - 1, 0):min(i0 + 3, W), :] = T_OCC
        ev[i0:i0 + 2, :] = -1
        ev[i0 + 1, 20::80] = 0                                 # unknown cells in one row: five frontier cells round each
    ev[2, 1000:1012] = ev[9, 3000:3030] = ev[29, 4090:] = 0    # gaps in the walls: the unknown beyond is seen through them
    starts = K.centres([(0, 3), (11, 2000), (31, H - 1), (30, 0), (20, 100)])
    got, want = _check(ev, starts, 64, 16, 200, 1, r=0, mu=1, S_max=8)
    assert got["n_frontier"][0] > 700 and got["gain"].max() >= 64 and (want["status"] == G.FOUND).sum() >= 4
    assert got["frontier"][0, 30:, H - 64:].any() and got["gain"][0, 30:, H - 64:].max() > 0
    assert G.LDS_LIMIT >= 4 * (2 * FO.bitmap_words(W * H) + 2 + 2048 + 16 * 522) > 64 * 1024


def test_gpu_largest_seeds():
    shared, _ = K.scanned_maps()
    kw = dict(S_max=96, origin=K.MAP_ORIGIN, cell=K.MAP_CELL)
    want = K.expected(shared, _scanned_starts(), 10, 65535, 16384, nearest=_scanned_nearest(False), **kw)
    got, _ = _check(shared, _scanned_starts(), 10, 65535, 16384, want=want, **kw)
    finite = got["ufield"][got["ufield"] != FO.INF]
    assert finite.min() >= (65535 * (16384 - 174)) >> 4 and finite.max() < 7 * (1 << 17) + (1 << 26)


def test_gpu_w_gain_0_is_the_nearest_frontier_plan():
    """Against FrontierPlanner.plan ON THE DEVICE, every shared output bit for bit."""
    from grid_checks import run_frontier
    ev, start = K.fleet_case()
    for max_seg, S_max in ((None, 64), (5, 80)):
        near = run_frontier(ev, start, 2, 2, max_seg, S_max)
        got = K.run(ev, start, 7, 0, 33, 0, 2, 2, max_seg, S_max)
        for k in near:
            assert np.array_equal(_bits(got[k]), _bits(near[k])), k
        assert np.array_equal(got["ufield"], near["field"]) and np.array_equal(got["n_sources"], near["n_frontier"])
        ok = near["target_cell"] >= 0
        assert np.array_equal(got["target_gain"][ok], got["gain"][0].reshape(-1)[near["target_cell"][ok]]) and (got["target_gain"][~ok] == -1).all()


def test_gpu_hand_written_gain_is_clamped():
    ev, start = K.fleet_case()
    rng = np.random.default_rng(12)
    gain = rng.integers(-50, 120, ev.shape).astype(np.int32)
    gain[::3, ::2] = rng.choice([I32_MIN, I32_MAX, -1, 0, 60, 61, 1 << 20], gain[::3, ::2].shape)
    got, want = _check(ev, start[:40], 5, 300, 60, 0, gain=gain)
    assert (want["status"] == G.FOUND).sum() >= 15 and np.array_equal(got["gain"][0], gain)
    src = got["frontier"][0] != 0
    assert (gain[src] < 0).any() and (gain[src] > 60).any()
    _check(ev, start[:40], 5, 300, 60, 10, gain=gain)          # min_gain reads the stored value: negative entries are no sources


@pytest.mark.parametrize("gain_a", [74, 75, 76])
def test_gpu_tie_and_dominated_source(gain_a):
    ev, gain = K.corridor(gain_a)
    kw = dict(K.CORRIDOR_KW)
    got, want = _check(ev, K.centres([(1, j) for j in range(12)]), kw["r_view"], kw["w_gain"], kw["g_cap"], kw["min_gain"], kw["r"], kw["mu"],
                       gain=gain)
    a, b = K.CORRIDOR_A[0] * 12 + K.CORRIDOR_A[1], K.CORRIDOR_B[0] * 12 + K.CORRIDOR_B[1]
    at_a = {74: 0, 75: 4, 76: 4}[gain_a]                       # dominated: nobody; the tie, and strictly better: j = 0..3
    assert got["target_cell"].tolist() == [a] * at_a + [b] * (12 - at_a) and got["n_sources"].tolist() == [2]
    assert got["ufield"][0][K.CORRIDOR_A] == {74: 25, 75: 25, 76: 24}[gain_a] and G.seed(gain_a, 16, 100) == {74: 26, 75: 25, 76: 24}[gain_a]


def test_gpu_min_gain_prunes_everything():
    shared, _ = K.scanned_maps()
    kw = dict(S_max=96, origin=K.MAP_ORIGIN, cell=K.MAP_CELL)
    want = K.expected(shared, _scanned_starts(), 10, 16, 174, 175, nearest=_scanned_nearest(False), **kw)
    got, _ = _check(shared, _scanned_starts(), 10, 16, 174, 175, want=want, **kw)
    assert got["n_sources"].tolist() == [0] and got["n_frontier"].tolist() == [153] and (got["ufield"] == FO.INF).all()
    assert set(got["status"].tolist()) <= {G.NO_PATH, G.OUTSIDE_GRID, G.START_OCCUPIED} and (got["sub_goals"] == SENTINEL).all()


@functools.lru_cache(maxsize=None)
def _fleet_want(max_seg, S_max):
    ev, start = K.fleet_case()
    return K.expected(ev, start, 6, 16, 40, 24, max_seg=max_seg, S_max=S_max)


def test_gpu_one_field_many_robots():
    ev, start = K.fleet_case()
    assert len(start) == 130                                   # two full blocks of lanes and a tail
    got, want = _check(ev, start, 6, 16, 40, 24, want=_fleet_want(None, 64))
    st = want["status"]
    assert st[:3].tolist() == [G.START_OCCUPIED, G.NO_PATH, G.NO_PATH] and st[9:12].tolist() == [G.OUTSIDE_GRID] * 3 and st[3] == G.FOUND
    assert want["cells"][3][0] != (3, 8)                       # inflated: snapped
    print("statuses", np.bincount(st, minlength=8).tolist(), "n_sources", got["n_sources"].tolist(), "n_frontier", got["n_frontier"].tolist())
    assert (st == G.FOUND).sum() >= 50 and (st == G.OUTSIDE_GRID).sum() >= 8 and (st == G.START_OCCUPIED).sum() >= 4
    found = st == G.FOUND
    assert (got["frontier"][0].reshape(-1)[got["target_cell"][found]] == 1).all() and (got["target_gain"][found] >= 24).all()
    assert 0 < got["n_sources"][0] < got["n_frontier"][0]


@pytest.mark.parametrize("max_seg", [5, None])
def test_gpu_spacing_cap_and_overflow(max_seg):
    ev, start = K.fleet_case()
    want = _fleet_want(max_seg, 80)
    b = int(np.argmax(np.where(want["status"] == G.FOUND, want["n_sub"], 0)))
    n = int(want["n_sub"][b])
    assert n >= 2
    tight, _ = _check(ev, start[b:b + 1], 6, 16, 40, 24, max_seg=max_seg, S_max=n - 1)
    assert tight["status"].tolist() == [G.PATH_OVERFLOW] and tight["n_sub"].tolist() == [0] and (tight["sub_goals"] == SENTINEL).all()
    assert tight["target_cell"][0] == want["target_cell"][b] and tight["path_cost"][0] == want["path_cost"][b]
    assert tight["target_gain"][0] == want["target_gain"][b] >= 24
    assert _check(ev, start[b:b + 1], 6, 16, 40, 24, max_seg=max_seg, S_max=n)[0]["status"][0] == G.FOUND       # exactly enough


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
    """Field + gain + utility field + path captured in one graph and replayed twice over poisoned buffers equal the eager call; two
    eager calls equal each other."""
    if case == "fleet":
        ev, start = K.fleet_case()
    else:
        W, H = G.sizes_at_the_lds_switch()[1]
        ev, start = K.rooms(W, H), K.points(np.random.default_rng(6), W, H, 16)
    W, H = ev.shape
    args = (6, 16, 40, 24)
    eager = [K.run(ev, start, *args) for _ in range(2)]
    for k in eager[0]:
        assert np.array_equal(_bits(eager[0][k]), _bits(eager[1][k])), k
    pl = K.planner(*args)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")
    out = K.buffers(len(start), 1, W, H, 64)
    graph = _captured(pl, d_ev, d_start, out, 64)
    for _ in range(2):
        K.poison(out)
        graph.replay()
        torch.cuda.synchronize()
        got = K.host(out)
        for k in eager[0]:
            assert np.array_equal(_bits(got[k]), _bits(eager[0][k])), k


def test_gpu_fields_alone_mapper_defaults_and_argument_checks():
    ev, start = K.fleet_case()
    mapper = lipmpc.OccupancyMapper(48, 36, ORIGIN, CELL, lidar_range=1.0, w_hit=T_OCC, w_miss=T_FREE)
    mapper.evidence.copy_(torch.as_tensor(ev))
    pl = lipmpc.InformedFrontierPlanner(6, 16, 40, 24)         # r_inflate 2, min_unknown 2, thresholds from the mapper
    want = _fleet_want(None, 64)
    g, f = pl.gain(mapper), pl.field(mapper)
    torch.cuda.synchronize()
    assert set(g) == {"field", "frontier", "n_frontier", "gain"} and set(f) == set(g) | {"ufield", "n_sources"}
    for k in ("frontier", "n_frontier", "gain"):
        assert np.array_equal(g[k].cpu().numpy(), want[k]) and np.array_equal(f[k].cpu().numpy(), want[k]), k
    assert np.array_equal(f["ufield"].view(torch.int32).cpu().numpy().view(np.uint32), want["ufield"])
    assert np.array_equal(f["field"].view(torch.int32).cpu().numpy().view(np.uint32), want["field"])       # the nearest-frontier field
    assert f["n_sources"].tolist() == want["n_sources"].tolist() and f["ufield"].dtype == torch.uint32 and f["gain"].dtype == torch.int32
    fresh = pl.plan(mapper, start[3:4])                        # placement from the mapper; rows past n_sub are 0 in a fresh out
    n = int(fresh["n_sub"][0])
    assert n >= 1 and (fresh["sub_goals"][0, n:] == 0).all() and int(fresh["target_gain"][0]) == want["target_gain"][3]
    assert set(fresh) == set(lipmpc.planner.informed_outputs(1, 1, 48, 36, 64))
    assert tuple(pl.plan(mapper, np.zeros((0, 2)))["sub_goals"].shape) == (0, 64, 2)
    with pytest.raises(ValueError):
        pl.plan(mapper.evidence, start[:2], origin=ORIGIN, cell=CELL)              # a tensor has no weights
    with pytest.raises(ValueError):
        K.planner(6, 16, 40).plan(mapper.evidence, start[:2])                      # ... and no placement
    with pytest.raises(ValueError):
        K.planner(6, 16, 40).plan(torch.zeros((2, 48, 36), dtype=torch.int32, device="cuda"), start[:5], origin=ORIGIN, cell=CELL)
