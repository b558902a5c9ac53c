"""GPU: the tiled informed explorer (include/lipmpc.h, TILED EXPLORERS; through TiledInformedFrontierPlanner and, where the
frontier bytes are hand-made, through the C calls) against tests/gain_oracle.py, bit for bit, on the smallest shapes at which the
kernels can go wrong.  Every shape comes from the tile sides TW x TH; every buffer starts poisoned."""
import numpy as np
import pytest

import field_tiled_cases as T
import gain_checks as GC
import gain_oracle as G
from gain_checks import CELL, ORIGIN, SENTINEL, T_FREE, T_OCC, bits, centres

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

TW, TH = T.TW, T.TH
POISON = -0x01010102                                          # int32 of the bytes FE FE FE FE: not a status, a count or a flag
UNSETTLED = lipmpc.RRT_FIELD_UNSETTLED


def _planner(r_view, w_gain, g_cap, min_gain=0, r=2, mu=2, max_seg=None, rounds=None):
    return lipmpc.TiledInformedFrontierPlanner(r_view, w_gain, g_cap, min_gain, r_inflate=r, min_unknown=mu, t_free=T_FREE, t_occ=T_OCC,
                                               max_seg=max_seg, rounds=rounds)


def _buffers(B, F, W, H, S_max):
    out = GC.buffers(B, F, W, H, S_max)
    for k in ("settled", "usettled"):
        out[k] = torch.full((F,), POISON, dtype=torch.int32, device="cuda")
    return out


def _run(ev, start, r_view, w_gain, g_cap, min_gain=0, r=2, mu=2, max_seg=None, S_max=64, gain=None, rounds=None, pl=None, origin=ORIGIN,
         cell=CELL):
    """One plan through the class into poisoned buffers.  ``gain``: a hand-written gain in the place of the gain call's -- then the
    class's own calls are made one by one, as tests/gain_checks.py's run does."""
    ev, start = np.ascontiguousarray(ev, np.int32), np.ascontiguousarray(np.asarray(start, np.float64).reshape(-1, 2))
    W, H = ev.shape[-2:]
    out = _buffers(len(start), 1 if ev.ndim == 2 else len(ev), W, H, S_max)
    pl = pl or _planner(r_view, w_gain, g_cap, min_gain, r, mu, max_seg, rounds)
    d_ev, d_start = torch.as_tensor(ev, device="cuda"), torch.as_tensor(start, device="cuda")
    if gain is None:
        got = pl.plan(d_ev, d_start, origin=origin, cell=cell, S_max=S_max, out=out)
        assert got is out and pl.last is out
    else:
        ev3, t_free, t_occ, org, cs = pl._map(d_ev, origin, cell)
        org, cs, org_c, cell_c = pl._placement(org, cs)
        pl._field(ev3, t_free, t_occ, out)
        out["gain"].copy_(torch.as_tensor(np.ascontiguousarray(gain, np.int32).reshape(ev3.shape), device="cuda"))
        pl._ufield(ev3, out)
        pl._path(ev3, t_occ, d_start, org_c, cell_c, S_max, out)
        pl._target(out, org, cs, H)
    torch.cuda.synchronize()
    return GC.host(out)


def _check(ev, start, r_view, w_gain, g_cap, min_gain=0, r=2, mu=2, max_seg=None, S_max=64, gain=None, want=None, nearest=None):
    if want is None:
        want = GC.expected(ev, start, r_view, w_gain, g_cap, min_gain, r, mu, max_seg, S_max, gain=gain, nearest=nearest)
    got = _run(ev, start, r_view, w_gain, g_cap, min_gain, r, mu, max_seg, S_max, gain)
    F = len(want["n_frontier"])
    assert got["settled"].tolist() == [1] * F and got["usettled"].tolist() == [1] * F
    GC.same(got, want, S_max)
    return got, want


def _gain_call(ev, frontier, r_view):
    """lipmpc_grid_frontier_gain_tiled_batch on hand-made frontier bytes (the call takes the given bytes), into a poisoned buffer."""
    ev, frontier = np.ascontiguousarray(ev, np.int32), np.ascontiguousarray(frontier, np.uint8)
    ev3 = ev if ev.ndim == 3 else ev[None]
    F, W, H = ev3.shape
    gain = torch.full((F, W, H), GC.POISON_I32, dtype=torch.int32, device="cuda")
    lipmpc._lib.call("lipmpc_grid_frontier_gain_tiled_batch", device=0, F=F, W=W, H=H, evidence=torch.as_tensor(ev3, device="cuda"),
                     t_free=T_FREE, t_occ=T_OCC, frontier=torch.as_tensor(frontier.reshape(ev3.shape), device="cuda"), r_view=r_view, gain=gain,
                     hip_stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return gain.cpu().numpy().reshape(ev.shape)


# -- 1. shapes ---------------------------------------------------------------------------------------------------------------
def test_two_by_two():
    ev = np.array([[-T_FREE, 0], [0, T_OCC]], np.int32)
    got, want = _check(ev, centres(((0, 0), (1, 1), (0, 1))), 3, 16, 8, r=0, mu=1)
    assert want["n_frontier"].tolist() == [1] and want["gain"][0][0, 0] == 2 and want["status"].tolist() == [G.FOUND, G.START_OCCUPIED, G.FOUND]


@pytest.mark.parametrize("W,H", [(TW, TH), (TW + 1, TH - 1), (TH - 1, TW + 1)])
def test_one_tile_and_one_cell_over_and_under(W, H):
    rng = np.random.default_rng(W * 1000 + H)
    ev = GC.speckled(rng, W, H)
    got, want = _check(ev, GC.points(rng, W, H, 12, margin=0.5), 8, 16, 120, min_gain=3, r=1)
    assert want["n_sources"][0] > 20 and (want["gain"] > 0).sum() > 20 and (want["status"] == G.FOUND).sum() >= 4


# -- 2. a window that spans four tiles -----------------------------------------------------------------------------------------
def test_windows_round_a_four_tile_corner():
    rng = np.random.default_rng(4)
    ev = GC.speckled(rng, 2 * TW, 2 * TH, p_free=0.5, p_solid=0.03)
    frontier = np.zeros(ev.shape, np.uint8)
    for c in T.CORNER:
        frontier[c] = 1
        ev[c] = -T_FREE
    want = G.gain(ev, T_FREE, T_OCC, frontier, 16)
    got = _gain_call(ev, frontier, 16)
    assert np.array_equal(got, want) and all(want[c] > 50 for c in T.CORNER) and (got[frontier == 0] == 0).all()


# -- 3. the largest radius on a small map ----------------------------------------------------------------------------------------
def test_r_view_64_on_a_speckled_map_just_over_a_tile():
    rng = np.random.default_rng(64)
    W, H = TW + 3, TH + 3
    ev = GC.speckled(rng, W, H, p_free=0.7, p_solid=0.02)
    got, want = _check(ev, GC.points(rng, W, H, 6), 64, 16, 2000, min_gain=10, r=1)
    assert want["gain"].max() > 100 and want["n_sources"][0] > 10


def test_all_unknown_but_one_cell():
    """The open-map gains: the whole disc where it fits the map (r_view 13 round the middle cell), the disc clipped by the grid on
    all four sides at r_view 64."""
    W, H = TW + 3, TH + 3
    ev = np.zeros((W, H), np.int32)
    mid = (W // 2, H // 2)
    ev[mid] = -T_FREE
    frontier = (ev < 0).astype(np.uint8)
    assert min(mid[0], W - 1 - mid[0], mid[1], H - 1 - mid[1]) >= 13
    assert _gain_call(ev, frontier, 13)[mid] == G.OPEN_MAP_GAINS[13] == G.gain(ev, T_FREE, T_OCC, frontier, 13)[mid]
    want = G.gain(ev, T_FREE, T_OCC, frontier, 64)
    got = _gain_call(ev, frontier, 64)
    assert np.array_equal(got, want) and W * H // 2 < want[mid] < min(G.OPEN_MAP_GAINS[64], W * H)
    # through the class too: the one free cell is the frontier (r_inflate 0, min_unknown 1)
    _check(ev, centres([mid]), 64, 16, 4000, r=0, mu=1)


# -- 4. a solid cell on a tile's rim ---------------------------------------------------------------------------------------------
def test_solid_on_the_rim_stops_rays_from_the_next_tile():
    """All unknown; a source three rows into tile (1, 0); the solid cell on the last row of tile (0, 0) straight ahead of it: the rays
    through it end there, so the cells behind it, which the source's own tile does not hold, are not counted."""
    ev = np.zeros((2 * TW, 2 * TH), np.int32)
    src, wall = (TW + 2, 10), (TW - 1, 10)
    ev[src] = -T_FREE
    frontier = (ev < 0).astype(np.uint8)
    open_gain = _gain_call(ev, frontier, 8)[src]
    ev[wall] = T_OCC
    want = G.gain(ev, T_FREE, T_OCC, frontier, 8)
    got = _gain_call(ev, frontier, 8)
    assert np.array_equal(got, want) and got[src] < open_gain - 1 and open_gain == G.gain(np.where(ev > 0, 0, ev), T_FREE, T_OCC, frontier, 8)[src]


# -- 5. maps without a frontier ----------------------------------------------------------------------------------------------------
def test_three_maps_with_no_few_and_many_frontier_cells():
    W, H = TW + 3, TH + 3
    rng = np.random.default_rng(5)
    none, few = np.full((W, H), -T_FREE, np.int32), np.full((W, H), -T_FREE, np.int32)
    few[W - 2:, H - 2:] = 0
    ev = np.stack([none, few, GC.speckled(rng, W, H)])
    start = centres([(3, 3), (3, 3), (3, 3)])
    got, want = _check(ev, start, 8, 16, 60, r=1)
    assert want["n_frontier"][0] == 0 and want["n_sources"].tolist()[0] == 0 and 0 < want["n_sources"][1] < 8 < want["n_sources"][2]
    assert got["status"][0] == G.NO_PATH and (got["ufield"][0] == G.INF).all()
    # a map without a source is settled before the first round: one round is budget enough for it
    one = _run(ev, start, 8, 16, 60, r=1, rounds=1)
    assert one["usettled"][0] == 1 and one["settled"][0] == 1 and one["status"][0] == G.NO_PATH and one["n_sources"][0] == 0


# -- 6. dominated sources across a border ---------------------------------------------------------------------------------------
def test_a_source_dominated_from_the_next_tile():
    """Hand-written gains: A = (TW - 1, TH - 1), the last cell of tile (0, 0), seed 50; B = (TW, TH + 1) in tile (1, 1), seed 0, 12
    cost units away: A is dominated, and robots beside A walk on to B."""
    ev = np.full((2 * TW, 2 * TH), -T_FREE, np.int32)
    ev[TW - 2, TH - 2] = ev[TW + 1, TH + 2] = 0
    a, b = (TW - 1, TH - 1), (TW, TH + 1)
    gain = np.zeros(ev.shape, np.int32)
    gain[a], gain[b] = 50, 100
    got, want = _check(ev, centres([a, (TW - 3, TH - 1), (0, 0), b]), 2, 16, 100, min_gain=1, r=0, mu=1, gain=gain)
    assert want["n_sources"].tolist() == [2] and want["ufield"][0][a] == 12 < G.seed(50, 16, 100)
    assert want["target_cell"].tolist() == [b[0] * 2 * TH + b[1]] * 4 and want["target_gain"].tolist() == [100] * 4


@pytest.mark.parametrize("along", ["j", "i"])
@pytest.mark.parametrize("gain_a", [74, 75, 76])
def test_the_corridor_tie_across_a_tile_border(gain_a, along):
    """tests/gain_checks.py's corridor with the tile border between A and B: 75 ties the route through A, 74 leaves A dominated,
    76 makes A strictly better."""
    n = (TH if along == "j" else TW) + 8
    a, b = n - 11, n - 6                                       # five cells apart, the border n - 8 between them
    ev = np.full((3, n), T_OCC, np.int32)
    ev[1, :] = -T_FREE
    ev[0, a] = ev[0, b] = 0
    gain = np.zeros((3, n), np.int32)
    gain[1, a], gain[1, b] = gain_a, 100
    cells = [(1, 0), (1, a), (1, a + 2), (1, n - 1)]
    if along == "i":
        ev, gain, cells = np.ascontiguousarray(ev.T), np.ascontiguousarray(gain.T), [(j, i) for i, j in cells]
    kw = dict(GC.CORRIDOR_KW)
    got, want = _check(ev, centres(cells), kw["r_view"], kw["w_gain"], kw["g_cap"], kw["min_gain"], r=kw["r"], mu=kw["mu"], gain=gain)
    H = ev.shape[1]
    at_a = (1 * H + a) if along == "j" else (a * H + 1)
    assert (want["target_cell"][0] == at_a) == (gain_a >= 75) and want["n_sources"].tolist() == [2]


# -- 7. w_gain = 0, min_gain = 0 is the plain tiled planner ---------------------------------------------------------------------
@pytest.mark.parametrize("id_", ["baffles", "spiral"])
def test_no_weight_is_the_plain_tiled_planner(id_):
    c, want = T.case(id_), T.oracle(id_, "frontier")
    kw = dict(r_inflate=c["r"], min_unknown=c["mu"], t_free=T.T_FREE, t_occ=T.T_OCC, max_seg=c["max_seg"])
    ev, start = torch.as_tensor(c["ev"], device="cuda"), torch.as_tensor(c["start"], device="cuda")
    plain = lipmpc.FrontierPlanner(tiled=True, **kw).plan(ev, start, origin=T.ORIGIN, cell=T.CELL, S_max=c["S_max"])
    mine = lipmpc.TiledInformedFrontierPlanner(4, 0, 16, 0, **kw).plan(ev, start, origin=T.ORIGIN, cell=T.CELL, S_max=c["S_max"])
    torch.cuda.synchronize()
    assert mine["settled"].tolist() == [1] and mine["usettled"].tolist() == [1] and plain["settled"].tolist() == [1]
    for k in ("sub_goals", "n_sub", "status", "path_cost", "target", "target_cell", "frontier", "n_frontier"):
        assert np.array_equal(bits(mine[k].cpu().numpy()), bits(plain[k].cpu().numpy()), equal_nan=False), k
    assert torch.equal(mine["field"].view(torch.int32), plain["field"].view(torch.int32))
    assert torch.equal(mine["ufield"].view(torch.int32), plain["field"].view(torch.int32))
    assert np.array_equal(mine["ufield"].view(torch.int32).cpu().numpy().view(np.uint32), want["field"])
    assert mine["n_sources"].tolist() == want["n_frontier"].tolist() and (mine["status"].cpu().numpy() == want["status"]).all()


# -- 8. the budget and the resume --------------------------------------------------------------------------------------------------
def _changes_down(ufld):
    """Per cell, how often its descent path down a utility field changes tile (a source that holds its own seed: 0); -1 on INF."""
    W, H = ufld.shape
    changes = np.full((W, H), -1, np.int64)
    for flat in np.argsort(ufld, axis=None, kind="stable"):
        c = (int(flat) // H, int(flat) % H)
        if ufld[c] == G.INF:
            break
        try:
            n = T.descent_step(ufld, c)
            changes[c] = changes[n] + (T.tile_of(c) != T.tile_of(n))
        except AssertionError:
            changes[c] = 0
    return changes


def _rounds_to_settle(ufld):
    """The round guarantee: every value is final after (the most tile changes of any descent path) + 1 rounds, and one more round, in
    which nothing falls, leaves no tile active."""
    return int(_changes_down(ufld).max()) + 2


def test_a_budget_too_small_then_resume_on_the_spiral():
    c, near = T.case("spiral"), T.oracle("spiral", "frontier")
    args = dict(r_view=4, w_gain=16, g_cap=40)
    want = GC.expected(c["ev"], c["start"], r=c["r"], mu=c["mu"], max_seg=c["max_seg"], S_max=c["S_max"], origin=T.ORIGIN, cell=T.CELL,
                       nearest=near, **args)
    # rounds=1 through the class: unsettled, and the path call says so and writes nothing else
    pl = _planner(r=c["r"], mu=c["mu"], max_seg=c["max_seg"], rounds=1, min_gain=0, **args)
    got = _run(c["ev"], c["start"], S_max=c["S_max"], pl=pl, origin=T.ORIGIN, cell=T.CELL, **args)
    B = len(c["start"])
    assert got["usettled"].tolist() == [0] and got["status"].tolist() == [UNSETTLED] * B and got["n_sub"].tolist() == [0] * B
    assert np.isnan(got["path_cost"]).all() and (got["sub_goals"] == SENTINEL).all() and np.isnan(got["target"]).all()
    assert got["target_cell"].tolist() == [-1] * B and got["target_gain"].tolist() == [-1] * B
    assert np.array_equal(got["gain"], want["gain"]) and np.array_equal(got["n_sources"], want["n_sources"])      # (local: no rounds)
    finite = got["ufield"][0] != G.INF
    assert (got["ufield"][0][finite] >= want["ufield"][0][finite]).all()                                          # costs of real paths
    # the C call: cold with one round, then resumes of one round, bounded by the round guarantee
    F, W, H = 1, *c["ev"].shape
    budget = _rounds_to_settle(want["ufield"][0])
    d = {k: torch.as_tensor(np.ascontiguousarray(want[k]), device="cuda") for k in ("frontier", "gain")}
    uf = torch.full((F, W, H), 0x5EED, dtype=torch.int32, device="cuda").view(torch.uint32)
    n_src, settled = (torch.full((F,), POISON, dtype=torch.int32, device="cuda") for _ in range(2))
    work = torch.full((lipmpc._lib.load().lipmpc_grid_tiled_workspace_bytes(F, W, H),), 0xFF, dtype=torch.uint8, device="cuda")
    ev = torch.as_tensor(c["ev"][None], device="cuda")

    def call(rounds, resume):
        lipmpc._lib.call("lipmpc_grid_frontier_utility_field_tiled_batch", device=0, F=F, W=W, H=H, evidence=ev, t_free=T.T_FREE,
                         t_occ=T.T_OCC, r_inflate=c["r"], frontier=d["frontier"], gain=d["gain"], w_gain=16, g_cap=40, min_gain=0, ufield=uf,
                         n_sources=n_src, work=work, work_bytes=work.numel(), max_rounds=rounds, resume=resume, settled=settled,
                         hip_stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return int(settled[0])
    assert call(1, 0) == 0
    at = None
    for r in range(2, budget + 1):
        if call(1, 1):
            at = r
            break
    print(f"spiral utility field: budget {budget} from the guarantee, settled after {at} rounds")
    assert at is not None and np.array_equal(uf.view(torch.int32).cpu().numpy().view(np.uint32), want["ufield"]) and n_src.tolist() == want["n_sources"].tolist()
    assert call(3, 1) == 1 and np.array_equal(uf.view(torch.int32).cpu().numpy().view(np.uint32), want["ufield"])       # a resume on a settled field
    # and through the class with rounds=None: every output the oracle's
    got = _run(c["ev"], c["start"], S_max=c["S_max"], r=c["r"], mu=c["mu"], max_seg=c["max_seg"], origin=T.ORIGIN, cell=T.CELL, **args)
    assert got["usettled"].tolist() == [1]
    GC.same(got, want, c["S_max"])


# -- 9. / 10. repeats on leftover workspace, graph replay ----------------------------------------------------------------------
def _baffles():
    c, near = T.case("baffles"), T.oracle("baffles", "frontier")
    args = dict(r_view=6, w_gain=16, g_cap=60, min_gain=2)
    want = GC.expected(c["ev"], c["start"], r=c["r"], mu=c["mu"], max_seg=c["max_seg"], S_max=c["S_max"], origin=T.ORIGIN, cell=T.CELL,
                       nearest=near, **args)
    return c, near, args, want


def test_two_cold_calls_on_workspace_left_over_from_another_shape():
    c, near, args, want = _baffles()
    pl = _planner(r=c["r"], mu=c["mu"], max_seg=c["max_seg"], **args)
    rng = np.random.default_rng(9)
    other = GC.speckled(rng, 4 * TW + 5, 3 * TH + 1)           # a larger map first: both workspaces are left full of its state
    _run(other, GC.points(rng, *other.shape, 4), pl=pl, **args)
    runs = [_run(c["ev"], c["start"], S_max=c["S_max"], pl=pl, origin=T.ORIGIN, cell=T.CELL, **args) for _ in range(2)]
    assert len(pl._works) == 1 and len(pl._uworks) == 1       # grown once, never again
    for k in runs[0]:
        assert np.array_equal(bits(runs[0][k]), bits(runs[1][k])), k
    assert runs[0]["usettled"].tolist() == [1]
    GC.same(runs[0], want, c["S_max"])


def test_graph_replay_with_fixed_rounds():
    c, near, args, want = _baffles()
    rounds = max(T.rounds_to_settle(near["field"][0]), _rounds_to_settle(want["ufield"][0]))      # from the round guarantee
    pl = _planner(r=c["r"], mu=c["mu"], max_seg=c["max_seg"], rounds=rounds, **args)
    (W, H), B = c["ev"].shape, len(c["start"])
    out = _buffers(B, 1, W, H, c["S_max"])
    ev, start = torch.as_tensor(c["ev"], device="cuda"), torch.as_tensor(c["start"], device="cuda")
    plan = lambda: pl.plan(ev, start, origin=T.ORIGIN, cell=T.CELL, S_max=c["S_max"], out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan()                                                 # warm-up outside the capture: the workspaces grow here
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = GC.host(out)
    works = len(pl._works), len(pl._uworks)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan()
    assert (len(pl._works), len(pl._uworks)) == works         # nothing reallocated while capturing
    for _ in range(2):
        GC.poison(out)
        for k in ("settled", "usettled"):
            out[k].fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        got = GC.host(out)
        for k in eager:
            assert np.array_equal(bits(got[k]), bits(eager[k])), k
        assert got["usettled"].tolist() == [1] and got["settled"].tolist() == [1]
        GC.same(got, want, c["S_max"])
    pl.rounds = None                                           # rounds=None reads `settled` on the host: not under capture
    with pytest.raises(RuntimeError, match="rounds"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            out["settled"].fill_(POISON)
            plan()


# -- 11. beyond the old cap -----------------------------------------------------------------------------------------------------
def test_363_x_362_the_first_shape_the_old_calls_refuse():
    c, near = T.case("363x362"), T.oracle("363x362", "frontier")
    assert 0 < near["n_frontier"][0] <= 16                     # a handful of frontier cells
    args = dict(r_view=12, w_gain=16, g_cap=200)
    with pytest.raises(RuntimeError) as e:
        GC.planner(r=c["r"], mu=c["mu"], max_seg=c["max_seg"], t=(T.T_FREE, T.T_OCC), **args).plan(
            torch.as_tensor(c["ev"], device="cuda"), torch.as_tensor(c["start"], device="cuda"), origin=T.ORIGIN, cell=T.CELL)
    assert e.value.code == -2
    want = GC.expected(c["ev"], c["start"], r=c["r"], mu=c["mu"], max_seg=c["max_seg"], S_max=c["S_max"], origin=T.ORIGIN, cell=T.CELL,
                       nearest=near, **args)
    got = _run(c["ev"], c["start"], S_max=c["S_max"], r=c["r"], mu=c["mu"], max_seg=c["max_seg"], origin=T.ORIGIN, cell=T.CELL, **args)
    assert got["settled"].tolist() == [1] and got["usettled"].tolist() == [1]
    GC.same(got, want, c["S_max"])


# -- 12. a large map, no Dijkstra ----------------------------------------------------------------------------------------------------
def test_1024_squared():
    """The gain of selected frontier cells against the oracle on crops that reach more than r_view beyond them (a ray never leaves
    the disc, so the crop's gain is the map's), and the utility field with w_gain = 0 against the tiled frontier field."""
    W = H = 1024
    r_view = 16
    rng = np.random.default_rng(1024)
    ev = np.full((W, H), -T_FREE, np.int32)
    ev[1000:] = 0
    picks = [(999, 1), (999, TH - 1), (999, TH), (999, 7 * TH + 31), (999, H - 2)]
    for i, j in picks:                                         # walls and holes in the unknown band before each pick
        lo, hi = max(j - 12, 0), min(j + 12, H)
        block = ev[1001:1012, lo:hi]
        block[rng.random(block.shape) < 0.15] = T_OCC
        block[rng.random(block.shape) < 0.2] = -T_FREE
    pl = lipmpc.TiledInformedFrontierPlanner(r_view, 0, 64, 0, r_inflate=0, min_unknown=2, t_free=T_FREE, t_occ=T_OCC)
    got = pl.field(torch.as_tensor(ev, device="cuda"))
    torch.cuda.synchronize()
    assert got["settled"].tolist() == [1] and got["usettled"].tolist() == [1]
    assert torch.equal(got["ufield"].view(torch.int32), got["field"].view(torch.int32)) and got["n_sources"].tolist() == got["n_frontier"].tolist()
    frontier, gain = got["frontier"][0].cpu().numpy(), got["gain"][0].cpu().numpy()
    assert (gain[frontier == 0] == 0).all() and frontier[999, 1:H - 1].all()
    m = r_view + 2
    for i, j in picks:
        i0, i1, j0, j1 = max(i - m, 0), min(i + m + 1, W), max(j - m, 0), min(j + m + 1, H)
        crop_fr = np.zeros((i1 - i0, j1 - j0), np.uint8)
        crop_fr[i - i0, j - j0] = 1
        want = G.gain(ev[i0:i1, j0:j1], T_FREE, T_OCC, crop_fr, r_view)[i - i0, j - j0]
        assert frontier[i, j] == 1 and gain[i, j] == want and want > 20, (i, j, gain[i, j], want)
    # the field itself, in closed form above the band on the columns away from the edges: 5 per row
    fld = got["field"][0].view(torch.int32).cpu().numpy()
    assert (fld[:1000, 4:H - 4] == 5 * (999 - np.arange(1000))[:, None]).all() and (fld[1000:][ev[1000:] == 0] == -1).all()
