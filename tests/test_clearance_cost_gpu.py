"""GPU: the clearance cost layer (include/lipmpc.h, lipmpc_grid_clearance_cost_batch) against the brute-force oracle of
tests/clearance_oracle.py, every byte: the smallest map, tile and bitmap-word borders, the map's corners, the ends of both parameter
ranges, maps narrower than the grown window, several maps in one call, the evidence form and a graph replay."""
import numpy as np
import pytest

import clearance_oracle as CO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

TW, TH, _ = lipmpc.tiled_info()
POISON = 0xA5


def _call(r, w, occ=None, ev=None, t_occ=3, cost=None):
    """One call on occ [M,W,H] uint8 or ev [M,W,H] int32 (numpy); the layer as numpy, from a buffer that held POISON."""
    src = occ if occ is not None else ev
    M, W, H = src.shape
    dev = torch.as_tensor(np.ascontiguousarray(src), device="cuda")
    if cost is None:
        cost = torch.full((M, W, H), POISON, dtype=torch.uint8, device="cuda")
    lipmpc._lib.call("lipmpc_grid_clearance_cost_batch", device=0, M=M, W=W, H=H, occ=dev if occ is not None else None,
                     evidence=dev if occ is None else None, t_occ=t_occ, r_clear=r, w_clear=w, cost=cost,
                     hip_stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return cost.cpu().numpy()


def _check(occ, r, w):
    occ = np.asarray(occ, np.uint8)
    occ = occ if occ.ndim == 3 else occ[None]
    got = _call(r, w, occ=occ)
    want = np.stack([CO.clearance_cost(m != 0, r, w) for m in occ])
    assert np.array_equal(got, want), (r, w, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    return got


def _random(W, H, seed, p=0.03):
    return (np.random.default_rng(seed).random((W, H)) < p).astype(np.uint8)


def test_two_by_two():
    for solid in ((), ((0, 0),), ((1, 0), (0, 1)), ((0, 0), (0, 1), (1, 0), (1, 1))):
        occ = np.zeros((2, 2), np.uint8)
        for c in solid:
            occ[c] = 7                                        # (solid = byte != 0)
        for r, w in ((1, 248), (2, 100), (31, 248)):
            _check(occ, r, w)


def test_random_map_over_the_tile_at_the_ends_of_both_ranges():
    """(TW + 3) x (TH + 3), 3 % solid: r_clear 1, 2, 7 and 31, w_clear 0, 1 and 248."""
    occ = _random(TW + 3, TH + 3, 1)
    assert occ.any()
    for r in (1, 2, 7, 31):
        for w in (0, 1, 248):
            g = _check(occ, r, w)[0]
            assert g.max() == w and (g[occ != 0] == w).all()


def test_one_cell_whose_disc_crosses_both_tile_borders_and_a_bitmap_word():
    occ = np.zeros((2 * TW, 2 * TH), np.uint8)
    occ[TW, TH] = 1
    g = _check(occ, 31, 248)[0]
    assert g[TW - 31, TH] == 0 and g[TW - 30, TH] > 0 and g[TW, TH - 30] > 0 and g[TW, TH + 30] > 0 and g[TW + 22, TH + 21] > 0
    assert g[TW, TH] == 248 and g[TW, TH - 1] == (248 * 960) // 961
    for r in (1, 16, 30):
        _check(occ, r, 200)


def test_solid_cells_in_the_four_corners_and_no_solid_cell():
    for W, H in ((2 * TW + 1, TH + 5), (TW - 3, 3 * TH - 1)):
        occ = np.zeros((W, H), np.uint8)
        occ[0, 0] = occ[0, H - 1] = occ[W - 1, 0] = occ[W - 1, H - 1] = 1
        _check(occ, 31, 248)
        _check(occ, 7, 33)
        assert not _check(np.zeros((W, H), np.uint8), 31, 248).any()


@pytest.mark.parametrize("shape", [(2, 4096), (4096, 2)])
def test_maps_narrower_than_the_grown_window(shape):
    occ = _random(*shape, 5, p=0.01)
    occ[0, 0] = occ[-1, -1] = 1
    _check(occ, 31, 248)
    _check(occ, 3, 9)


def test_three_maps_in_one_call():
    occ = np.stack([_random(TW + 3, 2 * TH + 1, s, p) for s, p in ((2, 0.03), (3, 0.0), (4, 0.2))])
    _check(occ, 9, 120)


def test_evidence_form():
    """solid = e >= t_occ: cells at t_occ - 1, t_occ, INT32_MIN and INT32_MAX; unknown cells (0) are no sources."""
    W, H, t_occ = TW + 3, TH + 3, 5
    rng = np.random.default_rng(6)
    ev = rng.integers(-3, 3, (2, W, H)).astype(np.int32)
    for m in range(2):
        cells = rng.integers(0, (W, H), (12, 2))
        for n, (i, j) in enumerate(cells):
            ev[m, i, j] = (t_occ - 1, t_occ, np.iinfo(np.int32).min, np.iinfo(np.int32).max)[n % 4]
    got = _call(6, 77, ev=ev, t_occ=t_occ)
    want = np.stack([CO.clearance_cost_evidence(e, t_occ, 6, 77) for e in ev])
    assert np.array_equal(got, want) and (got == 77).sum() == int((ev >= t_occ).sum()) > 0
    assert (got[ev == t_occ - 1] < 77).all() and (got[ev == np.iinfo(np.int32).min] < 77).all()
    # the largest threshold
    assert np.array_equal(_call(6, 77, ev=ev, t_occ=1 << 30), np.stack([CO.clearance_cost_evidence(e, 1 << 30, 6, 77) for e in ev]))


def test_the_planners_make_the_same_layer():
    occ = _random(TW + 3, TH + 3, 1)
    want = CO.clearance_cost(occ != 0, 4, 40)
    pl = lipmpc.GridFieldPlanner(tiled=True, r_clear=4, w_clear=40)
    got = pl.clearance_cost(lipmpc.GridMap(occ, (0.0, 0.0), 0.1))
    assert got.shape == (1,) + occ.shape and np.array_equal(got[0].cpu().numpy(), want)
    ev = torch.as_tensor(np.where(occ != 0, 3, -1).astype(np.int32), device="cuda")
    fp = lipmpc.FrontierPlanner(t_free=1, t_occ=3, tiled=True, r_clear=4, w_clear=40)
    assert np.array_equal(fp.clearance_cost(ev)[0].cpu().numpy(), want)
    with pytest.raises(ValueError, match="r_clear"):
        lipmpc.GridFieldPlanner(tiled=True).clearance_cost(lipmpc.GridMap(occ, (0.0, 0.0), 0.1))


def test_graph_replay():
    occ = np.stack([_random(TW + 3, TH + 3, 8), _random(TW + 3, TH + 3, 9)])
    want = np.stack([CO.clearance_cost(m != 0, 7, 248) for m in occ])
    dev = torch.as_tensor(occ, device="cuda")
    cost = torch.full(occ.shape, POISON, dtype=torch.uint8, device="cuda")

    def call():
        lipmpc._lib.call("lipmpc_grid_clearance_cost_batch", device=0, M=2, W=occ.shape[1], H=occ.shape[2], occ=dev, evidence=None, t_occ=0,
                         r_clear=7, w_clear=248, cost=cost, hip_stream=torch.cuda.current_stream().cuda_stream)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        cost.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(cost.cpu().numpy(), want)
