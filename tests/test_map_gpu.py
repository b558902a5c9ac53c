"""GPU: scans integrated into an evidence grid (lipmpc_map_update_batch, lipmpc.OccupancyMapper) against the numpy restatement of
the header's contract (tests/map_oracle.py), integer for integer.  The readings are the device's own (grid scan, polygon scan):
the oracle is fed the very doubles the kernel read."""
import numpy as np
import pytest

import grid_lidar_oracle as G
import map_oracle as M

pytestmark = pytest.mark.gpu

RANGE, CELL = 1.5, (0.05, 0.05)


def _states(torch, pos):
    st = np.zeros((len(pos), 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    return torch.as_tensor(st, device="cuda")


def _hits(torch, lipmpc, occ, origin, cell, pos, noise=None, resolution=360, lidar_range=RANGE):
    """The device's own grid scan of ``pos``: (state, hits) device tensors."""
    sensor = lipmpc.LidarSensor.from_grid(lipmpc.GridMap(occ, origin, cell), lidar_range=lidar_range, resolution=resolution,
                                          n_obs_max=24, v_max=64)
    st = _states(torch, pos)
    out = sensor.sense(st, None if noise is None else torch.as_tensor(noise, device="cuda"), with_debug=True, c_eta=True)
    return st, out["hits"]


def _both(torch, lipmpc, W, H, origin, cell, st, hits, pos, resolution=360, mask=None, lidar_range=RANGE, **kw):
    """Per-robot and shared maps of one update against the oracle; returns the shared evidence (numpy)."""
    B = len(pos)
    table = lipmpc.ray_table(resolution)
    h = hits.cpu().numpy()
    d_mask = None if mask is None else torch.as_tensor(mask, dtype=torch.int32, device="cuda")
    per = lipmpc.OccupancyMapper(W, H, origin, cell, lidar_range, resolution, per_robot=B, **kw)
    sh = lipmpc.OccupancyMapper(W, H, origin, cell, lidar_range, resolution, **kw)
    e_per, e_sh = per.update(st, hits, d_mask), sh.update(st, hits, d_mask)
    torch.cuda.synchronize()
    assert e_per.dtype == torch.int32 and tuple(e_per.shape) == (B, W, H) and tuple(e_sh.shape) == (W, H)
    okw = dict(depth=per.depth, w_hit=per.w_hit, w_miss=per.w_miss, mask=mask)
    want = M.update(np.zeros((B, W, H), np.int64), pos, h, origin, per.cell, lidar_range, table, **okw)
    got = e_per.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(e_sh.cpu().numpy(), want.sum(0))
    return want


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("case", ["fixture", "random"])
def test_gpu_evidence_equals_the_oracle(case, noisy):
    """48 robots, range 1.5, cells of 0.05, an evidence grid of 96 x 80 cells whose origin is not the true map's (some robots'
    windows are clipped by it, some lie outside): per-robot and shared evidence equal the oracle's integers."""
    torch = pytest.importorskip("torch")
    import lipmpc
    rng = np.random.default_rng(11 if case == "fixture" else 12)
    if case == "fixture":
        fx = G.fixture(n_robots=48)
        occ, origin, pos = fx["occ"], fx["origin"], fx["pos"]
        ev_origin = (1.013, 0.77)
    else:
        occ, origin = (rng.random((140, 150)) < 0.03).astype(np.uint8), (0.3, -0.2)
        pos = rng.uniform((0.8, 0.3), (6.8, 6.9), (48, 2))
        ev_origin = (1.487, 0.512)
    noise = 0.01 * rng.standard_normal((48, 360, 2)) if noisy else None
    st, hits = _hits(torch, lipmpc, occ, origin, CELL, pos, noise)
    want = _both(torch, lipmpc, 96, 80, ev_origin, CELL, st, hits, pos)
    touched = (want != 0).any(axis=(1, 2))
    print(f"{case} noisy={noisy}: {int(touched.sum())} robots touch the grid, {int((want > 0).sum())} hit cells, {int((want < 0).sum())} passed cells")
    assert touched.sum() >= 24 and not touched.all() and (want > 0).sum() > 100 and (want < 0).sum() > 20000


@pytest.mark.parametrize("resolution", [1, 7, 384])
def test_gpu_evidence_variants(resolution):
    """Cells of 0.05 x 0.08, W and H no multiples of 32; robots on the grid's border and outside it; a NaN state and a masked
    robot; other weights and depth; 1, 7 and 384 rays."""
    torch = pytest.importorskip("torch")
    import lipmpc
    rng = np.random.default_rng(20 + resolution)
    cell, origin, W, H = (0.05, 0.08), (-0.4, 0.3), 77, 45
    occ = (rng.random((W, H)) < 0.03).astype(np.uint8)
    lo, hi = np.array(origin), np.array(origin) + np.array(cell) * (W, H)
    B = 24
    pos = rng.uniform(lo - 1.0, hi + 1.0, (B, 2))
    pos[0], pos[1], pos[2], pos[3] = (lo[0], 1.0), (hi[0], 2.0), (1.0, lo[1] - 1e-9), (hi[0] + 0.7, hi[1] + 0.7)
    pos[4], pos[5] = (1.1, 1.3), (2.0, 2.0)
    noise = 0.01 * rng.standard_normal((B, resolution, 2))
    st, hits = _hits(torch, lipmpc, occ, origin, cell, pos, noise, resolution)
    st[4, 0] = float("nan")
    pos[4, 0] = np.nan
    mask = np.ones(B, np.int32); mask[5] = 0
    want = _both(torch, lipmpc, W, H, origin, cell, st, hits, pos, resolution, mask=mask, w_hit=7, w_miss=2, depth=0.031)
    assert not want[4].any() and not want[5].any() and (want != 0).any(axis=(1, 2)).sum() >= 10
    assert set(np.unique(want)) <= {-2, 0, 7}


def test_gpu_window_over_the_cap_is_refused():
    torch = pytest.importorskip("torch")
    import lipmpc
    mp = lipmpc.OccupancyMapper(64, 64, (0.0, 0.0), 0.05, lidar_range=5.5, resolution=8, depth=0.0)
    st, hits = torch.zeros((2, 5), dtype=torch.float64, device="cuda"), torch.zeros((2, 8, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError) as e:
        mp.update(st, hits)
    assert e.value.code == -2
    lipmpc.OccupancyMapper(64, 64, (0.0, 0.0), 0.05, lidar_range=5.4, resolution=8, depth=0.0).update(st, hits)      # 221 x 221 cells: fits
    torch.cuda.synchronize()


def test_gpu_linearity_determinism_and_graph_capture():
    """Two identical shared-map calls from zero give identical bits; two updates in a row are exactly twice one; an update
    captured in a graph on a side stream and replayed 3 times equals 3 eager updates."""
    torch = pytest.importorskip("torch")
    import lipmpc
    fx = G.fixture(n_robots=48)
    st, hits = _hits(torch, lipmpc, fx["occ"], fx["origin"], CELL, fx["pos"], 0.01 * np.random.default_rng(5).standard_normal((48, 360, 2)))
    new = lambda **kw: lipmpc.OccupancyMapper(150, 150, (0.0, 0.0), CELL, RANGE, **kw)
    a, b = new(), new()
    one = a.update(st, hits).clone()
    assert torch.equal(one, b.update(st, hits)) and int(one.abs().sum()) > 0
    assert torch.equal(a.update(st, hits), 2 * one)
    a.reset()
    assert not a.evidence.any()
    for kw in (dict(), dict(per_robot=48)):
        eager, cap = new(**kw), new(**kw)
        for _ in range(3):
            eager.update(st, hits)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            cap.update(st, hits)                             # warm-up outside the capture
            cap.reset()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                cap.update(st, hits)
            for _ in range(3):
                graph.replay()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(eager.evidence, cap.evidence) and int(eager.evidence.abs().sum()) > 0
        if not kw:
            assert torch.equal(eager.evidence, 3 * one)


def test_gpu_polygon_sensor_readings_map_the_same_way():
    """Readings of the polygon scan (LidarSensor(env_rings).sense(with_debug=True)), noisy: they lie anywhere, not on cell faces."""
    torch = pytest.importorskip("torch")
    import lipmpc
    fx = G.fixture(n_robots=8)
    sensor = lipmpc.LidarSensor(fx["rings"], lidar_range=RANGE, n_obs_max=24, v_max=64)
    st = _states(torch, fx["pos"])
    noise = torch.as_tensor(0.01 * np.random.default_rng(6).standard_normal((8, 360, 2)), device="cuda")
    hits = sensor.sense(st, noise, with_debug=True)["hits"]
    want = _both(torch, lipmpc, 170, 165, (-0.2, -0.1), CELL, st, hits, fx["pos"])
    assert (want > 0).sum() > 100
