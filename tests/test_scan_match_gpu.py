"""GPU: correlative scan matching (lipmpc_scan_match_batch, lipmpc.ScanMatcher) against the numpy restatement of the header's
contract (tests/scan_match_oracle.py): every output bit for bit, written into poisoned buffers.  The readings come from the grid
scan's oracle on the CPU, and the evidence is handed to the mapper as it is: the oracle is fed the very numbers the kernel reads."""
import numpy as np
import pytest

import scan_match_cases as K
import scan_match_oracle as S

pytestmark = pytest.mark.gpu

NAMES = ("offset_cells", "yaw_index", "offset", "score", "n_used", "matched")


def _poisoned(torch, matcher, B):
    out = matcher.alloc_outputs(B, torch.device("cuda", torch.cuda.current_device()))
    for name, t in out.items():
        t.fill_(float("nan") if t.dtype == torch.float64 else 0x5A)
    return out


def _equal(got, want, tag):
    for name in NAMES:
        g, w = got[name].cpu().numpy(), want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape)
        bad = np.argwhere(g.view(np.int64 if g.dtype == np.float64 else g.dtype) != w.view(np.int64 if w.dtype == np.float64 else w.dtype))
        assert len(bad) == 0, (tag, name, len(bad), bad[:4], g[tuple(bad[0])], w[tuple(bad[0])])


def _run(torch, lipmpc, evidence, pos, hits, *, origin, cell, n, lidar_range=K.RANGE, depth=None, clamp=8, min_score=1, min_gain=0,
         n_yaw=0, yaw_step=None, mask=None, tag=""):
    """One call on ``evidence`` ([W,H] shared, [B,W,H] per robot) against the oracle; returns the oracle's outputs."""
    B, Rr = hits.shape[:2]
    per = evidence.ndim == 3
    W, H = evidence.shape[-2:]
    mapper = lipmpc.OccupancyMapper(W, H, origin, cell, lidar_range, Rr, per_robot=B if per else None, depth=depth)
    mapper.evidence.copy_(torch.as_tensor(evidence.astype(np.int32)))
    matcher = lipmpc.ScanMatcher(n[0], n[1], clamp=clamp, min_score=min_score, min_gain=min_gain, n_yaw=n_yaw, yaw_step=yaw_step)
    st = np.zeros((B, 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    d_mask = None if mask is None else torch.as_tensor(mask, dtype=torch.int32, device="cuda")
    out = _poisoned(torch, matcher, B)
    got = matcher.match(mapper, torch.as_tensor(st, device="cuda"), torch.as_tensor(hits, device="cuda"), d_mask, out=out)
    torch.cuda.synchronize()
    assert got is out
    want = S.match(pos, hits, evidence, origin, mapper.cell, lidar_range, mapper.depth, n[0], n[1], clamp, min_score, min_gain, n_yaw=n_yaw,
                   yaw_step=yaw_step, mask=mask, rot=matcher.rot)
    _equal(got, want, tag)
    assert torch.equal(mapper.evidence.cpu(), torch.as_tensor(evidence.astype(np.int32)))      # read only
    return want


def _room_queries(rng, B, R, spread=0.1, shift=4):
    """B believed poses near the mapped line of the room, displaced by whole cells, with their readings (R rays, noisy)."""
    import map_oracle as M
    import lipmpc
    base = K.mapped_poses()[rng.integers(0, 12, B)] + rng.uniform(-spread, spread, (B, 2))
    hits = M.oracle_hits(base, K.room(), K.ORIGIN, K.CELL, K.RANGE, lipmpc.ray_table(R), 0.01 * rng.standard_normal((B, R, 2)))
    d = rng.integers(-shift, shift + 1, (B, 2)) * np.array(K.CELL)
    return base + d, hits + d[:, None, :]


@pytest.mark.parametrize("R", [1, 7, 90, 384])
@pytest.mark.parametrize("n", [(0, 0), (1, 0), (4, 4), (16, 16), (16, 3)])
def test_gpu_match_equals_the_oracle_in_the_room(R, n):
    """The room's evidence (48 x 40, what 12 scans along a line leave), 12 displaced noisy scans per case, a shared map."""
    torch = pytest.importorskip("torch")
    import lipmpc
    rng = np.random.default_rng(100 * R + 7 * n[0] + n[1])
    pos, hits = _room_queries(rng, 12, R)
    want = _run(torch, lipmpc, np.array(K.line_evidence()), pos, hits, origin=K.ORIGIN, cell=K.CELL, n=n, tag=(R, n))
    if R >= 90:
        assert want["n_used"].min() > 10 and (n[1] < 4 or want["matched"].sum() >= 4), want


@pytest.mark.parametrize("n_yaw", [0, 2, 16])
def test_gpu_match_with_yaws_on_random_evidence(n_yaw):
    """Evidence drawn at random in +-40 (clamp 20: both sides clamp), so that no two candidates tie by accident and every
    rotated cell matters; per-robot maps; R = 90; shifts of +-3 and yaw steps of 0.02."""
    torch = pytest.importorskip("torch")
    import lipmpc
    rng = np.random.default_rng(40 + n_yaw)
    B = 10
    pos, hits = _room_queries(rng, B, K.R)
    ev = rng.integers(-40, 41, (B, K.W, K.H))
    want = _run(torch, lipmpc, ev, pos, hits, origin=K.ORIGIN, cell=K.CELL, n=(3, 3), clamp=20, min_score=-10 ** 6, n_yaw=n_yaw,
                yaw_step=0.02, tag=n_yaw)
    if n_yaw:
        assert len(np.unique(want["yaw_index"])) >= 3 and want["matched"].all()


@pytest.mark.parametrize("shape", [(48, 40), (1, 40), (1, 1)])
def test_gpu_match_at_the_edges_of_the_map(shape):
    """Robots on the map's border and outside it on each side (the window leaves the map), dx != dy, an origin at 1e6, NaN readings,
    a NaN position, a position without a cell, masked robots; per-robot and shared maps; maps of 48 x 40, 1 x 40 and 1 x 1."""
    torch = pytest.importorskip("torch")
    import lipmpc
    import map_oracle as M
    Wm, Hm = shape
    rng = np.random.default_rng(Wm + Hm)
    cell, origin, R = (0.1, 0.07), (1e6, -3.0), 90
    lo, hi = np.array(origin), np.array(origin) + np.array(cell) * (Wm, Hm)
    B = 20
    pos = rng.uniform(lo - 1.2, hi + 1.2, (B, 2))
    mid = 0.5 * (lo + hi)
    pos[0], pos[1], pos[2], pos[3] = (lo[0], mid[1]), (hi[0], mid[1]), (mid[0], lo[1] - 1e-9), (mid[0], hi[1])
    pos[4], pos[5], pos[6], pos[7] = (lo[0] - 0.9, mid[1]), (hi[0] + 0.9, mid[1]), (mid[0], lo[1] - 0.9), (mid[0], hi[1] + 0.9)
    pos[8], pos[9] = mid, mid + 0.01
    # readings: a ring of walls around every robot, noisy, some missing
    ang = np.linspace(0.0, 2.0 * np.pi, R, endpoint=False)
    rad = rng.uniform(0.2, 1.5, (B, R))
    hits = pos[:, None, :] + rad[:, :, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)[None]
    hits[rng.random((B, R)) < 0.2] = np.nan
    hits[9, 3, 1] = np.nan
    hits[9, 4] = pos[9]                                    # a reading on the robot: L == 0
    pos[10, 0] = np.nan
    pos[11, 1] = 1e300
    mask = np.ones(B, np.int32); mask[12] = 0; mask[13] = 0
    for per in (False, True):
        ev = rng.integers(-30, 31, (B, Wm, Hm) if per else (Wm, Hm))
        want = _run(torch, lipmpc, ev, pos, hits, origin=origin, cell=cell, n=(4, 5), clamp=9, min_score=-10 ** 6, mask=mask,
                    n_yaw=1, yaw_step=0.02, depth=0.031, tag=(shape, per))
        for name in NAMES:
            assert not want[name][10:14].any(), name
        assert want["n_used"][:10].min() > 20
        if shape == (48, 40):
            assert want["matched"].sum() >= 8


@pytest.mark.parametrize("B", [1, 65, 300])
def test_gpu_match_batch_sizes(B):
    torch = pytest.importorskip("torch")
    import lipmpc
    rng = np.random.default_rng(B)
    pos, hits = _room_queries(rng, B, 24, shift=2)
    ev = np.array(K.line_evidence()) + rng.integers(-2, 3, (K.W, K.H))
    _run(torch, lipmpc, ev, pos, hits, origin=K.ORIGIN, cell=K.CELL, n=(2, 2), tag=B)


def test_gpu_match_acceptance_and_clamp():
    """The thresholds either side of what the scans score, and clamp 1 and 127 on evidence of +-100000."""
    torch = pytest.importorskip("torch")
    import lipmpc
    rng = np.random.default_rng(9)
    pos, hits = _room_queries(rng, 16, K.R)
    ev = np.array(K.line_evidence())
    base = _run(torch, lipmpc, ev, pos, hits, origin=K.ORIGIN, cell=K.CELL, n=(5, 5), min_score=-10 ** 6)
    best, gain = base["score"][:, 0], base["score"][:, 0] - base["score"][:, 1]
    for kw in (dict(min_score=int(np.median(best))), dict(min_score=int(np.median(best)) + 1), dict(min_gain=int(np.median(gain))),
               dict(min_gain=int(np.median(gain)) + 1), dict(min_score=2 ** 31 - 1), dict(min_score=-2 ** 31, min_gain=2 ** 31 - 1)):
        want = _run(torch, lipmpc, ev, pos, hits, origin=K.ORIGIN, cell=K.CELL, n=(5, 5), **{**dict(min_score=-10 ** 6), **kw})
        assert np.array_equal(want["score"], base["score"]) and want["matched"].sum() < base["matched"].sum(), kw
    big = np.where(ev > 0, 100000, np.where(ev < 0, -100000, 0))
    for clamp in (1, 127):
        want = _run(torch, lipmpc, big, pos, hits, origin=K.ORIGIN, cell=K.CELL, n=(5, 5), clamp=clamp, tag=clamp)
        assert np.abs(want["score"]).max() > 20 * clamp and (want["score"] % clamp == 0).all()


def test_gpu_match_largest_window_and_its_refusal():
    """Range 5.0 on cells of 0.05 with n = 8: a grown window of 221 x 221 = 48841 cells, the largest that fits; n_x = 9 is refused."""
    torch = pytest.importorskip("torch")
    import lipmpc
    rng = np.random.default_rng(21)
    Wm, Hm, cell, origin, R, B = 300, 260, (0.05, 0.05), (-1.0, 2.0), 48, 6
    assert S.grown_window(5.0, 0.0, cell, 8, 8) == (221, 221) and not S.window_fits(5.0, 0.0, cell, 9, 8)
    pos = rng.uniform((0.0, 3.0), (13.0, 14.0), (B, 2))
    pos[0], pos[1] = (-1.0 - 4.0, 2.0 - 4.0), (14.0 + 4.9, 15.0 + 4.9)       # only a corner of the window meets the map
    ang = np.linspace(0.0, 2.0 * np.pi, R, endpoint=False)
    hits = pos[:, None, :] + rng.uniform(0.3, 5.0, (B, R))[:, :, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)[None]
    ev = rng.integers(-20, 21, (Wm, Hm))
    want = _run(torch, lipmpc, ev, pos, hits, origin=origin, cell=cell, n=(8, 8), lidar_range=5.0, depth=0.0, clamp=15, min_score=-10 ** 6)
    assert want["matched"][2:].all()
    mapper = lipmpc.OccupancyMapper(Wm, Hm, origin, cell, 5.0, R, depth=0.0)
    st = torch.zeros((B, 5), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError) as e:
        lipmpc.ScanMatcher(9, 8, clamp=15, min_score=0, min_gain=0).match(mapper, st, torch.as_tensor(hits, device="cuda"))
    assert e.value.code == -2


def test_gpu_match_twice_and_in_a_graph():
    """Two calls give identical bits; a call captured in a graph and replayed after the evidence changed matches the new evidence."""
    torch = pytest.importorskip("torch")
    import lipmpc
    rng = np.random.default_rng(33)
    B = 16
    pos, hits = _room_queries(rng, B, K.R)
    ev0 = np.array(K.line_evidence())
    ev1 = np.roll(ev0, (2, -1), axis=(0, 1))
    mapper = lipmpc.OccupancyMapper(K.W, K.H, K.ORIGIN, K.CELL, K.RANGE, K.R)
    matcher = lipmpc.ScanMatcher(5, 5, clamp=8, min_score=1, min_gain=0, n_yaw=1, yaw_step=0.02)
    st = np.zeros((B, 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    d_st, d_hits = torch.as_tensor(st, device="cuda"), torch.as_tensor(hits, device="cuda")
    okw = dict(n_yaw=1, rot=matcher.rot)
    oracle = lambda ev: S.match(pos, hits, ev, K.ORIGIN, K.CELL, K.RANGE, mapper.depth, 5, 5, 8, 1, 0, **okw)
    mapper.evidence.copy_(torch.as_tensor(ev0.astype(np.int32)))
    a, b = matcher.match(mapper, d_st, d_hits), matcher.match(mapper, d_st, d_hits, out=_poisoned(torch, matcher, B))
    torch.cuda.synchronize()
    for name in NAMES:
        assert torch.equal(a[name], b[name]), name
    _equal(a, oracle(ev0), "eager")
    out = _poisoned(torch, matcher, B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        matcher.match(mapper, d_st, d_hits, out=out)         # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            matcher.match(mapper, d_st, d_hits, out=out)
        mapper.evidence.copy_(torch.as_tensor(ev1.astype(np.int32)).to("cuda"))
        for t in out.values():
            t.fill_(float("nan") if t.dtype == torch.float64 else 0x5A)
        graph.replay()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want0, want1 = oracle(ev0), oracle(ev1)
    assert not np.array_equal(want0["offset_cells"], want1["offset_cells"])
    _equal(out, want1, "replayed")
