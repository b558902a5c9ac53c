"""GPU: the sector split of the scans (lipmpc_lidar_c_eta_split_batch / lipmpc_lidar_grid_c_eta_split_batch, LidarSensor(split_rays=)).
Pieces, n_inferred, overflow and rings against tests/lidar_split_oracle.py fed the device's own hits, bit for bit; (c, eta) as the
other LiDAR tests hold it: within 1e-12 of oracle/lipmpc_oracle.py::closest_point_and_normal on the oracle's ring."""
import numpy as np
import pytest

import grid_lidar_oracle as G
import lidar_oracle as L
import lidar_split_oracle as S
from lidar_grid_checks import same_ring

pytestmark = pytest.mark.gpu

SPLITS = {360: (1, 2, 7, 30, 45, 180), 384: (1, 2, 7, 30, 45, 192), 90: (1, 2, 7, 30, 45)}      # 45 = R / 2 at R = 90


def _states(torch, pos):
    st = np.zeros((len(pos), 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    return torch.as_tensor(st, device="cuda")


def _scan(torch, sensor, pos, noise, **kw):
    out = sensor.sense(_states(torch, pos), None if noise is None else torch.as_tensor(noise, device="cuda"), with_debug=True, c_eta=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sensor(lipmpc, kind, fx, split, R=360, n_obs_max=24, v_max=64, occ=None, lidar_range=None):
    rng_ = fx["lidar_range"] if lidar_range is None else lidar_range
    if kind == "grid":
        grid = lipmpc.GridMap(fx["occ"] if occ is None else occ, fx["origin"], fx["cell"])
        return lipmpc.LidarSensor.from_grid(grid, lidar_range=rng_, resolution=R, n_obs_max=n_obs_max, v_max=v_max, split_rays=split)
    return lipmpc.LidarSensor(fx["rings"], lidar_range=rng_, resolution=R, n_obs_max=n_obs_max, v_max=v_max, split_rays=split)


def _nearly_in_line(pts):
    """A piece the oracle's rank test calls collinear although its points are not EXACTLY in line: noise-free readings of the
    polygon scan on an axis-parallel edge leave the line by a rounding (tests/test_lidar_grid_gpu.py says where and how often); the
    kernel's exact extreme-point count then keeps a ring 1e-16 wide that the oracle drops.  That is the unsplit polygon kernel's
    behaviour too, and no matter of the split: such scans are compared up to their pieces."""
    u = np.unique(pts, axis=0)
    if len(u) < 3 or L.hull_ring(pts) is not None:
        return False
    return not (np.all(u[:, 0] == u[0, 0]) or np.all(u[:, 1] == u[0, 1]))


def _check(g, pos, split, n_obs_max, v_max, skip_nearly_in_line=False):
    """One launch against the oracle.  Returns counts: pieces, rings compared, scans with more than 64 pieces, scans that
    overflowed the slots only, pieces that took no slot, scans skipped as nearly in line."""
    import lipmpc_oracle as O
    cnt = dict(pieces=0, rings=0, over64=0, slots=0, dropped=0, skipped=0, split_clusters=0)
    for b in range(len(pos)):
        valid = ~np.isnan(g["hits"][b, :, 0])
        sc = S.split_scan(g["hits"][b], valid, split, n_obs_max, v_max)
        assert np.array_equal(g["labels"][b], sc["labels"]), b
        assert np.array_equal(g["pieces"][b], sc["pieces"]), (b, split)
        cnt["pieces"] += sc["n_pieces"]
        cnt["split_clusters"] += int(sc["n_pieces"] - (sc["labels"].max() + 1 if valid.any() else 0))
        if skip_nearly_in_line and any(_nearly_in_line(g["hits"][b][sc["pieces"] == k]) for k in range(sc["n_pieces"])):
            cnt["skipped"] += 1
            continue
        assert g["overflow"][b] == sc["overflow"], (b, split, sc["n_pieces"])
        if sc["rings"] is None:
            cnt["over64"] += 1
            continue
        cnt["slots"] += sc["overflow"]
        n = len(sc["rings"])
        assert g["n_inferred"][b] == n, (b, split, g["n_inferred"][b], n)
        assert not g["obs_nv"][b, n:].any() and not g["c_eta"][b, n:].any()
        cnt["dropped"] += sc["n_pieces"] - n if not sc["overflow"] else 0
        for j, ring in enumerate(sc["rings"]):
            assert same_ring(g["obs_xy"][b, j, : g["obs_nv"][b, j]], ring), (b, j)
            c, eta, _, degen = O.closest_point_and_normal(pos[b], ring)
            if not degen:
                assert np.max(np.abs(g["c_eta"][b, j, :2] - c)) < 1e-12 and np.max(np.abs(g["c_eta"][b, j, 2:] - eta)) < 1e-12, (b, j)
            cnt["rings"] += 1
    return cnt


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("kind", ["grid", "ring"])
@pytest.mark.parametrize("R", [360, 384, 90])
def test_gpu_split_scans_equal_the_oracle(R, kind, noisy):
    """The 60 robots of the grid fixture through the grid sensor and the ring sensor, with seeded noise and without, at every
    split_rays of the list: pieces, overflow, n_inferred and rings bit for bit.  split_rays = 1 makes more than 64 pieces of most
    scans (flag only), 2 makes pieces of two readings (no slot), R / 2 leaves most clusters whole."""
    torch = pytest.importorskip("torch")
    import lipmpc
    fx = G.fixture()
    pos = fx["pos"]
    noise = 0.01 * np.random.default_rng(R).standard_normal((len(pos), R, 2)) if noisy else None
    total = dict()
    for split in SPLITS[R]:
        g = _scan(torch, _sensor(lipmpc, kind, fx, split, R), pos, noise)
        cnt = _check(g, pos, split, 24, 64, skip_nearly_in_line=(kind == "ring" and not noisy))
        print(f"R {R} {kind} noisy {noisy} split {split}: {cnt}")
        for k, v in cnt.items():
            total[k] = total.get(k, 0) + v
    # (that the comparison had something to compare: at least a ring per robot over the splits -- a noise-free scan of
    # axis-parallel boxes has a ring only where a piece goes round a corner, and split_rays 1 and 2 never give one)
    assert total["rings"] >= len(pos) and total["over64"] > 0 and total["dropped"] > 0 and total["split_clusters"] > 100
    assert total["skipped"] <= (len(SPLITS[R]) * len(pos)) // 2


def test_gpu_split_on_both_clustering_routes():
    """Scans that cluster by chains of consecutive readings and scans that take the general route (the fixture's walls plus
    scattered single cells, as tests/test_lidar_grid_gpu.py obtains either): the split stage behind both."""
    torch = pytest.importorskip("torch")
    import lipmpc
    from test_lidar_chain_rules import chain_labels
    rng = np.random.default_rng(303)
    fx = G.fixture()
    occ = fx["occ"] | (rng.random(fx["occ"].shape) < 0.004).astype(np.uint8)
    B = 96
    pos = rng.uniform(-0.5, 8.5, (B, 2))
    pos = pos[[not G.in_solid_cell(p, occ, fx["origin"], fx["cell"]) for p in pos]]
    noise = 0.01 * rng.standard_normal((len(pos), 360, 2))
    for split in (7, 30):
        g = _scan(torch, _sensor(lipmpc, "grid", fx, split, occ=occ), pos, noise)
        cnt = _check(g, pos, split, 24, 64)
        assert cnt["rings"] > len(pos) // 4 and cnt["split_clusters"] > 0
    scans = [g["hits"][b][~np.isnan(g["hits"][b, :, 0])] for b in range(len(pos))]
    by_chain = [chain_labels(p, 0.3, 3) is not None for p in scans if len(p)]
    print(f"{sum(by_chain)} scans by chains, {len(by_chain) - sum(by_chain)} by rows")
    assert sum(by_chain) > 0 and len(by_chain) - sum(by_chain) > 0


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("kind", ["grid", "ring"])
def test_gpu_split_off_is_the_parent(kind):
    """split_rays = 0 through the split entry points (reached by handing in a ``pieces`` buffer) equals the parent entry points
    bit for bit, pieces = labels; and split_rays = R / 2 changes nothing on a scan whose clusters all span at most R / 2 rays."""
    torch = pytest.importorskip("torch")
    import lipmpc
    fx = G.fixture()
    pos, R = fx["pos"], 360
    noise = 0.01 * np.random.default_rng(8).standard_normal((len(pos), R, 2))
    off = _sensor(lipmpc, kind, fx, 0)
    parent = _scan(torch, off, pos, noise)
    assert "pieces" not in parent
    out = off.alloc_outputs(len(pos), with_debug=True, c_eta=True)
    out["pieces"] = torch.full((len(pos), R), 77, dtype=torch.int32, device="cuda")
    twin = _scan(torch, off, pos, noise, out=out)
    for k in parent:
        assert _eq(parent[k], twin[k]), k
    assert _eq(twin["pieces"], twin["labels"])
    half = _scan(torch, _sensor(lipmpc, kind, fx, R // 2), pos, noise)
    def extent(rays):                                                    # consecutive rays a cluster covers, cyclically
        return 1 if len(rays) == 1 else R - max((rays[t] - rays[t - 1]) % R for t in range(len(rays))) + 1

    small = np.array([all(extent(np.nonzero(lab == k)[0]) <= R // 2 for k in range(lab.max() + 1)) for lab in parent["labels"]])
    assert small.sum() > len(pos) // 2
    for k in parent:
        if k != "obs_xy":
            assert _eq(parent[k][small], half[k][small]), k
    assert _eq(half["pieces"][small], half["labels"][small])
    for b in np.nonzero(small)[0]:                                       # (vertex slots beyond obs_nv hold whatever)
        for j in range(parent["n_inferred"][b]):
            n = parent["obs_nv"][b, j]
            assert _eq(parent["obs_xy"][b, j, :n], half["obs_xy"][b, j, :n])


def _room(n=40, cell=0.1):
    occ = np.zeros((n, n), np.uint8)
    occ[:2, :] = occ[-2:, :] = 1
    occ[:, :2] = occ[:, -2:] = 1
    return dict(occ=occ, origin=(0.0, 0.0), cell=(cell, cell), rings=None, lidar_range=4.5)


def _sides(g, pos, b=0):
    """eta . (p0 - c) of every slot in use."""
    n = g["n_inferred"][b]
    ce = g["c_eta"][b, :n]
    return (ce[:, 2] * (pos[b, 0] - ce[:, 0]) + ce[:, 3] * (pos[b, 1] - ce[:, 1]))


def test_gpu_closed_room_robot_inside():
    """A closed room, the robot inside, every ray hits, one cluster: the anchor is ray 0.  Noise-free at split_rays = 45 every
    slot's half-space has the robot on its free side; with splitting off the one hull holds the robot and its row is flipped --
    the defect.  split_rays = 1: 360 pieces, overflow = 1 and nothing else asserted; few slots: overflow of n_obs_max alone."""
    torch = pytest.importorskip("torch")
    import lipmpc
    room = _room()
    pos = np.array([[1.73, 2.21]])
    R = 360
    off = _scan(torch, _sensor(lipmpc, "grid", room, 0), pos, None)
    assert (off["labels"][0] == 0).all()                                 # every ray hits, one cluster
    assert off["n_inferred"][0] == 1 and _sides(off, pos)[0] < 0.0        # the defect: the robot is inside the one hull
    on = _scan(torch, _sensor(lipmpc, "grid", room, 45), pos, None)
    assert on["pieces"][0].tolist() == [r * 8 // R for r in range(R)]    # anchored at ray 0, eight pieces of 45 rays
    cnt = _check(on, pos, 45, 24, 64)
    assert on["overflow"][0] == 0 and on["n_inferred"][0] >= 4 and np.all(_sides(on, pos) > 0.0), _sides(on, pos)
    noisy = _scan(torch, _sensor(lipmpc, "grid", room, 45), pos, 0.01 * np.random.default_rng(2).standard_normal((1, R, 2)))
    _check(noisy, pos, 45, 24, 64)
    assert noisy["n_inferred"][0] == 8 and np.all(_sides(noisy, pos) > 0.0)
    # more than 64 pieces: the flag, and no fault (the next launch runs and is right)
    many = _scan(torch, _sensor(lipmpc, "grid", room, 1), pos, None)
    assert many["overflow"][0] == 1 and many["pieces"][0].tolist() == list(range(R))
    again = _scan(torch, _sensor(lipmpc, "grid", room, 45), pos, None)
    assert _eq(again["c_eta"], on["c_eta"])
    # eight pieces, four slots: overflow of n_obs_max alone; the first four committed pieces hold the slots
    few = _scan(torch, _sensor(lipmpc, "grid", room, 45, n_obs_max=4), pos, 0.01 * np.random.default_rng(2).standard_normal((1, R, 2)))
    cnt = _check(few, pos, 45, 4, 64)
    assert few["overflow"][0] == 1 and few["n_inferred"][0] == 4 and cnt["slots"] == 1 and cnt["over64"] == 0
    assert _eq(few["c_eta"][0], noisy["c_eta"][0, :4])
    # ... and of v_max alone: hulls of noisy walls with more vertices than the slots hold
    thin = _scan(torch, _sensor(lipmpc, "grid", room, 180, v_max=3), pos, 0.01 * np.random.default_rng(2).standard_normal((1, R, 2)))
    _check(thin, pos, 180, 24, 3)
    assert thin["overflow"][0] == 1


def test_gpu_cluster_across_ray_zero_and_dropped_pieces():
    """One box on the robot's +x side: its cluster straddles ray 0, the anchor is its first ray BELOW ray 0 (the largest gap lies in
    front of it), the pieces are numbered from there.  Pieces of fewer than 3 readings take no slot."""
    torch = pytest.importorskip("torch")
    import lipmpc
    occ = np.zeros((60, 60), np.uint8)
    occ[40:44, 20:40] = 1
    fx = dict(occ=occ, origin=(0.0, 0.0), cell=(0.05, 0.05), rings=None, lidar_range=1.5)
    pos = np.array([[1.0, 1.52]])
    noise = 0.01 * np.random.default_rng(4).standard_normal((1, 360, 2))
    g = _scan(torch, _sensor(lipmpc, "grid", fx, 7), pos, noise)
    lab, pc = g["labels"][0], g["pieces"][0]
    assert lab[0] == 0 and lab[359] == 0 and lab.max() == 0 and (lab == -2).sum() > 200      # one cluster, across ray 0
    first = int(np.nonzero(lab[180:] == 0)[0][0]) + 180
    assert pc[first] == 0 and 0 < pc[359] <= pc[0] and pc.max() == pc[np.nonzero(lab[:180] == 0)[0][-1]]
    cnt = _check(g, pos, 7, 24, 64)
    assert cnt["rings"] >= 6
    two = _scan(torch, _sensor(lipmpc, "grid", fx, 2), pos, noise)
    cnt = _check(two, pos, 2, 24, 64)
    assert two["pieces"][0].max() >= 20 and two["n_inferred"][0] == 0 and two["overflow"][0] == 0 and cnt["dropped"] >= 20


def test_gpu_split_batches_streams_graphs_and_leftover_state():
    """B = 65 and B = 1; a side stream; a graph replay; out buffers poisoned beforehand: the same bits every time."""
    torch = pytest.importorskip("torch")
    import lipmpc
    fx = G.fixture(n_robots=65)
    pos, R, split = fx["pos"], 360, 30
    noise = 0.01 * np.random.default_rng(6).standard_normal((65, R, 2))
    sensor = _sensor(lipmpc, "grid", fx, split)
    g = _scan(torch, sensor, pos, noise)
    _check(g, pos, split, 24, 64)
    for b in (0, 64):
        one = _scan(torch, sensor, pos[b:b + 1], noise[b:b + 1])
        for k in ("pieces", "labels", "n_inferred", "overflow", "c_eta", "obs_nv", "hits"):
            assert _eq(one[k][0], g[k][b]), (k, b)
    used = np.arange(64)[None, None, :] < g["obs_nv"][:, :, None]         # vertex slots beyond obs_nv keep what was there

    def same(out, what):
        torch.cuda.synchronize()
        for k in g:
            a = out[k].cpu().numpy()
            assert _eq(a[used] if k == "obs_xy" else a, g[k][used] if k == "obs_xy" else g[k]), (what, k)

    st, nz = _states(torch, pos), torch.as_tensor(noise, device="cuda")

    def poisoned():
        out = sensor.alloc_outputs(65, with_debug=True, c_eta=True)
        for v in out.values():
            v.view(torch.uint8).fill_(0xA5)
        return out

    same(sensor.sense(st, nz, out=poisoned()), "poisoned out")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = sensor.sense(st, nz, out=poisoned())
    torch.cuda.current_stream().wait_stream(side)
    same(out, "side stream")
    out = poisoned()
    with torch.cuda.stream(side):
        sensor.sense(st, nz, out=out)                                       # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sensor.sense(st, nz, out=out)
    for v in out.values():
        v.view(torch.uint8).fill_(0x5A)
    graph.replay()
    same(out, "graph replay")
    graph.replay()
    same(out, "second replay")


@pytest.mark.parametrize("kind", ["grid", "ring"])
def test_gpu_split_sense_plan_step_equals_scan_then_solve(kind):
    """sense_plan_step of a splitting sensor = the split scan + plan_step_batch_c_eta: the same bits; and the split changes what
    is solved (the rows differ from the unsplit sensor's)."""
    torch = pytest.importorskip("torch")
    import lipmpc
    fx = G.fixture()
    B = 16
    sensor = _sensor(lipmpc, kind, fx, 30, n_obs_max=12, v_max=32)
    sv = lipmpc.BatchedLipMpc(lipmpc.LipMpcParams(N=3, n_obs_max=12, v_max=32))
    st = _states(torch, fx["pos"][:B])
    goal = torch.tensor([[8.0, 8.0]] * B, dtype=torch.float64, device="cuda")
    foot = torch.ones((B,), dtype=torch.int8, device="cuda")
    noise = 0.01 * torch.randn((B, 360, 2), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    sen, out = sensor.sense_plan_step(sv, st, goal, foot, noise)
    torch.cuda.synchronize()
    sen, out = {k: v.clone() for k, v in sen.items()}, {k: v.clone() for k, v in out.items()}
    sen2 = sensor.sense(st, noise, c_eta=True, rings=False)
    out2 = sv.plan_step_batch_c_eta(st, goal, foot, sen2["c_eta"], overflow=sen2["overflow"])
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    for k in ("c_eta", "n_inferred", "overflow"):
        assert torch.equal(bits(sen[k]), bits(sen2[k])), k
    for k in ("U", "X", "theta", "omega", "obj", "status", "iters", "active"):
        assert torch.equal(bits(out[k]), bits(out2[k])), k
    plain = _sensor(lipmpc, kind, fx, 0, n_obs_max=12, v_max=32).sense(st, noise, c_eta=True, rings=False)
    torch.cuda.synchronize()
    assert int(sen["n_inferred"].sum()) > int(plain["n_inferred"].sum()) > 0
    assert set(out["status"].tolist()) <= {0, 1, 2, 3, 4, 5}
    with pytest.raises(ValueError):
        sensor.sense(st, noise)                                            # no split twin of the rings-only scan
    with pytest.raises(ValueError):
        lipmpc.LidarSensor(fx["rings"], resolution=360, split_rays=181)


def test_gpu_split_through_the_drop_in_class():
    """HumanoidMPCUnknownEnvironment(split_rays=) in a room of four wall polygons: the hook's half-spaces all have the robot on
    their free side; without the split the one hull of the walls holds the robot (a flipped row).  The 50-slot fallback sensor
    splits too: at split_rays = 20 the room is 18 pieces, more than the 12 default slots."""
    torch = pytest.importorskip("torch")
    import lipmpc
    walls = [np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 0.2], [0.0, 0.2]]), np.array([[0.0, 3.8], [4.0, 3.8], [4.0, 4.0], [0.0, 4.0]]),
             np.array([[0.0, 0.2], [0.2, 0.2], [0.2, 3.8], [0.0, 3.8]]), np.array([[3.8, 0.2], [4.0, 0.2], [4.0, 3.8], [3.8, 3.8]])]
    x, y = 1.73, 2.21

    def sides(split):
        mpc = lipmpc.HumanoidMPCUnknownEnvironment(goal=(3.0, 3.0), obstacles=walls, N_horizon=3, N_mpc_timesteps=4, init_state=(x, 0, y, 0, 0.0),
                                                   verbosity=0, lidar_range=4.5, noise_seed=3, split_rays=split)
        cs, etas = mpc._get_list_c_and_eta(x, y)
        return np.array([float(e[0, 0] * (x - c[0, 0]) + e[1, 0] * (y - c[1, 0])) for c, e in zip(cs, etas)]), mpc

    off, _ = sides(0)
    assert len(off) == 1 and off[0] < 0.0
    on, _ = sides(45)
    assert len(on) == 8 and np.all(on > 0.0)
    many, mpc = sides(20)
    assert len(many) == 18 and np.all(many > 0.0) and mpc._big_sensor is not None and mpc._big_sensor.split_rays == 20
