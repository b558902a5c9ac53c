"""GPU tests (-m gpu) of the polygon scan on large rings and long candidate lists: every case of tests/lidar_ring_cases.py through
LidarSensor.sense(with_debug=True, c_eta=True) into poisoned buffers with canaries round them, against oracle/lidar_oracle.py (which
tests/test_lidar_ring_cases_oracle.py pins to the reference on the boundary inputs and shows to reach the serial vertex loop, several
staging chunks, candidates without a cached circle, the full candidate list, a skipped ring, the reach of a long wall and 16-bit ring
indices).  The bars are those of tests/test_lidar.py: readings bit for bit (NaN exactly where the oracle has none), labels equal,
overflow as expected for EVERY robot, and for every robot whose flag is 0 n_inferred, every ring, and (c, eta) within 1e-12 of
lipmpc_oracle.closest_point_and_normal on the oracle's ring.  No robot of any case is left uncompared.

That the cases bite was shown once on builds of csrc/lipmpc_lidar_rays.inc with one VALUE changed each (no address, bound or loop limit),
this file run once per build on an MI355X:
  1. the serial loop's closing edge ends at vertex 1: gon9 / 40 / 152 / 153, two_hundreds, long_wall_12, boundaries_b_*, far_origin,
     odd_positions and the reference vectors of boundaries_b_*, gon9, gon40 fail (18 tests); tests/test_lidar.py passes on that build;
  2. bd / hx / hy set again for every chunk: gon152, gon153, edges_160, two_hundreds and all five cands cases fail (11 tests);
  3. `dd <= bd[p]`: the five cands cases fail (7 tests) -- on the tie ray alone; a tie at the SAME point (coincident rings, the mirror
     pair, a shared vertex, a hit at exactly the range) cannot show it;
  4. `cr2 = 0.0` for candidates at positions 64 and above changes NO output of any input: such a candidate's circle is centred on
     the robot (wx = wy = 0), the sector test reads 0 <= 0 and passes as it does with INFINITY; all 46 tests pass, rightly.  With
     `cr2 = -1.0` (those candidates never walked) the five cands cases fail (7 tests);
  5. reach without the ring's radius: the gon cases, long_wall, long_wall_12, res2 .. res383, far_origin, odd_positions and the
     reference vectors of gon9, gon40, long_wall fail (19 tests).
tests/test_lidar.py as it was notices 5 (ten tests) and, through its count of more than 100 readings on 300 squares, 2 and the
`-1.0` form of 4; it does not notice 1."""
import os

import numpy as np
import pytest

import lidar_ring_cases as C

pytestmark = pytest.mark.gpu

CANARY, ICANARY, GUARD = 4.25e100, -77, 64


def _same_ring(a, b):
    if len(a) != len(b):
        return False
    k = int(np.argmin(np.abs(b - a[0]).sum(1)))
    return np.array_equal(np.roll(b, -k, axis=0), a)


def _guarded(torch, shape, dtype):
    n, fill = int(np.prod(shape)), CANARY if dtype == torch.float64 else ICANARY
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return big, big[GUARD:GUARD + n].view(shape)


def _sensor(lipmpc, c, **kw):
    rings = C.rings_of(c, 0)
    return lipmpc.LidarSensor(rings, lidar_range=c["lidar_range"], resolution=c["resolution"], n_obs_max=kw.pop("n_obs_max", c["n_obs_max"]),
                              v_max=kw.pop("v_max", c["v_max"]), **kw)


def _state(torch, pos):
    st = np.zeros((len(pos), 5))
    st[:, 0], st[:, 2] = pos[:, 0], pos[:, 1]
    return torch.as_tensor(st, device="cuda")


def _maps(torch, c):
    """env_xy / env_nv of a case with one map per robot (else nothing: the sensor's shared map)."""
    if not c.get("per_robot"):
        return {}
    packed = [C.pack(m) for m in c["rings"]]
    return dict(env_xy=torch.as_tensor(np.stack([p[0] for p in packed]), device="cuda").contiguous(),
                env_nv=torch.as_tensor(np.stack([p[1] for p in packed]).astype(np.int32), device="cuda").contiguous())


def _scan(torch, sensor, c, noise, names=("n_inferred", "overflow", "obs_xy", "obs_nv", "c_eta", "hits", "labels"), maps=None, **kw):
    """One scan into poisoned, guarded buffers: the outputs as numpy, the canaries checked."""
    from importlib import import_module
    table = import_module("humanoid-navigation-using-mpc-ldcbf_amd.lidar").sensor_outputs(len(c["pos"]), sensor.n_obs_max, sensor.v_max,
                                                                                           sensor.resolution)
    big, out = {}, {}
    for k in names:
        big[k], out[k] = _guarded(torch, table[k][1], table[k][0])
    sensor.sense(_state(torch, c["pos"]), None if noise is None else torch.as_tensor(np.ascontiguousarray(noise), device="cuda"),
                 with_debug=True, c_eta="c_eta" in names, out=out, **(_maps(torch, c) if maps is None else maps), **kw)
    torch.cuda.synchronize()
    for k, b in big.items():
        b = b.cpu().numpy()
        fill = CANARY if b.dtype == np.float64 else ICANARY
        assert np.all(b[:GUARD] == fill) and np.all(b[-GUARD:] == fill), k
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def _identical(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _compare(c, g, want, expect):
    """One launch against the oracle's scans ``want`` and the expected flags."""
    import lipmpc_oracle as O
    n_rings = 0
    for b, o in enumerate(want):
        valid = ~np.isnan(g["hits"][b, :, 0])
        assert np.array_equal(valid, o["valid"]), (c["id"], b, np.nonzero(valid != o["valid"])[0][:8])
        assert np.array_equal(np.isnan(g["hits"][b, :, 1]), ~valid)
        bad = np.nonzero((_bits(g["hits"][b][valid]) != _bits(o["hits"][valid])).any(1))[0]
        assert np.array_equal(g["hits"][b][valid], o["hits"][valid]), (c["id"], b, np.nonzero(valid)[0][bad][:8])     # bit for bit
        assert np.array_equal(g["labels"][b], o["labels"]), (c["id"], b)
        assert g["overflow"][b] == expect[b], (c["id"], b, g["overflow"][b], expect[b])
        if expect[b]:
            continue
        n = len(o["rings"])
        assert g["n_inferred"][b] == n, (c["id"], b, g["n_inferred"][b], n)
        assert not g["obs_nv"][b, n:].any() and not g["c_eta"][b, n:].any()
        for j, ring in enumerate(o["rings"]):
            assert _same_ring(g["obs_xy"][b, j, : g["obs_nv"][b, j]], ring), (c["id"], b, j)
            p, eta, _, degen = O.closest_point_and_normal(c["pos"][b], ring)
            if not degen:
                assert np.max(np.abs(g["c_eta"][b, j, :2] - p)) < 1e-12 and np.max(np.abs(g["c_eta"][b, j, 2:] - eta)) < 1e-12, (c["id"], b, j)
            n_rings += 1
    return n_rings


@pytest.mark.parametrize("id_", C.IDS)
def test_gpu_ring_cases_against_the_oracle(id_):
    """Every case against the oracle; then again with the call ranking its robots first (an order buffer pre-filled with -7: the
    weight kernel walks the same rings, a robot inside a long ring and the robots at NaN / inf included) -- every output
    bit-identical; and through lipmpc_lidar_sense_batch, the entry point without the constraint assembly -- the same again."""
    torch = pytest.importorskip("torch")
    import lipmpc
    c, want = C.case(id_), C.oracle(id_)
    sensor = _sensor(lipmpc, c)
    assert sensor.n_env == len(C.rings_of(c, 0)) and sensor.v_env == C.route(id_)[0]["v_env"]
    maps = _maps(torch, c)
    g = _scan(torch, sensor, c, c["noise"], maps=maps, schedule=None)
    n_rings = _compare(c, g, want, c["expect_overflow"])
    print(id_, "readings", [int(o["valid"].sum()) for o in want], "rings compared", n_rings, "overflow", g["overflow"].tolist())
    if "odd" in c:
        for b in c["odd"]:
            assert np.isnan(g["hits"][b]).all() and np.all(g["labels"][b] == -2) and g["n_inferred"][b] == 0 and g["overflow"][b] == 0
    sched = sensor.make_schedule(len(c["pos"]))
    sched.fill_(-7)
    ranked = _scan(torch, sensor, c, c["noise"], maps=maps, schedule=sched)
    _identical(g, ranked, "ranked")
    sc = sched.cpu().numpy()
    assert sc[0] == len(c["pos"]) and np.array_equal(np.sort(sc[2:2 + len(c["pos"])]), np.arange(len(c["pos"])))
    plain = _scan(torch, sensor, c, c["noise"], names=("n_inferred", "overflow", "obs_xy", "obs_nv", "hits", "labels"), maps=maps)
    _identical({k: v for k, v in g.items() if k != "c_eta"}, plain, "lipmpc_lidar_sense_batch")


@pytest.mark.parametrize("id_", C.GOLDEN_IDS)
def test_gpu_ring_cases_against_the_reference(golden_dir, id_):
    """The kernel against the reference's own vectors (tests/golden/lidar_golden_edges.npz) under the noise the reference drew:
    readings bit for bit, scikit-learn's labels, Qhull's rings up to rotation."""
    torch = pytest.importorskip("torch")
    import lipmpc
    d = np.load(os.path.join(golden_dir, "lidar_golden_edges.npz"))
    c = C.case(id_)
    noise, nv, xy = d[id_ + "/noise"], d[id_ + "/inf_nv"], d[id_ + "/inf_xy"]
    g = _scan(torch, _sensor(lipmpc, c), c, noise, schedule=None)
    for b in range(len(c["pos"])):
        valid = d[id_ + "/valid"][b]
        assert np.array_equal(~np.isnan(g["hits"][b, :, 0]), valid), b
        assert np.array_equal(g["hits"][b][valid], (d[id_ + "/clean"][b] + noise[b])[valid]), b
        assert d[id_ + "/clustered"][b]
        assert np.array_equal(g["labels"][b], d[id_ + "/labels"][b]), b
        n = int((nv[b] > 0).sum())
        assert g["overflow"][b] == 0 and g["n_inferred"][b] == n, (b, g["n_inferred"][b], n)
        for j in range(n):
            assert _same_ring(g["obs_xy"][b, j, : g["obs_nv"][b, j]], xy[b, j, : nv[b, j]]), (b, j)


@pytest.mark.parametrize("id_", ["gon40", "cands_129"])
def test_gpu_split_off_is_the_parent_on_ring_cases(id_):
    """split_rays = 0 through lipmpc_lidar_c_eta_split_batch (reached by handing in a ``pieces`` buffer) equals
    lipmpc_lidar_c_eta_batch bit for bit, pieces = labels."""
    torch = pytest.importorskip("torch")
    import lipmpc
    c = C.case(id_)
    sensor = _sensor(lipmpc, c)
    parent = _scan(torch, sensor, c, c["noise"], schedule=None)
    twin = _scan(torch, sensor, c, c["noise"], names=("n_inferred", "overflow", "obs_xy", "obs_nv", "c_eta", "hits", "labels", "pieces"),
                 schedule=None)
    _identical(parent, {k: v for k, v in twin.items() if k != "pieces"}, "split off")
    assert np.array_equal(twin["pieces"], twin["labels"])
    _compare(c, twin, C.oracle(id_), c["expect_overflow"])


@pytest.mark.parametrize("id_", ["gon40", "edges_160"])
def test_gpu_one_call_step_equals_scan_then_solve_on_ring_cases(id_):
    """lipmpc_sense_plan_step_batch = lipmpc_lidar_c_eta_batch + lipmpc_plan_step_batch_c_eta with the scan's flags: the same bits
    (the assertion of tests/test_lidar_grid_gpu.py, on these maps; the solver's slots hold hulls of 32 vertices, so the robot inside
    the 40-gon overflows and gets no plan)."""
    torch = pytest.importorskip("torch")
    import lipmpc
    c = C.case(id_)
    B = len(c["pos"])
    sensor = _sensor(lipmpc, c, n_obs_max=24, v_max=32)
    sv = lipmpc.BatchedLipMpc(lipmpc.LipMpcParams(N=3, n_obs_max=24, v_max=32))
    st = _state(torch, c["pos"])
    goal = torch.tensor([[5.0, 5.0]] * B, dtype=torch.float64, device="cuda")
    foot = torch.ones((B,), dtype=torch.int8, device="cuda")
    noise = torch.as_tensor(c["noise"], device="cuda")
    sen, out = sensor.sense_plan_step(sv, st, goal, foot, noise)
    torch.cuda.synchronize()
    sen2 = sensor.sense(st, noise, c_eta=True, rings=False, schedule=None)
    out2 = sv.plan_step_batch_c_eta(st, goal, foot, sen2["c_eta"], overflow=sen2["overflow"])
    torch.cuda.synchronize()
    for k in ("c_eta", "n_inferred", "overflow"):
        assert torch.equal(sen[k], sen2[k]), k
    for k in ("U", "X", "theta", "omega", "obj", "status", "iters", "active"):
        assert torch.equal(out[k].view(torch.int64) if out[k].dtype == torch.float64 else out[k],
                           out2[k].view(torch.int64) if out2[k].dtype == torch.float64 else out2[k]), k
    # the scan's side of it is the oracle's: flags from the oracle's hulls against these slots
    want = C.oracle(id_)
    flags = [C.slots(o["hits"][o["valid"]], o["labels"][o["valid"]], 24, 32)[1] for o in want]
    assert sen["overflow"].tolist() == flags and flags == ([0, 1, 0] if id_ == "gon40" else [0, 0, 0])
    assert [int(s) == lipmpc.STATUS_SENSOR_OVERFLOW for s in out["status"]] == [bool(f) for f in flags]
    assert int(sen["n_inferred"].sum()) > 0


def test_gpu_no_state_is_left_between_scans_of_different_shapes():
    """cands_129 (three chunks, candidates without a circle), then a 9-gon map (one chunk, the serial vertex loop), then cands_129
    again -- one sensor, one stream, one order buffer: the third result is the first, bit for bit."""
    torch = pytest.importorskip("torch")
    import lipmpc
    c, other = C.case("cands_129"), C.case("gon9")
    B = len(c["pos"])
    sensor = _sensor(lipmpc, c)
    sched = sensor.make_schedule(B)
    sched.fill_(-7)
    xy, nv = C.pack(other["rings"])
    gon = dict(env_xy=torch.as_tensor(np.stack([xy] * B), device="cuda").contiguous(),
               env_nv=torch.as_tensor(np.stack([nv] * B).astype(np.int32), device="cuda").contiguous())
    first = _scan(torch, sensor, c, c["noise"], schedule=sched)
    between = _scan(torch, sensor, c, c["noise"], maps=gon, schedule=sched)
    third = _scan(torch, sensor, c, c["noise"], schedule=sched)
    _identical(first, third, "leftover state")
    _compare(c, third, C.oracle("cands_129"), c["expect_overflow"])
    assert not np.array_equal(between["hits"], first["hits"], equal_nan=True)
    # the scan in between is right as well: the 9-gon map at this sensor's 65 rays, from these robots
    mid = dict(other, id="gon9 at 65 rays", pos=c["pos"], resolution=c["resolution"], noise=c["noise"], n_obs_max=c["n_obs_max"], v_max=c["v_max"])
    _compare(mid, between, C.scan(mid, c["noise"]), [0] * B)


def test_gpu_refusals_of_the_ring_scan():
    """More than 65535 rings are refused as unsupported, 65535 with no robot are fine, v_env = 0 is an argument error: all before
    anything is enqueued (the one output each entry point insists on is handed in poisoned and stays so; every other pointer is NULL)."""
    torch = pytest.importorskip("torch")
    from helpers import raw_call
    scan = dict(device=0, resolution=65, env_shared=1, lidar_range=3.0, eps=0.3, min_samples=3, n_obs_max=12, v_max=32)
    xy = torch.full((1, 12, 32, 2), CANARY, dtype=torch.float64, device="cuda")
    nv = torch.full((1, 12), ICANARY, dtype=torch.int32, device="cuda")
    ce = torch.full((1, 12, 4), CANARY, dtype=torch.float64, device="cuda")
    for entry, out in (("lipmpc_lidar_sense_batch", dict(obs_xy=xy.data_ptr(), obs_nv=nv.data_ptr())),
                       ("lipmpc_lidar_c_eta_batch", dict(c_eta=ce.data_ptr()))):
        assert raw_call(entry, B=1, n_env=65536, v_env=4, **scan, **out) == -2          # LIPMPC_E_UNSUPPORTED
        assert raw_call(entry, B=0, n_env=65536, v_env=4, **scan, **out) == -2
        assert raw_call(entry, B=0, n_env=65535, v_env=4, **scan, **out) == 0           # LIPMPC_OK
        assert raw_call(entry, B=1, n_env=1, v_env=0, **scan, **out) == -1              # LIPMPC_E_ARG
        assert raw_call(entry, B=1, n_env=65535, v_env=4, **scan, **out) == -1          # (in range, but no state and no map: E_ARG)
    torch.cuda.synchronize()
    assert bool((xy == CANARY).all()) and bool((nv == ICANARY).all()) and bool((ce == CANARY).all())
