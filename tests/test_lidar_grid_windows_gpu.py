"""GPU: the grid scan (lipmpc_lidar_grid_c_eta_batch) off its one tested window -- every scanning case of tests/window_cases.py
(window shapes from 9 x 5 to the 49152-cell cap, resolutions 1 .. 384, robots exactly on cell boundaries, a large origin, the
2^30 cell limit, grids of one row / one cell / smaller than the window, a range of zero).  The hits against
tests/grid_lidar_oracle.py bit for bit, the rest of the launch against the oracle chain fed the device's own hits
(tests/lidar_grid_checks.py).  tests/test_window_cases_oracle.py shows that no case is vacuous."""
import ctypes as C

import numpy as np
import pytest

import lidar_oracle as L
import window_cases as WC
from helpers import raw_call
from lidar_grid_checks import check_chain, check_hits

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -2
N_OBS_MAX, V_MAX = 24, 64


def _states(torch, pos):
    st = np.zeros((len(pos), 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    return torch.as_tensor(st, device="cuda")


def _scan(torch, lipmpc, c, noise):
    sensor = lipmpc.LidarSensor.from_grid(lipmpc.GridMap(c["occ"], c["origin"], c["cell"]), lidar_range=c["lidar_range"],
                                          resolution=c["resolution"], n_obs_max=N_OBS_MAX, v_max=V_MAX)
    out = sensor.sense(_states(torch, c["pos"]), None if noise is None else torch.as_tensor(noise, device="cuda"), with_debug=True, c_eta=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case_id,noisy", [(i, False) for i in WC.SCAN_IDS] + [(i, True) for i in WC.SCAN_IDS if i not in WC.NOISE_FREE_IDS])
def test_gpu_grid_scan_windows(case_id, noisy):
    """Hits bit for bit (check_hits, the solid-cell rule included), labels / rings / (c, eta) by check_chain; robots without a
    cell or far from the grid: no reading, no flag, nothing inferred.  Noise only where the case is cheap: the cap cases run noise-free."""
    torch = pytest.importorskip("torch")
    import lipmpc
    c = WC.case(case_id)
    noise = WC.noise_of(c) if noisy else None
    g = _scan(torch, lipmpc, c, noise)
    oracle = WC.scan_oracle(case_id)
    n_hits, n_solid = check_hits(g, c["pos"], lambda b: WC.occ_of(c, b), c["origin"], c["cell"], c["lidar_range"], L.ray_table(c["resolution"]),
                                 noise, scan_of=lambda b: oracle[b][:2])
    n_rings = check_chain(g, c["pos"])
    print(f"{case_id} noisy={noisy}: {len(c['pos'])} robots, {n_hits} hits, {n_solid} in solid cells, {n_rings} rings")
    quiet = list(c["far"]) + list(c["unplaced"]) if case_id != "range0" else range(len(c["pos"]))
    for b in quiet:
        assert np.isnan(g["hits"][b]).all() and g["overflow"][b] == 0 and g["n_inferred"][b] == 0, b
        assert not g["c_eta"][b].any() and (g["labels"][b] == -2).all(), b
    assert n_hits == sum(int(valid.sum()) for _, valid, _ in oracle)


def _raw_scan(torch, c, occ, lidar_range=None, cell=None, B=None):
    """lipmpc_lidar_grid_c_eta_batch through the raw binding, every output sentinel-filled first: (status, outputs)."""
    B = len(c["pos"]) if B is None else B
    R = c["resolution"]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    org, cs = (C.c_double * 2)(*c["origin"]), (C.c_double * 2)(*(c["cell"] if cell is None else cell))
    st = _states(torch, c["pos"][:B])
    table = torch.as_tensor(L.ray_table(R), device="cuda")
    f64, i32 = torch.float64, torch.int32
    out = dict(c_eta=torch.full((B, N_OBS_MAX, 4), -7.5, dtype=f64, device="cuda"), n_inferred=torch.full((B,), -5, dtype=i32, device="cuda"),
               overflow=torch.full((B,), -5, dtype=i32, device="cuda"), obs_xy=torch.full((B, N_OBS_MAX, V_MAX, 2), -7.5, dtype=f64, device="cuda"),
               obs_nv=torch.full((B, N_OBS_MAX), -5, dtype=i32, device="cuda"), hits=torch.full((B, R, 2), -7.5, dtype=f64, device="cuda"),
               labels=torch.full((B, R), -5, dtype=i32, device="cuda"))
    rc = raw_call("lipmpc_lidar_grid_c_eta_batch", device=torch.cuda.current_device(), B=B, resolution=R, W=c["W"], H=c["H"], grid_shared=1,
                  origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p), lidar_range=c["lidar_range"] if lidar_range is None else lidar_range,
                  eps=L.DBSCAN_EPS, min_samples=L.DBSCAN_MIN_SAMPLES, n_obs_max=N_OBS_MAX, v_max=V_MAX, state=ptr(st), occ=ptr(occ), ray_table=ptr(table),
                  **{k: ptr(v) for k, v in out.items()}, hip_stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def test_gpu_window_over_the_cap_is_refused_and_writes_nothing():
    """5 x 9831 = 49155 cells: LIPMPC_E_UNSUPPORTED, every output as it was; the same call at 5 x 9829 runs (and is compared in
    test_gpu_grid_scan_windows)."""
    torch = pytest.importorskip("torch")
    import lipmpc  # noqa: F401
    c = WC.case("w5x9829")
    occ = torch.as_tensor(c["occ"], device="cuda")
    rc, out = _raw_scan(torch, c, occ, cell=WC.REFUSED["cell"], lidar_range=WC.REFUSED["lidar_range"])
    assert rc == E_UNSUPPORTED
    for k, v in out.items():
        assert (v == (-7.5 if v.dtype == np.float64 else -5)).all(), k
    rc, out = _raw_scan(torch, c, occ)
    assert rc == 0
    want = WC.oracle_hits("w5x9829")
    assert np.array_equal(out["hits"], want, equal_nan=True) and not (out["n_inferred"] == -5).any()


def test_gpu_occupancy_bytes_other_than_one():
    """Solid is `!= 0`: the same map with its solid cells written as 2, 128 and 255 gives the 0/1 call's outputs, bit for bit
    (GridMap turns every map into 0/1, so the bytes go in through the raw binding)."""
    torch = pytest.importorskip("torch")
    import lipmpc  # noqa: F401
    c = WC.case("w23x23")
    rc, ref = _raw_scan(torch, c, torch.as_tensor(c["occ"], device="cuda"))
    assert rc == 0 and np.array_equal(ref["hits"], WC.oracle_hits("w23x23"), equal_nan=True)
    rng = np.random.default_rng(7)
    for values in ((2,), (128,), (255,), (2, 128, 255)):
        occ = np.where(c["occ"] != 0, rng.choice(values, c["occ"].shape), 0).astype(np.uint8)
        rc, out = _raw_scan(torch, c, torch.as_tensor(occ, device="cuda"))
        assert rc == 0
        for k in ("hits", "labels", "n_inferred", "overflow"):
            assert np.array_equal(out[k], ref[k], equal_nan=True), (values, k)
        assert np.array_equal(out["c_eta"], ref["c_eta"]) and np.array_equal(out["obs_nv"], ref["obs_nv"])
