"""GPU: the map update (lipmpc_map_update_batch) off its one tested window -- every map case of tests/window_cases.py, in the
manner of tests/test_map_gpu.py: per-robot evidence equals tests/map_oracle.py integer for integer, shared evidence equals the
start plus the sum of what the robots add.  The readings are the device's own grid scan of the same case, with the case's
hand-written readings (non-finite, denormal, in the robot's own cell, beyond the window, in the window's last row and column)
uploaded as they are; one robot per case is masked; some cases start from a non-zero evidence grid, some use other weights.
tests/test_window_cases_oracle.py shows that no case is vacuous."""
import ctypes as C

import numpy as np
import pytest

import lidar_oracle as L
import window_cases as WC
from helpers import raw_call

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -2


def _states(torch, pos):
    st = np.zeros((len(pos), 5)); st[:, 0] = pos[:, 0]; st[:, 2] = pos[:, 1]
    return torch.as_tensor(st, device="cuda")


def _device_scan(torch, lipmpc, c):
    """hits [B,R,2] (numpy) of the device's own noise-free grid scan of the case."""
    sensor = lipmpc.LidarSensor.from_grid(lipmpc.GridMap(c["occ"], c["origin"], c["cell"]), lidar_range=c["lidar_range"],
                                          resolution=c["resolution"], n_obs_max=24, v_max=64)
    hits = sensor.sense(_states(torch, c["pos"]), None, with_debug=True, c_eta=True)["hits"]
    torch.cuda.synchronize()
    return hits.cpu().numpy()


@pytest.mark.parametrize("case_id", WC.MAP_IDS)
def test_gpu_map_update_windows(case_id):
    torch = pytest.importorskip("torch")
    import lipmpc
    c = WC.case(case_id)
    B, W, H = len(c["pos"]), c["W"], c["H"]
    hits = WC.map_readings(c, _device_scan(torch, lipmpc, c))
    mask, ev0 = WC.map_mask(c), WC.evidence0(c)
    st, d_hits, d_mask = _states(torch, c["pos"]), torch.as_tensor(hits, device="cuda"), torch.as_tensor(mask, device="cuda")
    kw = dict(w_hit=c["w_hit"], w_miss=c["w_miss"], depth=c["depth"])
    per = lipmpc.OccupancyMapper(W, H, c["origin"], c["cell"], c["lidar_range"], c["resolution"], per_robot=B, **kw)
    sh = lipmpc.OccupancyMapper(W, H, c["origin"], c["cell"], c["lidar_range"], c["resolution"], **kw)
    assert (per.depth, per.cell, per.lidar_range) == (c["depth"], c["cell"], c["lidar_range"])
    per.evidence.copy_(torch.as_tensor(ev0, device="cuda").expand(B, W, H))
    sh.evidence.copy_(torch.as_tensor(ev0, device="cuda"))
    e_per, e_sh = per.update(st, d_hits, d_mask), sh.update(st, d_hits, d_mask)
    torch.cuda.synchronize()
    assert e_per.dtype == torch.int32 and tuple(e_per.shape) == (B, W, H) and tuple(e_sh.shape) == (W, H)
    delta = WC.map_deltas(c, hits, mask)
    want, got = ev0[None].astype(np.int64) + delta, e_per.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(e_sh.cpu().numpy(), ev0.astype(np.int64) + delta.sum(0))
    n_hit, n_pass = int((delta == c["w_hit"]).sum()), int((delta == -c["w_miss"]).sum())
    print(f"{case_id}: {B} robots, {int(delta.any(axis=(1, 2)).sum())} touch the grid, {n_hit} hit cells, {n_pass} passed cells")
    assert n_hit > 0 and n_pass > 0 and not delta[1].any()
    for b in c["unplaced"]:
        assert not delta[b].any()


def test_gpu_window_refused_by_its_depth_leaves_the_evidence():
    """Range 1, cells of 1 / 4912.5: 5 x 9829 cells without a depth and with the cap case's, 5 x 9831 = 49155 with a depth of
    2e-4 -- LIPMPC_E_UNSUPPORTED through the raw binding and through the wrapper, the evidence as it was."""
    torch = pytest.importorskip("torch")
    import lipmpc
    c, d = WC.case("w5x9829"), WC.REFUSED_BY_DEPTH
    B, W, H, R = len(c["pos"]), c["W"], c["H"], c["resolution"]
    ev0 = np.random.default_rng(9).integers(-1000, 1000, (W, H)).astype(np.int32)
    ev = torch.as_tensor(ev0, device="cuda")
    st, hits = _states(torch, c["pos"]), torch.as_tensor(WC.map_readings(c, WC.oracle_hits("w5x9829")), device="cuda")
    table = torch.as_tensor(L.ray_table(R), device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    org, cs = (C.c_double * 2)(*c["origin"]), (C.c_double * 2)(*d["cell"])

    def rc(depth):
        r = raw_call("lipmpc_map_update_batch", device=torch.cuda.current_device(), B=B, resolution=R, W=W, H=H, grid_shared=1,
                     origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p), lidar_range=d["lidar_range"], depth=depth, w_hit=3, w_miss=1,
                     state=ptr(st), hits=ptr(hits), ray_table=ptr(table), evidence=ptr(ev), hip_stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return r

    assert rc(d["depth"]) == E_UNSUPPORTED and np.array_equal(ev.cpu().numpy(), ev0)
    mp = lipmpc.OccupancyMapper(W, H, c["origin"], d["cell"], d["lidar_range"], R, depth=d["depth"])
    mp.evidence.copy_(ev)
    with pytest.raises(RuntimeError) as e:
        mp.update(st, hits)
    torch.cuda.synchronize()
    assert e.value.code == E_UNSUPPORTED and np.array_equal(mp.evidence.cpu().numpy(), ev0)
    assert rc(0.0) == 0 and not np.array_equal(ev.cpu().numpy(), ev0)       # the same call without the depth fits, and maps
