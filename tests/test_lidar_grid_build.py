"""CPU: what the build must hold for the grid scan (lipmpc_lidar_grid_c_eta_batch): the symbols, the grid kernel's code object
(no scratch, no more LDS than the polygon kernel of the same build), and the refusals that never reach a device."""
import ctypes as C

import numpy as np
import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call


def test_library_exports_the_grid_entry_points():
    lib = lipmpc._lib.load()
    for name in ("lipmpc_lidar_grid_c_eta_batch", "lipmpc_sense_grid_plan_step_batch"):
        assert hasattr(lib, name) and name in lipmpc._lib.SIGNATURES
    assert lib.lipmpc_version() == 5                       # a backward-compatible addition
    assert lipmpc.GridMap and lipmpc.LidarSensor.from_grid


def test_grid_kernel_code_object():
    """The sense kernel's body instantiated for grids (lidar_grid_scan_kernel): no scratch, and no more LDS than the polygon instantiation of the same build
    (the 16 waves per compute unit are LDS-bound); both within the 128 registers of 4 waves per SIMD."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    grid = [v for k, v in res.items() if "lidar_grid_scan_kernel" in k]
    poly = [v for k, v in res.items() if "lidar_sense_kernel" in k]
    assert len(grid) == 1 and len(poly) == 1, sorted(k for k in res if "lidar" in k)
    grid, poly = grid[0], poly[0]
    print("grid", grid, "\npolygon", poly)
    assert grid["private_segment_fixed_size"] == 0 and grid["vgpr_spill_count"] == 0
    assert 0 < grid["group_segment_fixed_size"] <= poly["group_segment_fixed_size"]
    assert grid["vgpr_count"] <= 128 and poly["vgpr_count"] <= 128
    assert poly["private_segment_fixed_size"] == 0


def test_grid_refusals_reach_no_device():
    """Window too large (-2); resolution > 384, W or H < 1, a cell that is not positive (-1): decided on the host before anything
    is enqueued (no GPU here), through both entry points where they share the check."""
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    pointers = {n: one for n, t in lipmpc._lib.SIGNATURES["lipmpc_lidar_grid_c_eta_batch"][1] if t is C.c_void_p}
    org = (C.c_double * 2)(-1.0, -1.0)

    def rc(cell=(0.05, 0.05), **kw):
        cs = (C.c_double * 2)(*cell)
        args = dict(device=0, B=1, resolution=360, W=200, H=200, grid_shared=1, lidar_range=1.5, eps=0.3, min_samples=3, n_obs_max=12,
                    v_max=32)
        args.update(kw)
        return raw_call("lipmpc_lidar_grid_c_eta_batch", **dict(pointers, origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p)), **args)

    assert rc(B=0) == 0                                    # the same arguments pass: an empty batch enqueues nothing
    assert rc(lidar_range=3.0, cell=(0.01, 0.01)) == -2    # 605 x 605 cells in range: the window does not fit the LDS bitmap
    assert rc(lidar_range=3.0, cell=(0.05, 0.004)) == -2
    assert rc(B=0, lidar_range=5.4, cell=(0.05, 0.05)) == 0 and rc(lidar_range=5.5, cell=(0.05, 0.05)) == -2      # 221^2 <= 49152 < 225^2
    assert rc(resolution=385) == -1 and rc(resolution=0) == -1
    assert rc(W=0) == -1 and rc(H=0) == -1 and rc(H=-3) == -1
    assert rc(cell=(0.0, 0.05)) == -1 and rc(cell=(0.05, -0.05)) == -1 and rc(cell=(float("nan"), 0.05)) == -1
    assert rc(lidar_range=-1.0) == -1 and rc(lidar_range=float("inf")) == -1
    assert raw_call("lipmpc_lidar_grid_c_eta_batch", device=0, B=1, resolution=360, W=200, H=200, grid_shared=1, lidar_range=1.5, eps=0.3,
                    min_samples=3, n_obs_max=12, v_max=32) == -1                                                   # no origin / cell / c_eta
    assert raw_call("lipmpc_sense_grid_plan_step_batch", B=1, resolution=360, W=200, H=200, grid_shared=1, lidar_range=1.5, eps=0.3,
                    min_samples=3) == -1                                                                           # no handle
    assert lipmpc._lib.load().lipmpc_strerror(-2)
    # the Python map refuses what the library would
    with pytest.raises(ValueError):
        lipmpc.GridMap(np.zeros((4, 4)), (0.0, 0.0), 0.0)
    with pytest.raises(ValueError):
        lipmpc.GridMap(np.zeros((4,)), (0.0, 0.0), 0.1)
    g = lipmpc.GridMap(np.eye(4) * 7, (0.5, -0.5), (0.1, 0.2))
    assert g.shared and (g.W, g.H) == (4, 4) and g.occ.dtype == np.uint8 and g.occ.max() == 1 and g.cell == (0.1, 0.2)
