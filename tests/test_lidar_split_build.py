"""CPU: what the build must hold for the sector split of the scans (lipmpc_lidar_c_eta_split_batch /
lipmpc_lidar_grid_c_eta_split_batch): the symbols, the scan kernels' code objects (no scratch, LDS within 16 waves per compute
unit), and the refusals that never reach a device."""
import ctypes as C
import os
import re

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

SPLIT = ("lipmpc_lidar_c_eta_split_batch", "lipmpc_lidar_grid_c_eta_split_batch")
LDS_PER_CU = 160 * 1024            # bytes of LDS of a gfx950 compute unit


def test_library_declares_and_exports_the_split_entry_points():
    lib = lipmpc._lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lipmpc.h")).read()
    for name in SPLIT:
        assert hasattr(lib, name) and name in lipmpc._lib.SIGNATURES
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert lib.lipmpc_version() == 5                       # a backward-compatible addition
    # each twin takes its parent's argument list plus (split_rays, pieces) in front of the stream
    for name in SPLIT:
        parent = [n for n, _ in lipmpc._lib.SIGNATURES[name.replace("_split", "")][1]]
        twin = [n for n, _ in lipmpc._lib.SIGNATURES[name][1]]
        assert twin == parent[:-1] + ["split_rays", "pieces", "hip_stream"]


def test_scan_kernels_code_objects():
    """Both instantiations of the scan body with the split stage in them: no scratch, no spilled vector register, within the 128
    registers of 4 waves per SIMD, and no more LDS per wave (= per workgroup) than lets 16 waves share a compute unit's 160 KB --
    the occupancy the latency-bound scan lives on."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    kernels = {name: [v for k, v in res.items() if name in k] for name in ("lidar_sense_kernel", "lidar_grid_scan_kernel")}
    for name, found in kernels.items():
        assert len(found) == 1, (name, sorted(k for k in res if "lidar" in k))
        k = found[0]
        print(name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0
        assert k["vgpr_count"] <= 128
        assert 0 < k["group_segment_fixed_size"] <= LDS_PER_CU // 16


def test_split_refusals_reach_no_device():
    """split_rays < 0 or > resolution / 2: LIPMPC_E_ARG from both twins, decided on the host (no GPU here); B = 0 with a valid
    split enqueues nothing and passes."""
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    org, cs = (C.c_double * 2)(-1.0, -1.0), (C.c_double * 2)(0.05, 0.05)

    def ring(**kw):
        pointers = {n: one for n, t in lipmpc._lib.SIGNATURES[SPLIT[0]][1] if t is C.c_void_p}
        args = dict(device=0, B=0, resolution=360, n_env=1, v_env=4, env_shared=1, lidar_range=1.5, eps=0.3, min_samples=3, n_obs_max=12,
                    v_max=32, split_rays=0)
        args.update(kw)
        return raw_call(SPLIT[0], **pointers, **args)

    def grid(**kw):
        pointers = {n: one for n, t in lipmpc._lib.SIGNATURES[SPLIT[1]][1] if t is C.c_void_p}
        pointers.update(origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p))
        args = dict(device=0, B=0, resolution=360, W=200, H=200, grid_shared=1, lidar_range=1.5, eps=0.3, min_samples=3, n_obs_max=12,
                    v_max=32, split_rays=0)
        args.update(kw)
        return raw_call(SPLIT[1], **pointers, **args)

    for call in (ring, grid):
        assert call() == 0 and call(split_rays=1) == 0 and call(split_rays=180) == 0
        assert call(split_rays=181) == -1 and call(split_rays=-1) == -1
        assert call(resolution=90, split_rays=45) == 0 and call(resolution=90, split_rays=46) == -1
        assert call(resolution=7, split_rays=3) == 0 and call(resolution=7, split_rays=4) == -1
        assert call(resolution=385) == -1
