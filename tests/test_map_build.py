"""Scan integration and planning on a grid: C ABI and compiled resources (no GPU needed)."""
import ctypes as C

import lipmpc
import map_oracle as M
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2


def test_map_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name in ("lipmpc_map_update_batch", "lipmpc_rrt_plan_grid_batch"):
        assert name in lipmpc._lib.EXPORTS and name in lipmpc._lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    assert lib.lipmpc_version() == 5                       # backward-compatible additions
    assert lipmpc.OccupancyMapper is lipmpc.mapping.OccupancyMapper
    assert lipmpc.RRT_OUTSIDE_GRID == 7 and lipmpc.RRT_STATUS_NAMES[7] == "OUTSIDE_GRID"
    assert callable(lipmpc.RrtStarPlanner.plan_grid_batch) and callable(lipmpc.UnknownEnvFleet.run_replanning)


def test_map_kernels_code_object():
    """From the built library's gfx950 code objects: the scan integration and the two grid kernels of the planner exist once
    each and use no scratch; the integration kernel's LDS is the two window bitmaps the header's cap implies (2 x 49152 bits)."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in ("map_update_kernel", "rrt_setup_grid_kernel", "rrt_pack_grid_kernel"):
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == (M.LDS_BYTES if k == "map_update_kernel" else 0), (name, r)
    assert M.LDS_BYTES == 2 * M.WINDOW_CELLS // 8 == 12288


def test_map_refusals_reach_no_device():
    """Every refusal is decided on the host before anything is enqueued."""
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    ptrs = dict(state=one, hits=one, ray_table=one, evidence=one)
    org = (C.c_double * 2)(-1.0, -1.0)

    def rc(cell=(0.05, 0.05), origin=org, drop=(), **kw):
        cs = (C.c_double * 2)(*cell)
        args = dict(device=0, B=1, resolution=360, W=96, H=80, grid_shared=1, lidar_range=1.5, depth=0.025, w_hit=3, w_miss=1)
        args.update(kw)
        p = {k: v for k, v in dict(ptrs, origin=C.cast(origin, C.c_void_p), cell=C.cast(cs, C.c_void_p)).items() if k not in drop}
        return raw_call("lipmpc_map_update_batch", **p, **args)

    assert rc(B=0) == 0                                    # the same arguments pass: an empty batch enqueues nothing
    assert rc(resolution=0) == E_ARG and rc(resolution=385) == E_ARG and rc(B=0, resolution=384) == 0 and rc(B=-1) == E_ARG
    assert rc(W=0) == E_ARG and rc(H=0) == E_ARG and rc(H=-2) == E_ARG
    assert rc(cell=(0.0, 0.05)) == E_ARG and rc(cell=(0.05, -1.0)) == E_ARG and rc(cell=(float("nan"), 0.05)) == E_ARG
    assert rc(cell=(float("inf"), 0.05)) == E_ARG
    assert rc(lidar_range=-1.0) == E_ARG and rc(lidar_range=float("inf")) == E_ARG and rc(lidar_range=float("nan")) == E_ARG
    assert rc(depth=-0.01) == E_ARG and rc(depth=float("inf")) == E_ARG and rc(depth=float("nan")) == E_ARG and rc(B=0, depth=0.0) == 0
    for w in ("w_hit", "w_miss"):
        assert rc(**{w: 0}) == E_ARG and rc(**{w: 32768}) == E_ARG and rc(**{w: -3}) == E_ARG and rc(B=0, **{w: 32767}) == 0
    for missing in ("state", "hits", "ray_table", "evidence", "origin", "cell"):
        assert rc(drop=(missing,)) == E_ARG, missing
    # the window cap: (range + depth, cell) pairs as the oracle counts them
    for rng, depth, cell in ((5.4, 0.0, (0.05, 0.05)), (5.5, 0.0, (0.05, 0.05)), (5.4, 0.1, (0.05, 0.05)), (3.0, 0.005, (0.01, 0.01)),
                             (3.0, 0.0, (0.05, 0.004)), (1.5, 0.025, (0.05, 0.08))):
        want = 0 if M.window_fits(rng, depth, cell) else E_UNSUPPORTED
        assert rc(B=0, lidar_range=rng, depth=depth, cell=cell) == want, (rng, depth, cell)
    assert rc(lidar_range=5.5, depth=0.0) == E_UNSUPPORTED


def test_plan_grid_refusals_reach_no_device():
    lib = lipmpc._lib.load()
    p = lipmpc._lib.LipmpcRrtParamsC()
    assert lib.lipmpc_rrt_default_params(C.byref(p)) == 0
    one = C.c_void_p(8)
    ptrs = dict(occ=one, goal=one, seed=one, workspace=one, sub_goals=one, n_sub=one, status=one, path_cost=one)
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), cell=cs, **kw):
        args = dict(device=0, p=C.byref(p), B=1, W=64, H=64, grid_shared=1, S_max=8)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, origin=C.cast(org, C.c_void_p), cell=C.cast(cell, C.c_void_p)).items() if k not in drop}
        return raw_call("lipmpc_rrt_plan_grid_batch", **q, **args)

    assert rc(B=0) == 0
    assert rc(W=1) == E_ARG and rc(H=1) == E_ARG and rc(S_max=0) == E_ARG and rc(B=-1) == E_ARG
    assert rc(cell=(C.c_double * 2)(0.0, 0.1)) == E_ARG and rc(cell=(C.c_double * 2)(0.1, float("inf"))) == E_ARG
    for missing in tuple(ptrs) + ("origin", "cell"):
        assert rc(drop=(missing,)) == E_ARG, missing
    p.width, p.margin = 0, -1.0                            # ignored on a given grid
    assert rc(B=0) == 0
    p.n_samples = 6000                                     # the tree does not fit the LDS
    assert rc(B=0) == E_ARG
