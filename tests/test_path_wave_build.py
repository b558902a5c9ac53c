"""Wave-per-robot path calls: C ABI, refusals, compiled resources and the planners' keyword (no GPU needed)."""
import ctypes as C
import inspect

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
GOAL, FRONTIER, UTILITY = "lipmpc_grid_path_wave_batch", "lipmpc_grid_frontier_path_wave_batch", "lipmpc_grid_frontier_utility_path_wave_batch"
SAME_ARGUMENTS = {GOAL: "lipmpc_grid_path_weighted_batch", FRONTIER: "lipmpc_grid_frontier_path_weighted_batch",
                  UTILITY: "lipmpc_grid_frontier_utility_path_tiled_batch"}
KERNELS = ("wavewalk_goal_kernel", "wavewalk_frontier_kernel", "wavewalk_utility_kernel")
# the substrings by which the existing build tests count their kernels
COUNTED = ("tiled_", "tile_", "claim_", "keep_", "soft_", "grid_path_kernel", "frontier_path_kernel", "grid_field_", "frontier_field_",
           "frontier_utility_", "frontier_assign_", "frontier_gain_")
PLANNERS = [(lipmpc.GridFieldPlanner, {}), (lipmpc.FrontierPlanner, {}), (lipmpc.CoordinatedFrontierPlanner, dict(r_claim=4)),
            (lipmpc.TiledCoordinatedFrontierPlanner, dict(r_claim=4)), (lipmpc.InformedFrontierPlanner, dict(r_view=8, w_gain=16, g_cap=64)),
            (lipmpc.TiledInformedFrontierPlanner, dict(r_view=8, w_gain=16, g_cap=64))]


def _names(name):
    return [n for n, _ in lipmpc._lib.SIGNATURES[name][1]]


def test_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name, twin in SAME_ARGUMENTS.items():
        assert name in lipmpc._lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
        assert lipmpc._lib.SIGNATURES[name] == lipmpc._lib.SIGNATURES[twin]             # names, order and types
    assert lib.lipmpc_version() == 5                        # backward-compatible additions


def _pointers(names):
    one = C.c_void_p(8)                                     # device pointers: never dereferenced
    return {n: one for n in names}


def _rc(name, ptrs, base):
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)
    place = dict(origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p))

    def rc(drop=(), **kw):
        args = dict(base)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, **place).items() if k not in drop}
        return raw_call(name, **q, **args)
    rc.keep = org, cs
    return rc


CALLS = {
    GOAL: (("occ", "cost", "field", "field_status", "settled", "goal", "start", "sub_goals", "n_sub", "status", "path_cost"),
           dict(grid_shared=1), ("cost", "settled")),
    FRONTIER: (("evidence", "cost", "field", "n_frontier", "settled", "start", "sub_goals", "n_sub", "status", "path_cost", "target_cell"),
               dict(t_occ=3), ("cost", "settled")),
    UTILITY: (("evidence", "frontier", "gain", "ufield", "n_sources", "settled", "start", "sub_goals", "n_sub", "status", "path_cost",
               "target_cell", "target_gain"), dict(t_occ=3, w_gain=16, g_cap=64, min_gain=0), ("settled",)),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_refusals_reach_no_device(name):
    """The tiled path calls' ladder in every form: E_ARG, then the tiled caps, then B = 0 returns 0, then the null pointers -- all on the
    host, with pointers that are never dereferenced."""
    pointers, more, nullable = CALLS[name]
    rc = _rc(name, _pointers(pointers), dict(device=0, B=0, F=1, W=92, H=80, r_inflate=0, max_seg=5, S_max=1, hip_stream=None, **more))
    forms = [(), ("cost",), ("cost", "settled")] if "cost" in nullable else [(), ("settled",)]
    for form in forms:
        assert rc(drop=form) == 0 and rc(drop=form, F=0) == 0 and rc(drop=form, max_seg=0x7FFFFFFF) == 0
        # the tiled caps in every form: 363 x 362 is beyond the one-workgroup calls' 2^17 cells
        assert rc(drop=form, W=363, H=362) == 0 and rc(drop=form, W=4096, H=4096) == 0 and rc(drop=form, W=2, H=2) == 0
        assert rc(drop=form, B=-1) == E_ARG and rc(drop=form, B=4, F=2) == E_ARG and rc(drop=form, max_seg=4) == E_ARG
        assert rc(drop=form, S_max=0) == E_ARG and rc(drop=form, W=1) == E_ARG and rc(drop=form, H=1) == E_ARG
        assert rc(drop=form, r_inflate=17) == E_ARG and rc(drop=form, r_inflate=-1) == E_ARG and rc(drop=form, r_inflate=16) == 0
        assert rc(drop=form + ("origin",)) == E_ARG and rc(drop=form + ("cell",)) == E_ARG
        assert rc(drop=form, W=4097, H=2) == E_UNSUPPORTED and rc(drop=form, W=2, H=4097) == E_UNSUPPORTED
        assert rc(drop=form, W=65281, H=257) == E_UNSUPPORTED                                   # W * H > 2^24
        assert rc(drop=form, B=129, F=129, W=4096, H=4096) == E_UNSUPPORTED                     # F * (W * H + 64) > 2^31
        # E_ARG comes before the caps
        assert rc(drop=form, W=4097, H=2, max_seg=4) == E_ARG and rc(drop=form, W=4097, H=2, S_max=0) == E_ARG
        assert rc(drop=form, W=4097, H=2, B=4, F=2) == E_ARG and rc(drop=form + ("origin",), W=4097, H=2) == E_ARG
        if "t_occ" in more:
            assert rc(drop=form, t_occ=0) == E_ARG and rc(drop=form, t_occ=(1 << 30) + 1) == E_ARG and rc(drop=form, W=4097, H=2, t_occ=0) == E_ARG
        # B = 0 returns before the null-pointer checks; with B > 0 every pointer but the nullable ones is needed
        for missing in (p for p in pointers if p not in nullable):
            assert rc(drop=form + (missing,)) == 0, missing
            assert rc(B=3, F=1, drop=form + (missing,)) == E_ARG and rc(B=3, F=3, drop=form + (missing,)) == E_ARG, missing
            assert rc(B=3, F=3, W=4097, H=2, drop=form + (missing,)) == E_UNSUPPORTED, missing
    if "cost" in nullable:                                   # a cost layer without the settled word: E_ARG, first
        assert rc(drop=("settled",)) == E_ARG and rc(drop=("settled",), B=3) == E_ARG and rc(drop=("settled",), W=4097, H=2) == E_ARG
    else:
        for bad in (dict(w_gain=-1), dict(w_gain=65536), dict(g_cap=0), dict(g_cap=16385), dict(min_gain=-1), dict(min_gain=16385)):
            assert rc(**bad) == E_ARG and rc(W=4097, H=2, **bad) == E_ARG, bad


def test_wave_kernels_code_object():
    """From the built library's gfx950 code objects: each new kernel exists once, uses no scratch and spills nothing, and -- two
    passes, every piece of state in registers, four waves that share nothing -- uses NO LDS at all (docs: DESIGN.md, the wave-per-robot
    path calls); a workgroup is 256 threads; no name holds a substring by which the existing build tests count theirs."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in KERNELS:
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 256, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)              # eight waves a SIMD: occupancy is not the registers' to limit
        assert not any(s in name for s in COUNTED), name
    assert len([n for n in res if "wavewalk_" in n]) == len(KERNELS)
    # the one-lane path kernels are all still there, once each
    for k in ("grid_path_kernel", "frontier_path_kernel", "frontier_utility_path_kernel", "tiled_goal_descent_kernel",
              "tiled_frontier_descent_kernel", "soft_goal_descent_kernel", "soft_frontier_descent_kernel", "tile_utility_descent_kernel"):
        assert len([n for n in res if k in n and "wavewalk" not in n]) == 1, k


def test_planner_keyword():
    """paths: keyword-only, "lane" by default, off before __init__, anything else a ValueError before a device is asked for."""
    for cls, kw in PLANNERS:
        p = inspect.signature(cls).parameters
        assert p["paths"].default == "lane" and p["paths"].kind is inspect.Parameter.KEYWORD_ONLY
        for k in cls.__mro__:
            if "__init__" in vars(k) and k is not object:
                assert "paths" not in inspect.signature(k.__init__).parameters, k
        for bad in ("Wave", "lanes", "", None, 64, True):
            with pytest.raises(ValueError, match="paths"):
                cls(**kw, paths=bad, device="no such device")
