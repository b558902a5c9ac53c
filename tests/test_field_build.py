"""The grid field planner: C ABI and compiled resources (no GPU needed)."""
import ctypes as C

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
FIELD, PATH = "lipmpc_grid_field_batch", "lipmpc_grid_path_batch"


def test_field_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name in (FIELD, PATH):
        assert name in lipmpc._lib.EXPORTS and name in lipmpc._lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    assert [n for n, _ in lipmpc._lib.SIGNATURES[FIELD][1]] == [
        "device", "F", "W", "H", "grid_shared", "origin", "cell", "occ", "goal", "r_inflate", "field", "field_status", "hip_stream"]
    assert [n for n, _ in lipmpc._lib.SIGNATURES[PATH][1]] == [
        "device", "B", "F", "W", "H", "origin", "cell", "occ", "grid_shared", "field", "field_status", "goal", "start", "r_inflate",
        "max_seg", "S_max", "sub_goals", "n_sub", "status", "path_cost", "hip_stream"]
    assert lib.lipmpc_version() == 5                       # backward-compatible additions
    assert lipmpc.GridFieldPlanner is lipmpc.planner.GridFieldPlanner and lipmpc.FIELD_INF == 0xFFFFFFFF
    assert callable(lipmpc.GridFieldPlanner.field) and callable(lipmpc.GridFieldPlanner.plan_grid_batch)


def test_field_kernels_code_object():
    """From the built library's gfx950 code objects: the two field kernels (field in LDS / in the output buffer) and the path
    kernel exist once each, use no scratch and spill nothing; their LDS is dynamic (sized to the map), so the static part is at
    most the workgroup reduction's few words."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in ("grid_field_lds_kernel", "grid_field_global_kernel", "grid_path_kernel"):
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] <= (0 if k == "grid_path_kernel" else 256), (name, r)     # (256: the slack the LDS rule keeps)


def _pointers(names):
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    return {n: one for n in names}


def test_field_refusals_reach_no_device():
    """Every refusal is decided on the host before anything is enqueued."""
    ptrs = _pointers(("occ", "goal", "field", "field_status"))
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), cell=cs, origin=org, **kw):
        args = dict(device=0, F=0, W=92, H=80, grid_shared=1, r_inflate=0)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, origin=C.cast(origin, C.c_void_p), cell=C.cast(cell, C.c_void_p)).items() if k not in drop}
        return raw_call(FIELD, **q, **args)

    assert rc() == 0                                       # the same arguments pass: F = 0 enqueues nothing
    assert rc(F=-1) == E_ARG
    assert rc(W=1) == E_ARG and rc(H=1) == E_ARG and rc(W=0) == E_ARG and rc(H=-3) == E_ARG and rc(W=2, H=2) == 0
    for bad in ((0.0, 0.1), (0.1, -1.0), (float("nan"), 0.1), (0.1, float("inf"))):
        assert rc(cell=(C.c_double * 2)(*bad)) == E_ARG, bad
    for bad in ((float("nan"), 0.0), (0.0, float("inf")), (float("-inf"), 0.0)):
        assert rc(origin=(C.c_double * 2)(*bad)) == E_ARG, bad
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_inflate=16) == 0
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    for missing in tuple(ptrs):
        assert rc(F=1, drop=(missing,)) == E_ARG, missing
    # the RRT planner's caps
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED and rc(W=4096, H=32) == 0
    assert rc(W=363, H=362) == E_UNSUPPORTED and rc(W=512, H=256) == 0 and rc(W=512, H=257) == E_UNSUPPORTED


def test_path_refusals_reach_no_device():
    ptrs = _pointers(("occ", "field", "field_status", "goal", "start", "sub_goals", "n_sub", "status", "path_cost"))
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), cell=cs, origin=org, **kw):
        args = dict(device=0, B=0, F=1, W=92, H=80, grid_shared=1, r_inflate=0, max_seg=5, S_max=1)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, origin=C.cast(origin, C.c_void_p), cell=C.cast(cell, C.c_void_p)).items() if k not in drop}
        return raw_call(PATH, **q, **args)

    assert rc() == 0 and rc(F=0) == 0                      # B = 0 enqueues nothing (F = 1, or F = B)
    assert rc(B=-1) == E_ARG and rc(B=-1, F=-1) == E_ARG
    assert rc(B=4, F=2) == E_ARG and rc(B=4, F=0) == E_ARG and rc(B=0, F=3) == E_ARG
    assert rc(max_seg=4) == E_ARG and rc(max_seg=0) == E_ARG and rc(max_seg=0x7FFFFFFF) == 0
    assert rc(S_max=0) == E_ARG and rc(S_max=-1) == E_ARG
    assert rc(W=1) == E_ARG and rc(H=1) == E_ARG
    assert rc(cell=(C.c_double * 2)(0.0, 0.1)) == E_ARG and rc(cell=(C.c_double * 2)(0.1, float("inf"))) == E_ARG
    assert rc(origin=(C.c_double * 2)(float("nan"), 0.0)) == E_ARG
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    for missing in tuple(ptrs):
        assert rc(B=3, F=1, drop=(missing,)) == E_ARG and rc(B=3, F=3, drop=(missing,)) == E_ARG, missing
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=363, H=362) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED


def test_planner_parameters_are_checked():
    """(The constructor itself needs a device: only what it refuses before it asks for one is checked here.)"""
    import inspect
    sig = inspect.signature(lipmpc.GridFieldPlanner.__init__)
    assert [p for p in sig.parameters][1:3] == ["r_inflate", "max_seg"]
    assert sig.parameters["r_inflate"].default == 0 and sig.parameters["max_seg"].default is None
    sig = inspect.signature(lipmpc.GridFieldPlanner.plan_grid_batch)
    assert [p for p in sig.parameters][1:] == ["goal", "grid", "start", "S_max", "seeds", "out"] and sig.parameters["S_max"].default == 64
