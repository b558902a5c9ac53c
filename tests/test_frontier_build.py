"""The frontier explorer: C ABI and compiled resources (no GPU needed)."""
import ctypes as C
import inspect

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
FIELD, PATH = "lipmpc_grid_frontier_field_batch", "lipmpc_grid_frontier_path_batch"


def test_frontier_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name in (FIELD, PATH):
        assert name in lipmpc._lib.EXPORTS and name in lipmpc._lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    assert [n for n, _ in lipmpc._lib.SIGNATURES[FIELD][1]] == [
        "device", "F", "W", "H", "evidence", "t_free", "t_occ", "r_inflate", "min_unknown", "frontier", "field", "n_frontier", "hip_stream"]
    assert [n for n, _ in lipmpc._lib.SIGNATURES[PATH][1]] == [
        "device", "B", "F", "W", "H", "origin", "cell", "evidence", "t_occ", "field", "n_frontier", "start", "r_inflate", "max_seg",
        "S_max", "sub_goals", "n_sub", "status", "path_cost", "target_cell", "hip_stream"]
    assert lib.lipmpc_version() == 5                       # backward-compatible additions
    assert lipmpc.FrontierPlanner is lipmpc.planner.FrontierPlanner
    assert callable(lipmpc.FrontierPlanner.field) and callable(lipmpc.FrontierPlanner.plan)
    assert callable(lipmpc.UnknownEnvFleet.run_exploring)


def test_frontier_kernels_code_object():
    """From the built library's gfx950 code objects: the two frontier field kernels (field in LDS / in the output buffer) and the
    path kernel exist once each, use no scratch and spill nothing; the field kernels' static LDS is the frontier count and the
    workgroup reduction's words, within the slack the LDS rule keeps."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    for k in ("frontier_field_lds_kernel", "frontier_field_global_kernel", "frontier_path_kernel"):
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] <= (0 if k == "frontier_path_kernel" else 256), (name, r)


def _pointers(names):
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    return {n: one for n in names}


def test_frontier_field_refusals_reach_no_device():
    """Every refusal is decided on the host before anything is enqueued."""
    ptrs = _pointers(("evidence", "frontier", "field", "n_frontier"))

    def rc(drop=(), **kw):
        args = dict(device=0, F=0, W=92, H=80, t_free=1, t_occ=3, r_inflate=2, min_unknown=2)
        args.update(kw)
        return raw_call(FIELD, **{k: v for k, v in ptrs.items() if k not in drop}, **args)

    assert rc() == 0                                       # the same arguments pass: F = 0 enqueues nothing
    assert rc(drop=("frontier",)) == 0                     # (optional)
    assert rc(F=-1) == E_ARG
    assert rc(W=1) == E_ARG and rc(H=1) == E_ARG and rc(W=0) == E_ARG and rc(H=-3) == E_ARG and rc(W=2, H=2) == 0
    for name in ("t_free", "t_occ"):
        assert rc(**{name: 0}) == E_ARG and rc(**{name: -1}) == E_ARG and rc(**{name: (1 << 30) + 1}) == E_ARG, name
        assert rc(**{name: -(1 << 31)}) == E_ARG and rc(**{name: (1 << 31) - 1}) == E_ARG, name
        assert rc(**{name: 1 << 30}) == 0 and rc(**{name: 1}) == 0, name
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_inflate=16) == 0 and rc(r_inflate=0) == 0
    assert rc(min_unknown=0) == E_ARG and rc(min_unknown=9) == E_ARG and rc(min_unknown=1) == 0 and rc(min_unknown=8) == 0
    for missing in ("evidence", "field", "n_frontier"):
        assert rc(F=1, drop=(missing,)) == E_ARG and rc(F=3, drop=(missing,)) == E_ARG, missing
    # the existing caps
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED and rc(W=4096, H=32) == 0
    assert rc(W=363, H=362) == E_UNSUPPORTED and rc(W=512, H=256) == 0 and rc(W=512, H=257) == E_UNSUPPORTED


def test_frontier_path_refusals_reach_no_device():
    ptrs = _pointers(("evidence", "field", "n_frontier", "start", "sub_goals", "n_sub", "status", "path_cost", "target_cell"))
    org, cs = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(0.1, 0.1)

    def rc(drop=(), cell=cs, origin=org, **kw):
        args = dict(device=0, B=0, F=1, W=92, H=80, t_occ=3, r_inflate=0, max_seg=5, S_max=1)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, origin=C.cast(origin, C.c_void_p), cell=C.cast(cell, C.c_void_p)).items() if k not in drop}
        return raw_call(PATH, **q, **args)

    assert rc() == 0 and rc(F=0) == 0                      # B = 0 enqueues nothing (F = 1, or F = B)
    assert rc(B=-1) == E_ARG and rc(B=-1, F=-1) == E_ARG
    assert rc(B=4, F=2) == E_ARG and rc(B=4, F=0) == E_ARG and rc(B=0, F=3) == E_ARG
    assert rc(max_seg=4) == E_ARG and rc(max_seg=0) == E_ARG and rc(max_seg=0x7FFFFFFF) == 0
    assert rc(S_max=0) == E_ARG and rc(S_max=-1) == E_ARG
    assert rc(t_occ=0) == E_ARG and rc(t_occ=(1 << 30) + 1) == E_ARG and rc(t_occ=1 << 30) == 0
    assert rc(W=1) == E_ARG and rc(H=1) == E_ARG
    assert rc(cell=(C.c_double * 2)(0.0, 0.1)) == E_ARG and rc(cell=(C.c_double * 2)(0.1, float("inf"))) == E_ARG
    assert rc(origin=(C.c_double * 2)(float("nan"), 0.0)) == E_ARG
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    for missing in tuple(ptrs):
        assert rc(B=3, F=1, drop=(missing,)) == E_ARG and rc(B=3, F=3, drop=(missing,)) == E_ARG, missing
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=363, H=362) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED


def test_frontier_planner_parameters():
    """(The constructor needs a device to finish: what it refuses before it asks for one is checked here.)"""
    import pytest
    sig = inspect.signature(lipmpc.FrontierPlanner.__init__)
    assert [p for p in sig.parameters][1:] == ["r_inflate", "min_unknown", "t_free", "t_occ", "max_seg", "device"]
    assert [sig.parameters[p].default for p in ("r_inflate", "min_unknown", "t_free", "t_occ", "max_seg", "device")] == [2, 2, None, None, None, None]
    sig = inspect.signature(lipmpc.FrontierPlanner.plan)
    assert [p for p in sig.parameters][1:] == ["mapper_or_evidence", "start", "origin", "cell", "S_max", "out"] and sig.parameters["S_max"].default == 64
    assert [p for p in inspect.signature(lipmpc.FrontierPlanner.field).parameters][1:] == ["mapper_or_evidence", "out"]
    for bad in (dict(r_inflate=17), dict(r_inflate=-1), dict(min_unknown=0), dict(min_unknown=9), dict(t_free=0), dict(t_occ=(1 << 30) + 1),
                dict(max_seg=4)):
        with pytest.raises(ValueError):
            lipmpc.FrontierPlanner(**bad)
    sig = inspect.signature(lipmpc.UnknownEnvFleet.run_exploring)
    assert [p for p in sig.parameters][1:] == ["state0", "first_foot", "k_max", "explorer", "replan_every", "lookahead", "noise", "noise_seed",
                                                "delta", "stop_obj", "use_graph", "S_max"]
