"""Soft clearance: C ABI, refusals, compiled resources and the planners' keywords (no GPU needed)."""
import ctypes as C
import inspect
import os

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
COST = "lipmpc_grid_clearance_cost_batch"
FIELD, FRONTIER = "lipmpc_grid_field_weighted_batch", "lipmpc_grid_frontier_field_weighted_batch"
PATH, FRONTIER_PATH = "lipmpc_grid_path_weighted_batch", "lipmpc_grid_frontier_path_weighted_batch"
TILED = {FIELD: "lipmpc_grid_field_tiled_batch", FRONTIER: "lipmpc_grid_frontier_field_tiled_batch",
         PATH: "lipmpc_grid_path_tiled_batch", FRONTIER_PATH: "lipmpc_grid_frontier_path_tiled_batch"}
BYTES = "lipmpc_grid_tiled_workspace_bytes"
BIG = 1 << 40


def _names(name):
    return [n for n, _ in lipmpc._lib.SIGNATURES[name][1]]


def test_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name in (COST, FIELD, FRONTIER, PATH, FRONTIER_PATH):
        assert name in lipmpc._lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    assert _names(COST) == ["device", "M", "W", "H", "occ", "evidence", "t_occ", "r_clear", "w_clear", "cost", "hip_stream"]
    for weighted, tiled in TILED.items():                   # the tiled calls' arguments plus one input, cost
        assert [n for n in _names(weighted) if n != "cost"] == _names(tiled) and _names(weighted).count("cost") == 1
        types = dict(lipmpc._lib.SIGNATURES[weighted][1])
        assert types["cost"] is C.c_void_p and all(types[n] is t for n, t in lipmpc._lib.SIGNATURES[tiled][1])
    assert lib.lipmpc_version() == 5                        # backward-compatible additions
    assert lipmpc.planner.COST_MAX == 248 and lipmpc.planner.R_CLEAR_MAX == 31
    header = open(os.path.join(os.path.dirname(lipmpc._lib.LIB_PATH), "..", "include", "lipmpc.h")).read()
    assert "#define LIPMPC_COST_MAX 248" in header and "255 * 2^24" in header


def _pointers(names):
    one = C.c_void_p(8)                                     # device pointers: never dereferenced
    return {n: one for n in names}


def _placement(origin=(0.0, 0.0), cell=(0.1, 0.1)):
    org, cs = (C.c_double * 2)(*origin), (C.c_double * 2)(*cell)
    return dict(origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p)), (org, cs)


def _rc(name, ptrs, base):
    place, keep = _placement()

    def rc(drop=(), **kw):
        args = dict(base)
        args.update(kw)
        q = {k: v for k, v in dict(ptrs, **place).items() if k in _names(name) and k not in drop}
        q.update({k: None for k in drop})
        return raw_call(name, **q, **args)
    rc.keep = keep
    return rc


def test_cost_layer_refusals_reach_no_device():
    """E_ARG, then E_UNSUPPORTED, then M = 0 returns 0: every refusal is decided on the host before anything is enqueued."""
    base = dict(device=0, M=0, W=92, H=80, t_occ=3, r_clear=4, w_clear=16, hip_stream=None)
    occ, ev = _rc(COST, _pointers(("occ", "cost")), base), _rc(COST, _pointers(("evidence", "cost")), base)
    both, neither = _rc(COST, _pointers(("occ", "evidence", "cost")), base), _rc(COST, _pointers(("cost",)), base)
    for rc in (occ, ev):
        assert rc() == 0 and rc(W=2, H=2) == 0 and rc(W=4096, H=4096) == 0 and rc(W=2, H=4096) == 0
        assert rc(M=-1) == E_ARG and rc(W=1) == E_ARG and rc(H=1) == E_ARG
        assert rc(r_clear=0) == E_ARG and rc(r_clear=32) == E_ARG and rc(r_clear=1) == 0 and rc(r_clear=31) == 0
        assert rc(w_clear=-1) == E_ARG and rc(w_clear=249) == E_ARG and rc(w_clear=0) == 0 and rc(w_clear=248) == 0
        assert rc(drop=("cost",)) == E_ARG
        assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED and rc(W=65281, H=257) == E_UNSUPPORTED
        assert rc(M=129, W=4096, H=4096) == E_UNSUPPORTED   # M * (W * H + 64) > 2^31
        # E_ARG comes before the caps
        assert rc(W=4097, H=2, r_clear=32) == E_ARG and rc(W=4097, H=2, w_clear=249) == E_ARG and rc(W=4097, H=2, drop=("cost",)) == E_ARG
    assert both() == E_ARG and neither() == E_ARG and both(W=4097, H=2) == E_ARG and neither(W=4097, H=2) == E_ARG
    # t_occ belongs to the evidence form
    assert ev(t_occ=0) == E_ARG and ev(t_occ=(1 << 30) + 1) == E_ARG and ev(t_occ=1 << 30) == 0 and occ(t_occ=0) == 0


@pytest.mark.parametrize("name", [FIELD, FRONTIER])
def test_weighted_field_refusals_reach_no_device(name):
    """The tiled field calls' refusals in their order -- E_ARG, E_UNSUPPORTED, the workspace, F = 0 -- with a null cost as E_ARG."""
    if name == FIELD:
        ptrs = _pointers(("occ", "cost", "goal", "field", "field_status", "work", "settled"))
        base = dict(device=0, F=0, W=92, H=80, grid_shared=1, r_inflate=0, work_bytes=BIG, max_rounds=1, resume=0, hip_stream=None)
    else:
        ptrs = _pointers(("evidence", "cost", "frontier", "field", "n_frontier", "work", "settled"))
        base = dict(device=0, F=0, W=92, H=80, t_free=1, t_occ=3, r_inflate=0, min_unknown=2, work_bytes=BIG, max_rounds=1, resume=0,
                    hip_stream=None)
    rc = _rc(name, ptrs, base)
    assert rc() == 0 and rc(W=2, H=2) == 0 and rc(W=363, H=362) == 0 and rc(W=4096, H=4096) == 0
    assert rc(F=-1) == E_ARG and rc(W=1) == E_ARG and rc(H=1) == E_ARG
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_inflate=16) == 0
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED and rc(W=65281, H=257) == E_UNSUPPORTED
    for W, H, other in ((92, 80, 0), (4097, 2, E_UNSUPPORTED)):
        assert rc(W=W, H=H) == other
        for missing in ("work", "settled", "cost"):
            assert rc(W=W, H=H, drop=(missing,)) == E_ARG, missing
        for bad in (0, -1, 65537):
            assert rc(W=W, H=H, max_rounds=bad) == E_ARG, bad
        for bad in (-1, 2):
            assert rc(W=W, H=H, resume=bad) == E_ARG, bad
    assert rc(max_rounds=65536, resume=1) == 0
    for F, W, H in ((0, 92, 80), (1, 92, 80), (3, 363, 362)):
        need = raw_call(BYTES, F=F, W=W, H=H)
        assert need > 0 and rc(F=F, W=W, H=H, work_bytes=need - 1) == E_ARG and rc(F=F, W=W, H=H, work_bytes=0) == E_ARG
    for missing in [p for p in ptrs if p != "frontier"]:
        assert rc(drop=(missing,)) == E_ARG, missing
    if name == FIELD:
        assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    else:
        assert rc(drop=("frontier",)) == 0
        assert rc(t_free=0) == E_ARG and rc(t_occ=(1 << 30) + 1) == E_ARG and rc(min_unknown=0) == E_ARG and rc(min_unknown=9) == E_ARG


@pytest.mark.parametrize("name", [PATH, FRONTIER_PATH])
def test_weighted_path_refusals_reach_no_device(name):
    if name == PATH:
        ptrs = _pointers(("occ", "cost", "field", "field_status", "settled", "goal", "start", "sub_goals", "n_sub", "status", "path_cost"))
        base = dict(device=0, B=0, F=1, W=92, H=80, grid_shared=1, r_inflate=0, max_seg=5, S_max=1, hip_stream=None)
    else:
        ptrs = _pointers(("evidence", "cost", "field", "n_frontier", "settled", "start", "sub_goals", "n_sub", "status", "path_cost",
                          "target_cell"))
        base = dict(device=0, B=0, F=1, W=92, H=80, t_occ=3, r_inflate=0, max_seg=5, S_max=1, hip_stream=None)
    rc = _rc(name, ptrs, base)
    assert rc() == 0 and rc(F=0) == 0 and rc(W=363, H=362) == 0 and rc(W=4096, H=4096) == 0
    assert rc(max_seg=0x7FFFFFFF) == 0                      # "no cap", as for the tiled calls
    assert rc(B=-1) == E_ARG and rc(B=4, F=2) == E_ARG and rc(max_seg=4) == E_ARG and rc(S_max=0) == E_ARG
    assert rc(W=1) == E_ARG and rc(H=1) == E_ARG and rc(r_inflate=17) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED
    for missing in tuple(ptrs):
        assert rc(B=3, F=1, drop=(missing,)) == E_ARG and rc(B=3, F=3, drop=(missing,)) == E_ARG, missing


def test_clearance_kernels_code_object():
    """From the built library's gfx950 code objects: every new kernel exists once (the cost kernel once per input form), uses no
    scratch and spills nothing; the weighted round kernel's static LDS stays within what tests/test_field_tiled_build.py allows
    tiled_round_kernel -- a tile with its halo; the descent kernels use no LDS; the cost kernel's bitmap of the grown tile is 94 rows
    of 128 bits."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    tw, th, _ = lipmpc.tiled_info()
    kernels = {"soft_cost_kernel": 2, "soft_round_kernel": 1, "soft_goal_descent_kernel": 1, "soft_frontier_descent_kernel": 1}
    for k, count in kernels.items():
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == count, (k, sorted(mine))
        for name, r in mine.items():
            print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
            if k == "soft_round_kernel":
                halo = (tw + 2) * (th + 2)
                assert 4 * halo <= r["group_segment_fixed_size"] <= 4 * halo + halo // 8 + 512 <= 160 * 1024 // 8, (name, r)
            elif "descent" in k:
                assert r["group_segment_fixed_size"] == 0, (name, r)
            else:
                rows = tw + 2 * lipmpc.planner.R_CLEAR_MAX
                assert 16 * rows <= r["group_segment_fixed_size"] <= 16 * rows + 512, (name, r)
    assert len([n for n in res if "soft_" in n]) == sum(kernels.values())
    # no new kernel's name holds a substring by which the existing build tests count theirs
    for name in (n for n in res if "soft_" in n):
        assert not any(s in name for s in ("tiled_", "tile_", "claim_", "keep_", "grid_path_kernel", "frontier_path_kernel", "grid_field_lds_kernel"))
    # the round kernel is the existing one's size class: the same LDS, one more 64-bit register pair at the most in flight
    old, = (r for n, r in res.items() if "tiled_round_kernel" in n)
    new, = (r for n, r in res.items() if "soft_round_kernel" in n)
    assert new["group_segment_fixed_size"] == old["group_segment_fixed_size"]


def test_planner_keywords():
    """r_clear / w_clear: keyword-only, off before __init__, both or neither, tiled only, refused by the unweighted planners -- every
    refusal a ValueError before a device is asked for."""
    for cls in (lipmpc.GridFieldPlanner, lipmpc.FrontierPlanner):
        p = inspect.signature(cls).parameters
        assert p["r_clear"].default is None and p["w_clear"].default is None
        assert p["r_clear"].kind is p["w_clear"].kind is inspect.Parameter.KEYWORD_ONLY
        assert "r_clear" not in inspect.signature(cls.__init__).parameters and "w_clear" not in inspect.signature(cls.__init__).parameters
        with pytest.raises(ValueError, match="tiled"):
            cls(r_clear=4, w_clear=16)
        with pytest.raises(ValueError, match="tiled"):
            cls(tiled=False, r_clear=4, w_clear=16)
        for kw in (dict(r_clear=4), dict(w_clear=16)):
            with pytest.raises(ValueError, match="go together"):
                cls(tiled=True, **kw)
        for kw in (dict(r_clear=0, w_clear=16), dict(r_clear=32, w_clear=16), dict(r_clear=4, w_clear=-1), dict(r_clear=4, w_clear=249)):
            with pytest.raises(ValueError, match="clearance"):
                cls(tiled=True, **kw)
        assert "cost" not in inspect.signature(cls.plan_grid_batch if cls is lipmpc.GridFieldPlanner else cls.plan).parameters
        assert "cost" not in inspect.signature(cls.field).parameters
    unweighted = [(lipmpc.CoordinatedFrontierPlanner, dict(r_claim=4)), (lipmpc.TiledCoordinatedFrontierPlanner, dict(r_claim=4)),
                  (lipmpc.InformedFrontierPlanner, dict(r_view=8, w_gain=16, g_cap=64)),
                  (lipmpc.TiledInformedFrontierPlanner, dict(r_view=8, w_gain=16, g_cap=64))]
    for cls, kw in unweighted:
        for more in (dict(r_clear=4, w_clear=16), dict(r_clear=4), dict(w_clear=0), dict(r_clear=31, w_clear=248)):
            with pytest.raises(ValueError, match="unweighted"):
                cls(**kw, **more)
