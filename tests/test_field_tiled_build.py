"""The tiled field calls: C ABI, refusals and compiled resources (no GPU needed)."""
import ctypes as C
import inspect

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
INFO, BYTES = "lipmpc_grid_tiled_info", "lipmpc_grid_tiled_workspace_bytes"
FIELD, FRONTIER = "lipmpc_grid_field_tiled_batch", "lipmpc_grid_frontier_field_tiled_batch"
PATH, FRONTIER_PATH = "lipmpc_grid_path_tiled_batch", "lipmpc_grid_frontier_path_tiled_batch"
TILED_TAIL = ["work", "work_bytes", "max_rounds", "resume", "settled", "hip_stream"]
BIG = 1 << 40                                              # a work_bytes no shape within the caps needs


def _names(name):
    return [n for n, _ in lipmpc._lib.SIGNATURES[name][1]]


def test_tiled_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name in (INFO, BYTES, FIELD, FRONTIER, PATH, FRONTIER_PATH):
        assert name in lipmpc._lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    # the field calls: the one-workgroup calls' arguments, then the tiled ones; the path calls: one more input, settled
    assert _names(FIELD) == _names("lipmpc_grid_field_batch")[:-1] + TILED_TAIL
    assert _names(FRONTIER) == _names("lipmpc_grid_frontier_field_batch")[:-1] + TILED_TAIL
    for tiled, plain in ((PATH, "lipmpc_grid_path_batch"), (FRONTIER_PATH, "lipmpc_grid_frontier_path_batch")):
        assert [n for n in _names(tiled) if n != "settled"] == _names(plain) and "settled" in _names(tiled)
    assert lib.lipmpc_version() == 5                       # backward-compatible additions
    assert lipmpc.RRT_FIELD_UNSETTLED == 8 and lipmpc.RRT_STATUS_NAMES[8] == "FIELD_UNSETTLED"
    for cls in (lipmpc.GridFieldPlanner, lipmpc.FrontierPlanner):         # keyword-only, off before __init__, whose signature stays
        p = inspect.signature(cls).parameters
        assert p["tiled"].default is False and p["rounds"].default is None
        assert p["tiled"].kind is p["rounds"].kind is inspect.Parameter.KEYWORD_ONLY
        assert "tiled" not in inspect.signature(cls.__init__).parameters
    with pytest.raises(ValueError, match="rounds"):
        lipmpc.GridFieldPlanner(rounds=4)                  # (refused before a device is asked for: rounds without tiled)
    with pytest.raises(ValueError, match="rounds"):
        lipmpc.FrontierPlanner(tiled=True, rounds=65537)
    with pytest.raises(ValueError, match="tiled"):
        lipmpc.CoordinatedFrontierPlanner(r_claim=4, tiled=True)
    with pytest.raises(ValueError, match="tiled"):
        lipmpc.InformedFrontierPlanner(r_view=8, w_gain=16, g_cap=64, tiled=True)


def test_tiled_info_and_workspace_size():
    tw, th, cap = lipmpc.tiled_info()
    assert tw >= 2 and th >= 2 and cap == 1 << 24
    one = C.c_int64()
    assert raw_call(INFO, tile_w=None, tile_h=C.c_void_p(C.addressof(one)), max_cells=C.c_void_p(C.addressof(one))) == E_ARG
    size = lambda F, W, H: raw_call(BYTES, F=F, W=W, H=H)
    assert size(-1, 8, 8) == E_ARG and size(1, 1, 8) == E_ARG and size(1, 8, 1) == E_ARG
    assert size(1, 4097, 2) == E_UNSUPPORTED and size(1, 2, 4097) == E_UNSUPPORTED and size(1, 4096, 4096) > 0
    assert size(1, 65281, 257) == E_UNSUPPORTED            # 2^24 + 1 cells
    assert size(129, 4096, 4096) == E_UNSUPPORTED and size(128, 4096, 4095) > 0       # the threads of one launch
    # monotone in F, W and H (and it grows over a tile border and over a bitmap word)
    shapes = [2, 3, tw - 1, tw, tw + 1, th - 1, th, th + 1, 2 * th, 362, 363, 1024, 4096]
    for F in (0, 1, 2, 3, 64):
        for a, b in zip(shapes, shapes[1:]):
            for other in (2, 63, 362):
                assert size(F, a, other) <= size(F, b, other) and size(F, other, a) <= size(F, other, b), (F, a, b, other)
                assert size(F, a, other) <= size(F + 1, a, other)
    assert size(1, tw, th) < size(1, tw + 1, th) and size(1, tw, th) < size(1, tw, th + 1) and size(1, 363, 362) < size(2, 363, 362)


def _pointers(names):
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
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


@pytest.mark.parametrize("name", [FIELD, FRONTIER])
def test_tiled_field_refusals_reach_no_device(name):
    """E_ARG, then E_UNSUPPORTED, then F = 0 returns 0: every refusal is decided on the host before anything is enqueued."""
    if name == FIELD:
        ptrs = _pointers(("occ", "goal", "field", "field_status", "work", "settled"))
        base = dict(device=0, F=0, W=92, H=80, grid_shared=1, r_inflate=0, work_bytes=BIG, max_rounds=1, resume=0, hip_stream=None)
    else:
        ptrs = _pointers(("evidence", "frontier", "field", "n_frontier", "work", "settled"))
        base = dict(device=0, F=0, W=92, H=80, t_free=1, t_occ=3, r_inflate=0, min_unknown=2, work_bytes=BIG, max_rounds=1, resume=0,
                    hip_stream=None)
    rc = _rc(name, ptrs, base)
    assert rc() == 0 and rc(W=2, H=2) == 0                 # the same arguments pass: F = 0 enqueues nothing
    assert rc(W=363, H=362) == 0 and rc(W=4096, H=4096) == 0          # beyond the one-workgroup calls' cap
    assert rc(F=-1) == E_ARG and rc(W=1) == E_ARG and rc(H=1) == E_ARG
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_inflate=16) == 0
    # the caps, whatever F
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED and rc(W=65281, H=257) == E_UNSUPPORTED
    # what the tiled calls add, each alone -- and each BEFORE the caps
    for W, H, other in ((92, 80, 0), (4097, 2, E_UNSUPPORTED)):
        assert rc(W=W, H=H) == other
        assert rc(W=W, H=H, drop=("work",)) == E_ARG and rc(W=W, H=H, drop=("settled",)) == E_ARG
        for bad in (0, -1, 65537):
            assert rc(W=W, H=H, max_rounds=bad) == E_ARG, bad
        for bad in (-1, 2):
            assert rc(W=W, H=H, resume=bad) == E_ARG, bad
    assert rc(max_rounds=65536, resume=1) == 0
    for F, W, H in ((0, 92, 80), (1, 92, 80), (3, 363, 362)):
        need = raw_call(BYTES, F=F, W=W, H=H)
        assert need > 0 and rc(F=F, W=W, H=H, work_bytes=need - 1) == E_ARG and rc(F=F, W=W, H=H, work_bytes=0) == E_ARG
    assert rc(work_bytes=raw_call(BYTES, F=0, W=92, H=80)) == 0
    required = [p for p in ptrs if p != "frontier"]        # (frontier may be NULL, as for the one-workgroup call)
    for missing in required:
        assert rc(drop=(missing,)) == E_ARG, missing
    if name == FIELD:
        place, keep = _placement(cell=(0.0, 0.1))
        assert raw_call(name, **ptrs, **dict(place), **base) == E_ARG
        assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    else:
        assert rc(drop=("frontier",)) == 0
        assert rc(t_free=0) == E_ARG and rc(t_occ=(1 << 30) + 1) == E_ARG and rc(min_unknown=0) == E_ARG and rc(min_unknown=9) == E_ARG


@pytest.mark.parametrize("name", [PATH, FRONTIER_PATH])
def test_tiled_path_refusals_reach_no_device(name):
    if name == PATH:
        ptrs = _pointers(("occ", "field", "field_status", "settled", "goal", "start", "sub_goals", "n_sub", "status", "path_cost"))
        base = dict(device=0, B=0, F=1, W=92, H=80, grid_shared=1, r_inflate=0, max_seg=5, S_max=1, hip_stream=None)
    else:
        ptrs = _pointers(("evidence", "field", "n_frontier", "settled", "start", "sub_goals", "n_sub", "status", "path_cost", "target_cell"))
        base = dict(device=0, B=0, F=1, W=92, H=80, t_occ=3, r_inflate=0, max_seg=5, S_max=1, hip_stream=None)
    rc = _rc(name, ptrs, base)
    assert rc() == 0 and rc(F=0) == 0 and rc(W=363, H=362) == 0 and rc(W=4096, H=4096) == 0
    assert rc(B=-1) == E_ARG and rc(B=4, F=2) == E_ARG and rc(max_seg=4) == E_ARG and rc(S_max=0) == E_ARG
    assert rc(W=1) == E_ARG and rc(H=1) == E_ARG and rc(r_inflate=17) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED
    for missing in tuple(ptrs):
        assert rc(B=3, F=1, drop=(missing,)) == E_ARG and rc(B=3, F=3, drop=(missing,)) == E_ARG, missing


def test_one_workgroup_calls_keep_their_cap():
    """The four existing calls refuse 363 x 362 as before."""
    place, keep = _placement()
    ptrs = _pointers(("occ", "goal", "field", "field_status"))
    assert raw_call("lipmpc_grid_field_batch", device=0, F=0, W=363, H=362, grid_shared=1, r_inflate=0, hip_stream=None, **ptrs, **place) == E_UNSUPPORTED
    ptrs = _pointers(("evidence", "frontier", "field", "n_frontier"))
    assert raw_call("lipmpc_grid_frontier_field_batch", device=0, F=0, W=363, H=362, t_free=1, t_occ=3, r_inflate=0, min_unknown=2,
                    hip_stream=None, **ptrs) == E_UNSUPPORTED


def test_tiled_kernels_code_object():
    """From the built library's gfx950 code objects: every new kernel exists once, uses no scratch and spills nothing; the round
    kernel's LDS is static -- a tile with its halo -- and far within the 160 KiB of a workgroup, so that many tiles share a CU."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    tw, th, _ = lipmpc.tiled_info()
    kernels = {"tiled_bitmaps_kernel": 2, "tiled_blocked_kernel": 2, "tiled_goal_seed_kernel": 1, "tiled_frontier_seed_kernel": 1,
               "tiled_round_kernel": 1, "tiled_settle_kernel": 1, "tiled_goal_descent_kernel": 1, "tiled_frontier_descent_kernel": 1}
    for k, count in kernels.items():
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == count, (k, sorted(mine))
        for name, r in mine.items():
            print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
            assert r["group_segment_fixed_size"] <= 160 * 1024, (name, r)
            if k == "tiled_round_kernel":
                halo = (tw + 2) * (th + 2)
                assert 4 * halo <= r["group_segment_fixed_size"] <= 4 * halo + halo // 8 + 512 <= 160 * 1024 // 8, (name, r)
            elif "descent" in k:
                assert r["group_segment_fixed_size"] == 0, (name, r)
    assert len([n for n in res if "tiled_" in n]) == sum(kernels.values())
