"""The tiled explorers (include/lipmpc.h, TILED EXPLORERS): C ABI, refusals in their stated order, compiled resources and the two
large-map planner classes (no GPU needed)."""
import ctypes as C
import inspect

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
GAIN, UFIELD, UPATH = ("lipmpc_grid_frontier_gain_tiled_batch", "lipmpc_grid_frontier_utility_field_tiled_batch",
                       "lipmpc_grid_frontier_utility_path_tiled_batch")
ASSIGN, ASSIGN_BYTES = "lipmpc_grid_frontier_assign_tiled_batch", "lipmpc_grid_frontier_assign_tiled_workspace_bytes"
GAIN_LDS = "lipmpc_grid_frontier_gain_tiled_lds_bytes"               # host only: what the gain call passes at launch
BYTES = "lipmpc_grid_tiled_workspace_bytes"
TILED_TAIL = ["work", "work_bytes", "max_rounds", "resume", "settled", "hip_stream"]
BIG = 1 << 40                                              # a work_bytes no shape within the caps needs
ONE = C.c_void_p(8)                                        # device pointers: never dereferenced
POINTERS = {
    GAIN: ("evidence", "frontier", "gain"),
    UFIELD: ("evidence", "frontier", "gain", "ufield", "n_sources", "work", "settled"),
    UPATH: ("evidence", "frontier", "gain", "ufield", "n_sources", "settled", "start", "sub_goals", "n_sub", "status", "path_cost",
            "target_cell", "target_gain"),
    ASSIGN: ("frontier", "field", "settled", "start", "may_claim", "work", "sub_goals", "n_sub", "status", "path_cost", "target_cell",
             "claim_round", "n_claims", "claims_settled"),
}


def _names(name):
    return [n for n, _ in lipmpc._lib.SIGNATURES[name][1]]


def test_the_five_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name in (GAIN, UFIELD, UPATH, ASSIGN, ASSIGN_BYTES, GAIN_LDS):
        assert name in lipmpc._lib.EXPORTS and name in lipmpc._lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    assert lib.lipmpc_version() == 5                       # backward-compatible additions
    # the gain: the one-workgroup call's arguments, word for word
    assert _names(GAIN) == _names("lipmpc_grid_frontier_gain_batch")
    # the utility field: what the frontier field call was given, the one-workgroup utility call's own (without `field`), the tail
    front = _names("lipmpc_grid_frontier_field_batch")
    plain = _names("lipmpc_grid_frontier_utility_field_batch")
    given = front[:front.index("min_unknown")]             # device F W H evidence t_free t_occ r_inflate
    own = [n for n in plain[plain.index("frontier"):-1] if n != "field"]
    assert _names(UFIELD) == given + own + TILED_TAIL and "field" not in _names(UFIELD)
    # the path: one more input, settled
    assert [n for n in _names(UPATH) if n != "settled"] == _names("lipmpc_grid_frontier_utility_path_batch") and "settled" in _names(UPATH)
    # the claims: settled behind field, the workspace's size and the budget behind work, claims_settled behind n_claims
    more = {"settled": "field", "work_bytes": "work", "max_rounds": "work_bytes", "claims_settled": "n_claims"}
    names = _names(ASSIGN)
    assert [n for n in names if n not in more] == _names("lipmpc_grid_frontier_assign_batch")
    for n, before in more.items():
        assert names[names.index(n) - 1] == before, n
    assert _names(ASSIGN_BYTES) == ["W", "H"] and lipmpc._lib.SIGNATURES[ASSIGN_BYTES][0] is C.c_int64
    assert _names(GAIN_LDS) == ["r_view"] and lipmpc._lib.SIGNATURES[GAIN_LDS][0] is C.c_int64


def _placement(origin=(0.0, 0.0), cell=(0.1, 0.1)):
    org, cs = (C.c_double * 2)(*origin), (C.c_double * 2)(*cell)
    return dict(origin=C.cast(org, C.c_void_p), cell=C.cast(cs, C.c_void_p)), (org, cs)


def _rc(name, base, placed=False):
    place, keep = _placement() if placed else ({}, None)

    def rc(drop=(), ptr=None, **kw):
        args = dict(base)
        args.update(kw)
        q = {k: v for k, v in dict({n: ONE for n in POINTERS[name]}, **place).items() if k not in drop}
        q.update(ptr or {})                                # another address for some pointer
        return raw_call(name, **q, **args)
    rc.keep = keep
    return rc


def _caps(rc, count):
    """E_ARG before the caps, the caps before "nothing to do"; 363 x 362 and 4096 x 4096 pass."""
    assert rc() == 0 and rc(W=2, H=2) == 0 and rc(W=363, H=362) == 0 and rc(W=4096, H=4096) == 0
    assert rc(W=1) == E_ARG and rc(H=1) == E_ARG and rc(W=0) == E_ARG and rc(H=-3) == E_ARG
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED and rc(W=65281, H=257) == E_UNSUPPORTED     # 2^24 + 1 cells
    assert rc(**{count: -1}) == E_ARG and rc(**{count: 1 << 31}) == E_ARG
    assert rc(W=4097, H=2, **{count: -1}) == E_ARG


def _gain_ranges(rc):
    assert rc(w_gain=-1) == E_ARG and rc(w_gain=65536) == E_ARG and rc(w_gain=0) == 0 and rc(w_gain=65535) == 0
    assert rc(g_cap=0) == E_ARG and rc(g_cap=16385) == E_ARG and rc(g_cap=1) == 0 and rc(g_cap=16384) == 0
    assert rc(min_gain=-1) == E_ARG and rc(min_gain=16385) == E_ARG and rc(min_gain=0) == 0 and rc(min_gain=16384) == 0
    assert rc(W=4097, H=2, w_gain=-1) == E_ARG and rc(W=4097, H=2, g_cap=0) == E_ARG and rc(W=4097, H=2, min_gain=16385) == E_ARG


def test_tiled_gain_refusals_reach_no_device():
    rc = _rc(GAIN, dict(device=0, F=0, W=92, H=80, t_free=1, t_occ=3, r_view=10, hip_stream=None))
    _caps(rc, "F")
    assert rc(F=129, W=4096, H=4096) == E_UNSUPPORTED      # the threads of one launch
    assert rc(r_view=0) == E_ARG and rc(r_view=65) == E_ARG and rc(r_view=1) == 0 and rc(r_view=64) == 0
    for t in ("t_free", "t_occ"):
        assert rc(**{t: 0}) == E_ARG and rc(**{t: (1 << 30) + 1}) == E_ARG and rc(**{t: 1 << 30}) == 0
    for missing in POINTERS[GAIN]:
        assert rc(drop=(missing,)) == E_ARG and rc(F=3, drop=(missing,)) == E_ARG and rc(W=4097, H=2, drop=(missing,)) == E_ARG, missing
    assert rc(W=4097, H=2, r_view=0) == E_ARG


def test_tiled_utility_field_refusals_reach_no_device():
    rc = _rc(UFIELD, dict(device=0, F=0, W=92, H=80, t_free=1, t_occ=3, r_inflate=2, w_gain=16, g_cap=174, min_gain=0, work_bytes=BIG,
                          max_rounds=1, resume=0, hip_stream=None))
    _caps(rc, "F")
    _gain_ranges(rc)
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_inflate=16) == 0
    assert rc(t_free=0) == E_ARG and rc(t_occ=(1 << 30) + 1) == E_ARG
    # what the tiled tail adds, each alone -- and each BEFORE the caps
    for W, H, other in ((92, 80, 0), (4097, 2, E_UNSUPPORTED)):
        assert rc(W=W, H=H) == other
        for bad in (0, -1, 65537):
            assert rc(W=W, H=H, max_rounds=bad) == E_ARG, bad
        for bad in (-1, 2):
            assert rc(W=W, H=H, resume=bad) == E_ARG, bad
        for missing in POINTERS[UFIELD]:
            assert rc(W=W, H=H, drop=(missing,)) == E_ARG and rc(W=W, H=H, F=3, drop=(missing,)) == E_ARG, missing
    assert rc(max_rounds=65536, resume=1) == 0
    # the caps come before the workspace's size, the size before "nothing to do"
    assert rc(W=4097, H=2, work_bytes=0) == E_UNSUPPORTED and rc(F=129, W=4096, H=4096, work_bytes=0) == E_UNSUPPORTED
    for F, W, H in ((0, 92, 80), (1, 92, 80), (3, 363, 362)):
        need = raw_call(BYTES, F=F, W=W, H=H)
        assert need > 0 and rc(F=F, W=W, H=H, work_bytes=need - 1) == E_ARG and rc(F=F, W=W, H=H, work_bytes=0) == E_ARG
    assert rc(work_bytes=raw_call(BYTES, F=0, W=92, H=80)) == 0


def test_tiled_utility_path_refusals_reach_no_device():
    rc = _rc(UPATH, dict(device=0, B=0, F=0, W=92, H=80, t_occ=3, w_gain=16, g_cap=174, min_gain=0, r_inflate=2, max_seg=5, S_max=1,
                         hip_stream=None), placed=True)
    _caps(rc, "B")
    _gain_ranges(rc)
    assert rc(B=0, F=1) == 0 and rc(B=3, F=2) == E_ARG and rc(B=3, F=2, W=4097, H=2) == E_ARG and rc(B=3, F=1, W=4097, H=2) == E_UNSUPPORTED
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(max_seg=4) == E_ARG and rc(S_max=0) == E_ARG and rc(t_occ=0) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG and rc(W=4097, H=2, drop=("cell",)) == E_ARG
    place, keep = _placement(cell=(0.0, 0.1))
    assert raw_call(UPATH, **{n: ONE for n in POINTERS[UPATH]}, **place, device=0, B=0, F=0, W=92, H=80, t_occ=3, w_gain=16, g_cap=174,
                    min_gain=0, r_inflate=2, max_seg=5, S_max=1, hip_stream=None) == E_ARG
    for missing in POINTERS[UPATH]:
        assert rc(drop=(missing,)) == E_ARG and rc(B=3, F=3, drop=(missing,)) == E_ARG and rc(W=4097, H=2, drop=(missing,)) == E_ARG, missing


def test_tiled_assign_refusals_reach_no_device():
    rc = _rc(ASSIGN, dict(device=0, B=0, W=92, H=80, r_inflate=0, r_claim=15, max_claims=64, max_seg=5, S_max=1, work_bytes=BIG,
                          max_rounds=8, hip_stream=None), placed=True)
    _caps(rc, "B")
    assert rc(drop=("may_claim",)) == 0                    # (optional)
    assert rc(r_inflate=-1) == E_ARG and rc(r_inflate=17) == E_ARG and rc(r_inflate=16) == 0
    assert rc(r_claim=-1) == E_ARG and rc(r_claim=4097) == E_ARG and rc(r_claim=0) == 0 and rc(r_claim=4096) == 0
    assert rc(max_claims=-1) == E_ARG and rc(max_claims=4097) == E_ARG and rc(max_claims=0) == 0 and rc(max_claims=4096) == 0
    assert rc(max_seg=4) == E_ARG and rc(S_max=0) == E_ARG
    assert rc(drop=("origin",)) == E_ARG and rc(drop=("cell",)) == E_ARG
    for bad in (0, -1, 65537):
        assert rc(max_rounds=bad) == E_ARG and rc(W=4097, H=2, max_rounds=bad) == E_ARG, bad
    # the launches of one call: max_claims * max_rounds <= 2^20, an argument error (before the caps)
    assert rc(max_claims=16, max_rounds=65536) == 0 and rc(max_claims=17, max_rounds=65536) == E_ARG
    assert rc(max_claims=4096, max_rounds=256) == 0 and rc(max_claims=4096, max_rounds=257) == E_ARG
    assert rc(W=4097, H=2, max_claims=4096, max_rounds=257) == E_ARG and rc(max_claims=0, max_rounds=65536) == 0
    for missing in POINTERS[ASSIGN]:
        if missing != "may_claim":
            assert rc(drop=(missing,)) == E_ARG and rc(B=3, drop=(missing,)) == E_ARG and rc(W=4097, H=2, drop=(missing,)) == E_ARG, missing
    # the 64-bit key lies at the workspace's first word: a work that is not 8-byte aligned is an argument error
    for bad in (4, 9, 12):
        assert rc(ptr=dict(work=C.c_void_p(bad))) == E_ARG and rc(W=4097, H=2, ptr=dict(work=C.c_void_p(bad))) == E_ARG, bad
    assert rc(ptr=dict(work=C.c_void_p(16))) == 0
    assert rc(W=4097, H=2, work_bytes=0) == E_UNSUPPORTED
    for W, H in ((92, 80), (363, 362)):
        need = raw_call(ASSIGN_BYTES, W=W, H=H)
        assert need > 0 and rc(W=W, H=H, work_bytes=need - 1) == E_ARG and rc(W=W, H=H, work_bytes=need) == 0


def test_assign_workspace_size_is_monotone():
    tw, th, _ = lipmpc.tiled_info()
    size = lambda W, H: raw_call(ASSIGN_BYTES, W=W, H=H)
    assert size(1, 8) == E_ARG and size(8, 1) == E_ARG
    assert size(4097, 2) == E_UNSUPPORTED and size(2, 4097) == E_UNSUPPORTED and size(65281, 257) == E_UNSUPPORTED and size(4096, 4096) > 0
    shapes = [2, 3, tw - 1, tw, tw + 1, th - 1, th, th + 1, 2 * th, 362, 363, 1024, 4096]
    for a, b in zip(shapes, shapes[1:]):
        for other in (2, 63, 362):
            assert size(a, other) < size(b, other) and size(other, a) < size(other, b), (a, b, other)
    assert size(92, 80) >= 4 * 92 * 80                     # field_k alone


def test_tiled_explorer_kernels_code_object():
    """From the built library's gfx950 code objects: every new kernel exists once, uses no scratch and spills nothing.  The gain
    kernel's LDS is all dynamic (the header's formula: 49,304 bytes at r_view = 64, within the 64 KiB a launch gets without asking);
    the seed and the claim kernel hold the workgroup reduction's words, everything else nothing."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    tw, th, _ = lipmpc.tiled_info()
    static = {"tile_gain_kernel": 0, "tile_utility_seed_kernel": 0, "tile_utility_descent_kernel": 0, "claim_setup_kernel": 0,
              "claim_robots_kernel": 0, "claim_seed_kernel": 256, "claim_pick_kernel": 0, "claim_take_kernel": 256, "claim_finish_kernel": 0}
    for k, lds in static.items():
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] == lds, (name, r)

    def gain_lds(r):                                       # the header's statement
        grown = (tw + 2 * r) * (th + 2 * r)
        return 4 * (2 * (2 * -(-grown // 64) + 2) + 2 + tw * th + 16 * 2 * -(-(2 * r + 1) ** 2 // 64))
    # ... held to what the host passes at launch, at every radius
    size = lambda r: raw_call(GAIN_LDS, r_view=r)
    assert size(0) == E_ARG and size(65) == E_ARG and size(-1) == E_ARG
    assert [size(r) for r in range(1, 65)] == [gain_lds(r) for r in range(1, 65)]
    assert size(64) == 49304 and size(1) == 8920 and size(64) <= 64 * 1024      # (no more than a launch gets without asking)
    # the existing kernels these calls reuse are still there once each
    for k, count in {"tiled_round_kernel": 1, "tiled_settle_kernel": 1, "tiled_bitmaps_kernel": 2, "tiled_blocked_kernel": 2}.items():
        assert len([n for n in res if k in n]) == count, k


def test_large_map_planner_classes():
    """(The constructors need a device to finish: what they refuse before they ask for one is checked here.)"""
    inf, coord = lipmpc.TiledInformedFrontierPlanner, lipmpc.TiledCoordinatedFrontierPlanner
    assert inf is lipmpc.planner.TiledInformedFrontierPlanner and coord is lipmpc.planner.TiledCoordinatedFrontierPlanner
    assert issubclass(inf, lipmpc.InformedFrontierPlanner) and issubclass(coord, lipmpc.CoordinatedFrontierPlanner)
    for cls in (inf, coord):
        p = inspect.signature(cls).parameters
        assert p["rounds"].default is None and p["rounds"].kind is inspect.Parameter.KEYWORD_ONLY
        assert "rounds" not in inspect.signature(cls.__init__).parameters
    assert [p for p in inspect.signature(inf.__init__).parameters][1:] == ["r_view", "w_gain", "g_cap", "min_gain", "frontier_planner_kwargs"]
    assert [p for p in inspect.signature(coord.__init__).parameters][1:] == ["r_claim", "max_claims", "frontier_planner_kwargs"]
    assert inspect.signature(inf.plan) == inspect.signature(lipmpc.InformedFrontierPlanner.plan)
    assert inspect.signature(coord.plan) == inspect.signature(lipmpc.CoordinatedFrontierPlanner.plan)
    for bad in (0, -1, 65537):
        with pytest.raises(ValueError, match="rounds"):
            inf(r_view=8, w_gain=16, g_cap=64, rounds=bad)
        with pytest.raises(ValueError, match="rounds"):
            coord(r_claim=4, rounds=bad)
    with pytest.raises(ValueError, match="2\\^20"):
        coord(r_claim=4, max_claims=4096, rounds=257)      # the launches of one claim call
    for bad in (dict(r_view=0), dict(w_gain=65536), dict(g_cap=0), dict(min_gain=-1), dict(r_inflate=17)):
        with pytest.raises(ValueError):
            inf(**dict(dict(r_view=8, w_gain=16, g_cap=64), **bad))
    for bad in (dict(r_claim=-1), dict(r_claim=4, max_claims=4097), dict(r_claim=4, min_unknown=0)):
        with pytest.raises(ValueError):
            coord(**bad)
    # the one-workgroup classes keep refusing tiled=True, and their message names the large-map class
    with pytest.raises(ValueError, match="tiled.*TiledCoordinatedFrontierPlanner"):
        lipmpc.CoordinatedFrontierPlanner(r_claim=4, tiled=True)
    with pytest.raises(ValueError, match="tiled.*TiledInformedFrontierPlanner"):
        lipmpc.InformedFrontierPlanner(r_view=8, w_gain=16, g_cap=64, tiled=True)
    table = lipmpc.planner.tiled_assign_outputs(3, 20, 24, 64)
    assert set(table) == (set(lipmpc.planner.assign_outputs(3, 20, 24, 64)) - {"work"}) | {"claims_settled"}
