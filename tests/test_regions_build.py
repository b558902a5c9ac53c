"""Frontier regions: C ABI, Python signatures, compiled resources and the refusals that need no device (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import pytest

import lipmpc
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2
CALL, BYTES = "lipmpc_grid_frontier_regions_batch", "lipmpc_grid_frontier_regions_workspace_bytes"
ARGS = ["device", "F", "W", "H", "frontier", "min_size", "R_max", "work", "work_bytes", "label", "size", "rep", "table", "n_regions",
        "hip_stream"]
POINTERS = ("frontier", "work", "label", "size", "rep", "table", "n_regions")
KERNELS = ("regions_tile_kernel", "regions_border_kernel", "regions_flatten_kernel", "regions_count_kernel", "regions_scan_kernel",
           "regions_rank_kernel", "regions_sum_kernel", "regions_key_kernel", "regions_table_kernel")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lipmpc.h")


def _names(name):
    return [n for n, _ in lipmpc._lib.SIGNATURES[name][1]]


def test_symbols_are_exported_and_bound():
    lib = lipmpc._lib.load()
    for name in (CALL, BYTES):
        assert name in lipmpc._lib.EXPORTS and name in lipmpc._lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    assert _names(CALL) == ARGS and _names(BYTES) == ["F", "W", "H", "R_max"]
    assert lib.lipmpc_version() == 5                       # a backward-compatible addition
    for name in ("frontier_regions", "regions_outputs"):
        assert name in dir(lipmpc) and callable(getattr(lipmpc, name))
    assert list(lipmpc.regions_outputs(2, 3, 4, 5)) == ["label", "size", "rep", "table", "n_regions"]
    assert lipmpc.regions_outputs(2, 3, 4, 5)["table"][1] == (2, 5, 5) and lipmpc.regions_outputs(2, 3, 4, 5)["n_regions"][1] == (2, 3)


def test_the_header_prototype_names_the_bindings_arguments_and_states_the_launch_count():
    with open(HEADER) as f:
        text = f.read()
    proto = re.search(r"\nint " + CALL + r"\((.*?)\);", text, re.S).group(1)
    assert [p.split()[-1].lstrip("*") for p in proto.replace("\n", " ").split(",")] == ARGS
    proto = re.search(r"\nint64_t " + BYTES + r"\((.*?)\);", text, re.S).group(1)
    assert [p.split()[-1] for p in proto.split(",")] == ["F", "W", "H", "R_max"]
    flat = " ".join(text.split()).replace(" * ", " ")
    assert "a fixed sequence of 9 launches, whatever the mask holds and whatever its size" in flat
    assert "8 F W H + 64 F R_max + 65536 bytes" in flat and "tests/regions_oracle.py" in flat
    assert "nine launches" in " ".join(lipmpc.frontier_regions.__doc__.split())
    assert "lipmpc_grid_frontier_regions_batch" in lipmpc.FrontierPlanner.regions.__doc__


def test_kernels_code_object():
    """From the built library's gfx950 code objects: the nine new kernels exist once each, use no scratch and spill nothing."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    assert len([n for n in res if "regions_" in n]) == len(KERNELS)
    for k in KERNELS:
        mine = {name: r for name, r in res.items() if k in name}
        assert len(mine) == 1, (k, sorted(mine))
        (name, r), = mine.items()
        print(k, {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 8192, (name, r)          # the tile's parent words; the scans' 256 partial sums


def test_the_workspace_is_monotone_and_under_the_bound():
    size = getattr(lipmpc._lib.load(), BYTES)
    for F in (0, 1, 3, 64):
        for W, H in ((2, 2), (2, 3), (32, 64), (33, 65), (363, 362), (4000, 2), (1024, 1024)):
            for R in (0, 1, 1024, 1 << 20):
                n = size(F, W, H, R)
                assert n > 0 and n % 8 == 0, (F, W, H, R, n)
                assert n <= 8 * F * W * H + 64 * F * R + 65536, (F, W, H, R, n)
                assert size(F + 1, W, H, R) > n and size(F, W + 1, H, R) >= n and size(F, W, H + 1, R) >= n
                assert size(F, W + 32, H + 64, R) >= n and (R == 1 << 20 or size(F, W, H, R + 1) >= n)
                if F:
                    assert size(F, W + 32, H + 64, R) > n and (R == 1 << 20 or size(F, W, H, R + 1) > n)
    # 4096 x 4096 with the default table: a root's rank per cell, 64 MiB, and next to nothing beside it
    assert 4 * 4096 * 4096 < size(1, 4096, 4096, 1024) < 4 * 4096 * 4096 + (1 << 17)
    assert size(-1, 8, 8, 4) == E_ARG and size(1, 1, 8, 4) == E_ARG and size(1, 8, 1, 4) == E_ARG
    assert size(1, 8, 8, -1) == E_ARG and size(1, 8, 8, (1 << 20) + 1) == E_ARG and size(1, 8, 8, 1 << 20) > 0
    assert size(1, 4097, 2, 4) == E_UNSUPPORTED and size(1, 2, 4097, 4) == E_UNSUPPORTED and size(1, 4097, 2, -1) == E_ARG
    # F * W * H <= 2^31
    assert size(128, 4096, 4096, 4) > 0 and size(129, 4096, 4096, 4) == E_UNSUPPORTED
    assert size(1 << 29, 2, 2, 0) > 0 and size((1 << 29) + 1, 2, 2, 0) == E_UNSUPPORTED and size(1 << 62, 2, 2, 0) == E_UNSUPPORTED


def test_refusals_reach_no_device_in_order():
    """Every refusal is decided on the host before anything is enqueued: ARG, then UNSUPPORTED, then F = 0."""
    size = getattr(lipmpc._lib.load(), BYTES)
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    ptrs = {n: one for n in POINTERS}

    def rc(drop=(), **kw):
        args = dict(device=0, F=0, W=92, H=80, min_size=1, R_max=16, work_bytes=1 << 40)
        args.update(kw)
        return raw_call(CALL, **dict({k: v for k, v in ptrs.items() if k not in drop and k not in kw}, **args))

    assert rc() == 0 and rc(drop=("rep",)) == 0 and rc(R_max=0, drop=("table",)) == 0 and rc(R_max=0, drop=("table", "rep")) == 0
    assert rc(drop=("table",)) == E_ARG and rc(R_max=0) == 0                       # table may be null iff R_max == 0
    assert rc(F=-1) == E_ARG and rc(W=1) == E_ARG and rc(H=1) == E_ARG
    assert rc(min_size=0) == E_ARG and rc(min_size=(1 << 24) + 1) == E_ARG and rc(min_size=1 << 24) == 0
    assert rc(R_max=-1) == E_ARG and rc(R_max=(1 << 20) + 1) == E_ARG and rc(R_max=1 << 20) == 0
    assert rc(work=C.c_void_p(12)) == E_ARG and rc(work=C.c_void_p(16)) == 0       # 8-byte aligned
    for missing in POINTERS:
        if missing not in ("rep", "table"):
            assert rc(drop=(missing,)) == E_ARG and rc(F=3, drop=(missing,)) == E_ARG, missing
    assert rc(work_bytes=size(0, 92, 80, 16) - 1) == E_ARG and rc(work_bytes=size(0, 92, 80, 16)) == 0
    assert rc(F=3, work_bytes=size(3, 92, 80, 16) - 1) == E_ARG and rc(F=3, W=363, H=362, work_bytes=size(3, 92, 80, 16)) == E_ARG
    assert rc(F=3, R_max=17, work_bytes=size(3, 92, 80, 16)) == E_ARG
    # an argument error comes before the caps, the caps before "nothing to do"
    assert rc(W=4097, H=2) == E_UNSUPPORTED and rc(W=2, H=4097) == E_UNSUPPORTED and rc(F=129, W=4096, H=4096) == E_UNSUPPORTED
    assert rc(W=4097, H=2, min_size=0) == E_ARG and rc(W=4097, H=2, drop=("label",)) == E_ARG and rc(W=4097, H=2, R_max=-1) == E_ARG
    assert rc(F=129, W=4096, H=4096, drop=("n_regions",)) == E_ARG and rc(W=4097, H=2, work=C.c_void_p(12)) == E_ARG


def test_constructor_refusals_that_need_no_device():
    L = lipmpc
    gk = dict(w_gain=16, g_cap=40, r_keep=3, keep_ratio16=24, keep_slack=4)
    region = dict(gain_from="region")
    for make, word in (
            # r_view must be None with "region": both keywords are named
            (lambda: L.InformedFrontierPlanner(8, 16, 40, **region), r"gain_from='region' with r_view 8"),
            (lambda: L.TiledInformedFrontierPlanner(8, 16, 40, **region), r"gain_from='region' with r_view 8"),
            (lambda: L.CoordinatedFrontierPlanner(5, r_view=3, w_gain=16, g_cap=40, **region), r"gain_from='region' with r_view 3"),
            (lambda: L.TiledCoordinatedFrontierPlanner(5, r_view=3, w_gain=16, g_cap=40, **region), r"gain_from='region' with r_view 3"),
            (lambda: L.GainKeepFrontierPlanner(5, r_view=3, **gk, **region), r"gain_from='region' with r_view 3"),
            (lambda: L.TiledGainKeepFrontierPlanner(5, r_view=3, **gk, **region), r"gain_from='region' with r_view 3"),
            # "representative" requires "region"
            (lambda: L.InformedFrontierPlanner(8, 16, 40, target="representative"), "needs gain_from='region'"),
            (lambda: L.InformedFrontierPlanner(8, 16, 40, gain_from="view", target="representative"), "needs gain_from='region'"),
            (lambda: L.InformedFrontierPlanner(8, 16, 40, gain_from="size"), "gain_from 'size'"),
            (lambda: L.InformedFrontierPlanner(None, 16, 40, gain_from="region", target="centroid"), "target 'centroid'"),
            # the planners that issue no gain call, per-robot fields and clearance refuse both options
            (lambda: L.FrontierPlanner(**region), "not supported"),
            (lambda: L.FrontierPlanner(target="cell"), "not supported"),
            (lambda: L.GridFieldPlanner(gain_from="view"), "not supported"),
            (lambda: L.CoordinatedFrontierPlanner(5, **region), "not supported"),
            (lambda: L.CoordinatedFrontierPlanner(5, r_keep=3, keep_ratio16=24, keep_slack=4, target="cell"), "not supported"),
            (lambda: L.RobotFieldsFrontierPlanner(5, **region), "not supported"),
            (lambda: L.RobotFieldsFrontierPlanner(5, gain_from="view", target="cell"), "not supported"),
            (lambda: L.FrontierPlanner(tiled=True, r_clear=2, w_clear=3, **region), "r_clear"),
            (lambda: L.GridFieldPlanner(tiled=True, r_clear=2, w_clear=3, target="cell"), "r_clear"),
            (lambda: L.InformedFrontierPlanner(None, 16, 40, r_clear=2, w_clear=3, **region), "r_clear"),
            # the ranges of w_gain, g_cap and min_gain stay
            (lambda: L.InformedFrontierPlanner(None, 65536, 40, **region), "w_gain"),
            (lambda: L.InformedFrontierPlanner(None, 16, 0, **region), "g_cap"),
            (lambda: L.InformedFrontierPlanner(None, 16, 40, 16385, **region), "min_gain"),
            (lambda: L.CoordinatedFrontierPlanner(5, w_gain=16, g_cap=16385, **region), "g_cap"),
            (lambda: L.CoordinatedFrontierPlanner(5, w_gain=16, **region), "go together")):
        with pytest.raises(ValueError, match=word):
            make()
    # without the options nothing changes: r_view stays required
    with pytest.raises(TypeError):
        L.InformedFrontierPlanner(None, 16, 40)
    with pytest.raises(ValueError, match="r_view"):
        L.GainKeepFrontierPlanner(5, r_view=None, **gk)
    # the options are keyword-only and leave every signature what it was
    for cls in (L.InformedFrontierPlanner, L.TiledInformedFrontierPlanner, L.CoordinatedFrontierPlanner, L.GainKeepFrontierPlanner,
                L.TiledGainKeepFrontierPlanner):
        assert not {"gain_from", "target"} & set(inspect.signature(cls.__init__).parameters)
        assert "regions" in dir(cls)
    assert list(inspect.signature(L.FrontierPlanner.regions).parameters) == ["self", "mapper_or_evidence", "min_size", "R_max", "out"]
    assert list(inspect.signature(L.frontier_regions).parameters) == ["frontier", "min_size", "R_max", "out"]
    assert inspect.signature(L.frontier_regions).parameters["R_max"].default == 1024
