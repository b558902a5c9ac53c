"""Correlative scan matching: C ABI and compiled resources (no GPU needed)."""
import ctypes as C

import lipmpc
import scan_match_oracle as S
from code_object import kernel_resources
from helpers import raw_call

E_ARG, E_UNSUPPORTED = -1, -2


def test_scan_match_symbol_is_exported_and_bound():
    lib = lipmpc._lib.load()
    name = "lipmpc_scan_match_batch"
    assert name in lipmpc._lib.EXPORTS and name in lipmpc._lib.SIGNATURES and hasattr(lib, name)
    assert getattr(lib, name).argtypes == [t for _, t in lipmpc._lib.SIGNATURES[name][1]]
    assert lib.lipmpc_version() == 5                       # a backward-compatible addition
    assert lipmpc.ScanMatcher is lipmpc.mapping.ScanMatcher
    header = open(lipmpc._lib.LIB_PATH.rsplit("/", 2)[0] + "/include/lipmpc.h").read()
    assert "+ lipmpc_scan_match_batch" in header.split("#define LIPMPC_VARIANT_BASE")[0]      # in the list of additions


def test_scan_match_kernel_code_object():
    """From the built library's gfx950 code object: the kernel exists once, uses no scratch and spills nothing; its LDS holds the
    byte window of the header's cap and stays within the 64 KiB a workgroup may have."""
    res = kernel_resources(lipmpc._lib.LIB_PATH)
    mine = {name: r for name, r in res.items() if "scan_match_kernel" in name}
    assert len(mine) == 1, sorted(mine)
    (name, r), = mine.items()
    print("scan_match_kernel", {f: r.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
    assert S.WINDOW_CELLS < r["group_segment_fixed_size"] <= 65536, (name, r)


def test_scan_match_matcher_arguments():
    import pytest
    new = lambda *a, **kw: lipmpc.ScanMatcher(*a, **{**dict(clamp=8, min_score=1, min_gain=0), **kw})
    m = new(4, 3, n_yaw=2, yaw_step=0.02)
    assert (m.n_x, m.n_y, m.n_yaw, m.clamp, m.min_score, m.min_gain) == (4, 3, 2, 8, 1, 0)
    assert m.rot.shape == (5, 2) and tuple(m.rot[2]) == (1.0, 0.0) and (m.rot == S.rot_table(2, 0.02)).all()
    assert new(0, 0).rot is None
    with pytest.raises(TypeError):
        lipmpc.ScanMatcher(4, 4)                           # the scoring parameters have no defaults
    with pytest.raises(TypeError):
        lipmpc.ScanMatcher(4, 4, 8, 1, 0)                  # ... and are keyword-only
    for bad in (dict(n_x=17), dict(n_y=-1), dict(n_yaw=17, yaw_step=0.01), dict(n_yaw=1), dict(clamp=0), dict(clamp=128),
                dict(min_gain=-1), dict(n_yaw=1, yaw_step=float("nan"))):
        with pytest.raises(ValueError):
            new(**{**dict(n_x=4, n_y=4), **bad})


def test_scan_match_refusals_reach_no_device():
    """Every refusal is decided on the host before anything is enqueued."""
    one = C.c_void_p(8)                                    # device pointers: never dereferenced
    outs = ("offset_cells", "yaw_index", "offset", "score", "n_used", "matched")
    ptrs = dict(state=one, hits=one, evidence=one, rot_table=one, **{k: one for k in outs})
    org = (C.c_double * 2)(-1.0, -1.0)

    def rc(cell=(0.05, 0.05), origin=org, drop=(), **kw):
        cs = (C.c_double * 2)(*cell)
        args = dict(device=0, B=1, resolution=360, W=96, H=80, grid_shared=1, lidar_range=1.5, depth=0.025, n_x=4, n_y=4, n_yaw=2, clamp=8,
                    min_score=1, min_gain=0)
        args.update(kw)
        p = {k: v for k, v in dict(ptrs, origin=C.cast(origin, C.c_void_p), cell=C.cast(cs, C.c_void_p)).items() if k not in drop}
        return raw_call("lipmpc_scan_match_batch", **p, **args)

    assert rc(B=0) == 0                                    # the same arguments pass: an empty batch enqueues nothing
    assert rc(resolution=0) == E_ARG and rc(resolution=385) == E_ARG and rc(B=0, resolution=384) == 0 and rc(B=-1) == E_ARG
    assert rc(W=0) == E_ARG and rc(H=0) == E_ARG and rc(H=-2) == E_ARG
    assert rc(cell=(0.0, 0.05)) == E_ARG and rc(cell=(0.05, -1.0)) == E_ARG and rc(cell=(float("nan"), 0.05)) == E_ARG
    assert rc(cell=(float("inf"), 0.05)) == E_ARG
    assert rc(lidar_range=-1.0) == E_ARG and rc(lidar_range=float("inf")) == E_ARG and rc(lidar_range=float("nan")) == E_ARG
    assert rc(depth=-0.01) == E_ARG and rc(depth=float("inf")) == E_ARG and rc(depth=float("nan")) == E_ARG and rc(B=0, depth=0.0) == 0
    for n in ("n_x", "n_y", "n_yaw"):
        assert rc(**{n: -1}) == E_ARG and rc(**{n: 17}) == E_ARG and rc(B=0, **{n: 16}) == 0 and rc(B=0, **{n: 0}) == 0, n
    assert rc(clamp=0) == E_ARG and rc(clamp=128) == E_ARG and rc(clamp=-8) == E_ARG and rc(B=0, clamp=1) == 0 and rc(B=0, clamp=127) == 0
    assert rc(min_gain=-1) == E_ARG and rc(B=0, min_gain=2 ** 31 - 1) == 0
    assert rc(B=0, min_score=-2 ** 31) == 0 and rc(B=0, min_score=2 ** 31 - 1) == 0
    assert rc(drop=("rot_table",)) == E_ARG and rc(B=0, drop=("rot_table",)) == E_ARG       # only n_yaw == 0 goes without a table
    assert rc(B=0, n_yaw=0, drop=("rot_table",)) == 0
    for missing in ("state", "hits", "evidence", "origin", "cell") + outs:
        assert rc(drop=(missing,)) == E_ARG, missing
    # the window cap: the update's window grown by the search, as the oracle counts it
    n_fit = n_not = 0
    for rng, depth, cell, n_x, n_y in ((5.0, 0.0, (0.05, 0.05), 8, 8), (5.0, 0.0, (0.05, 0.05), 9, 8), (5.0, 0.0, (0.05, 0.05), 8, 9),
                                       (5.4, 0.0, (0.05, 0.05), 0, 0), (5.4, 0.0, (0.05, 0.05), 1, 0), (5.4, 0.0, (0.05, 0.05), 0, 1),
                                       (1.5, 0.025, (0.05, 0.08), 16, 16), (3.0, 0.005, (0.01, 0.01), 0, 0), (3.0, 0.0, (0.05, 0.004), 16, 2),
                                       (3.0, 0.0, (0.05, 0.006), 16, 16), (3.0, 0.0, (0.05, 0.006), 3, 16), (1.5, 0.05, (0.1, 0.1), 16, 16),
                                       (2.0, 0.0, (0.05, 0.05), 16, 16)):
        fits = S.window_fits(rng, depth, cell, n_x, n_y)
        n_fit, n_not = n_fit + fits, n_not + (not fits)
        assert rc(B=0, lidar_range=rng, depth=depth, cell=cell, n_x=n_x, n_y=n_y) == (0 if fits else E_UNSUPPORTED), (rng, depth, cell, n_x, n_y)
    assert n_fit >= 4 and n_not >= 4
    assert rc(lidar_range=5.4, depth=0.0, n_x=1) == E_UNSUPPORTED
