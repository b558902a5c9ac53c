"""CPU: the inputs of tests/test_rrt_sizes_gpu.py (tests/rrt_size_cases.py) reach what they are meant to reach, shown on the
oracle alone: the statuses, tree sizes on both sides of the tree kernel's 256-thread stride, rewiring, a sampler that runs dry,
LDS sizes on both sides of 64 KiB and of the 160 KiB limit.  A device test on inputs that end early or grow a tree of three
vertices would pass whatever the kernels did."""
import ctypes as C
import functools

import numpy as np
import pytest

import lipmpc
import rrt_grid_oracle as RG
import rrt_oracle as R
import rrt_size_cases as S

RING = S.ring_cases() + [S.packing_case()[0], S.batch65_case()]
GRID = S.grid_cases() + [S.replay_case()]
BY_ID = {c["id"]: c for c in RING + GRID}
assert len(BY_ID) == len(RING) + len(GRID)


@functools.lru_cache(maxsize=None)
def plans(case_id):
    """The oracle's plans of a case, one per problem, on numpy's own cost grid."""
    c = BY_ID[case_id]
    if "occ" in c:
        return [RG.plan_grid(c["occ"], c["origin"], c["cell"], p["goal"], start=p["start"], seed=p["seed"], **c["params"])
                for p in c["problems"]]
    return [R.plan(p["rings"], p["goal"], start=p["start"], seed=p["seed"], **c["params"]) for p in c["problems"]]


@pytest.mark.parametrize("case_id", list(BY_ID))
def test_case_reaches_its_status_and_tree_size(case_id):
    """Statuses as the case lists them; a valid tree; at least ``bar`` vertices for 3 of the 4 seeds; in a FOUND plan with
    r_rewire >= 6, at least one vertex that rewiring gave a younger parent."""
    c, res = BY_ID[case_id], plans(case_id)
    print(case_id, [(RG.STATUS_NAMES[o["status"]], len(o["cells"]), o["draws"], o["samples"]) for o in res][:8])
    for b, st in c["expect"].items():
        assert res[b]["status"] == st, (b, RG.STATUS_NAMES[res[b]["status"]], RG.STATUS_NAMES[st])
    for b, o in enumerate(res):
        if o["og"] is not None and o["C"] is not None:
            assert R.check_tree(o) == [], b
        assert o["samples"] <= c["params"]["n"] and o["draws"] <= 64 * c["params"]["n"] and len(o["cells"]) <= o["samples"] + 1
        if o["status"] == R.FOUND and c["params"]["r_rewire"] >= 6 and c["bar"] is not None and c["bar"] >= 20:
            assert (o["parent"] > np.arange(len(o["parent"]))).any(), (b, "no rewiring")
    if c["bar"] is not None:
        assert len(res) == 4 and sum(len(o["cells"]) >= c["bar"] for o in res) >= 3, [len(o["cells"]) for o in res]


def test_ring_grids_have_the_listed_dims():
    dims = {i: (plans(i)[0]["tf"]["W"] + 1, plans(i)[0]["tf"]["H"] + 1) for i in ("width7", "width257", "tall", "wide")}
    assert dims == {"width7": (8, 6), "width257": (258, 176), "tall": (8, 2193), "wide": (2001, 8)}, dims


def test_tree_sizes_around_the_stride():
    """n = 1, 2, 255, 256, 257, 513 (seed 9): V = 1, 2, 240, 241, 242, 456; r_rewire = 8192: V = 281; the big tree beyond 1500
    vertices, the tree at the LDS limit beyond 256."""
    for n, V in S.N_CASE_V.items():
        assert len(plans(f"n{n}")[0]["cells"]) == V, n
    assert len(plans("n513")[0]["cells"]) > 256
    assert len(plans("rewire8192")[0]["cells"]) == S.REWIRE_ALL_V
    assert min(len(o["cells"]) for o in plans("lds_tree")) > 1500
    assert min(len(o["cells"]) for o in plans("lds_limit")) > 256


def test_sampler_runs_dry():
    """Every draw of the cap is used and the samples stay short of n; with start and goal the only free cells no draw is valid."""
    for o in plans("dry"):
        assert o["draws"] == 64 * 40 and 0 < o["samples"] < 40, (o["draws"], o["samples"])
    for o in plans("dry_empty"):
        assert (len(o["cells"]), o["draws"], o["samples"], o["status"]) == (1, 256, 0, R.NO_PATH)


def test_lds_sizes():
    assert S.lds_bytes(R.N_SAMPLES, R.MAX_CELLS) == 58668                      # the defaults: below 64 KiB
    assert S.lds_bytes(200, 1 << 19) == 71420 and S.lds_bytes(4000, 1 << 14) > 64 * 1024
    assert S.lds_bytes(1160, 1 << 20) == 163836 <= S.LDS_LIMIT < S.lds_bytes(1161, 1 << 20) == 163864
    for i in ("lds_bitmap", "lds_tree", "lds_limit"):
        assert 64 * 1024 < S.lds_bytes(BY_ID[i]["params"]["n"], BY_ID[i]["params"]["max_cells"]) <= S.LDS_LIMIT, i
    assert S.lds_bytes(BY_ID["replay"]["params"]["n"], BY_ID["replay"]["params"]["max_cells"]) < 64 * 1024
    # the occupancy kernel's hulls: 83 obstacle slots of 64 vertices are the most that fit 64 KiB
    lds_grid = lambda n_obs: 12 * n_obs * S.PACK_V_MAX + 20 * n_obs
    assert lds_grid(S.PACK_N_OBS) <= 64 * 1024 < lds_grid(S.PACK_N_OBS + 1)


def test_workspace_bytes_refuses_past_the_lds_limit():
    """(n, max_cells) = (1160, 2^20) and (5836, 2^10) are the last ones accepted."""
    lib = lipmpc._lib.load()
    for n, cells, ok in ((1160, 1 << 20, True), (1161, 1 << 20, False), (5836, 1 << 10, True), (5837, 1 << 10, False)):
        p = lipmpc._lib.LipmpcRrtParamsC()
        assert lib.lipmpc_rrt_default_params(C.byref(p)) == 0
        p.n_samples, p.max_cells = n, cells
        assert (lib.lipmpc_rrt_workspace_bytes(C.byref(p), 1) > 0) == ok == (S.lds_bytes(n, cells) <= S.LDS_LIMIT), (n, cells)


def test_packing_rings_degenerate_as_meant():
    """On the packing case's grid the 64-gon keeps a hull of many points, the repeated ring one of 4, the collinear ring one of 2
    and the small ring one of 1; the slots that must not be read lie outside the bounds."""
    case, xy, nv = S.packing_case()
    tf = plans("packing")[0]["tf"]
    hull = lambda r: R.int_hull(np.stack(R.to_cell(tf, r[:, 0], r[:, 1]), 1))
    sizes = [len(hull(r)) for r in case["problems"][0]["rings"]]
    assert sizes[2] >= 8 and sizes[3:6] == [4, 2, 1], sizes
    assert nv.max() > S.PACK_V_MAX and nv.min() < 0 and (nv == 0).any()
    assert tf["max_x"] < 10 and tf["min_x"] > -10 and np.abs(xy).max() == 1e6
    for b, o in enumerate(plans("packing")):
        assert o["og"].sum() > 100, b
