"""GPU: the RRT* planner away from its default sizes (tests/rrt_size_cases.py; tests/test_rrt_sizes_oracle.py shows on the CPU
what each case reaches): grid sides on both sides of the 64-thread blocks of the distance transform and of the 256-cell chunks
of the ballot words, grids of 2 and of 4096 cells a side and of exactly max_cells cells, trees of 1 vertex and of 3000, r_rewire
of 1 and of 8192, a sampler that runs dry, the tree kernel with more than 64 KiB of LDS up to 4 bytes under its limit, obstacle
slots that fill the occupancy kernel's LDS, B = 65, and a plan replayed from a captured graph.

Every problem of every batch goes through tests/rrt_checks.py against the oracle fed the device's own cost grid: bit for bit,
C itself within 2 ulp of numpy's."""
import ctypes as C

import numpy as np
import pytest

import rrt_oracle as R
import rrt_size_cases as S
from rrt_checks import check_grid_plan, check_ring_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402


def _host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ring_planner(p):
    return lipmpc.RrtStarPlanner(width_grid_size=p["width"], n=p["n"], r_rewire=p["r_rewire"], margin=p["margin"],
                                 max_cells=p["max_cells"])


def _run_ring(case, xy=None, nv=None):
    """Plan the case's problems in one plan_batch and hold every one of them to the oracle."""
    probs = case["problems"]
    if xy is None:
        xy, nv = lipmpc.pack_rings([q["rings"] for q in probs], max(len(q["rings"]) for q in probs),
                                   max(len(r) for q in probs for r in q["rings"]))
    res = _host(_ring_planner(case["params"]).plan_batch(np.array([q["goal"] for q in probs], float), xy, nv,
                                                         start=np.array([q["start"] for q in probs], float),
                                                         seeds=[q["seed"] for q in probs], with_tree=True, with_grids=True))
    for b, q in enumerate(probs):
        check_ring_plan(res, b, q, (case["id"], b), **case["params"])
    for b, st in case["expect"].items():
        assert res["status"][b] == st, (case["id"], b, R.STATUS_NAMES[res["status"][b]])
    print(case["id"], [(R.STATUS_NAMES[s], int(t[0, 0]), int(t[0, 2])) for s, t in zip(res["status"], res["tree"])][:4])
    return res


def _run_grid(case):
    probs, p = case["problems"], case["params"]
    planner = lipmpc.RrtStarPlanner(n=p["n"], r_rewire=p["r_rewire"], max_cells=p["max_cells"])
    res = _host(planner.plan_grid_batch(np.array([q["goal"] for q in probs], float),
                                        lipmpc.GridMap(case["occ"], case["origin"], case["cell"]),
                                        np.array([q["start"] for q in probs], float), seeds=[q["seed"] for q in probs],
                                        with_tree=True, with_grids=True))
    for b, q in enumerate(probs):
        check_grid_plan(res, b, case["occ"], case["origin"], case["cell"], q, (case["id"], b), **p)
    for b, st in case["expect"].items():
        assert res["status"][b] == st, (case["id"], b, R.STATUS_NAMES[res["status"][b]])
    print(case["id"], [(R.STATUS_NAMES[s], int(t[0, 0]), int(t[0, 2])) for s, t in zip(res["status"], res["tree"])])
    return res


@pytest.mark.parametrize("case", S.ring_cases(), ids=S.case_ids(S.ring_cases()))
def test_ring_plan_sizes(case):
    """Widths 1 .. 257 and 2000, a grid 2193 cells tall, n = 1 .. 513, r_rewire = 1, 2 and 8192: 4 seeds each."""
    _run_ring(case)


def test_obstacle_slots_fill_the_occupancy_kernels_lds():
    """83 slots of 64 vertices (65 404 bytes of hulls in LDS), with obs_nv above v_max, zero and negative, a repeated, a
    collinear and a one-cell ring; the oracle is given the clipped rings."""
    case, xy, nv = S.packing_case()
    res = _run_ring(case, xy, nv)
    assert (res["status"] == R.FOUND).all()


def test_batch_of_65():
    res = _run_ring(S.batch65_case())
    assert (res["status"] == R.FOUND).sum() >= 33


@pytest.mark.parametrize("case", S.grid_cases(), ids=S.case_ids(S.grid_cases()))
def test_grid_plan_sizes(case):
    """Given grids from 2 x 2 to 4096 x 2, at and over the cell cap, the dry sampler, the tree kernel's LDS above 64 KiB."""
    res = _run_grid(case)
    if case["id"].startswith("dry"):
        n = case["params"]["n"]
        assert (res["tree"][:, 0, 2] == 64 * n).all() and (res["tree"][:, 0, 3] < n).all(), res["tree"][:, 0]


def test_one_sample_past_the_lds_limit_is_refused():
    """n = 1161 at max_cells = 2^20 needs 163 864 bytes of LDS, 24 more than there are."""
    with pytest.raises(ValueError):
        lipmpc.RrtStarPlanner(n=1161, r_rewire=6, max_cells=1 << 20)


def test_graph_replay_gives_the_eager_bytes():
    """One plan on a given grid -- the zeroing of its outputs and the call as plan_grid_batch issues it -- captured on a side
    stream after a warm-up, on outputs allocated before the capture; replayed twice with every output overwritten in between: each
    replay leaves the eager call's bytes, which are the oracle's plan."""
    case = S.replay_case()
    probs, p = case["problems"], case["params"]
    B, n = len(probs), p["n"]
    planner = lipmpc.RrtStarPlanner(n=n, r_rewire=p["r_rewire"], max_cells=p["max_cells"])
    grid = lipmpc.GridMap(case["occ"], case["origin"], case["cell"]).to(planner.device)
    goal = torch.as_tensor(np.array([q["goal"] for q in probs], float), device=planner.device)
    start = torch.as_tensor(np.array([q["start"] for q in probs], float), device=planner.device)
    seeds = planner._seeds([q["seed"] for q in probs], B)
    eager = planner.plan_grid_batch(goal, grid, start, seeds=[q["seed"] for q in probs], with_tree=True, with_grids=True)
    want = _host(eager)
    for b, q in enumerate(probs):
        check_grid_plan(want, b, case["occ"], case["origin"], case["cell"], q, ("eager", b), **p)
    assert (want["status"] == R.FOUND).sum() >= 3

    table = lipmpc.planner.plan_outputs(B, n + 1, p["max_cells"], n)
    out = {k: torch.zeros(shape, dtype=dt, device=planner.device) for k, (dt, shape, _) in table.items()}
    ws = planner._workspace(B)

    def launch():
        for t in out.values():
            t.zero_()
        lipmpc._lib.call("lipmpc_rrt_plan_grid_batch", device=planner.device_index, p=C.byref(planner.params), B=B,
                         **grid._args(B, planner.device), start=start, goal=goal, seed=seeds, workspace=ws, **out, S_max=n + 1,
                         hip_stream=torch.cuda.current_stream(planner.device).cuda_stream)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    for _ in range(2):
        for t in out.values():
            t.view(torch.uint8).fill_(0xA5)
        graph.replay()
        got = _host(out)
        for k in table:
            assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k
