"""GPU: the exploring fleet with claims from per-robot fields (RobotFieldsFrontierPlanner in UnknownEnvFleet.run_exploring, taken as it
is) on the recorded 64 x 56 scene of tests/test_assign_fleet_gpu.py (tests/golden/exploration_assigned.npz), with and without the keep
keywords.  Every replan of the device run is recorded -- the evidence, the positions, who may claim, the previous targets -- and the
FIRST one is replayed on the host by tests/robot_fields_oracle.py; two runs give the same bits; the result rows have the documented
shapes; the coverage of every recorded seed is held to a bar from this rule's own CPU chains, as tests/test_assign_keep_fleet_gpu.py
does it.  No test asserts "sooner": the finishing samples are recorded, not asserted."""
import functools
import os

import numpy as np
import pytest

import frontier_oracle as FR
import robot_fields_oracle as RF
import test_assign_fleet_gpu as AF

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

KEEP = dict(r_keep=6, keep_ratio16=24, keep_slack=8)
RECORDED = ("status", "target_cell", "n_claims", "claim_round", "n_sub", "path_cost")


class _Recording(lipmpc.RobotFieldsFrontierPlanner):
    """The planner under test, with a copy (on the device) of every replan's inputs and answers."""

    def _record(self, method, mapper, start, kw):
        ins = dict(evidence=mapper.evidence.clone(), start=start.clone(), may_claim=kw["may_claim"].clone())
        if kw.get("prev_target") is not None:
            ins["prev"] = kw["prev_target"].clone()
        out = method(mapper, start, **kw)
        self.calls.append(dict(ins, **{k: out[k].clone() for k in RECORDED + (("kept", "n_kept") if "kept" in out else ())}))
        return out

    def plan(self, mapper, start, **kw):
        return self._record(super().plan, mapper, start, kw)

    def replan(self, mapper, start, **kw):
        return self._record(super().replan, mapper, start, kw)


def _explorer(**keep):
    d = AF._scene()[0]
    pl = _Recording(int(d["r_claim"]), len(d["starts"]), r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]), **keep)
    pl.calls = []
    return pl


@functools.lru_cache(maxsize=None)
def _runs(keep):
    """The first recorded seed, twice (the first run's replans are the ones recorded)."""
    d = AF._scene()[0]
    fleet, mapper, _ = AF._fleet()
    seed = d["seeds"].tolist()[0]
    pl = _explorer(**(KEEP if keep else {}))
    first = AF._explore(fleet, mapper, pl, seed)
    calls = [{k: v.cpu().numpy() for k, v in c.items()} for c in pl.calls]
    return first, AF._explore(fleet, mapper, pl, seed), calls


@pytest.mark.parametrize("keep", [False, True])
def test_gpu_two_runs_give_the_same_bits_and_the_rows_have_their_shapes(keep):
    d = AF._scene()[0]
    first, again, calls = _runs(keep)
    same = lambda a, b: np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if a.dtype == np.float64 else b)
    for k, v in first.items():
        if isinstance(v, np.ndarray):
            assert same(v, again[k]), k
        elif isinstance(v, dict):
            assert all(same(x, again[k][j]) for j, x in v.items()), k
        else:
            assert v == again[k], k
    n, B = first["n_replans"], len(d["starts"])
    assert B == 4 and first["n_claims"].shape == (n,) and (0 <= first["n_claims"]).all() and (first["n_claims"] <= B).all()
    assert ("n_kept" in first) == ("n_jumps" in first) == keep
    if keep:
        assert first["n_kept"].shape == first["n_jumps"].shape == (n,) and first["n_kept"].dtype == np.int32
        assert (0 <= first["n_kept"]).all() and (first["n_kept"] <= first["n_claims"]).all()
        assert (0 <= first["n_jumps"]).all() and (first["n_jumps"] <= B).all() and first["n_kept"][0] == 0 and first["n_jumps"][0] == 0
    assert len(calls) == n + 1                                 # every replan and the closing plan


@functools.lru_cache(maxsize=None)
def _every_seed(keep):
    d = AF._scene()[0]
    fleet, mapper, _ = AF._fleet()
    pl = _explorer(**(KEEP if keep else {}))
    return {s: AF._explore(fleet, mapper, pl, s) for s in d["seeds"].tolist()}


@pytest.mark.parametrize("keep", [False, True])
def test_gpu_coverage_against_the_cpu_chains_and_the_finishing_samples(keep):
    """tests/test_assign_keep_fleet_gpu.py's coverage check, against the CPU chains of THIS rule (tests/golden/exploration_robot_fields.npz:
    the same scene, starts, seeds and noise, ``max_claims`` = B, KEEP its recorded setting).  The bar is that test's, min - (max - min),
    taken over the chains of both recorded rules on the field -- twelve chains whose coverage runs from 0.9977 to 1.0: how far a
    different replan decision moves the coverage is the reference's own measure of what the device's different solver may cost.  At most
    one seed may miss it.  The finishing samples are recorded, not asserted."""
    d, occ, cells = AF._scene()
    k = np.load(os.path.join(AF.HERE, "golden", "exploration_robot_fields.npz"))
    rules = k["rules"].tolist()
    mine = rules.index("robot fields kept %d/%d/%d" % tuple(KEEP.values()) if keep else "robot fields")
    assert k["seeds"].tolist() == d["seeds"].tolist() and [int(v) for v in k["keep"]] == list(KEEP.values())
    assert int(k["r_claim"]) == int(d["r_claim"]) and int(k["max_recover"]) == int(d["max_recover"])
    cpu = k["field/coverage"]
    bar = float(cpu.min() - (cpu.max() - cpu.min()))
    runs = _every_seed(keep)
    w_miss, every = int(d["weights"][1]), int(d["replan_every"])
    cov = {s: float((r["evidence"][cells] <= -w_miss).sum() / cells.sum()) for s, r in runs.items()}
    at = {s: (int(np.argmax(r["n_frontier"][:, 0] == 0)) * every if (r["n_frontier"][:, 0] == 0).any() else -1) for s, r in runs.items()}
    print("coverage: device", {s: round(c, 4) for s, c in cov.items()}, "CPU chains of this rule", np.round(cpu[mine], 4).tolist(), "bar", round(bar, 4))
    print("finished at: device", at, "CPU", k["field/finished_at"][mine].tolist(), "(recorded, not asserted)")
    print("device: claims", {s: int(r["n_claims"].sum()) for s, r in runs.items()},
          "keeps", {s: int(r["n_kept"].sum()) for s, r in runs.items()} if keep else "-", "last status", {s: r["last_status"].tolist() for s, r in runs.items()})
    for r in runs.values():
        assert (r["n_claims"][r["n_frontier"][:, 0] == 0] == 0).all()
        if keep:
            assert (r["n_kept"] <= r["n_claims"]).all()
    assert sum(c < bar for c in cov.values()) <= 1, (cov, bar)


@pytest.mark.parametrize("keep", [False, True])
def test_gpu_the_first_replan_is_the_oracles_on_the_same_snapshot(keep):
    d = AF._scene()[0]
    first, _, calls = _runs(keep)
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    c = calls[0]
    B = len(d["starts"])
    if keep:
        assert np.array_equal(c["prev"], np.full(B, -1))          # the fleet has no memory yet
    want = RF.plan_batch(c["evidence"].reshape(W, H), w_miss, w_hit, origin, cell, c["start"], int(d["r_claim"]), B, c.get("prev"),
                         tuple(KEEP.values()) if keep else (0, 16, 0), int(d["r_inflate"]), int(d["min_unknown"]), None, 64,
                         may_claim=c["may_claim"])
    for k in ("status", "target_cell", "claim_round", "n_sub"):
        assert np.array_equal(c[k], want[k]), (k, c[k], want[k])
    assert np.array_equal(c["path_cost"].view(np.int64), want["path_cost"].view(np.int64))
    assert c["n_claims"].tolist() == [want["n_claims"]] == [first["n_claims"][0]] and want["n_claims"] > 0
    if keep:
        assert np.array_equal(c["kept"], want["kept"]) and c["n_kept"].tolist() == [want["n_kept"]] == [0]
