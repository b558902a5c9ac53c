"""GPU: the exploring fleet with claim hysteresis (a CoordinatedFrontierPlanner with r_keep in UnknownEnvFleet.run_exploring) on the
recorded scene of tests/test_assign_fleet_gpu.py (tests/golden/exploration_assigned.npz).  Every replan of the device run is
recorded -- the evidence, the positions, who may claim, the previous targets it was given, and what it answered -- and replayed on
the host by tests/assign_keep_oracle.py; two runs give the same bits; the new result rows have the documented shapes; a planner
without r_keep makes the run of before.  The finishing sample is recorded, not asserted."""
import functools
import os

import numpy as np
import pytest

import assign_keep_oracle as K
import frontier_oracle as FR
import test_assign_fleet_gpu as AF

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

KEEP = dict(r_keep=6, keep_ratio16=24, keep_slack=8)
RECORDED = ("status", "target_cell", "n_claims", "n_kept", "kept", "claim_round")


class _Recording(lipmpc.CoordinatedFrontierPlanner):
    """The planner under test, with a copy (on the device) of every replan's inputs and answers."""

    def replan(self, mapper, start, **kw):
        ins = dict(evidence=mapper.evidence.clone(), start=start.clone(), may_claim=kw["may_claim"].clone(), prev=kw["prev_target"].clone())
        out = super().replan(mapper, start, **kw)
        self.calls.append(dict(ins, **{k: out[k].clone() for k in RECORDED}))
        return out


def _explorer(cls=_Recording, **keep):
    d = AF._scene()[0]
    pl = cls(int(d["r_claim"]), int(d["max_claims"]), r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]), **keep)
    pl.calls = []
    return pl


@functools.lru_cache(maxsize=None)
def _runs():
    """The first recorded seed, twice with r_keep (the second run's replans are the ones replayed) and once without."""
    d = AF._scene()[0]
    fleet, mapper, _ = AF._fleet()
    seed = d["seeds"].tolist()[0]
    keeper = _explorer(**KEEP)
    first = AF._explore(fleet, mapper, keeper, seed)
    keeper.calls.clear()
    again = AF._explore(fleet, mapper, keeper, seed)
    calls = [{k: v.cpu().numpy() for k, v in c.items()} for c in keeper.calls]
    plain = AF._explore(fleet, mapper, _explorer(lipmpc.CoordinatedFrontierPlanner), seed)
    return first, again, calls, plain


def test_gpu_two_runs_give_the_same_bits_and_the_rows_have_their_shapes():
    d = AF._scene()[0]
    first, again, calls, _ = _runs()
    same = lambda a, b: np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if a.dtype == np.float64 else b)
    for k, v in first.items():
        if isinstance(v, np.ndarray):
            assert same(v, again[k]), k
        elif isinstance(v, dict):
            assert all(same(x, again[k][j]) for j, x in v.items()), k
        else:
            assert v == again[k], k
    n, B = first["n_replans"], len(d["starts"])
    assert first["n_kept"].shape == first["n_jumps"].shape == first["n_claims"].shape == (n,) and first["n_kept"].dtype == np.int32
    assert (0 <= first["n_kept"]).all() and (first["n_kept"] <= first["n_claims"]).all() and (first["n_claims"] <= B).all()
    assert (0 <= first["n_jumps"]).all() and (first["n_jumps"] <= B).all() and first["n_kept"][0] == 0 and first["n_jumps"][0] == 0
    assert len(calls) == n + 1                                 # every replan and the closing plan
    every = int(d["replan_every"])
    at = int(np.argmax(first["n_frontier"][:, 0] == 0)) * every if (first["n_frontier"][:, 0] == 0).any() else -1
    print("finished at", at, "keeps per replan", first["n_kept"].tolist(), "jumps", first["n_jumps"].tolist(), "claims",
          first["n_claims"].tolist(), "(recorded, not asserted)")
    assert first["n_kept"].sum() > 0                           # the keep phase did something on this scene


def test_gpu_every_replan_is_the_oracles_on_the_same_snapshot():
    d = AF._scene()[0]
    first, again, calls, _ = _runs()
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    B, n = len(d["starts"]), first["n_replans"]
    prev = np.full(B, -1, np.int32)
    for i, c in enumerate(calls):
        assert np.array_equal(c["prev"], prev), (i, c["prev"], prev)           # the fleet's memory: the last replan's FOUND targets
        want = K.plan_batch(c["evidence"].reshape(W, H), w_miss, w_hit, origin, cell, c["start"], int(d["r_claim"]), c["prev"], KEEP["r_keep"],
                            KEEP["keep_ratio16"], KEEP["keep_slack"], int(d["max_claims"]), int(d["r_inflate"]), int(d["min_unknown"]), None, 64,
                            may_claim=c["may_claim"])
        for k in ("status", "target_cell", "kept", "claim_round"):
            assert np.array_equal(c[k], want[k]), (i, k, c[k], want[k])
        assert c["n_kept"].tolist() == [want["n_kept"]] and c["n_claims"].tolist() == [want["n_claims"]], i
        if i < n:                                              # (the closing plan is not counted and leaves the memory alone)
            assert again["n_kept"][i] == want["n_kept"] and again["n_claims"][i] == want["n_claims"]
            found = (c["status"] == FR.FOUND) & (prev >= 0)
            d2 = (c["target_cell"] // H - prev // H) ** 2 + (c["target_cell"] % H - prev % H) ** 2
            assert again["n_jumps"][i] == int((found & (d2 > KEEP["r_keep"] ** 2)).sum()), i
            prev = np.where(c["status"] == FR.FOUND, c["target_cell"], -1).astype(np.int32)


def test_gpu_without_r_keep_the_run_is_the_one_of_before():
    """The result has the keys of before and no others, and every array of it equals, bit for bit, the run that
    tests/test_assign_fleet_gpu.py makes for the same seed with its own planner -- the run that module holds to the oracle."""
    first, _, _, plain = _runs()
    assert set(first) - set(plain) == {"n_kept", "n_jumps"} and set(plain) - set(first) == set()
    theirs = AF._runs()[0][AF._scene()[0]["seeds"].tolist()[0]]
    assert set(plain) == set(theirs)
    same = lambda a, b: np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if a.dtype == np.float64 else b)
    for k, v in theirs.items():
        if isinstance(v, np.ndarray):
            assert same(v, plain[k]), k
        elif isinstance(v, dict):
            assert all(same(x, plain[k][j]) for j, x in v.items()), k
        else:
            assert v == plain[k], k


@functools.lru_cache(maxsize=None)
def _every_seed():
    d = AF._scene()[0]
    fleet, mapper, _ = AF._fleet()
    keeper = _explorer(lipmpc.CoordinatedFrontierPlanner, **KEEP)
    return {s: AF._explore(fleet, mapper, keeper, s) for s in d["seeds"].tolist()}


def test_gpu_coverage_against_the_cpu_chains_and_the_finishing_samples():
    """tests/test_assign_fleet_gpu.py's coverage check against the CPU chains of tests/golden/exploration_kept.npz (the same scene,
    starts, seeds and noise; KEEP is its first recorded setting).  The bar is that test's, min - (max - min), taken over the kept
    chains of ALL recorded settings: the six chains of one setting all reach 1.0, so their own spread is 0 and says nothing; the
    eighteen differ only in the keep parameters, and how far that moves the coverage is the reference's own measure of what a
    different replan decision costs.  At most one seed may miss it.  The finishing samples are recorded, not asserted."""
    d, occ, cells = AF._scene()
    k = np.load(os.path.join(AF.HERE, "golden", "exploration_kept.npz"))
    rules = k["rules"].tolist()
    mine = rules.index("kept %d/%d/%d" % (KEEP["r_keep"], KEEP["keep_ratio16"], KEEP["keep_slack"]))
    assert k["seeds"].tolist() == d["seeds"].tolist() and [int(v) for v in k["keeps"][mine - 2]] == list(KEEP.values())
    assert int(k["r_claim"]) == int(d["r_claim"]) and int(k["max_recover"]) == int(d["max_recover"])
    cpu = k["field/coverage"][2:]
    bar = float(cpu.min() - (cpu.max() - cpu.min()))
    runs = _every_seed()
    w_miss, every = int(d["weights"][1]), int(d["replan_every"])
    cov = {s: float((r["evidence"][cells] <= -w_miss).sum() / cells.sum()) for s, r in runs.items()}
    at = {s: (int(np.argmax(r["n_frontier"][:, 0] == 0)) * every if (r["n_frontier"][:, 0] == 0).any() else -1) for s, r in runs.items()}
    print("coverage: device", {s: round(c, 4) for s, c in cov.items()}, "CPU kept chains", np.round(cpu, 4).tolist(), "bar", round(bar, 4))
    print("finished at: device", at, "CPU kept", k["field/finished_at"][mine].tolist(), "CPU assigned", k["field/finished_at"][1].tolist(),
          "CPU nearest", k["field/finished_at"][0].tolist(), "(recorded, not asserted)")
    print("device: keeps", {s: int(r["n_kept"].sum()) for s, r in runs.items()}, "jumps", {s: int(r["n_jumps"].sum()) for s, r in runs.items()},
          "CPU keeps", k["field/n_kept"][mine].tolist(), "last status", {s: r["last_status"].tolist() for s, r in runs.items()})
    for r in runs.values():
        assert (r["n_kept"] <= r["n_claims"]).all() and (r["n_claims"][r["n_frontier"][:, 0] == 0] == 0).all()
    assert sum(c < bar for c in cov.values()) <= 1, (cov, bar)
