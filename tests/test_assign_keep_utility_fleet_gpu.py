"""GPU: the exploring fleet with claim hysteresis for the gain-seeded claims (GainKeepFrontierPlanner and
TiledGainKeepFrontierPlanner in UnknownEnvFleet.run_exploring) on the recorded open-field scene of tests/test_assign_fleet_gpu.py
(tests/golden/exploration_assigned.npz).  The first replans of the device run are recorded -- the evidence, the positions, who may
claim, the previous targets it was given, and what it answered -- and replayed on the host by tests/assign_keep_utility_oracle.py;
two runs give the same bits; the large-map class makes the same run; the result has n_claims, n_kept and n_jumps rows; coverage is
held against the CPU chains of tests/golden/exploration_gain_kept.npz.  The finishing sample is printed, not asserted."""
import functools
import os

import numpy as np
import pytest

import assign_keep_utility_oracle as KU
import frontier_oracle as FR
import test_assign_fleet_gpu as AF

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402

GAIN = dict(r_view=15, w_gain=16, g_cap=120, min_gain=0)
KEEP = dict(r_keep=6, keep_ratio16=24, keep_slack=8)
RECORDED = ("status", "target_cell", "target_gain", "n_claims", "n_kept", "kept", "claim_round")
REPLAYED = 5                                                  # the replans held to the oracle: the first ones, where the map is small


def _recording(base):
    class Recording(base):
        """The planner under test, with a copy (on the device) of every replan's inputs and answers."""

        def replan(self, mapper, start, **kw):
            ins = dict(evidence=mapper.evidence.clone(), start=start.clone(), may_claim=kw["may_claim"].clone(), prev=kw["prev_target"].clone())
            out = super().replan(mapper, start, **kw)
            self.calls.append(dict(ins, **{k: out[k].clone() for k in RECORDED}))
            return out
    return Recording


def _explorer(cls, **kw):
    d = AF._scene()[0]
    pl = cls(int(d["r_claim"]), int(d["max_claims"]), r_inflate=int(d["r_inflate"]), min_unknown=int(d["min_unknown"]), **GAIN, **KEEP, **kw)
    pl.calls = []
    return pl


def _explore(fleet, mapper, explorer, seed):
    r = AF._explore(fleet, mapper, explorer, seed)
    r["closing"].update({k: explorer.last[k].cpu().numpy().copy() for k in ("target_gain", "kept", "n_kept")})
    return r


@functools.lru_cache(maxsize=None)
def _runs():
    """The first recorded seed: twice with GainKeepFrontierPlanner (the second run's replans are the ones replayed), once with
    TiledGainKeepFrontierPlanner."""
    d = AF._scene()[0]
    fleet, mapper, _ = AF._fleet()
    seed = d["seeds"].tolist()[0]
    keeper = _explorer(_recording(lipmpc.GainKeepFrontierPlanner))
    first = _explore(fleet, mapper, keeper, seed)
    keeper.calls.clear()
    again = _explore(fleet, mapper, keeper, seed)
    calls = [{k: v.cpu().numpy() for k, v in c.items()} for c in keeper.calls]
    tiled = _explore(fleet, mapper, _explorer(lipmpc.TiledGainKeepFrontierPlanner), seed)
    return first, again, calls, tiled


def _same(a, b, what):
    bits = lambda v: v.view(np.int64) if v.dtype == np.float64 else v
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(bits(v), bits(b[k])), (what, k)
        elif isinstance(v, dict):
            assert all(np.array_equal(bits(x), bits(b[k][j])) for j, x in v.items()), (what, k)
        else:
            assert v == b[k], (what, k)


def _finished_at(r, every):
    return int(np.argmax(r["n_frontier"][:, 0] == 0)) * every if (r["n_frontier"][:, 0] == 0).any() else -1


def test_gpu_two_runs_give_the_same_bits_and_the_rows_have_their_shapes():
    d = AF._scene()[0]
    first, again, calls, _ = _runs()
    _same(first, again, "two runs")
    n, B = first["n_replans"], len(d["starts"])
    assert {"n_claims", "n_kept", "n_jumps"} <= set(first)
    assert first["n_kept"].shape == first["n_jumps"].shape == first["n_claims"].shape == (n,) and first["n_kept"].dtype == np.int32
    assert (0 <= first["n_kept"]).all() and (first["n_kept"] <= first["n_claims"]).all() and (first["n_claims"] <= B).all()
    assert (0 <= first["n_jumps"]).all() and (first["n_jumps"] <= B).all() and first["n_kept"][0] == 0 and first["n_jumps"][0] == 0
    assert len(calls) == n + 1                                 # every replan and the closing plan
    assert first["n_kept"].sum() > 0                           # the keep phase did something on this scene
    print("finished at", _finished_at(first, int(d["replan_every"])), "keeps per replan", first["n_kept"].tolist(), "jumps",
          first["n_jumps"].tolist(), "claims", first["n_claims"].tolist(), "(recorded, not asserted)")


def test_gpu_the_first_replans_are_the_oracles_on_the_same_snapshots():
    d = AF._scene()[0]
    first, again, calls, _ = _runs()
    (W, H), origin, cell = d["grid"].tolist(), tuple(d["origin"].tolist()), tuple(d["cell"].tolist())
    w_hit, w_miss = (int(v) for v in d["weights"])
    B = len(d["starts"])
    prev = np.full(B, -1, np.int32)
    kept = 0
    for i, c in enumerate(calls[:REPLAYED]):
        assert np.array_equal(c["prev"], prev), (i, c["prev"], prev)           # the fleet's memory: the last replan's FOUND targets
        want = KU.plan_batch(c["evidence"].reshape(W, H), w_miss, w_hit, origin, cell, c["start"], int(d["r_claim"]), GAIN["r_view"],
                             GAIN["w_gain"], GAIN["g_cap"], c["prev"], KEEP["r_keep"], KEEP["keep_ratio16"], KEEP["keep_slack"], GAIN["min_gain"],
                             int(d["max_claims"]), int(d["r_inflate"]), int(d["min_unknown"]), None, 64, may_claim=c["may_claim"])
        for k in ("status", "target_cell", "target_gain", "kept", "claim_round"):
            assert np.array_equal(c[k], want[k]), (i, k, c[k], want[k])
        assert c["n_kept"].tolist() == [want["n_kept"]] and c["n_claims"].tolist() == [want["n_claims"]], i
        assert again["n_kept"][i] == want["n_kept"] and again["n_claims"][i] == want["n_claims"]
        found = (c["status"] == FR.FOUND) & (prev >= 0)
        d2 = (c["target_cell"] // H - prev // H) ** 2 + (c["target_cell"] % H - prev % H) ** 2
        assert again["n_jumps"][i] == int((found & (d2 > KEEP["r_keep"] ** 2)).sum()), i
        prev = np.where(c["status"] == FR.FOUND, c["target_cell"], -1).astype(np.int32)
        kept += want["n_kept"]
    assert kept > 0                                            # the replayed replans include keepers


def test_gpu_the_large_map_class_makes_the_same_run():
    """Every slot settles (rounds=None), so every replan's outputs are the one-workgroup class's bit for bit, and so is the run."""
    first, _, _, tiled = _runs()
    assert set(tiled) == set(first) and tiled["n_kept"].sum() > 0
    _same(first, tiled, "tiled")


@functools.lru_cache(maxsize=None)
def _every_seed():
    d = AF._scene()[0]
    fleet, mapper, _ = AF._fleet()
    keeper = _explorer(lipmpc.GainKeepFrontierPlanner)
    return {s: AF._explore(fleet, mapper, keeper, s) for s in d["seeds"].tolist()}


def test_gpu_coverage_against_the_cpu_chains_and_the_finishing_samples():
    """tests/test_assign_keep_fleet_gpu.py's coverage check against the CPU chains of tests/golden/exploration_gain_kept.npz (the
    same scene, starts, seeds and noise; KEEP is its first recorded setting).  The bar is that test's, min - (max - min), taken over
    the chains of BOTH recorded settings of the new rule: they differ only in the keep parameters, and how far that moves the
    coverage is the reference's own measure of what a different replan decision costs.  At most one seed may miss it.  The
    finishing samples are recorded, not asserted."""
    d, occ, cells = AF._scene()
    k = np.load(os.path.join(AF.HERE, "golden", "exploration_gain_kept.npz"))
    rules = k["rules"].tolist()
    mine = rules.index("seeded 0 + keep %d/%d/%d" % tuple(KEEP.values()))
    new = [i for i, r in enumerate(rules) if r.startswith("seeded 0 + keep")]
    assert k["seeds"].tolist() == d["seeds"].tolist() and k["gain"].tolist() == list(GAIN.values()) and len(new) == len(k["keeps"]) >= 2
    assert int(k["r_claim"]) == int(d["r_claim"]) and int(k["max_recover"]) == int(d["max_recover"])
    cpu = k["field/coverage"][new]
    bar = float(cpu.min() - (cpu.max() - cpu.min()))
    runs = _every_seed()
    w_miss, every = int(d["weights"][1]), int(d["replan_every"])
    cov = {s: float((r["evidence"][cells] <= -w_miss).sum() / cells.sum()) for s, r in runs.items()}
    print("coverage: device", {s: round(c, 4) for s, c in cov.items()}, "CPU chains of the rule", np.round(cpu, 4).tolist(), "bar", round(bar, 4))
    print("finished at: device", {s: _finished_at(r, every) for s, r in runs.items()}, "CPU", k["field/finished_at"][mine].tolist(),
          "CPU seeded 0", k["field/finished_at"][rules.index("seeded 0")].tolist(), "(recorded, not asserted)")
    print("device: keeps", {s: int(r["n_kept"].sum()) for s, r in runs.items()}, "jumps", {s: int(r["n_jumps"].sum()) for s, r in runs.items()},
          "CPU keeps", k["field/n_kept"][mine].tolist(), "CPU jumps", k["field/n_jumps"][mine].tolist(),
          "last status", {s: r["last_status"].tolist() for s, r in runs.items()})
    for r in runs.values():
        assert (r["n_kept"] <= r["n_claims"]).all() and (r["n_claims"][r["n_frontier"][:, 0] == 0] == 0).all() and r["n_kept"].sum() > 0
    assert sum(c < bar for c in cov.values()) <= 1, (cov, bar)
