"""Time the neighbour LDCBF rows (lipmpc_neighbour_c_eta_batch: grid sort, 3 x 3 walk, rows -- six launches per call) and write
profiles/neighbours.json.  Needs the GPU.

Robots of one group, uniform in a square sized for a mean n_near of about 2 and of about 8 (side = sqrt(B pi R^2 / n_near)), at
B = 4096 and B = 32768; sense_range 1.5, radius 0.25, k_rows 4, 12 obstacle slots, share 0.5.  Per shape: warm-up, then rounds of
`reps` back-to-back calls between two device events, the shapes alternating from round to round; median / min / max of the
rounds.  The structural check is derived, not measured: at equal density time(32768) / time(4096) is 8 for a linear method
and 64 for a quadratic one; a ratio above 16 is flagged (`scaling_flagged`).

--parent-bench / --bench: files (one per run) holding the JSON line bench.py printed in the same session with the parent commit's
library and with this one (config 2: `bench.py --gpus 1`); their ms_per_step are recorded next to the figures (the step solver is
not touched by the neighbour rows: the two are the same code)."""
import argparse
import json
import math
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import lipmpc  # noqa: E402

SENSE_RANGE, RADIUS, K_ROWS, N_OBS_MAX = 1.5, 0.25, 4, 12
SCALING_LIMIT = 16.0


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_line(path):
    """The last JSON object line of a file bench.py's output was kept in."""
    for line in reversed(open(path).read().splitlines()):
        line = line.strip()
        if line.startswith("{") and line.endswith("}"):
            rec = json.loads(line)
            return {k: rec.get(k) for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup")}
    raise SystemExit(f"{path}: no JSON line")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbours.json"))
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-bench", nargs="+", default=[], metavar="FILE")
    ap.add_argument("--bench", nargs="+", default=[], metavar="FILE")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    nb = lipmpc.NeighbourRows(RADIUS, SENSE_RANGE, K_ROWS)
    shapes = {}
    for target in (2, 8):
        for B in (4096, 32768):
            side = math.sqrt(B * math.pi * SENSE_RANGE ** 2 / target)
            gen = torch.Generator(device=dev).manual_seed(B + target)
            st = torch.zeros((B, 5), dtype=torch.float64, device=dev)
            st[:, 0], st[:, 2] = (torch.rand((2, B), dtype=torch.float64, device=dev, generator=gen) * side).unbind(0)
            ce = torch.zeros((B, N_OBS_MAX, 4), dtype=torch.float64, device=dev)
            first = torch.randint(0, 5, (B,), dtype=torch.int32, device=dev, generator=gen)       # as after a scan: a few rows taken
            out = nb.alloc_outputs(B)
            shapes[(target, B)] = dict(side=side, call=lambda st=st, ce=ce, first=first, out=out: nb.append(st, ce, first, out=out), out=out)
    for s in shapes.values():                                 # warm up every shape
        for _ in range(20):
            s["call"]()
    torch.cuda.synchronize()
    ms = {k: [] for k in shapes}
    for _ in range(a.rounds):
        for k, s in shapes.items():
            ms[k].append(events_ms(s["call"], a.reps))
    res = {"what": "lipmpc_neighbour_c_eta_batch, ms per call (six launches: clear, bin, runs, scatter, search, rows), device events around "
                   "`reps` back-to-back calls, median / min / max over rounds that alternate between the shapes; one group, robots uniform "
                   "in a square, first_slot random in 0..4",
           "device": torch.cuda.get_device_name(0), "sense_range": SENSE_RANGE, "radius": RADIUS, "k_rows": K_ROWS, "n_obs_max": N_OBS_MAX,
           "share": 0.5, "reps_per_round": a.reps, "rounds": a.rounds, "shapes": [], "scaling": []}
    med = {}
    for (target, B), s in shapes.items():
        n_near, n_rows = s["out"]["n_near"].double(), s["out"]["n_rows"].double()
        med[(target, B)] = float(np.median(ms[(target, B)]))
        res["shapes"].append({"robots": B, "target_mean_n_near": target, "square_side": s["side"], "mean_n_near": float(n_near.mean()),
                              "max_n_near": int(n_near.max()), "mean_n_rows": float(n_rows.mean()),
                              "crowded_robots": int((s["out"]["n_near"] > s["out"]["n_rows"]).sum()),
                              "ms_per_call": {"median": med[(target, B)], "min": float(min(ms[(target, B)])), "max": float(max(ms[(target, B)]))},
                              "ns_per_robot": 1e6 * med[(target, B)] / B})
    flagged = False
    for target in (2, 8):
        ratio = med[(target, 32768)] / med[(target, 4096)]
        flagged |= ratio > SCALING_LIMIT
        res["scaling"].append({"target_mean_n_near": target, "time_32768_over_4096": ratio, "linear": 8, "quadratic": 64,
                               "flag_above": SCALING_LIMIT, "flagged": bool(ratio > SCALING_LIMIT)})
    res["scaling_flagged"] = bool(flagged)
    from code_object import kernel_resources
    res["kernels"] = {re.search(r"nb_[a-z]+_kernel(?:ILi\d+E)?", k).group(0):
                      {"vgpr": r["vgpr_count"], "sgpr": r["sgpr_count"], "scratch_bytes": r["private_segment_fixed_size"], "lds_bytes": r["group_segment_fixed_size"]}
                      for k, r in kernel_resources(lipmpc._lib.LIB_PATH).items() if "nb_" in k}
    if a.parent_bench or a.bench:
        res["step_config2"] = {"what": "bench.py --gpus 1 (config 2) with the parent commit's library and with this commit's, run alternately "
                                       "in the same session, in the order listed",
                               "parent_commit": [bench_line(f) for f in a.parent_bench], "this_commit": [bench_line(f) for f in a.bench]}
    res["not_measured"] = ["per-kernel times (no kernel trace was taken)", "hardware counters", "robots in several groups", "clustered (non-uniform) robots",
                           "k_rows above 4 (the 16-candidate search kernel)"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"shapes": res["shapes"], "scaling": res["scaling"]}, indent=1))
    if flagged:
        print("SCALING FLAGGED: time(32768) / time(4096) above", SCALING_LIMIT)


if __name__ == "__main__":
    main()
