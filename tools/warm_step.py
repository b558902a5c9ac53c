"""Warm-start records on the step path (lipmpc_set_warm_start): cost and iterations of one step launch, cold vs warm.

On the bench batch (bench.make_inputs, B = 4096, N = 8, 10 obstacles) per mode (exact, interior = FLAG_INTERIOR, the mode of
the compat classes and UnknownEnvFleet) and per handle:
  default     the mode's own handle (exact: presolve on, the dispatching kernel)
  flag        FLAG_WARM_START without a record (every row kept, cold start)
  warm        FLAG_WARM_START with the record the previous step left (the batch one MPC step on, bench.one_step_later)
ms per launch (HIP events, median), mean and max-per-wave (4 problems of 16 lanes) interior-point iterations, mean finish
rounds (diag word 0).  Then a 40-sample host-driven loop (plan_step_batch + advance) with a record against rollout with
FLAG_INTERIOR | FLAG_WARM_START on the same robots.  Prints one JSON object.

    python tools/warm_step.py [--reps 20] [--out profiles/warm_step.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lipmpc  # noqa: E402
from bench import make_inputs, one_step_later  # noqa: E402


def _stats(o, G=16):
    it = o["iters"].cpu().numpy()
    waves = it[: len(it) // (64 // G) * (64 // G)].reshape(-1, 64 // G).max(axis=1)
    return dict(iters_mean=float(it.mean()), iters_max_per_wave_mean=float(waves.mean()),
                finish_rounds_mean=float(o["diag"][:, 0].cpu().numpy().mean()),
                solved_or_uncertified=float(np.isin(o["status"].cpu().numpy(), (0, 4)).mean()))


def _time(fn, reps, before=None):
    ts = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from importlib import import_module
    synth = import_module("humanoid-navigation-using-mpc-ldcbf_amd.synth")
    B, N, n_obs = 4096, 8, 10
    dev = torch.device("cuda", 0)
    inp = make_inputs(lipmpc, synth, B, N, n_obs, 0, 0, dev, 0)
    st, ft, goal, xy, nv, delta = inp["state"], inp["foot"], inp["goal"], inp["obs_xy"], inp["obs_nv"], inp["delta"]
    st_b, ft_b = one_step_later(inp["walker"], st, ft, goal, xy, nv, delta)
    res = dict(B=B, N=N, n_obs=n_obs, reps=args.reps)
    for mode, base in (("exact", 0), ("interior", lipmpc.FLAG_INTERIOR)):
        P = lambda fl: lipmpc.LipMpcParams(N=N, n_obs_max=n_obs, v_max=5, flags=base | fl)
        r = {}
        for name, fl in (("default", 0), ("flag", lipmpc.FLAG_WARM_START)):
            sv = lipmpc.BatchedLipMpc(P(fl))
            out = sv.alloc_outputs(B, with_diag=True)
            sv.plan_step_batch(st_b, goal, ft_b, xy, nv, delta, out=out, with_diag=True)
            r[name] = dict(ms=_time(lambda: sv.plan_step_batch(st_b, goal, ft_b, xy, nv, delta, out=out), args.reps), **_stats(out))
        sv = lipmpc.BatchedLipMpc(P(lipmpc.FLAG_WARM_START))
        assert sv.set_warm_start(B)
        out = sv.alloc_outputs(B, with_diag=True)
        sv.plan_step_batch(st, goal, ft, xy, nv, delta, out=out)           # the previous step leaves the record
        saved = sv.warm_record.clone()
        run = lambda: sv.plan_step_batch(st_b, goal, ft_b, xy, nv, delta, out=out)
        ms = _time(run, args.reps, before=lambda: sv.warm_record.copy_(saved))
        sv.warm_record.copy_(saved)
        run()
        torch.cuda.synchronize()
        r["warm"] = dict(ms=ms, records_with_result=float((saved[:, 0] == 1.0).float().mean()), **_stats(out))
        res[mode] = r
    # 40-sample host-driven warm loop against the rollout (interior mode, as the closed loops run)
    K = args.samples
    P = lipmpc.LipMpcParams(N=N, n_obs_max=n_obs, v_max=5, flags=lipmpc.FLAG_INTERIOR | lipmpc.FLAG_WARM_START)
    loop = {}
    for name, warm in (("host_warm", True), ("host_cold_flag", False)):
        sv = lipmpc.BatchedLipMpc(P)
        if warm:
            assert sv.set_warm_start(B)
        out = sv.alloc_outputs(B)
        s, f = st.clone(), ft.clone()
        its = torch.zeros((B,), dtype=torch.int64, device=dev)
        sv.plan_step_batch(s, goal, f, xy, nv, delta, out=out)            # sample 0 untimed (first launch of the handle)
        its += out["iters"]
        sv.advance(s, f, out)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(K - 1):
            sv.plan_step_batch(s, goal, f, xy, nv, delta, out=out)
            its += out["iters"]
            sv.advance(s, f, out)
        b.record()
        torch.cuda.synchronize()
        loop[name] = dict(ms_samples_1_to_K=a.elapsed_time(b), iters_per_step=float(its.double().mean()) / K)
    sv = lipmpc.BatchedLipMpc(P)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ro = sv.rollout(st, goal, ft, xy, nv, delta, k_max=K, mpc_step=1, stop_obj=-1.0)
    b.record()
    torch.cuda.synchronize()
    n = ro["n_steps"].double()
    loop["rollout_warm"] = dict(ms_total=a.elapsed_time(b),
                                iters_per_step=float((ro["total_iters"].double() / n.clamp(min=1)).mean()),
                                mean_samples=float(n.mean()))
    res["loop_40"] = loop
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
