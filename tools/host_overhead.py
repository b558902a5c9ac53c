"""Dev tool: host time per enqueued call of the entry points that marshal the longest argument lists -- plan_step_batch,
LidarSensor.sense_plan_step, fleet_update -- at B = 4 and B = 4096, 500 calls each after 10 of warm-up.
python tools/host_overhead.py [TREE]: imports lipmpc from TREE (default: this checkout; LIPMPC_LIB picks the library) and
prints one JSON line of microseconds per call."""
import json
import os
import sys
import time

import torch

TREE = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
import lipmpc  # noqa: E402

CALLS, WARM_UP, K_MAX = 500, 10, 8
dev = torch.device("cuda", 0)
f64 = dict(dtype=torch.float64, device=dev)


def per_call_us(fn):
    for _ in range(WARM_UP):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return round(1e6 * (t1 - t0) / CALLS, 3)


res = {"tree": TREE, "calls": CALLS}
square = [[1.0, 1.0], [2.0, 1.0], [2.0, 2.0], [1.0, 2.0]]
for B in (4, 4096):
    sv = lipmpc.BatchedLipMpc(lipmpc.LipMpcParams(N=8, n_obs_max=10, v_max=5), 0)
    st, goal = torch.zeros((B, 5), **f64), torch.ones((B, 2), **f64) * 5
    foot = torch.ones((B,), dtype=torch.int8, device=dev)
    xy, nv = torch.zeros((B, 10, 5, 2), **f64), torch.zeros((B, 10), dtype=torch.int32, device=dev)
    out = sv.alloc_outputs(B)
    res[f"plan_step_batch_B{B}_us"] = per_call_us(lambda: sv.plan_step_batch(st, goal, foot, xy, nv, None, out=out))

    sensor = lipmpc.LidarSensor([square], lidar_range=3.0, device=0)
    sv = lipmpc.BatchedLipMpc(lipmpc.LipMpcParams(N=3, n_obs_max=sensor.n_obs_max, v_max=sensor.v_max, flags=lipmpc.FLAG_INTERIOR), 0)
    sen, out = sensor.alloc_outputs(B, rings=False, c_eta=True), sv.alloc_outputs(B)
    res[f"sense_plan_step_B{B}_us"] = per_call_us(lambda: sensor.sense_plan_step(sv, st, goal, foot, None, None, sen=sen, out=out))

    # the device-side sample counter passes K_MAX during the warm-up: every timed call is the full launch, its rows ignored
    i32 = dict(dtype=torch.int32, device=dev)
    fleet = dict(state=st.clone(), first_foot=foot.clone(), walking=torch.ones((B,), dtype=torch.int8, device=dev),
                 last_obj=torch.full((B,), float("inf"), **f64), n_steps=torch.zeros((B,), **i32), last_status=torch.zeros((B,), **i32),
                 n_overflow=torch.zeros((B,), **i32), sample=torch.zeros((1,), **i32), X_pred=torch.zeros((B, K_MAX + 1, 5), **f64),
                 U_pred=torch.zeros((B, K_MAX, 3), **f64))
    res[f"fleet_update_B{B}_us"] = per_call_us(lambda: sv.fleet_update(fleet, out, overflow=sen["overflow"]))
print(json.dumps(res))
