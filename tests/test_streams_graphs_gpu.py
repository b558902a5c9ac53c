"""Step launches of one handle across streams and graphs (-m gpu).

A 32-lane handle in the exact mode runs its steps as a split launch (classification -> index lists -> one kernel per solver
body) on a workspace that holds one launch's class keys and lists.  These tests hold the launches that could meet on such a
workspace -- two streams without ordering, a captured graph next to eager launches and to a workspace that grew or was
registered again, the handle's history before a call -- to the eager answer of the same batch launched alone on one stream,
bit for bit: the split launch is deterministic from run to run.  NaN-aware equality only for the float outputs of unsolved
problems.  The eager answers themselves are held to the C oracle in test_gpu_configs.py / test_params_gpu.py.

Concurrent launches here always have the same batch size, and every batch is launched eagerly first, so that on a handle
whose launches did share one workspace every list position a body could read holds an index below B.  No test empties the
allocator's cache once a buffer a graph holds may have been released (torch.cuda.graph does so only as a capture begins): a
released buffer stays mapped, and a stray write lands in a tensor the test owns (the canaries)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import lipmpc  # noqa: E402
from helpers import crowded_batch  # noqa: E402

STEP_KEYS = ("U", "X", "theta", "omega", "obj", "status", "iters", "active", "working", "diag", "c_eta")
CANARY = 0x5A5A5A5A
GATE_FACTOR = 20          # the held-back stream sleeps at least this many eager launches
MAX_SLEEP_MS = 150.0


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _batch(N, n_obs, B, seed):
    st, goal, foot, xy, nv = crowded_batch(N, n_obs, B, seed=seed)
    return [_dev(st, torch.float64), _dev(goal, torch.float64), _dev(foot, torch.int8), _dev(xy, torch.float64),
            _dev(nv, torch.int32), None]


def _assert_same(got, ref, tag, keys=STEP_KEYS):
    """Every output present in ``ref`` bit for bit; NaN == NaN only in the float rows of problems ``ref`` did not solve."""
    unsolved = ~torch.isin(ref["status"], torch.tensor([lipmpc.STATUS_SOLVED, lipmpc.STATUS_UNCERTIFIED], device=ref["status"].device))
    n = 0
    for k in keys:
        if k not in ref:
            continue
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, k)
        if a.dtype == torch.float64:
            same = a.view(torch.int64) == b.view(torch.int64)
            rows = unsolved.view(-1, *([1] * (a.dim() - 1))).expand_as(a)
            same |= a.isnan() & b.isnan() & rows
        else:
            same = a == b
        bad = int((~same).reshape(a.shape[0], -1).any(dim=1).sum())
        assert bad == 0, f"{tag}: {k} differs on {bad} of {a.shape[0]} problems"
        n += 1
    assert n >= 5, (tag, n)


def _events_ms(fn, stream=None):
    s = stream or torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record(s)
        fn()
        e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def _sleep_cycles(ms):
    """torch.cuda._sleep cycles for about ``ms`` milliseconds, from one timed sleep."""
    probe = 2_000_000
    _events_ms(lambda: torch.cuda._sleep(probe))                   # (first launch of the sleep kernel)
    t = _events_ms(lambda: torch.cuda._sleep(probe))
    assert t > 0.0
    return max(1, int(probe * ms / t))


def _gated(first, second, eager_ms):
    """``first`` on stream A behind a sleep, ``second`` on stream B with no dependency on A; both streams wait for the inputs.
    Returns (their results, the sleep's length in ms measured by events on A)."""
    cycles = _sleep_cycles(min(MAX_SLEEP_MS, 2.5 * GATE_FACTOR * eager_ms))
    cur = torch.cuda.current_stream()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sa.wait_stream(cur)
    sb.wait_stream(cur)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(sa):
        e0.record(sa)
        torch.cuda._sleep(cycles)
        e1.record(sa)
        ra = first()
    with torch.cuda.stream(sb):
        rb = second()
    torch.cuda.synchronize()
    return ra, rb, e0.elapsed_time(e1)


def _classes(sv, B):
    """(class of every problem, problems per class) of the handle's last split launch (launched on this stream)."""
    ws = sv._ws.cpu().numpy()
    return ws[8:8 + B] // 16, ws[:5].copy()


@pytest.mark.parametrize("N,n_obs", [(12, 9), (16, 30)])
def test_one_handle_on_two_unordered_streams(N, n_obs):
    """T1: two batches of the same size on two streams of ONE handle, the first held back by a sleep: each stream's launch
    must solve its own batch from its own classification (with one workspace per handle, the held-back launch rewrote the
    lists the other launch's side-stream bodies then read).  Which launch such a race hits, and whether it shows at all,
    depends on how the runtime maps the streams onto its few hardware queues: a stream that shares a queue with a side stream
    waiting for the held-back fork waits too.  One workspace per stream is correct under every mapping."""
    B = 1024
    sv = lipmpc.BatchedLipMpc(lipmpc.LipMpcParams(N=N, n_obs_max=n_obs, v_max=5))
    assert sv._split_capable
    A, Bb = _batch(N, n_obs, B, seed=7 * N + n_obs), _batch(N, n_obs, B, seed=7 * N + n_obs + 1)
    kw = dict(with_c_eta=True, with_diag=True, with_working=True)
    ref_a = sv.plan_step_batch(*A, **kw)
    torch.cuda.synchronize()
    cls_a, cnt_a = _classes(sv, B)
    ref_b = sv.plan_step_batch(*Bb, **kw)
    torch.cuda.synchronize()
    cls_b, cnt_b = _classes(sv, B)
    ckw = dict(with_diag=True, with_working=True)
    ref_ca = sv.plan_step_batch_c_eta(*A[:3], ref_a["c_eta"], **ckw)
    ref_cb = sv.plan_step_batch_c_eta(*Bb[:3], ref_b["c_eta"], **ckw)
    torch.cuda.synchronize()
    # the race could not hide: the batches spread over the bodies, and differently
    assert np.mean(cls_a != cls_b) >= 0.10, np.mean(cls_a != cls_b)
    assert (cnt_a > 0).sum() >= 3 and (cnt_b > 0).sum() >= 3, (cnt_a, cnt_b)
    assert int(np.isin(ref_a["status"].cpu().numpy(), (0, 4)).sum()) > B // 3
    o = sv.alloc_outputs(B, **kw)
    sv.plan_step_batch(*A, out=o)
    eager_ms = _events_ms(lambda: sv.plan_step_batch(*A, out=o))
    cases = (("A held back", lambda: sv.plan_step_batch(*A, **kw), lambda: sv.plan_step_batch(*Bb, **kw), ref_a, ref_b),
             ("B held back", lambda: sv.plan_step_batch(*Bb, **kw), lambda: sv.plan_step_batch(*A, **kw), ref_b, ref_a),
             ("c_eta, A held back", lambda: sv.plan_step_batch_c_eta(*A[:3], ref_a["c_eta"], **ckw),
              lambda: sv.plan_step_batch_c_eta(*Bb[:3], ref_b["c_eta"], **ckw), ref_ca, ref_cb))
    for tag, first, second, ref1, ref2 in cases:
        g1, g2, slept = _gated(first, second, eager_ms)
        assert slept >= GATE_FACTOR * eager_ms, (tag, slept, eager_ms)       # the gate held
        _assert_same(g2, ref2, f"{tag}: the launch that was not held back")
        _assert_same(g1, ref1, f"{tag}: the held-back launch")


def _canaries(nbytes, n=64):
    """``n`` int32 tensors of ``nbytes`` bytes filled with CANARY: the caching allocator may hand any of them a block of that
    size that was just released."""
    return [torch.full((nbytes // 4,), CANARY, dtype=torch.int32, device="cuda") for _ in range(n)]


@pytest.mark.parametrize("after", ["growth", "set_workspace", "set_schedule"])
def test_captured_step_survives_growth_and_reregistration(after):
    """T2: a step captured at B1 = 600 keeps working after the handle grew its workspace for a larger eager batch, or had a
    workspace / schedule registered again -- and the replay writes nowhere but into its own buffers (canaries of the old
    buffer's size stay untouched).  T3 (growth): the replay and an eager launch of another batch on a third stream, unordered,
    are both correct."""
    N, n_obs, B1, B2 = 12, 9, 600, 1500
    sv = lipmpc.BatchedLipMpc(lipmpc.LipMpcParams(N=N, n_obs_max=n_obs, v_max=5))
    args = _batch(N, n_obs, B1, seed=91)
    st2 = args[0].clone()
    st2[:, 0] += 0.03
    st2[:, 2] -= 0.02                                   # the new states the replay will see
    big = _batch(N, n_obs, B2, seed=92)
    other = _batch(N, n_obs, B1, seed=93)
    kw = dict(with_c_eta=True, with_diag=True, with_working=True)
    if after == "set_schedule":
        sv.set_schedule(B1)
    ref = sv.plan_step_batch(st2, *args[1:], **kw)      # the eager B1 answer on the new states
    ref_other = sv.plan_step_batch(*other, **kw)
    torch.cuda.synchronize()
    assert int(np.isin(ref["status"].cpu().numpy(), (0, 4)).sum()) > B1 // 3
    out = sv.alloc_outputs(B1, **kw)
    sv.plan_step_batch(*args, out=out)                  # warm-up outside the capture
    torch.cuda.synchronize()
    old_bytes = (4 * int(sv.lib.lipmpc_schedule_words(B1)) if after == "set_schedule"
                 else int(sv.lib.lipmpc_workspace_bytes(sv._h, B1)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            sv.plan_step_batch(*args, out=out)
    torch.cuda.current_stream().wait_stream(side)
    if after == "growth":
        sv.plan_step_batch(*big)
    elif after == "set_workspace":
        sv.set_workspace(B1)
    else:
        sv.set_schedule(B1)
    torch.cuda.synchronize()
    canaries = _canaries(old_bytes)
    args[0].copy_(st2)
    for k in ("U", "X", "status", "iters", "active"):
        out[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    _assert_same(out, ref, f"replay after {after}")
    for i, c in enumerate(canaries):
        assert bool((c == CANARY).all()), f"canary {i} of {len(canaries)} written by the replay after {after}"
    if after != "growth":
        return
    # T3: the replay on one stream, an eager launch of another batch on a third, no ordering between them
    for k in ("U", "X", "status", "iters", "active"):
        out[k].zero_()
    s1, s3 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s3.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        g.replay()
    with torch.cuda.stream(s3):
        got_other = sv.plan_step_batch(*other, **kw)
    torch.cuda.synchronize()
    _assert_same(out, ref, "replay beside an eager launch")
    _assert_same(got_other, ref_other, "eager launch beside a replay")


def test_captured_warm_step_survives_record_growth():
    """T2 for the warm-start record: a warm step captured with a record of B1 = 600 problems keeps its record after
    set_warm_start grew it to B2 -- the handle keeps every buffer it registered, the record as the workspace and the
    schedule.  The replay reads and writes the record it was captured with and nothing else (canaries of that record's size
    stay untouched, the grown record stays zero), and equals, bit for bit, the same two steps run eagerly on a second handle
    whose record never grew."""
    N, n_obs, B1, B2 = 8, 10, 600, 1500
    P = lipmpc.LipMpcParams(N=N, n_obs_max=n_obs, v_max=5, flags=lipmpc.FLAG_WARM_START)
    sv, never_grew = lipmpc.BatchedLipMpc(P), lipmpc.BatchedLipMpc(P)
    assert sv.set_warm_start(B1) and never_grew.set_warm_start(B1)
    args = _batch(N, n_obs, B1, seed=97)
    st2 = args[0].clone()
    st2[:, 0] += 0.03
    st2[:, 2] -= 0.02                                   # the states of the second step
    kw = dict(with_c_eta=True, with_diag=True, with_working=True)
    never_grew.plan_step_batch(*args, **kw)
    ref = never_grew.plan_step_batch(st2, *args[1:], **kw)
    out = sv.alloc_outputs(B1, **kw)
    sv.plan_step_batch(*args, out=out)                  # the first step, outside the capture: its result is in the record
    torch.cuda.synchronize()
    assert int(np.isin(ref["status"].cpu().numpy(), (0, 4)).sum()) > B1 // 3
    assert int((sv.warm_record[:, 0] == 1.0).sum()) > B1 // 3          # the second step starts warm
    old_bytes = 8 * B1 * sv.warm_words
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            sv.plan_step_batch(*args, out=out)
    torch.cuda.current_stream().wait_stream(side)
    assert sv.set_warm_start(B2)
    torch.cuda.synchronize()
    canaries = _canaries(old_bytes)
    args[0].copy_(st2)
    for k in ("U", "X", "status", "iters", "active"):
        out[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    _assert_same(out, ref, "warm replay after the record grew")
    for i, c in enumerate(canaries):
        assert bool((c == CANARY).all()), f"canary {i} of {len(canaries)} written by the warm replay after the record grew"
    assert tuple(sv.warm_record.shape) == (B2, sv.warm_words) and not bool(sv.warm_record.any())


def test_first_split_launch_inside_a_capture_is_refused():
    """T4: the first split launch of a handle makes its side streams and events, which a capture must not see: it raises a
    RuntimeError before anything is enqueued, and the handle works normally afterwards -- eagerly and captured."""
    N, n_obs, B = 12, 9, 600
    args = _batch(N, n_obs, B, seed=95)
    P = lipmpc.LipMpcParams(N=N, n_obs_max=n_obs, v_max=5)
    first = lipmpc.BatchedLipMpc(P)
    ref = first.plan_step_batch(*args)
    sv = lipmpc.BatchedLipMpc(P)
    out = sv.alloc_outputs(B)
    for v in out.values():
        v.fill_(-1)
    marker = torch.zeros((1,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="capture"):
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                marker.add_(1.0)                            # (the graph is not empty)
                sv.plan_step_batch(*args, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g.replay()                                               # holds the marker's kernel alone
    torch.cuda.synchronize()
    assert float(marker[0]) == 1.0
    for k, v in out.items():
        assert bool((v == -1).all()), k                      # nothing of the step was enqueued or captured
    got = sv.plan_step_batch(*args)                          # afterwards: the handle works ...
    torch.cuda.synchronize()
    _assert_same(got, ref, "eager after the refused capture")
    g2 = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g2, stream=side):
            sv.plan_step_batch(*args, out=out)               # ... and its launches can be captured
    torch.cuda.current_stream().wait_stream(side)
    g2.replay()
    torch.cuda.synchronize()
    _assert_same(out, ref, "replay after the refused capture")


def _lidar_scene():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_golden.npz"))
    env, env_nv = d["env"][0], d["env_nv"][0]
    return [env[j][: env_nv[j]] for j in range(env.shape[0]) if env_nv[j] > 0]


def _lidar_batch(B, seed):
    rng = np.random.default_rng(seed)
    st = np.zeros((B, 5))
    st[:, 0], st[:, 2] = rng.uniform(-0.8, 5.8, B), rng.uniform(-0.8, 5.8, B)
    st[:, 4] = rng.uniform(-1, 1, B)
    noise = 0.01 * rng.standard_normal((B, 360, 2))
    goal = np.tile([[5.0, 5.0]], (B, 1))
    foot = np.where(rng.random(B) < 0.5, 1, -1).astype(np.int8)
    return _dev(st, torch.float64), _dev(noise, torch.float64), _dev(goal, torch.float64), _dev(foot, torch.int8)


def test_answers_do_not_depend_on_the_handle_history():
    """T5: LidarSensor.sense_plan_step and plan_step_batch_c_eta on a 32-lane handle give the same bits on a fresh handle,
    after the handle served a larger plan_step_batch, after it served one on another stream, and in a graph replay."""
    N, n_obs, v_max, B = 12, 12, 32, 1024
    sensor = lipmpc.LidarSensor(_lidar_scene(), lidar_range=1.5)
    assert sensor.n_obs_max == n_obs and sensor.v_max == v_max
    P = lipmpc.LipMpcParams(N=N, n_obs_max=n_obs, v_max=v_max)
    st, noise, goal, foot = _lidar_batch(B, seed=21)
    big = _batch(N, n_obs, 2048, seed=22)
    xy = torch.zeros((2048, n_obs, v_max, 2), dtype=torch.float64, device="cuda")
    xy[:, :, :5] = big[3]
    big[3] = xy.contiguous()                                 # the crowded rings in this handle's v_max layout
    same = _batch(N, n_obs, B, seed=23)
    xy = torch.zeros((B, n_obs, v_max, 2), dtype=torch.float64, device="cuda")
    xy[:, :, :5] = same[3]
    same[3] = xy.contiguous()
    sen0 = sensor.sense(st, noise, c_eta=True, rings=False)
    assert float(sen0["n_inferred"].double().mean()) > 1.0

    def sense_step(sv, sen=None, out=None):
        s, o = sensor.sense_plan_step(sv, st, goal, foot, noise, sen=sen, out=out)
        return dict(o, **{"sen_" + k: v for k, v in s.items()})

    def c_eta_step(sv, sen=None, out=None):
        return sv.plan_step_batch_c_eta(st, goal, foot, sen0["c_eta"], None, out=out, overflow=sen0["overflow"])

    sen_keys = ("sen_c_eta", "sen_n_inferred", "sen_overflow")
    for name, step in (("sense_plan_step", sense_step), ("plan_step_batch_c_eta", c_eta_step)):
        keys = STEP_KEYS + (sen_keys if step is sense_step else ())
        h0 = lipmpc.BatchedLipMpc(P)
        fresh = step(h0)
        torch.cuda.synchronize()
        assert int(np.isin(fresh["status"].cpu().numpy(), (0, 4)).sum()) > B // 3, name
        sv = lipmpc.BatchedLipMpc(P)                         # served a larger batch first
        sv.plan_step_batch(*big)
        got = step(sv)
        torch.cuda.synchronize()
        _assert_same(got, fresh, f"{name} after a larger plan_step_batch", keys)
        sv = lipmpc.BatchedLipMpc(P)                         # served one on another stream first
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            sv.plan_step_batch(*same)
        torch.cuda.current_stream().wait_stream(s)
        got = step(sv)
        torch.cuda.synchronize()
        _assert_same(got, fresh, f"{name} after a launch on another stream", keys)
        sen = sensor.alloc_outputs(B, rings=False, c_eta=True)           # in a graph replay
        out = sv.alloc_outputs(B)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                step(sv, sen=sen, out=out)
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        got = dict(out, **{"sen_" + k: v for k, v in sen.items()})
        _assert_same(got, fresh, f"{name} in a graph replay", keys)


def test_lidar_auto_schedule_on_two_streams():
    """T6: LidarSensor.sense(c_eta=True) beyond one round of waves ranks its robots in an order buffer per (batch size,
    stream): two scans of the same size on two unordered streams, one held back, both equal their eager scans."""
    B = 4096
    sensor = lipmpc.LidarSensor(_lidar_scene(), lidar_range=1.5)
    sa, na, _, _ = _lidar_batch(B, seed=31)
    sb, nb, _, _ = _lidar_batch(B, seed=32)
    ref_a = sensor.sense(sa, na, c_eta=True)
    ref_b = sensor.sense(sb, nb, c_eta=True)
    torch.cuda.synchronize()
    assert not torch.equal(ref_a["n_inferred"], ref_b["n_inferred"])
    eager_ms = _events_ms(lambda: sensor.sense(sa, na, c_eta=True))
    keys = ("c_eta", "n_inferred", "overflow", "obs_xy", "obs_nv")
    for tag, (s1, n1, r1), (s2, n2, r2) in (("A held back", (sa, na, ref_a), (sb, nb, ref_b)),
                                            ("B held back", (sb, nb, ref_b), (sa, na, ref_a))):
        g1, g2, slept = _gated(lambda: sensor.sense(s1, n1, c_eta=True), lambda: sensor.sense(s2, n2, c_eta=True), eager_ms)
        assert slept >= GATE_FACTOR * eager_ms, (tag, slept, eager_ms)
        for got, ref, which in ((g2, r2, "not held back"), (g1, r1, "held back")):
            for k in keys:
                assert torch.equal(got[k].view(torch.int64) if got[k].dtype == torch.float64 else got[k],
                                   ref[k].view(torch.int64) if ref[k].dtype == torch.float64 else ref[k]), (tag, which, k)
