"""Bit-for-bit tripwire at the shapes tests/test_bitwise_headline.py does not reach (-m gpu): every 16-lane horizon with
0, 2 and 5 obstacle slots (N = 1 .. 4 run the 8-variable factorisation), 32-lane horizons with 4 and 13 slots (register
and streamed rows, split launch), each with the default flags, FLAG_INTERIOR and FLAG_NO_PRESOLVE, and one rollout of
6 samples at N = 3 and at N = 8.

Same digest scheme as the headline tripwire: SHA-256 over the raw bytes of U, X, obj, status, iters, active, working,
theta, omega of one plan_step_batch (of the defined rows of X_pred and U_pred, then n_steps, last_status, total_iters
for a rollout).  B = 13 problems per case: on 16 lanes three full waves and one with a single live group.

Inputs: helpers.closed_loop_problems at the `asym` parameter set (no symmetry of the robot hides a swapped block), the
first 13 problems of walks of 5 steps.  The walk's states come out of the numpy oracle, whose last bits may depend on the
host's linear algebra library, so they are put on a grid of 2^-20 before use: the batch is then the same bytes on any host.

The expected digests were recorded on an MI355X from the build of commit f7b171e (the parent of the change that
introduced this file).  Every step case also goes through the oracle comparison of tests/test_params_gpu.py (_compare, at
its bars; the interior iterate at the 4e-4 of test_interior_flag_at_asym), so digests recorded from a wrong build cannot
pass silently; a rollout's first sample is held to the step's own answer (1e-7, the bar of the smoke run).

    python tests/test_bitwise_small_shapes.py      prints the digests of the current build (to record new ones)"""
import hashlib
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NAMES = ("U", "X", "obj", "status", "iters", "active", "working", "theta", "omega")
ROLLOUT_NAMES = ("X_pred", "U_pred", "n_steps", "last_status", "total_iters")
B = 13
PARAM_SET = "asym"
SHAPES = [(N, m) for N in range(1, 9) for m in (0, 2, 5)] + [(N, m) for N in (9, 12, 16) for m in (4, 13)]
FLAG_NAMES = ("default", "interior", "no_presolve")
ROLLOUTS = [(3, 5), (8, 5)]
K_ROLLOUT = 6
GRID = 2.0 ** 20

_problems = {}


def _flags(lipmpc, name):
    return {"default": 0, "interior": lipmpc.FLAG_INTERIOR, "no_presolve": lipmpc.FLAG_NO_PRESOLVE}[name]


def _batch(N, n_obs):
    """The first B problems of closed-loop walks at the asym constants, states on the 2^-20 grid; cached per shape."""
    if (N, n_obs) not in _problems:
        import lipmpc
        from helpers import closed_loop_problems, lip_params, oracle_params
        Po = oracle_params(lip_params(PARAM_SET, N=N, n_obs_max=n_obs, v_max=5))
        probs = list(itertools.islice(closed_loop_problems(N, n_obs, 10 ** 6, 5, seed=100 * N + n_obs, params=Po), B))
        xy, nv = lipmpc.pack_rings([p[3] for p in probs], n_obs, 5)
        _problems[(N, n_obs)] = dict(state=np.round(np.array([p[0] for p in probs]) * GRID) / GRID,
                                     goal=np.array([p[1] for p in probs], float), foot=np.array([p[2] for p in probs], np.int8),
                                     xy=xy, nv=nv, delta=np.zeros(B))
    return _problems[(N, n_obs)]


def _args(torch, bt, n_obs):
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    return (dev(bt["state"], torch.float64), dev(bt["goal"], torch.float64), dev(bt["foot"], torch.int8),
            dev(bt["xy"], torch.float64) if n_obs else None, dev(bt["nv"], torch.int32) if n_obs else None,
            dev(bt["delta"], torch.float64))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _step(torch, lipmpc, N, n_obs, flag):
    from helpers import lip_params
    P = lip_params(PARAM_SET, N=N, n_obs_max=n_obs, v_max=5, flags=_flags(lipmpc, flag))
    bt = _batch(N, n_obs)
    out = lipmpc.BatchedLipMpc(P).plan_step_batch(*_args(torch, bt, n_obs), with_c_eta=n_obs > 0, with_diag=True, with_working=True)
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in out.items()}
    return P, bt, g, {k: _sha(g[k]) for k in NAMES}


def _rollout(torch, lipmpc, N, n_obs):
    from helpers import lip_params
    P = lip_params(PARAM_SET, N=N, n_obs_max=n_obs, v_max=5)
    bt = _batch(N, n_obs)
    sv = lipmpc.BatchedLipMpc(P)
    ro = sv.rollout(*_args(torch, bt, n_obs), k_max=K_ROLLOUT, mpc_step=1)
    step = sv.plan_step_batch(*_args(torch, bt, n_obs))
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in ro.items()}
    n = r["n_steps"]
    # rows beyond n_steps are undefined: only the defined ones are hashed
    r["X_pred"] = np.concatenate([r["X_pred"][b, : n[b] + 1].ravel() for b in range(B)])
    r["U_pred"] = np.concatenate([ro["U_pred"].cpu().numpy()[b, : n[b]].ravel() for b in range(B)])
    return ro, step, {k: _sha(r[k]) for k in ROLLOUT_NAMES}


def _case_id(N, n_obs, flag):
    return f"N{N}_obs{n_obs}_{flag}"


# recorded from commit f7b171e on an MI355X (python tests/test_bitwise_small_shapes.py)
EXPECTED = {
    "N1_obs0_default": {
        "U": "fbc6e4d0dd8c48312177217f3e838506d7c75da1cc2f3aa7d23990e8bb6098ae",
        "X": "bc91f720096a2a748539ddd52c5b9c3eea2485e9f83bf36f422615170ccb4598",
        "obj": "3cb2ec147836d8e8aafcf945d9bd1406def02a85607518f4988e787c18e08da5",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "54e06e03ea18293e1608e75a6d3e862b0d050297f9129012da7dcab09d93a75b",
        "active": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "working": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "theta": "12da640ca9b4d5e53209a08a9f818604518d16397ae22585c45c68dfb2830f53",
        "omega": "4e0a3052cb6f1e0e6555010c85485eb8f1a64291d677a4b257789b151b78a820",
    },
    "N1_obs0_interior": {
        "U": "b375c50c66a8969ae144eee8350f42454ead4abdda933ba351af3228021cf2a7",
        "X": "51574aaeda71bcc0f395e4d14765fb8050525975c061f4557d519700567ab3d2",
        "obj": "09bfdef6b94e12587173b95fafe7b15ac26233a530b51c5a3f44375bada78d4b",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "1d84dc1e6f8403cd3db3afe976b9bc296be77e7d7c5a0aebeadfdf317ed68be5",
        "active": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "working": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "theta": "12da640ca9b4d5e53209a08a9f818604518d16397ae22585c45c68dfb2830f53",
        "omega": "4e0a3052cb6f1e0e6555010c85485eb8f1a64291d677a4b257789b151b78a820",
    },
    "N1_obs0_no_presolve": {
        "U": "fbc6e4d0dd8c48312177217f3e838506d7c75da1cc2f3aa7d23990e8bb6098ae",
        "X": "bc91f720096a2a748539ddd52c5b9c3eea2485e9f83bf36f422615170ccb4598",
        "obj": "3cb2ec147836d8e8aafcf945d9bd1406def02a85607518f4988e787c18e08da5",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "54e06e03ea18293e1608e75a6d3e862b0d050297f9129012da7dcab09d93a75b",
        "active": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "working": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "theta": "12da640ca9b4d5e53209a08a9f818604518d16397ae22585c45c68dfb2830f53",
        "omega": "4e0a3052cb6f1e0e6555010c85485eb8f1a64291d677a4b257789b151b78a820",
    },
    "N1_obs2_default": {
        "U": "ac53bebf4a303df5e8cafe7291ef0985c1895c5f1dc26a02590663747fa60123",
        "X": "bc65257fecc823138545933c4ff9ee880039d4176c57251a167e38d9ac4d9aad",
        "obj": "473ebe6c45d5e5c1d9fa8bb06ec7ab3007711b9f39b5ddc26b870f440faed92d",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "712a45a85882795a1dda51f4fcd77d20718ff7d745066b313c696df8867457e7",
        "active": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "working": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "theta": "12da640ca9b4d5e53209a08a9f818604518d16397ae22585c45c68dfb2830f53",
        "omega": "4e0a3052cb6f1e0e6555010c85485eb8f1a64291d677a4b257789b151b78a820",
    },
    "N1_obs2_interior": {
        "U": "b422c2c66fdddda7b5081a2b41b9f9c0a8e95b56394958b25c773e32b795483e",
        "X": "311c835420d364d7410d2af18a8d02978da227469911f07a1361dfb6bd86e02b",
        "obj": "dd6077d2b6d01917b1c2536551886e1ae2b5b5ea89eb19ac4e5b578c888e4b5c",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "02b5fceeebe07ceb1af34db91e634be42be57dabdd5e2c1a2daedbdefb859d86",
        "active": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "working": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "theta": "12da640ca9b4d5e53209a08a9f818604518d16397ae22585c45c68dfb2830f53",
        "omega": "4e0a3052cb6f1e0e6555010c85485eb8f1a64291d677a4b257789b151b78a820",
    },
    "N1_obs2_no_presolve": {
        "U": "b686c5a260adad928174f4d740e60a302e67d079ba2bece1abb4837d50502488",
        "X": "f818925f215f055951163a9bae47201b7eb5c151ae6ca0b88c25ba6bf370e63a",
        "obj": "b753dde2d0a840762739532ab442c8d5eceb23a14b1fdad6482edd7db3dceaac",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "712a45a85882795a1dda51f4fcd77d20718ff7d745066b313c696df8867457e7",
        "active": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "working": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "theta": "12da640ca9b4d5e53209a08a9f818604518d16397ae22585c45c68dfb2830f53",
        "omega": "4e0a3052cb6f1e0e6555010c85485eb8f1a64291d677a4b257789b151b78a820",
    },
    "N1_obs5_default": {
        "U": "6ce9a24b674a72a4cdc6fd86483ae345bf24bfb95a31f8d8c6d458014bb9f023",
        "X": "5ed07106b89803d6405527a068e77c8341ce59bec491953e0c36bb1180a84a98",
        "obj": "473ebe6c45d5e5c1d9fa8bb06ec7ab3007711b9f39b5ddc26b870f440faed92d",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "54e06e03ea18293e1608e75a6d3e862b0d050297f9129012da7dcab09d93a75b",
        "active": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "working": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "theta": "12da640ca9b4d5e53209a08a9f818604518d16397ae22585c45c68dfb2830f53",
        "omega": "4e0a3052cb6f1e0e6555010c85485eb8f1a64291d677a4b257789b151b78a820",
    },
    "N1_obs5_interior": {
        "U": "9c3ef31fc8d7942a2f9b800480fb2790ad3dd8ad9cc72e6b8bbac607004b836d",
        "X": "3c41b8d6948a191dd25450ef48d60f7211b7f67494ddf60809f00dfa1a89062f",
        "obj": "870286984481dc450da52242a7228ed96dd9e5ddb41286c26ffaaeae873a43ab",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "1d84dc1e6f8403cd3db3afe976b9bc296be77e7d7c5a0aebeadfdf317ed68be5",
        "active": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "working": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "theta": "12da640ca9b4d5e53209a08a9f818604518d16397ae22585c45c68dfb2830f53",
        "omega": "4e0a3052cb6f1e0e6555010c85485eb8f1a64291d677a4b257789b151b78a820",
    },
    "N1_obs5_no_presolve": {
        "U": "6da74894a60e49b9e24440ca1e823bf9bb6a1b63eff30e3af962f1cc2a0c7e95",
        "X": "e145e6e9d0e5b6d2ea2aed4a7677206540d95de404b0fe8ee10baf79b725d3a9",
        "obj": "3ea5df828e9ade6055973bfcb1cc186cd97409776b5d4b1618fb3ce90e9fa8b5",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "54e06e03ea18293e1608e75a6d3e862b0d050297f9129012da7dcab09d93a75b",
        "active": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "working": "27eaaa719687008e8c83eadfe298ecabc6bf9b84153b808f24e068e8e1c2db74",
        "theta": "12da640ca9b4d5e53209a08a9f818604518d16397ae22585c45c68dfb2830f53",
        "omega": "4e0a3052cb6f1e0e6555010c85485eb8f1a64291d677a4b257789b151b78a820",
    },
    "N2_obs0_default": {
        "U": "e7ae940d8403ba4460700c12b81787c4c532008d9f05c42021902e4f9f1722ca",
        "X": "a76c98f2a413b386ccf9065ddd046f3769641874d14dc585b8b9ccae65f63dcc",
        "obj": "ae66f7e06363bca0b71c2041d307d47f384c4657989818d060a5e044a1e0af77",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "fc66d67ed5380a6a1c277519ff0b01201943dff2205c07ee1914fcc0eb69d91e",
        "active": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "working": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "theta": "cb396c41683e021d555ec004296f8cd831060d8913c5b3b554ac9e11d86b7141",
        "omega": "640b57a844948972e610bb41e4fda96cb00fccdbecaaee58ac59824393860dc9",
    },
    "N2_obs0_interior": {
        "U": "722e37c457ad0811c6bf2ea58fcccc326ad8514e9da2180ffc298829df65a128",
        "X": "21fe9021b59f65274a15ea2201e3b87ee0a9352fa0106d4c9d745da37754560e",
        "obj": "f3681044c113010879b4522d857e8d164691d2d43266606f0ebfdfbe2fb99e6f",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "32b4d3a6e3a4f38b98cbeffc54be923a6c046999b337fed3b304afcb14bfd96c",
        "active": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "working": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "theta": "cb396c41683e021d555ec004296f8cd831060d8913c5b3b554ac9e11d86b7141",
        "omega": "640b57a844948972e610bb41e4fda96cb00fccdbecaaee58ac59824393860dc9",
    },
    "N2_obs0_no_presolve": {
        "U": "e7ae940d8403ba4460700c12b81787c4c532008d9f05c42021902e4f9f1722ca",
        "X": "a76c98f2a413b386ccf9065ddd046f3769641874d14dc585b8b9ccae65f63dcc",
        "obj": "ae66f7e06363bca0b71c2041d307d47f384c4657989818d060a5e044a1e0af77",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "fc66d67ed5380a6a1c277519ff0b01201943dff2205c07ee1914fcc0eb69d91e",
        "active": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "working": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "theta": "cb396c41683e021d555ec004296f8cd831060d8913c5b3b554ac9e11d86b7141",
        "omega": "640b57a844948972e610bb41e4fda96cb00fccdbecaaee58ac59824393860dc9",
    },
    "N2_obs2_default": {
        "U": "8853746534251d9b87daebcf665875d6f2fd7491e6788d78d4c6ee10fe41e641",
        "X": "a377d7246110b933013eb88c2295539b4a7ab33b93060fa182a3dfb492600828",
        "obj": "182038dbc49307a98e8df336c7eaf3ac714897f4b5cae52372932c786c4cabbe",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "4b02cd0766879a47b06acefd88a38a6e5786a15505a4b74e825c0d851475178d",
        "active": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "working": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "theta": "cb396c41683e021d555ec004296f8cd831060d8913c5b3b554ac9e11d86b7141",
        "omega": "640b57a844948972e610bb41e4fda96cb00fccdbecaaee58ac59824393860dc9",
    },
    "N2_obs2_interior": {
        "U": "fe90374e4431b60af18dc6bfd9c1c17c869b4fb6734876cd8fae5cf5982014b4",
        "X": "605956f31f29ea6ec958e5835af17133acd0b4dc07ddaa1024b5d297248cb8c6",
        "obj": "c122fd6ee24d4445f2b44eefd2f4d177ee59ba8566573a2d685c20577b9e79b8",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "eb169ea24132434965bd562c9a3f0701ae4ddd84bd60bbbca558e793b628bf62",
        "active": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "working": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "theta": "cb396c41683e021d555ec004296f8cd831060d8913c5b3b554ac9e11d86b7141",
        "omega": "640b57a844948972e610bb41e4fda96cb00fccdbecaaee58ac59824393860dc9",
    },
    "N2_obs2_no_presolve": {
        "U": "7d1720d8501b7bcab1afdfbf87c63f30f8512a3a817da1de098ff2b6e488ae57",
        "X": "571fe2db960d38e8c96bd4496e8685302b42b3c2439eef83f8ca1c5ac1a6e9e3",
        "obj": "182038dbc49307a98e8df336c7eaf3ac714897f4b5cae52372932c786c4cabbe",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "4b02cd0766879a47b06acefd88a38a6e5786a15505a4b74e825c0d851475178d",
        "active": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "working": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "theta": "cb396c41683e021d555ec004296f8cd831060d8913c5b3b554ac9e11d86b7141",
        "omega": "640b57a844948972e610bb41e4fda96cb00fccdbecaaee58ac59824393860dc9",
    },
    "N2_obs5_default": {
        "U": "11acaac5170034cf13fed29f41cb5bb0ff1bf1e09bce85fc190988b7caae4d87",
        "X": "a5ad47ed7e0db1c43ff1b84c0be40b58f66fd73af4e65684e3e2165e297ab2f4",
        "obj": "51d24844501d79c32d0b701294e33fe8b556711af81014665b9b1ec668ca6853",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "faca72532d120294fdd60658254f0e67c253279949e029d1e8e0a27a2721c889",
        "active": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "working": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "theta": "cb396c41683e021d555ec004296f8cd831060d8913c5b3b554ac9e11d86b7141",
        "omega": "640b57a844948972e610bb41e4fda96cb00fccdbecaaee58ac59824393860dc9",
    },
    "N2_obs5_interior": {
        "U": "950a22d4956b0c11e0a5fdd6e6fd177390eece9476bde6b003939d171da4e37c",
        "X": "9b6280ce9e40830ff4e6a5c86ef46ecdf4884f3804c5e2af557753a4bf457bdd",
        "obj": "9fcbceb4272ffcd46f3b4a21e36be26ee1cc0ea9ef8cd0d5ca4add1ffe827ae9",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "9351ef717d7841ef9963ae252360b82ff2d009de2d12b784345a2261f6e9b42c",
        "active": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "working": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "theta": "cb396c41683e021d555ec004296f8cd831060d8913c5b3b554ac9e11d86b7141",
        "omega": "640b57a844948972e610bb41e4fda96cb00fccdbecaaee58ac59824393860dc9",
    },
    "N2_obs5_no_presolve": {
        "U": "ca75f6ef1470ba94ce50617fa00e6fb2abb0dbf9a79e391c37a99d968b54ae1e",
        "X": "fbd4d6d111f82231ee6f332ebdbbfd8431a862b1b3b542eca269fc077438f46a",
        "obj": "98dbf25dbd9a9028a8dd940e983255076b581f4ea4690d99b59c59808649a65e",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "4b02cd0766879a47b06acefd88a38a6e5786a15505a4b74e825c0d851475178d",
        "active": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "working": "fb4bf0f850acf1bac34420df0183dc18cddcf60817ab4ab4e14d7d5f26d9afee",
        "theta": "cb396c41683e021d555ec004296f8cd831060d8913c5b3b554ac9e11d86b7141",
        "omega": "640b57a844948972e610bb41e4fda96cb00fccdbecaaee58ac59824393860dc9",
    },
    "N3_obs0_default": {
        "U": "e794f272bcf732f1add3357397445da9d5a5048b04475211c76b7055c88b2f81",
        "X": "eb66b546b403f46d7b89fd08fb4989a5824bc2f6f9db5d11dcbb3b43d5631bb4",
        "obj": "eb48cd2122e9a611bfd13ee9564be98a55b74f2f152cf6b0df0ab855433ccc99",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "1f383916120071d7e22ec3b13d8824edca4075b83e5977e051c7f1725cfc96b2",
        "active": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "working": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "theta": "43a37f84f8cabdd63fd4ed835e91828f7a05bc9c53500e10c2e69f8401452894",
        "omega": "0ee462fb048bd7c4338e6ca9902e29a7c82d0dd648968dda579a4935288913d8",
    },
    "N3_obs0_interior": {
        "U": "8cb449828020b7e63394af439241dda3e78417f5df12f4209e41517f5dab8704",
        "X": "92661655d7cb09078b27be22cf14c5e6339c64549ce43164ca20c0572c69cb94",
        "obj": "c6a8247a29e2b6c68b20606357320b5c1f433ca942bfb5c9ea50a148d0bb95e3",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "e29f9a1920108858b4d0634e8369c2f2787c05d446d2fa372eaa8e39a4356694",
        "active": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "working": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "theta": "43a37f84f8cabdd63fd4ed835e91828f7a05bc9c53500e10c2e69f8401452894",
        "omega": "0ee462fb048bd7c4338e6ca9902e29a7c82d0dd648968dda579a4935288913d8",
    },
    "N3_obs0_no_presolve": {
        "U": "e794f272bcf732f1add3357397445da9d5a5048b04475211c76b7055c88b2f81",
        "X": "eb66b546b403f46d7b89fd08fb4989a5824bc2f6f9db5d11dcbb3b43d5631bb4",
        "obj": "eb48cd2122e9a611bfd13ee9564be98a55b74f2f152cf6b0df0ab855433ccc99",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "1f383916120071d7e22ec3b13d8824edca4075b83e5977e051c7f1725cfc96b2",
        "active": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "working": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "theta": "43a37f84f8cabdd63fd4ed835e91828f7a05bc9c53500e10c2e69f8401452894",
        "omega": "0ee462fb048bd7c4338e6ca9902e29a7c82d0dd648968dda579a4935288913d8",
    },
    "N3_obs2_default": {
        "U": "4ca22fe36b2479b5542d4ee0c234c4f9458e347fc1a7228ad4e86c0ecc09c2bb",
        "X": "cc5cbad3c3f2ef36c59926b196c607208dade0ee10a6354ac1d80b4c4013dd9b",
        "obj": "1dcdcf01b01e8a91bb9c15823ef17d6653a1ce149cfd5dfba1ddf400cb8f72b0",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "8488d6a1c0ef68f893804342c0aedebb8f6810a1f472b2321922a510a5277163",
        "active": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "working": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "theta": "43a37f84f8cabdd63fd4ed835e91828f7a05bc9c53500e10c2e69f8401452894",
        "omega": "0ee462fb048bd7c4338e6ca9902e29a7c82d0dd648968dda579a4935288913d8",
    },
    "N3_obs2_interior": {
        "U": "814d887cdce1adb16f80484db6ea337691adaa15623369aab787779e72b3464b",
        "X": "284a4a8018175e831d17b418d9519c14d533d43e079b06d3ffdc667bf7b9edf0",
        "obj": "7a18a260a6ee52c5674fb5f24d783c6828e97cccfc64050403e53170a0587f10",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "ced517f2dbb9a8330875c30e27532e49ae12e50ae300f1ecf69862a9605ab161",
        "active": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "working": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "theta": "43a37f84f8cabdd63fd4ed835e91828f7a05bc9c53500e10c2e69f8401452894",
        "omega": "0ee462fb048bd7c4338e6ca9902e29a7c82d0dd648968dda579a4935288913d8",
    },
    "N3_obs2_no_presolve": {
        "U": "3c8b7b15625010527101483485b0ed4accbbf52657bb9e430d282a7b1516a3e1",
        "X": "e919bf95785f77b81c8ac45a6688d139bd233639da22a21183e71f2f3ab44c3d",
        "obj": "ca744a72731852f9debd439aa2c85d2aea6c321a9cf64e7b0a16902f9d7a66a9",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "8488d6a1c0ef68f893804342c0aedebb8f6810a1f472b2321922a510a5277163",
        "active": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "working": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "theta": "43a37f84f8cabdd63fd4ed835e91828f7a05bc9c53500e10c2e69f8401452894",
        "omega": "0ee462fb048bd7c4338e6ca9902e29a7c82d0dd648968dda579a4935288913d8",
    },
    "N3_obs5_default": {
        "U": "9ac0436a15dbab28670c0c561f4f070e9f575540b72ddd7f5ef48382713d128a",
        "X": "eca82a9a5566d662df10b13614b920526170299150c69af0c0d3b9413d4454d6",
        "obj": "ad73e60c906cef9b3274707c376769eee7bdfb068bc6c01a97ca45872bb605ae",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "b2dda7e08772d957e104c9468326d6e8826f43950fa7459378f769a877ba67ff",
        "active": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "working": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "theta": "43a37f84f8cabdd63fd4ed835e91828f7a05bc9c53500e10c2e69f8401452894",
        "omega": "0ee462fb048bd7c4338e6ca9902e29a7c82d0dd648968dda579a4935288913d8",
    },
    "N3_obs5_interior": {
        "U": "b848c23161129ce2ab20b48898d54acfe18b69e057d1ec7d4eeb36eb1f84035b",
        "X": "c14a94535b4b37ac196f439bec40a1e2380f9d440e46859c08dbef8315974e68",
        "obj": "ccc6b6e33092e6aa1b6134bad6110f24a6c155f9e4768195e1dda5613cdc30aa",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "d47de358a1745e47f9e9e007246fcfdf8c9224acd3e30c399ba86b4b2bdfaf7f",
        "active": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "working": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "theta": "43a37f84f8cabdd63fd4ed835e91828f7a05bc9c53500e10c2e69f8401452894",
        "omega": "0ee462fb048bd7c4338e6ca9902e29a7c82d0dd648968dda579a4935288913d8",
    },
    "N3_obs5_no_presolve": {
        "U": "9540c86f49dd1afeaa372624f7e21bd55562bad16733d87bb2669e4d278f4f0b",
        "X": "8128e4cdb304eec82996c2818ce485058dba854d56fc22c23f72d39baf541017",
        "obj": "98877d0e336cf99271511529984950893caa46106ce792f1c78daab7f254db79",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "6374924f165df284b7174f20f1fa95f57a002f523963e410c4150b0a5f19d2c6",
        "active": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "working": "ae841f90cc6f0ed806161501b9228143796b30fcc1e4ea6f3da45b2de7a69668",
        "theta": "43a37f84f8cabdd63fd4ed835e91828f7a05bc9c53500e10c2e69f8401452894",
        "omega": "0ee462fb048bd7c4338e6ca9902e29a7c82d0dd648968dda579a4935288913d8",
    },
    "N4_obs0_default": {
        "U": "3eb2f6bbe51bbbc748923d02ee9211752a725cb4c752a5b00b7f706eb1c19d99",
        "X": "143558eb372b89f98880a3bdf383ccb2dd7600dd4eb0afbcb104ad9617cbeeac",
        "obj": "70d78ee2eb384d34d535a00746f51b422603f9ec469d74287285c73a8cf1b57f",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "b42d619337cab8720fdc68e2885cc7546c932f90f6ea303c0c3a8f4a562d65b2",
        "active": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "working": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "theta": "31dfa502a039578b38c3411effd2d58e0e5a225ed22c7ec94db3cabd93c01e6d",
        "omega": "b82ce9f5797242d1f99ad01288ca18ab091a1d5c23ec9fe29a7c1c15b5ac1ba6",
    },
    "N4_obs0_interior": {
        "U": "a6f181f0034b3d959104ae3a2145fcbd7ff7200e0680d552302a9190f334f8cf",
        "X": "2fecf555451582e6d4852b703df2aea5e21938994a9c3fb992bb37a739f5d17b",
        "obj": "060d9372dd56a6d06cb38dfa4a386ca25336db556d260c78cd62076df6886f61",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "e21ccd7cd9197020007f48947fbaa11fc337c8a49735456638f65138d648e61b",
        "active": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "working": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "theta": "31dfa502a039578b38c3411effd2d58e0e5a225ed22c7ec94db3cabd93c01e6d",
        "omega": "b82ce9f5797242d1f99ad01288ca18ab091a1d5c23ec9fe29a7c1c15b5ac1ba6",
    },
    "N4_obs0_no_presolve": {
        "U": "3eb2f6bbe51bbbc748923d02ee9211752a725cb4c752a5b00b7f706eb1c19d99",
        "X": "143558eb372b89f98880a3bdf383ccb2dd7600dd4eb0afbcb104ad9617cbeeac",
        "obj": "70d78ee2eb384d34d535a00746f51b422603f9ec469d74287285c73a8cf1b57f",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "b42d619337cab8720fdc68e2885cc7546c932f90f6ea303c0c3a8f4a562d65b2",
        "active": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "working": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "theta": "31dfa502a039578b38c3411effd2d58e0e5a225ed22c7ec94db3cabd93c01e6d",
        "omega": "b82ce9f5797242d1f99ad01288ca18ab091a1d5c23ec9fe29a7c1c15b5ac1ba6",
    },
    "N4_obs2_default": {
        "U": "80ddae77ba1f2865de6ac2b7d3faadfc010499a3fa745ff20d1eedd75f959eef",
        "X": "1b6b96fefab5b9912c27b0032af1d67e22641ff071800b8b78153f8d70f96c09",
        "obj": "4575c7302f9c5053d8abad25255b8b763b8e573e00e5affe78b0e9dc0f641900",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "b939016de48a1da2cac50080f79eb9e16a79273c1acea48c8d3baea3d4a9f9f2",
        "active": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "working": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "theta": "31dfa502a039578b38c3411effd2d58e0e5a225ed22c7ec94db3cabd93c01e6d",
        "omega": "b82ce9f5797242d1f99ad01288ca18ab091a1d5c23ec9fe29a7c1c15b5ac1ba6",
    },
    "N4_obs2_interior": {
        "U": "f1ca86808372f9fbe1d2c7c93f6b4fc8fd6a0ee1a8a5a9bf2733960b1ee071e8",
        "X": "6314f2f4418d9139a6542a7bc8c508872364438c8e04c73492a2ac258ced4762",
        "obj": "0677a6d6f5ad0255df722831247006187418c71314dfc0b6859b23a1056f9d23",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "75b9095da90b7e4c2bf7f6ec807b0050d283408f02a907f9ce9fbaea513cd2cf",
        "active": "ef39d815d65d37f1fcff3b4e3841a591f61545eaf570f37e0618395f0d769518",
        "working": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "theta": "31dfa502a039578b38c3411effd2d58e0e5a225ed22c7ec94db3cabd93c01e6d",
        "omega": "b82ce9f5797242d1f99ad01288ca18ab091a1d5c23ec9fe29a7c1c15b5ac1ba6",
    },
    "N4_obs2_no_presolve": {
        "U": "754bbd7ece87efefbfa28bde5efeaa6e5a35fb490ad7daad8dab98dcbda0b4f4",
        "X": "ad2aad47ee3ba24ee11a69ff4aaa38daea1353bbe97dcdaf5326e57edfe8dd8d",
        "obj": "4575c7302f9c5053d8abad25255b8b763b8e573e00e5affe78b0e9dc0f641900",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "b939016de48a1da2cac50080f79eb9e16a79273c1acea48c8d3baea3d4a9f9f2",
        "active": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "working": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "theta": "31dfa502a039578b38c3411effd2d58e0e5a225ed22c7ec94db3cabd93c01e6d",
        "omega": "b82ce9f5797242d1f99ad01288ca18ab091a1d5c23ec9fe29a7c1c15b5ac1ba6",
    },
    "N4_obs5_default": {
        "U": "f89566124580674c3c8dd7b670f6bb86277829655222bc4c87733bc8530ae1ec",
        "X": "4c14f6af7ae862c27a068b24b35b96059760670c93b326aedb4b04f242d49939",
        "obj": "70d78ee2eb384d34d535a00746f51b422603f9ec469d74287285c73a8cf1b57f",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "10b78cf34e6a22ce4e8597de657ff3dbf1964f544164595f6915e358ee2f0a49",
        "active": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "working": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "theta": "31dfa502a039578b38c3411effd2d58e0e5a225ed22c7ec94db3cabd93c01e6d",
        "omega": "b82ce9f5797242d1f99ad01288ca18ab091a1d5c23ec9fe29a7c1c15b5ac1ba6",
    },
    "N4_obs5_interior": {
        "U": "f8b27d105eeaba3e813a707235bfa22083713f5cb09b37f5f7d568644901aac0",
        "X": "5022139f6318da831f4c2bb1c2f7a68f326085c172612bb1360c8741d45b994d",
        "obj": "fdbfa3046bceb74c82897846ceb26f6ba19fbd30a3def78f3d07314150373362",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "a5063085adfbc2dd164302aed5fd946d41ce447dee9cb5f8cf62c959983de4b9",
        "active": "ef39d815d65d37f1fcff3b4e3841a591f61545eaf570f37e0618395f0d769518",
        "working": "ef39d815d65d37f1fcff3b4e3841a591f61545eaf570f37e0618395f0d769518",
        "theta": "31dfa502a039578b38c3411effd2d58e0e5a225ed22c7ec94db3cabd93c01e6d",
        "omega": "b82ce9f5797242d1f99ad01288ca18ab091a1d5c23ec9fe29a7c1c15b5ac1ba6",
    },
    "N4_obs5_no_presolve": {
        "U": "0fa4f44e8d590d806a505030cda560cec1064ed80c1e4d87b4db024c60e2bdc5",
        "X": "cc31c03482d06231e5f2e9b91dfd00437c110b725872a92da6424fe3a9bc951b",
        "obj": "70d78ee2eb384d34d535a00746f51b422603f9ec469d74287285c73a8cf1b57f",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "10b78cf34e6a22ce4e8597de657ff3dbf1964f544164595f6915e358ee2f0a49",
        "active": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "working": "bfb387505c6f57c664254155ff9abc980ef9b35e01a4ef47708df010c9d578ef",
        "theta": "31dfa502a039578b38c3411effd2d58e0e5a225ed22c7ec94db3cabd93c01e6d",
        "omega": "b82ce9f5797242d1f99ad01288ca18ab091a1d5c23ec9fe29a7c1c15b5ac1ba6",
    },
    "N5_obs0_default": {
        "U": "54ee767e2f45a1da9a12563c6b94261d908c24dc4dc94cb74465a45e045247db",
        "X": "3ed1f2e916d95484d520d16384b638db388c9e2e00c1f30b155679b7b3d64beb",
        "obj": "da4efe71904690621ea39da609f2a66989f04bd6f97a15530f24f871115823c8",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "62eea90634973890fdb8bb481e94d5dc350490a2481512bb3dc1eaf3f8305de8",
        "active": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "working": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "theta": "6956f091d89985b05aa555a88ef7b7b53f4bf448df97ba3526877b446aa92555",
        "omega": "2f040f225bbb6027392ae8d7d2eb615cd74416e67fb2584232a24e3b5a4a7f9d",
    },
    "N5_obs0_interior": {
        "U": "95d138518acd2b28a93c1ef584aa2f127497c9fe88beb8f6c45bbe39ba2abc64",
        "X": "cbed10c9c3e686bdd63f29f926d27bcfdc6f0c0ab0f895daec6e6f2a8aa43f5d",
        "obj": "39d7caf8383f832b5a0a514b26cc8f4c876a28946857800f72451d4bf89abbe1",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "ed58ab9183818d4ed97d7e1c680755c78d1d8ccc7a3a4123af0520410bf9b1d8",
        "active": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "working": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "theta": "6956f091d89985b05aa555a88ef7b7b53f4bf448df97ba3526877b446aa92555",
        "omega": "2f040f225bbb6027392ae8d7d2eb615cd74416e67fb2584232a24e3b5a4a7f9d",
    },
    "N5_obs0_no_presolve": {
        "U": "54ee767e2f45a1da9a12563c6b94261d908c24dc4dc94cb74465a45e045247db",
        "X": "3ed1f2e916d95484d520d16384b638db388c9e2e00c1f30b155679b7b3d64beb",
        "obj": "da4efe71904690621ea39da609f2a66989f04bd6f97a15530f24f871115823c8",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "62eea90634973890fdb8bb481e94d5dc350490a2481512bb3dc1eaf3f8305de8",
        "active": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "working": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "theta": "6956f091d89985b05aa555a88ef7b7b53f4bf448df97ba3526877b446aa92555",
        "omega": "2f040f225bbb6027392ae8d7d2eb615cd74416e67fb2584232a24e3b5a4a7f9d",
    },
    "N5_obs2_default": {
        "U": "ec9ac1d086f8fd8affaf4f4015af0279248fae6541fd7a2b8bf2521972efb6d0",
        "X": "c8adb5f3ac73887fefac6fb862e15b606af1a52f7c0adce44c084192d3695bbb",
        "obj": "cfb779e7444cc1ebae8afed8cde3fb074c3fd7321619c316e554503abc47ac5b",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "00294e4ddebad2fb97f1a586ea749d419c45feb73ce5f835fe23b927e0311ad5",
        "active": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "working": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "theta": "6956f091d89985b05aa555a88ef7b7b53f4bf448df97ba3526877b446aa92555",
        "omega": "2f040f225bbb6027392ae8d7d2eb615cd74416e67fb2584232a24e3b5a4a7f9d",
    },
    "N5_obs2_interior": {
        "U": "391c69fd6340585f3e1f16051f5e9a27c16384d74d08f3512cae2ad753897217",
        "X": "30511a6646e97c525f779988bcf25881b723339fad6c1b6add393601c79e15fd",
        "obj": "4878198e821c5c6f667ccdcbf6e92aa07aa99b8a2d30de74f91eeecf7a391ecd",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "55b47deae01575f1279e1d484c0aff4d988668ebaf3aa54aa9c05645f71a28d0",
        "active": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "working": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "theta": "6956f091d89985b05aa555a88ef7b7b53f4bf448df97ba3526877b446aa92555",
        "omega": "2f040f225bbb6027392ae8d7d2eb615cd74416e67fb2584232a24e3b5a4a7f9d",
    },
    "N5_obs2_no_presolve": {
        "U": "cfabed7445732d20015704fc5a6e1bc532eb4f0071a24f97557fa8fc3368b0bc",
        "X": "de3e4981ef0678c2699c25b4db14e7a6e44716e732eea502a6a8cec37f7bcca3",
        "obj": "2d154da6f1636b8f73b097470e1e780959e65b6e95572392cf5c8c4cc1a9fca6",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "af859521c73b9ed34664878734f25aa26066d83407d1c5e8ba46a12b492edaa8",
        "active": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "working": "9962c4fc5e7f71dc60d6799ca813fa6fa87a779cd29a6a12a993d25b88586d50",
        "theta": "6956f091d89985b05aa555a88ef7b7b53f4bf448df97ba3526877b446aa92555",
        "omega": "2f040f225bbb6027392ae8d7d2eb615cd74416e67fb2584232a24e3b5a4a7f9d",
    },
    "N5_obs5_default": {
        "U": "630aac5e256f90df40feda76fee64c1f9f368c97572b99c8fca8072885b14004",
        "X": "c6f3d9859c74cb35257d216a5f88ed727f8a20e54d152d9f170bbfe385608080",
        "obj": "2d154da6f1636b8f73b097470e1e780959e65b6e95572392cf5c8c4cc1a9fca6",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "d990ee95a055b2b5b37e2d6dfead4a82ae329aebfd59349d23c86b715409d7cc",
        "active": "2ba54ebff62139cc2ece41f575aab3a1526957cee741324fed41d091726a5931",
        "working": "2ba54ebff62139cc2ece41f575aab3a1526957cee741324fed41d091726a5931",
        "theta": "6956f091d89985b05aa555a88ef7b7b53f4bf448df97ba3526877b446aa92555",
        "omega": "2f040f225bbb6027392ae8d7d2eb615cd74416e67fb2584232a24e3b5a4a7f9d",
    },
    "N5_obs5_interior": {
        "U": "cd8f18105a1728811d572cdf9162d0745ccfb4514b3d44e1d7713037f80d0075",
        "X": "754d22da91f072b5fa36924c6e6ba6f5916674cb15ee893a11d5b8691e935d0a",
        "obj": "67dafc0d60bf703c0e176d3f04f2a2c0d8fda206fe049aa9fb5005076dd5659d",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "d5d17a9a750ea159a789ba36411d46955dc471a30aa02b9943e375a8ee4d6cb7",
        "active": "2ba54ebff62139cc2ece41f575aab3a1526957cee741324fed41d091726a5931",
        "working": "2ba54ebff62139cc2ece41f575aab3a1526957cee741324fed41d091726a5931",
        "theta": "6956f091d89985b05aa555a88ef7b7b53f4bf448df97ba3526877b446aa92555",
        "omega": "2f040f225bbb6027392ae8d7d2eb615cd74416e67fb2584232a24e3b5a4a7f9d",
    },
    "N5_obs5_no_presolve": {
        "U": "19203e4bcc37d55dab7c9fb239b0e2e047dfbb84f702b07a10ada880330b1beb",
        "X": "0e9296fe03f8c20e73b0f5a6d7f95c7ea2961d9f183ded87612a2df921facd19",
        "obj": "2d154da6f1636b8f73b097470e1e780959e65b6e95572392cf5c8c4cc1a9fca6",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "10b78cf34e6a22ce4e8597de657ff3dbf1964f544164595f6915e358ee2f0a49",
        "active": "2ba54ebff62139cc2ece41f575aab3a1526957cee741324fed41d091726a5931",
        "working": "2ba54ebff62139cc2ece41f575aab3a1526957cee741324fed41d091726a5931",
        "theta": "6956f091d89985b05aa555a88ef7b7b53f4bf448df97ba3526877b446aa92555",
        "omega": "2f040f225bbb6027392ae8d7d2eb615cd74416e67fb2584232a24e3b5a4a7f9d",
    },
    "N6_obs0_default": {
        "U": "e1ce7979817eaa022532b99d1bdd60047de865ddb15d56d529d49dbf81b1be89",
        "X": "67e11f204f6b4876b67f5cec691ad15a17fcb33b058c11dac7768c75a457ae2b",
        "obj": "4d8f7c21a8378fb9426e4b416b34dab4b750d9f67abc05cde5b386b7cb58fe46",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "b939016de48a1da2cac50080f79eb9e16a79273c1acea48c8d3baea3d4a9f9f2",
        "active": "9c8c23af4020e80055c46af1fa340ab26a0908e3946f6c90de0dcb0ec9bf2836",
        "working": "9c8c23af4020e80055c46af1fa340ab26a0908e3946f6c90de0dcb0ec9bf2836",
        "theta": "43631f571ea13252188d49fb2c5ca0a2cc79f55e3e80638595c99df27113e980",
        "omega": "7ff4eb6b2a86596ca4d7f006cbd4a30a321400d55374bd28a75b1b5cb539c4e0",
    },
    "N6_obs0_interior": {
        "U": "25a069ccfbe73c5c530c5840cf6833a4a3d762e6c75ce40dd5f8bd14d7a3d4a6",
        "X": "8bc56b0aac5719bf5d50ef1518265221fc24752f9b0c05b8ab9f9bfb27c8f056",
        "obj": "357cf0e09d93e496cfc5e4ae8a83d253a7d98da399f3fd9fb6f561629a906cb3",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "891f6593a1de40cf9fd6fbce63f0f1e3c8fe171c4109d75814270b58065420d1",
        "active": "9c8c23af4020e80055c46af1fa340ab26a0908e3946f6c90de0dcb0ec9bf2836",
        "working": "9c8c23af4020e80055c46af1fa340ab26a0908e3946f6c90de0dcb0ec9bf2836",
        "theta": "43631f571ea13252188d49fb2c5ca0a2cc79f55e3e80638595c99df27113e980",
        "omega": "7ff4eb6b2a86596ca4d7f006cbd4a30a321400d55374bd28a75b1b5cb539c4e0",
    },
    "N6_obs0_no_presolve": {
        "U": "e1ce7979817eaa022532b99d1bdd60047de865ddb15d56d529d49dbf81b1be89",
        "X": "67e11f204f6b4876b67f5cec691ad15a17fcb33b058c11dac7768c75a457ae2b",
        "obj": "4d8f7c21a8378fb9426e4b416b34dab4b750d9f67abc05cde5b386b7cb58fe46",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "b939016de48a1da2cac50080f79eb9e16a79273c1acea48c8d3baea3d4a9f9f2",
        "active": "9c8c23af4020e80055c46af1fa340ab26a0908e3946f6c90de0dcb0ec9bf2836",
        "working": "9c8c23af4020e80055c46af1fa340ab26a0908e3946f6c90de0dcb0ec9bf2836",
        "theta": "43631f571ea13252188d49fb2c5ca0a2cc79f55e3e80638595c99df27113e980",
        "omega": "7ff4eb6b2a86596ca4d7f006cbd4a30a321400d55374bd28a75b1b5cb539c4e0",
    },
    "N6_obs2_default": {
        "U": "1d6759af42f7e8481d1d91b442d942e52ea7f1c25da22b0f1bb2a8add5247f0e",
        "X": "0c5e025b6007f81bf44e9219814ae9a00e0edf0ea476119275d28d3f1a8159dc",
        "obj": "4d8f7c21a8378fb9426e4b416b34dab4b750d9f67abc05cde5b386b7cb58fe46",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "229cb89e700e61f63b9ffdbd32406c9ba4796652021cf626f4ad724ea9a643b8",
        "active": "55806004eebb36bc533cdc625af0e73e1da622aaaf69399cb291d7ef1ccf0af0",
        "working": "55806004eebb36bc533cdc625af0e73e1da622aaaf69399cb291d7ef1ccf0af0",
        "theta": "43631f571ea13252188d49fb2c5ca0a2cc79f55e3e80638595c99df27113e980",
        "omega": "7ff4eb6b2a86596ca4d7f006cbd4a30a321400d55374bd28a75b1b5cb539c4e0",
    },
    "N6_obs2_interior": {
        "U": "aea1970768c284a0d62a499277f311045bdb4846ce8efdb6d1b9f66101688b90",
        "X": "e43cbbe46747d0385af363459afecc4780275fd7a7f2091709c10789cdbe0196",
        "obj": "26e74a78d99b1c19cdc82be8da42e57aace3d16eca6a35ebe78d04f67f1f4291",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "bd0e36fd2ba82077406e8fa80616ca94425fcede11a27bc02e12480109f1c236",
        "active": "55806004eebb36bc533cdc625af0e73e1da622aaaf69399cb291d7ef1ccf0af0",
        "working": "55806004eebb36bc533cdc625af0e73e1da622aaaf69399cb291d7ef1ccf0af0",
        "theta": "43631f571ea13252188d49fb2c5ca0a2cc79f55e3e80638595c99df27113e980",
        "omega": "7ff4eb6b2a86596ca4d7f006cbd4a30a321400d55374bd28a75b1b5cb539c4e0",
    },
    "N6_obs2_no_presolve": {
        "U": "4e05866a80ea00ff430437028d59818d4e33362195ad506e50eef0271ae7089e",
        "X": "62edad7767ea902e904deda423feec9a2b11d360dcd0042259f057748a91d11b",
        "obj": "4d8f7c21a8378fb9426e4b416b34dab4b750d9f67abc05cde5b386b7cb58fe46",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "229cb89e700e61f63b9ffdbd32406c9ba4796652021cf626f4ad724ea9a643b8",
        "active": "55806004eebb36bc533cdc625af0e73e1da622aaaf69399cb291d7ef1ccf0af0",
        "working": "55806004eebb36bc533cdc625af0e73e1da622aaaf69399cb291d7ef1ccf0af0",
        "theta": "43631f571ea13252188d49fb2c5ca0a2cc79f55e3e80638595c99df27113e980",
        "omega": "7ff4eb6b2a86596ca4d7f006cbd4a30a321400d55374bd28a75b1b5cb539c4e0",
    },
    "N6_obs5_default": {
        "U": "9ddf09511bd0f9f94588127c9a4fa61586f1b64016bad21037875e6a61b4890f",
        "X": "4c38bc98317ab2957f43f42d884861197d17669bb28f564664a8dd510ccdba80",
        "obj": "6cda08450c523cac3893611c28564483ec8be59658ff73d99c3e33a6709d8c13",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "559a0a074b24d0c73a182a451dc002ea30538941d2ceac501294040b9291ced6",
        "active": "259b52806a158362e65c8b4d842fb01b50f3f9be8eae9e9e451c496319c5175e",
        "working": "259b52806a158362e65c8b4d842fb01b50f3f9be8eae9e9e451c496319c5175e",
        "theta": "43631f571ea13252188d49fb2c5ca0a2cc79f55e3e80638595c99df27113e980",
        "omega": "7ff4eb6b2a86596ca4d7f006cbd4a30a321400d55374bd28a75b1b5cb539c4e0",
    },
    "N6_obs5_interior": {
        "U": "6e029a2208d87cdf01cfa096a8eb2050667a1584af808332ee0f98802b4c31bf",
        "X": "8229aea8dd4ce5b33ee58f2759f5b7eb1b24a16f4a5ac0ee3ba49f63399d5fad",
        "obj": "156a890affe5152c4eb90f6867a18da32bc55a23c1676b65562c0ab70889c8ad",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "79647a09b52108a090f4b9908b38b29a9e2b577b40ea93f79ce9786a6c8dd627",
        "active": "259b52806a158362e65c8b4d842fb01b50f3f9be8eae9e9e451c496319c5175e",
        "working": "259b52806a158362e65c8b4d842fb01b50f3f9be8eae9e9e451c496319c5175e",
        "theta": "43631f571ea13252188d49fb2c5ca0a2cc79f55e3e80638595c99df27113e980",
        "omega": "7ff4eb6b2a86596ca4d7f006cbd4a30a321400d55374bd28a75b1b5cb539c4e0",
    },
    "N6_obs5_no_presolve": {
        "U": "34ad55035f90b6dbd1d27e89c16b7870e438346b354562e4551409be553619f4",
        "X": "c631705ad9ff8e071ea4687e4c3b3dc746398142d176cdc67684108385355f62",
        "obj": "6cda08450c523cac3893611c28564483ec8be59658ff73d99c3e33a6709d8c13",
        "status": "7955cb2de90dd9efc6df9fdbf5f5d10c114f4135a9a6b52db1003be749e32f7a",
        "iters": "c3f04b9d0f09d5c7d1316e35cac4fff02f30007642642e2e6b70389f7dbe9ca1",
        "active": "259b52806a158362e65c8b4d842fb01b50f3f9be8eae9e9e451c496319c5175e",
        "working": "259b52806a158362e65c8b4d842fb01b50f3f9be8eae9e9e451c496319c5175e",
        "theta": "43631f571ea13252188d49fb2c5ca0a2cc79f55e3e80638595c99df27113e980",
        "omega": "7ff4eb6b2a86596ca4d7f006cbd4a30a321400d55374bd28a75b1b5cb539c4e0",
    },
    "N7_obs0_default": {
        "U": "d0ab162c2d16db2810475bbb2f4d30d0bbb5391402c0e96f5a514b58dfdf8575",
        "X": "228761d8e8ea7af46305dfa5d62e47adb06e3c37b4f4865efc35056072f84958",
        "obj": "a9e0bda9a478370d3e2317d27da81a6e22c1e81ea581716b57fa4a97ba7d377f",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "ef3341cde3bb49f63b814ed800b32d3081ba98812995f6c20cf554bf8aaf5111",
        "active": "3c6841d8ea417a2668fd2add0e7e3b69725450c27c9783962c1cd395fa2635fd",
        "working": "3c6841d8ea417a2668fd2add0e7e3b69725450c27c9783962c1cd395fa2635fd",
        "theta": "c0cf7d2eb18eec89726ed6d9e307261b17bdd305bc1fd7a4de80d90017ab71ff",
        "omega": "c94632c8ee7b696778c7da5982571ad1f1c3545988eec7b7080e2b2257c2eb1e",
    },
    "N7_obs0_interior": {
        "U": "a4b9753e948bf6967f2ae92600d886033d8d0517172a8b66c0c78b5db45048c2",
        "X": "7c43ba2f0f2d0bc114c1b1c669ecd8298f21b1e17ca3ed67383d917f80e459f2",
        "obj": "8c155e4a371c2469e9b4e337046b63d4f466bae5e254ebfa5d1674d9d47649c6",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "027c05936f53dc60ba3e66d9b9f101fce551d0fd3683e4383edeb9fc0305c3a7",
        "active": "3c6841d8ea417a2668fd2add0e7e3b69725450c27c9783962c1cd395fa2635fd",
        "working": "3c6841d8ea417a2668fd2add0e7e3b69725450c27c9783962c1cd395fa2635fd",
        "theta": "c0cf7d2eb18eec89726ed6d9e307261b17bdd305bc1fd7a4de80d90017ab71ff",
        "omega": "c94632c8ee7b696778c7da5982571ad1f1c3545988eec7b7080e2b2257c2eb1e",
    },
    "N7_obs0_no_presolve": {
        "U": "d0ab162c2d16db2810475bbb2f4d30d0bbb5391402c0e96f5a514b58dfdf8575",
        "X": "228761d8e8ea7af46305dfa5d62e47adb06e3c37b4f4865efc35056072f84958",
        "obj": "a9e0bda9a478370d3e2317d27da81a6e22c1e81ea581716b57fa4a97ba7d377f",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "ef3341cde3bb49f63b814ed800b32d3081ba98812995f6c20cf554bf8aaf5111",
        "active": "3c6841d8ea417a2668fd2add0e7e3b69725450c27c9783962c1cd395fa2635fd",
        "working": "3c6841d8ea417a2668fd2add0e7e3b69725450c27c9783962c1cd395fa2635fd",
        "theta": "c0cf7d2eb18eec89726ed6d9e307261b17bdd305bc1fd7a4de80d90017ab71ff",
        "omega": "c94632c8ee7b696778c7da5982571ad1f1c3545988eec7b7080e2b2257c2eb1e",
    },
    "N7_obs2_default": {
        "U": "760d897c05412ec743983eb8f45a3c1c49f638f9c90bdb945a90751a86e29e4a",
        "X": "11f04f3582fe12d4abf7d9530204b5916c1fae8451667732c1af6cfc50fbd372",
        "obj": "a9e0bda9a478370d3e2317d27da81a6e22c1e81ea581716b57fa4a97ba7d377f",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "c79344c8ee1d3b26e19d1088b0a8303997f37c4a1ef4a05d5b026a0984096979",
        "active": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "working": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "theta": "c0cf7d2eb18eec89726ed6d9e307261b17bdd305bc1fd7a4de80d90017ab71ff",
        "omega": "c94632c8ee7b696778c7da5982571ad1f1c3545988eec7b7080e2b2257c2eb1e",
    },
    "N7_obs2_interior": {
        "U": "c1829b81fe38b274721d9c26580f9655812c8591be411e823ce261cef3c89aba",
        "X": "01db68a7b6a8141bcaf5a3414399100f69eb5e27506782aeb325f8c90c3d4a1a",
        "obj": "e94299507953ef5b187e99ccccf115f7334d64cfcab104c8c2261e20a8c314a9",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "6a32e8b941ffff803f7f5862a2a1049327ad08586956085cb8a84d9ed8c0927b",
        "active": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "working": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "theta": "c0cf7d2eb18eec89726ed6d9e307261b17bdd305bc1fd7a4de80d90017ab71ff",
        "omega": "c94632c8ee7b696778c7da5982571ad1f1c3545988eec7b7080e2b2257c2eb1e",
    },
    "N7_obs2_no_presolve": {
        "U": "d70757a53efd5128f90a62e68230b237459bbe73a87c80c39bf7262715a162d5",
        "X": "4eeb3de8a3b2b6c3257275e756a28ff588fddbfd14dd57b8bc4e57276cc13e51",
        "obj": "a9e0bda9a478370d3e2317d27da81a6e22c1e81ea581716b57fa4a97ba7d377f",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "c79344c8ee1d3b26e19d1088b0a8303997f37c4a1ef4a05d5b026a0984096979",
        "active": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "working": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "theta": "c0cf7d2eb18eec89726ed6d9e307261b17bdd305bc1fd7a4de80d90017ab71ff",
        "omega": "c94632c8ee7b696778c7da5982571ad1f1c3545988eec7b7080e2b2257c2eb1e",
    },
    "N7_obs5_default": {
        "U": "33c65ec22f016555b42b2bfe89962730b82597975a9c0402a88591ae4752ad06",
        "X": "60583c270bb93cfacb4c9a887c1763760a9aea5663ddfc509ecbce5fb68510d6",
        "obj": "a9e0bda9a478370d3e2317d27da81a6e22c1e81ea581716b57fa4a97ba7d377f",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "7c4f409b54b78b3f14d95ba1175de84c0983d356b870b14b5078ad182d35c9a4",
        "active": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "working": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "theta": "c0cf7d2eb18eec89726ed6d9e307261b17bdd305bc1fd7a4de80d90017ab71ff",
        "omega": "c94632c8ee7b696778c7da5982571ad1f1c3545988eec7b7080e2b2257c2eb1e",
    },
    "N7_obs5_interior": {
        "U": "8125716076a1285fa76f0c7e3e83c6dfcd8eec90b1925a0bad585f3647035a30",
        "X": "b34dc9e485a7b2c67db9ce06cbd933608aeffbc81b82b44c3accd249faf85e0b",
        "obj": "9b7b3f73c210d08bdc5667e1c945b9d4ffe02619d5b86888950c8d329842fa3f",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "1d93875b5b3da6f9c513d4a8de171a0b917c7073cb3b8763f537b63e9dbfa208",
        "active": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "working": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "theta": "c0cf7d2eb18eec89726ed6d9e307261b17bdd305bc1fd7a4de80d90017ab71ff",
        "omega": "c94632c8ee7b696778c7da5982571ad1f1c3545988eec7b7080e2b2257c2eb1e",
    },
    "N7_obs5_no_presolve": {
        "U": "8539419b828ef12c4fb007f96b6e09d3e057a9b05963d1cd8240aafd68bfbd63",
        "X": "839237dcde2f17315631059c6d5f8bcb469365f647617bbe00994b0fd1cd2114",
        "obj": "a9e0bda9a478370d3e2317d27da81a6e22c1e81ea581716b57fa4a97ba7d377f",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "1b07bdcaf50215a8a6d9bf3b17c43174f1e7398a53fa91afa1bf0133362c6bfa",
        "active": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "working": "5c693b46f3bcb921d29a177247ea95e5530cecc987d5cb67859c2d63d7c5d78d",
        "theta": "c0cf7d2eb18eec89726ed6d9e307261b17bdd305bc1fd7a4de80d90017ab71ff",
        "omega": "c94632c8ee7b696778c7da5982571ad1f1c3545988eec7b7080e2b2257c2eb1e",
    },
    "N8_obs0_default": {
        "U": "3f9b2604b4c038211efd1ab8b2308a48ad6beb1e0150bcb55fb09ce222b0f8a4",
        "X": "6ab7e96a45b0378e4897acf284461d59bc11f2c7da4a39d18da5975ab149ff83",
        "obj": "32fdb338c60b2873f4754022a3b9b413df92c636f053feb44e2d348bcc319a59",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "224320b88d4db7eef40af1c6dce395f7fad520c0fe736d4471d5027a03eb9105",
        "active": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "working": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "theta": "a6d2575b3e8012b33456a6ce23de403b9dae3525bfd64ba68b6805059c487860",
        "omega": "d1da1d04429af62b8a61f40f3bc1da613b2937aef81d29dc2e42b1a8e4bf3d78",
    },
    "N8_obs0_interior": {
        "U": "7cbad2bec8ebbeee571a71d38b7b116f9a53cd1267ffd9393cf9046a8350ec67",
        "X": "1cf4e7f390aa4161ec338791357083d9fcf060ebf4282e4b28e82d099d5148d6",
        "obj": "195e8f15eedb7de72683824723fcb09a643a45d108eef1106cdd5a7e96b8108d",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "272acad528cf31c50466f384d77ee0463ed56586a96d50b98c279a5760ec33cf",
        "active": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "working": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "theta": "a6d2575b3e8012b33456a6ce23de403b9dae3525bfd64ba68b6805059c487860",
        "omega": "d1da1d04429af62b8a61f40f3bc1da613b2937aef81d29dc2e42b1a8e4bf3d78",
    },
    "N8_obs0_no_presolve": {
        "U": "3f9b2604b4c038211efd1ab8b2308a48ad6beb1e0150bcb55fb09ce222b0f8a4",
        "X": "6ab7e96a45b0378e4897acf284461d59bc11f2c7da4a39d18da5975ab149ff83",
        "obj": "32fdb338c60b2873f4754022a3b9b413df92c636f053feb44e2d348bcc319a59",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "224320b88d4db7eef40af1c6dce395f7fad520c0fe736d4471d5027a03eb9105",
        "active": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "working": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "theta": "a6d2575b3e8012b33456a6ce23de403b9dae3525bfd64ba68b6805059c487860",
        "omega": "d1da1d04429af62b8a61f40f3bc1da613b2937aef81d29dc2e42b1a8e4bf3d78",
    },
    "N8_obs2_default": {
        "U": "c8585643b7da2875456caf61cd2e77dabd9ccec08f27eb7a2b02deecc3bf0728",
        "X": "1898ed59a398acb8e3a49ac8d53e3ac73420ba9937f442feaf9e9c076c34d004",
        "obj": "eb4d1c4b11fa9d961aa12b224c451e91465a93a432eb0f0822d724414df07f73",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "74f442bdbb2b1fe402f65e4ccd2076c00f2c7e07db11f5e31263f0fdbe20cac0",
        "active": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "working": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "theta": "a6d2575b3e8012b33456a6ce23de403b9dae3525bfd64ba68b6805059c487860",
        "omega": "d1da1d04429af62b8a61f40f3bc1da613b2937aef81d29dc2e42b1a8e4bf3d78",
    },
    "N8_obs2_interior": {
        "U": "bc5ca50a04380ce880613f956b410fcc020d553260b4cb51ea7efbcdd9271619",
        "X": "d4624d14b4c7a87d7b7a7b6d33024eb79e3bb22fc7d94b5f33b86af9706f5293",
        "obj": "6a93943727164abcb486f9ed109b6b766fa19a87d81e6075d6bf04d2b2928c99",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "b939016de48a1da2cac50080f79eb9e16a79273c1acea48c8d3baea3d4a9f9f2",
        "active": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "working": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "theta": "a6d2575b3e8012b33456a6ce23de403b9dae3525bfd64ba68b6805059c487860",
        "omega": "d1da1d04429af62b8a61f40f3bc1da613b2937aef81d29dc2e42b1a8e4bf3d78",
    },
    "N8_obs2_no_presolve": {
        "U": "f138313e123bfe311d59ffaf882eaacbe185096b0b2fb9c42bd91124cec17d58",
        "X": "1373bef00aef84968b3e62acd6a9504e652591fa3958a67e3328c9caeba81ca6",
        "obj": "d8c12b1a20454288cb2c809347b411537cb75042ca460eb6c9024abeed8f77a2",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "74f442bdbb2b1fe402f65e4ccd2076c00f2c7e07db11f5e31263f0fdbe20cac0",
        "active": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "working": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "theta": "a6d2575b3e8012b33456a6ce23de403b9dae3525bfd64ba68b6805059c487860",
        "omega": "d1da1d04429af62b8a61f40f3bc1da613b2937aef81d29dc2e42b1a8e4bf3d78",
    },
    "N8_obs5_default": {
        "U": "f104f3616b25d815aa8a2b39e8e3587ef05c14e3a3d857e45b298386551e9a23",
        "X": "d4a1c2fea43ebd825643210a4c53ea5b233e2bcb921c5fc2ac1a0458fe69b541",
        "obj": "9811673b2b60bd805a06cdfcb2b3def96971410f208083eefd4b9aec7acd4f89",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "53e7bad4fad5ab07ba4a175812605cdee7ac2906bf4af7b6220d0aeb8d83ef86",
        "active": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "working": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "theta": "a6d2575b3e8012b33456a6ce23de403b9dae3525bfd64ba68b6805059c487860",
        "omega": "d1da1d04429af62b8a61f40f3bc1da613b2937aef81d29dc2e42b1a8e4bf3d78",
    },
    "N8_obs5_interior": {
        "U": "315daf1084cb50c90d387fb901cbf16eeb482f51aa68a21a9bd142034771c8c3",
        "X": "78366b1a498ba11d655d6fd4c4802d4bfe3280c3e28227d3a90ea6c91e69bb75",
        "obj": "aa32c417bc0040efa90179bce7f2c143aa1bf19ef424bb6d12f5f3803f5a8bb8",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "fdb2ca317c594890e9d81f3dd1bd1d356302c3aafbfcf13c1e43ff0826e03d8a",
        "active": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "working": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "theta": "a6d2575b3e8012b33456a6ce23de403b9dae3525bfd64ba68b6805059c487860",
        "omega": "d1da1d04429af62b8a61f40f3bc1da613b2937aef81d29dc2e42b1a8e4bf3d78",
    },
    "N8_obs5_no_presolve": {
        "U": "01045d93056909c295e6966a2d5842b1f54104ad045860df714c98c9652356f9",
        "X": "5de298052d668bc7479702af5da314435fd787adfad792c8e0297f906ae49264",
        "obj": "9158775e7b937df87008358a692b3a3b8a915eb18da7c21a229e9a30eaecfb42",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "6f183d146c6c6a437c613d424731547ca0000c5cd28bf66cec09aede36d15a86",
        "active": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "working": "2f1532f0feb7b6dc17e6655bcbc75723fe2b06db705a55e3702d90e5d206c585",
        "theta": "a6d2575b3e8012b33456a6ce23de403b9dae3525bfd64ba68b6805059c487860",
        "omega": "d1da1d04429af62b8a61f40f3bc1da613b2937aef81d29dc2e42b1a8e4bf3d78",
    },
    "N9_obs4_default": {
        "U": "d56cc9ed2db559d03f269ca8948ae843ca5a42adc6ab2672504472b24bb5d507",
        "X": "3b12f3b941bdd7daf0ec3553bad7afb856fea0620fcd2f972d9d82af1e961354",
        "obj": "29c158e46eab4c0ed454ee7bb673af7fbbb0df2d56d2cc650c286b46233fcc5a",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "5ecc964a43cbe1306730c88932db690e05463878288e46bd26248f9e709394bb",
        "active": "87d61d906ca7b2253d3efe4a74bf712b2283cf77a070d485f3f13a21a09e55b8",
        "working": "87d61d906ca7b2253d3efe4a74bf712b2283cf77a070d485f3f13a21a09e55b8",
        "theta": "67dd2cc568e2d0f671afd02df388d5cf6d9644453bcf6ada35d4ea33004c23e1",
        "omega": "808ee46fb06cb27eb194db6e1450f91c5de73e915e0caeae7cd7a0437607c5f8",
    },
    "N9_obs4_interior": {
        "U": "a726329932bfa4341a011f42601bff0c486f7713b0630b9b220d68765db6eebc",
        "X": "bdabb00ef121c0ee3de56508df6ed85b584599282598c8d0888bfd89f2b59e04",
        "obj": "531b4fa9e98474c1143c201e8cd828da309cc43e858be225041c7a6a8e636d90",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "ba62dbc86d6bf7e78cd2b6dab6f1184ad68fec552fd4467317dcfca4fd47f0ed",
        "active": "87d61d906ca7b2253d3efe4a74bf712b2283cf77a070d485f3f13a21a09e55b8",
        "working": "87d61d906ca7b2253d3efe4a74bf712b2283cf77a070d485f3f13a21a09e55b8",
        "theta": "67dd2cc568e2d0f671afd02df388d5cf6d9644453bcf6ada35d4ea33004c23e1",
        "omega": "808ee46fb06cb27eb194db6e1450f91c5de73e915e0caeae7cd7a0437607c5f8",
    },
    "N9_obs4_no_presolve": {
        "U": "bf3eddf8d3f80b4dc58a0d3efa41e09632de4d23070d7d33939fd1886b52fda2",
        "X": "36cd5202081dad288108a154fbba4d10a4b3987fc540f8a94923969eca82cfd5",
        "obj": "fe4c23f044e520f4dd24566fa70bf1abccacc0837ffa4e8d8955fb37da40715a",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "b70b6b2213fec7a43123c680b7f386bab645ca68ecdb9cd4fca0b7f5b852b1d3",
        "active": "87d61d906ca7b2253d3efe4a74bf712b2283cf77a070d485f3f13a21a09e55b8",
        "working": "87d61d906ca7b2253d3efe4a74bf712b2283cf77a070d485f3f13a21a09e55b8",
        "theta": "67dd2cc568e2d0f671afd02df388d5cf6d9644453bcf6ada35d4ea33004c23e1",
        "omega": "808ee46fb06cb27eb194db6e1450f91c5de73e915e0caeae7cd7a0437607c5f8",
    },
    "N9_obs13_default": {
        "U": "e6190369161d54cf112e8228cdea47dfe405c46888ea6cb08fa1688abea8e1d5",
        "X": "246e28a5716c20af416247b70a63d7feec8ffa466cb855a3993bc536fef34ad4",
        "obj": "1cc72618fa34902935d15b7802bbf9aadb9dfd75c0e72b5a21596a9fd8ccd605",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "b28eca6c53029b03134cac3f7d38177e5ec052ece9945c63d5c6356130e8de33",
        "active": "3f6645eefb9cfb4a8dd02658012b03140330d8cf1d2548d25a1ae12ac683da91",
        "working": "3f6645eefb9cfb4a8dd02658012b03140330d8cf1d2548d25a1ae12ac683da91",
        "theta": "67dd2cc568e2d0f671afd02df388d5cf6d9644453bcf6ada35d4ea33004c23e1",
        "omega": "808ee46fb06cb27eb194db6e1450f91c5de73e915e0caeae7cd7a0437607c5f8",
    },
    "N9_obs13_interior": {
        "U": "6edda6d401e5f58473038a61af99b1eaac8b6cb6440b938fa4353fe9b72a648c",
        "X": "1b2a67ddcb1c2818f1aacf212f2c6cc69b92e197049d561960017a126ed5c81d",
        "obj": "844687205d592c7805c25d611fe695c669c4c4795621d4c33d5464732c993651",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "166c6a673abdbe6f692f09f9fd14791f54e4f5f95575c350f8b996f5b8a94ed2",
        "active": "3f6645eefb9cfb4a8dd02658012b03140330d8cf1d2548d25a1ae12ac683da91",
        "working": "3f6645eefb9cfb4a8dd02658012b03140330d8cf1d2548d25a1ae12ac683da91",
        "theta": "67dd2cc568e2d0f671afd02df388d5cf6d9644453bcf6ada35d4ea33004c23e1",
        "omega": "808ee46fb06cb27eb194db6e1450f91c5de73e915e0caeae7cd7a0437607c5f8",
    },
    "N9_obs13_no_presolve": {
        "U": "a3c0bb826b49ae6a64ef0286122598ee41ceeef1d927428548d86a229a5d69eb",
        "X": "4a6106b4216a0a8c61b2c848dd9fbb92589766ccfb69b6f6b534f8f0b3eb840f",
        "obj": "4e9844b9efb16ffe8fd12c5aefde2afa7f84138f87491613ac1e21e6aed78514",
        "status": "ebf736e51bd940e8eb5b124e6dcf27c932294e60646453cc544492dd3bdb895e",
        "iters": "e70f7574ce6256eed208d7a34b97edca5fce6e015ddbf59dc400128fcb535374",
        "active": "3f6645eefb9cfb4a8dd02658012b03140330d8cf1d2548d25a1ae12ac683da91",
        "working": "3f6645eefb9cfb4a8dd02658012b03140330d8cf1d2548d25a1ae12ac683da91",
        "theta": "67dd2cc568e2d0f671afd02df388d5cf6d9644453bcf6ada35d4ea33004c23e1",
        "omega": "808ee46fb06cb27eb194db6e1450f91c5de73e915e0caeae7cd7a0437607c5f8",
    },
    "N12_obs4_default": {
        "U": "e034f97d81244b2ac25819dd842c928ed7297dc5c20b9623409618226f5eb569",
        "X": "af6df75476a233385a4b860701a8accee9d53ac282d7762e74bc041143d811b6",
        "obj": "b7d5b3d4ca14bfd81348a81daa709331b51af8afd1779acae18f553802eed351",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "ed03fa173d72b1e9057bf2afb36de6c516138b6ca71a9d5aa2b386ee6cc9fd11",
        "active": "6cd37bae9d369f541a05e08a842256fe44ed3c2e823b0606dfa9933d67589af3",
        "working": "6cd37bae9d369f541a05e08a842256fe44ed3c2e823b0606dfa9933d67589af3",
        "theta": "bcff7ff85df48384b23db43bb9e25358f1964d8c894a292c5d6f76e3727affb4",
        "omega": "120ced018d5ca4b20664127cf464a45099e0434f6c2cef1a70b2a3f6a9dca4a8",
    },
    "N12_obs4_interior": {
        "U": "ac3fdfcf0ca350ace9bf6ed56a7c7dbfb1e99a1aab3f9727d38c760d694828a3",
        "X": "29263c5b73743ce796f9130f0b04845c5d620c90ec68551cadf88e3d4bc0e840",
        "obj": "7b992eccd456c9c8f03af482dd4edd8680b2381ddf1dfea89d9a74aece8dcf08",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "56f40136cd1005a768fd38e3bc3eebb5f2ee92870320ceb3d219a7a71d2fbbf3",
        "active": "6cd37bae9d369f541a05e08a842256fe44ed3c2e823b0606dfa9933d67589af3",
        "working": "6cd37bae9d369f541a05e08a842256fe44ed3c2e823b0606dfa9933d67589af3",
        "theta": "bcff7ff85df48384b23db43bb9e25358f1964d8c894a292c5d6f76e3727affb4",
        "omega": "120ced018d5ca4b20664127cf464a45099e0434f6c2cef1a70b2a3f6a9dca4a8",
    },
    "N12_obs4_no_presolve": {
        "U": "e2d91770e7511125ffac64aabd2335d15d26957e2b36c34ede70b231b82c3275",
        "X": "e3210c2d3ed20bef02d7d0b341c17c26db6b5be0a25bf947bd8fff16c67dc9bf",
        "obj": "b7d5b3d4ca14bfd81348a81daa709331b51af8afd1779acae18f553802eed351",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "c4faa470c265eda0d02c9f09a0a2bb9ca077dc6a673cdd94a0e2d4cdb8ade395",
        "active": "6cd37bae9d369f541a05e08a842256fe44ed3c2e823b0606dfa9933d67589af3",
        "working": "6cd37bae9d369f541a05e08a842256fe44ed3c2e823b0606dfa9933d67589af3",
        "theta": "bcff7ff85df48384b23db43bb9e25358f1964d8c894a292c5d6f76e3727affb4",
        "omega": "120ced018d5ca4b20664127cf464a45099e0434f6c2cef1a70b2a3f6a9dca4a8",
    },
    "N12_obs13_default": {
        "U": "374e64a40fce02329702c0f0407db6550fef7398fe4c95a63d6a9c3eb1f9745c",
        "X": "f18cbeb751cad654d4baf93691488ad49a59d0e44e293c2ce3107c0cbd005c8a",
        "obj": "b7d5b3d4ca14bfd81348a81daa709331b51af8afd1779acae18f553802eed351",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "4787e25e04f56b4915bcebb2b13ccb16ad9b777115d46852d3e3e36c96ddd8b6",
        "active": "35ae44499f333624046e03d047aa75916d5a66fe75ce1269fbb192471bdac54d",
        "working": "35ae44499f333624046e03d047aa75916d5a66fe75ce1269fbb192471bdac54d",
        "theta": "bcff7ff85df48384b23db43bb9e25358f1964d8c894a292c5d6f76e3727affb4",
        "omega": "120ced018d5ca4b20664127cf464a45099e0434f6c2cef1a70b2a3f6a9dca4a8",
    },
    "N12_obs13_interior": {
        "U": "da292a34fe3f49f3dbfacb56f237087052a8c4ec25a1732f6e0ba0714329225f",
        "X": "5f2b7dfc8e8369e36b4657a143b0cc393e8bad7f39a503716a33db8949bbed3f",
        "obj": "79863191d7339e56a4ba5d6e663e368b91b7da87a2fa98a1044ad06b2ae01a23",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "27f1ee97fd03ec4a16d7937136d29c89b0c0f5d919fb6f7337281f5ed884eb72",
        "active": "35ae44499f333624046e03d047aa75916d5a66fe75ce1269fbb192471bdac54d",
        "working": "35ae44499f333624046e03d047aa75916d5a66fe75ce1269fbb192471bdac54d",
        "theta": "bcff7ff85df48384b23db43bb9e25358f1964d8c894a292c5d6f76e3727affb4",
        "omega": "120ced018d5ca4b20664127cf464a45099e0434f6c2cef1a70b2a3f6a9dca4a8",
    },
    "N12_obs13_no_presolve": {
        "U": "5226aa07db8808d3a6c3848b7c149cac5d8989bdec611c20fb1417851f9b1dba",
        "X": "0d8f11f9bff61210ce2ee1970ffdc2fa88f94e719111a4964b47b185e84c2d4b",
        "obj": "b7d5b3d4ca14bfd81348a81daa709331b51af8afd1779acae18f553802eed351",
        "status": "8e7edf76961e26a7cadb5aa2a5fe8edc5aafb79919b455343930c66d9db43fa6",
        "iters": "400a08952946f126c684439fb9208646830da87a0cf608400a735568ef3a9055",
        "active": "35ae44499f333624046e03d047aa75916d5a66fe75ce1269fbb192471bdac54d",
        "working": "35ae44499f333624046e03d047aa75916d5a66fe75ce1269fbb192471bdac54d",
        "theta": "bcff7ff85df48384b23db43bb9e25358f1964d8c894a292c5d6f76e3727affb4",
        "omega": "120ced018d5ca4b20664127cf464a45099e0434f6c2cef1a70b2a3f6a9dca4a8",
    },
    "N16_obs4_default": {
        "U": "039f52845384faa4155f325d075b14353758b351b406a3147f04dcf91082d407",
        "X": "4905096d27c7aec25ffd23d7b63cb1311f132fc935106a325276f495b155b584",
        "obj": "48d2837bc1459500e2513ba213723944f0eab6e5ce7bacc0f78012d3ff9f4bee",
        "status": "d76764951f52ca8d874af418c0976c30f5bc07f3f1555110541c43b0a3346fb6",
        "iters": "bb49e4dafc1826b1a962a073f87eaa74bec8bb3af1fd71fd11682c7d4403aefa",
        "active": "fa49cd74563b4831c09b7b4a84b05d9b9ff2695704a7aa0dd05ebed5d5d2ad33",
        "working": "fa49cd74563b4831c09b7b4a84b05d9b9ff2695704a7aa0dd05ebed5d5d2ad33",
        "theta": "1f793ccda57a76dab6d641d964a156d6e654931a9f01554681da17319ca28a10",
        "omega": "ec04da046827a1795de1b056f9491c0b7783c41189756e9e628edd433c0066ce",
    },
    "N16_obs4_interior": {
        "U": "cd9ed0df20f5a9645eb08369eb79239be8ac9a198f652b031f933379b6fe7bc3",
        "X": "77647a16c128d4fea8a6f21f7b58d40e598ca94eb81d95b810e949bc0e2d93bd",
        "obj": "f1b06680093799331217b20e8ca6c8deaafad3be414d9d8f2b6bb52ca2b0a55b",
        "status": "d76764951f52ca8d874af418c0976c30f5bc07f3f1555110541c43b0a3346fb6",
        "iters": "3ff1c4b5ca762c1e12e36d5c51d947120f56fe273e8b0f9ba93859ca39237567",
        "active": "fa49cd74563b4831c09b7b4a84b05d9b9ff2695704a7aa0dd05ebed5d5d2ad33",
        "working": "fa49cd74563b4831c09b7b4a84b05d9b9ff2695704a7aa0dd05ebed5d5d2ad33",
        "theta": "1f793ccda57a76dab6d641d964a156d6e654931a9f01554681da17319ca28a10",
        "omega": "ec04da046827a1795de1b056f9491c0b7783c41189756e9e628edd433c0066ce",
    },
    "N16_obs4_no_presolve": {
        "U": "fadcae5b4c1dee7605e6b897291e5df225bb26ebc91e145056b7ee0633480939",
        "X": "c2248db45459f99d2aef0e51ad52b614a2e029ed14b4c56ec49eb0f955751d0d",
        "obj": "48d2837bc1459500e2513ba213723944f0eab6e5ce7bacc0f78012d3ff9f4bee",
        "status": "d76764951f52ca8d874af418c0976c30f5bc07f3f1555110541c43b0a3346fb6",
        "iters": "aba74cb4dd0f96fc6bf7f5177b8b92993ffa1710a6f9a02b78a57e5d7bab32be",
        "active": "fa49cd74563b4831c09b7b4a84b05d9b9ff2695704a7aa0dd05ebed5d5d2ad33",
        "working": "fa49cd74563b4831c09b7b4a84b05d9b9ff2695704a7aa0dd05ebed5d5d2ad33",
        "theta": "1f793ccda57a76dab6d641d964a156d6e654931a9f01554681da17319ca28a10",
        "omega": "ec04da046827a1795de1b056f9491c0b7783c41189756e9e628edd433c0066ce",
    },
    "N16_obs13_default": {
        "U": "ed0947f5a81d314ec99d29ed29a7ac8abd36467b48e79bebe8a95ec5228250e0",
        "X": "6b3b440436c68d215383746331274cb401e69b65c4970d494d5d63adc754e2c2",
        "obj": "c63b2382be859af15cfa38a786896497c8c43bc8dac5a23ad5ad4cac3054c0ec",
        "status": "d76764951f52ca8d874af418c0976c30f5bc07f3f1555110541c43b0a3346fb6",
        "iters": "be01b70f381c4c71c04eb689a4e33f29fa8290dcfc69c1a0b816b536d6fc1512",
        "active": "882081b7e652c148ee6f363680978d03e711563a6e7664e53b8b9005de87f368",
        "working": "882081b7e652c148ee6f363680978d03e711563a6e7664e53b8b9005de87f368",
        "theta": "1f793ccda57a76dab6d641d964a156d6e654931a9f01554681da17319ca28a10",
        "omega": "ec04da046827a1795de1b056f9491c0b7783c41189756e9e628edd433c0066ce",
    },
    "N16_obs13_interior": {
        "U": "bc09509bf84b836777f5cfb4e7c65c86c661b1cd294738c08020b24eab9e7abf",
        "X": "a5d243c17a682a9d2b3141445cbb75588796d791ac0a0b49e3cfe2ee5b2c508e",
        "obj": "f6df67e579b651a52b366e9c51c851a7bee224790297d4a761de04f8f41eab28",
        "status": "d76764951f52ca8d874af418c0976c30f5bc07f3f1555110541c43b0a3346fb6",
        "iters": "c6b2dc924da59d29be81d98ce7271a665a471ddc2dc809c74062b94c39994bff",
        "active": "882081b7e652c148ee6f363680978d03e711563a6e7664e53b8b9005de87f368",
        "working": "882081b7e652c148ee6f363680978d03e711563a6e7664e53b8b9005de87f368",
        "theta": "1f793ccda57a76dab6d641d964a156d6e654931a9f01554681da17319ca28a10",
        "omega": "ec04da046827a1795de1b056f9491c0b7783c41189756e9e628edd433c0066ce",
    },
    "N16_obs13_no_presolve": {
        "U": "58d8836e3b0813d6b071bcb0f016a9a3887b5114d66c48ec94fd6f5306a0f09b",
        "X": "6c86a12279a94f43a65439b7d94e8cefb6b39ba9ced07849ee776af950c27129",
        "obj": "c63b2382be859af15cfa38a786896497c8c43bc8dac5a23ad5ad4cac3054c0ec",
        "status": "d76764951f52ca8d874af418c0976c30f5bc07f3f1555110541c43b0a3346fb6",
        "iters": "0c2ca5c519bbbd6ea9f092e926252ef56f9dc1b363f61f22f2b47ef747548499",
        "active": "882081b7e652c148ee6f363680978d03e711563a6e7664e53b8b9005de87f368",
        "working": "882081b7e652c148ee6f363680978d03e711563a6e7664e53b8b9005de87f368",
        "theta": "1f793ccda57a76dab6d641d964a156d6e654931a9f01554681da17319ca28a10",
        "omega": "ec04da046827a1795de1b056f9491c0b7783c41189756e9e628edd433c0066ce",
    },
    "rollout_N3_obs5": {
        "X_pred": "2136b013c687b4eff1b0a00744e2cd0050c72907a29910034aabe1ee815841ab",
        "U_pred": "836008db8a1eef0104e9120596d1bc2ab877f1af712887ee207842c348ee50b2",
        "n_steps": "da868d0b0ec7bd3a9c39e5048573f44d31ee10efa5fd96bfffe627bb63e57d9e",
        "last_status": "5f62c1fd73b210a0108f8315a5cdc6ba88d9e3c7cb5fe4188d2c7d298f8d7623",
        "total_iters": "398139ade596b8079b22f9835c65b97691e5752ee5781445be4560a553607729",
    },
    "rollout_N8_obs5": {
        "X_pred": "34d584b64d93efd865c5cdd1c229592561491e103de10eff5499dc086e2b1e39",
        "U_pred": "9300072ac4be2708bd43e44c85fdff2f9e8bcf4c3f207ac994c1f757b885019a",
        "n_steps": "90bae9312894707bec371344b65165e008a4babff40f56305fed716984ef1dae",
        "last_status": "1dec46180be8969101752df122b25e94b9bbcf03ff966d35346facb9264fd95b",
        "total_iters": "27ea784971a6563d1cb8d11f998b56659bcd12f6561a9c469c02ac08f1d08207",
    },
}


@pytest.mark.gpu
@pytest.mark.parametrize("flag", FLAG_NAMES)
@pytest.mark.parametrize("N,n_obs", SHAPES)
def test_step_outputs_bit_identical_to_recorded(N, n_obs, flag):
    torch = pytest.importorskip("torch")
    import c_oracle
    import lipmpc
    from test_params_gpu import _compare
    P, bt, g, got = _step(torch, lipmpc, N, n_obs, flag)
    name = _case_id(N, n_obs, flag)
    ref = c_oracle.plan_step_batch(P, bt["state"], bt["goal"], bt["foot"], bt["xy"] if n_obs else None, bt["nv"] if n_obs else None,
                                   bt["delta"], n_threads=8)
    # (min_ok, _compare's floor on the share of the batch certified on both sides, describes the batch, not the agreement:
    # a walk of closed_loop_problems ends with the problem its oracle did not solve, so up to one problem in every walk is a
    # failure by construction -- 3 of 13 at N = 1.  Those must carry the same status on both sides, as every problem must.)
    _compare(f"small shapes {PARAM_SET} {name}", g, ref, tol=4e-4 if flag == "interior" else 1e-5, min_ok=0.0)
    moved = [k for k in NAMES if got[k] != EXPECTED[name][k]]
    assert not moved, (name, moved, got)


@pytest.mark.gpu
@pytest.mark.parametrize("N,n_obs", ROLLOUTS)
def test_rollout_outputs_bit_identical_to_recorded(N, n_obs):
    torch = pytest.importorskip("torch")
    import lipmpc
    ro, step, got = _rollout(torch, lipmpc, N, n_obs)
    name = f"rollout_N{N}_obs{n_obs}"
    walked = ro["n_steps"].cpu().numpy() >= 1
    assert walked.sum() >= B // 2, (name, ro["n_steps"])
    d = np.abs(ro["U_pred"].cpu().numpy()[walked, 0, :2] - step["U"].cpu().numpy()[walked, 0])
    assert d.max() < 1e-7, (name, d.max())
    moved = [k for k in ROLLOUT_NAMES if got[k] != EXPECTED[name][k]]
    assert not moved, (name, moved, got)


if __name__ == "__main__":
    import json
    import torch
    import lipmpc
    rec = {_case_id(N, m, f): _step(torch, lipmpc, N, m, f)[3] for (N, m) in SHAPES for f in FLAG_NAMES}
    rec.update({f"rollout_N{N}_obs{m}": _rollout(torch, lipmpc, N, m)[2] for (N, m) in ROLLOUTS})
    print(json.dumps(rec, indent=1))
