"""Stats rows from the greedy-myopic rollout, the parts that need no GPU:

  * the oracle (oracle/env_np.py OracleEnv + greedy) reproduces the reference's GreedyMyopic run
    behind tests/golden/services_greedy.npz (make_golden_greedy_services.py) action for action, so
    the fixture's Metrics are those of the controller the device implements;
  * the inputs of tests/test_greedy_stats_gpu.py exercise the controller under the oracle (they do
    not degenerate into all-on or all-off clusters whose rows would hide a wrong sum);
  * mdr_greedy_rollout_stats' argument guards that come before any device call.
"""
import ctypes as C
import json
import random

import numpy as np
import pytest

import golden_util as gu
from greedy_stats_inputs import SEED, SHAPES, overrides, synthetic_pop
from oracle import env_np as O


def test_oracle_reproduces_the_greedy_services_fixture():
    d = gu.load("services_greedy.npz")
    meta = json.loads(bytes(d["meta_json"]).decode())
    N, T = meta["N"], meta["T"]
    assert (N, T, meta["controller"], meta["resets"]) == (50, 120, "greedy_myopic", 3)
    assert meta["min_key_gap"] > 0.0  # (no two houses ever tied: the reference's unstable sort had no say)
    assert d["actions"].shape == (T, N)
    for f in ("cumul_avg_reward", "cumul_signal_error", "cumul_squared_max_error_temp"):
        assert d[f"metrics_{f}"].shape == (T,)
    props = gu.props_from_overrides({"cluster_prop.nb_agents": N,
                                     "power_grid_prop.signal_properties.mode": meta["signal"]})
    ora = O.OracleEnv(props, random.Random(meta["seed"]))
    ora.reset()
    ora.reset()
    cop = props.cluster_prop.house_prop.hvac_prop.cop
    for t in range(T):
        a = O.greedy(ora.T, ora.pop["target"], ora.pop["cap"], cop, ora.lock, float(ora.S))
        np.testing.assert_array_equal(a, d["actions"][t].astype(bool), err_msg=f"t={t}")
        ora.step(a)


# (n = 130 runs 1 and 31 ticks from the same start: the 1-tick case is the 31-tick one's first tick)
@pytest.mark.parametrize("n,ticks", [s for s in SHAPES if s[1] > 1])
def test_gpu_shapes_exercise_the_controller(n, ticks):
    props = gu.props_from_overrides(overrides(n))
    ora = O.OracleEnv(props, random.Random(SEED), population=synthetic_pop(props, n, SEED))
    cop = props.cluster_prop.house_prop.hvac_prop.cop
    tg, caps = ora.pop["target"], ora.pop["cap"]
    on_counts, lock_counts, pos, neg = set(), set(), 0, 0
    for t in range(ticks):
        a = O.greedy(ora.T, tg, caps, cop, ora.lock, float(ora.S))
        if t > 0:
            assert 0 < int(a.sum()) < n, f"tick {t}: one action only"
        d = ora.T - tg
        pos += int(np.sum(d > 0))
        neg += int(np.sum(d < 0))
        o, _ = ora.step(a)
        on_counts.add(int(np.sum(o["on"])))
        lock_counts.add(int(np.sum(o["lock"])))
    print(f"n={n} ticks={ticks}: ON counts {len(on_counts)}, lockout counts {len(lock_counts)}, "
          f"T>target {pos}, T<target {neg}")
    assert len(on_counts) >= 3 and len(lock_counts) >= 3
    assert pos > 0 and neg > 0


def test_argument_guards_without_gpu():
    """MDR_EARG (-1), each with its own message, before the context is looked at (so before any HIP
    call): negative sizes, a negative first row, rows asked for without a row buffer, a null context."""
    from mdr_amd import _lib

    lib = _lib.load()
    f = lib.mdr_greedy_rollout_stats
    one = C.c_void_p(16)  # (never dereferenced: every call below is refused first)
    for bad in ((-1, 0, 0), (1, -1, 0), (1, 0, -1)):  # n, act_stride, rew_stride
        assert f(None, bad[0], one, one, bad[1], one, bad[2], None, one, 0, None) == -1
        assert b"mdr_greedy_rollout_stats: negative size" in lib.mdr_last_error()
    assert f(None, 1, one, one, 0, one, 0, None, one, -1, None) == -1
    assert b"negative row0" in lib.mdr_last_error()
    assert f(None, 1, one, one, 0, one, 0, None, None, 0, None) == -1
    assert b"null stats rows" in lib.mdr_last_error()
    assert f(None, 1, one, one, 0, one, 0, None, one, 0, None) == -1
    assert b"null argument" in lib.mdr_last_error()
    assert f(None, 0, None, None, 0, None, 0, None, None, 0, None) == -1  # (n = 0 still needs a context)
    assert b"null argument" in lib.mdr_last_error()
