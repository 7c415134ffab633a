"""Stats rows from the greedy-myopic rollout: ``Environment.greedy_rollout(T, stats=RolloutStats)``
(mdr_greedy_rollout_stats: k_tick_stats behind every tick's step into one of 32 slots of block
partials, k_tick_rows_finish once per 32 ticks), its per-tick fallback,
``services.evaluate_controller(env, "greedy", T)`` and ``ServerLoop(controller="greedy", rollout_ticks=K)``.

Reference: GreedyMyopic.get_action (server/app/core/agents/controllers/greedy_myopic_controller.py:
67-104), Metrics.update (server/app/services/metrics_service.py:108-157) and TrainingManager.test
(server/app/services/training_manager.py:265-295).

What is compared with what.  The twin of every run is the per-tick loop ``greedy_actions(out=a)`` ->
``step_tensor(a, ctrl="greedy_keys")`` -> ``Shard.tick_stats(reward, row)``, which
tests/test_env_parity_gpu.py pins to the oracle and tests/test_tick_stats_gpu.py to the host sums.
The rollout's per-house expressions, and the operands and order of every addition of a row, are that
loop's kernels' (k_tick_stats unchanged; k_tick_rows_finish adds a slot's block partials in
k_tick_stats_finish's order), so everything is compared with ``==`` / ``torch.equal``: rows,
actions, rewards, state, P, tick, clock and signal.  The Metrics golden and the hand-made
TrainingManager.test use tests/test_bangbang_stats_gpu.py's tolerances for the same arithmetic
(rtol 1e-12, atol 1e-9 on the accumulators): the device adds the houses in a blocked order where
the reference adds them one by one.
"""
import copy
import json
import random

import numpy as np
import pytest

import golden_util as gu
from greedy_stats_inputs import FORM_N, SEED, SHAPES, overrides

pytestmark = pytest.mark.gpu

_TWINS = {}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def make_env(n, pmode="individual_L2", signal="sinusoidals", extra=None):
    from mdr_amd.environment import Environment

    ov = overrides(n, pmode, signal)
    ov.update(extra or {})
    return Environment(gu.props_from_overrides(ov), rng=random.Random(SEED), population="synthetic", seed=SEED)


def facts(env):
    sh = env.shard
    dev = {"t_air": sh.t_air.clone(), "t_mass": sh.t_mass.clone(), "hvac": sh.hvac.clone()}
    return dev, (env._tick, env.date_time, env._cluster_power(), float(env.current_od_temp),
                 float(env.power_grid.current_signal), env.rng.getstate())


def assert_same_facts(torch, a, b, what=""):
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), f"{what} {k}"
    assert a[1] == b[1], what


def twin_loop(torch, env, T):
    """T ticks of the per-tick loop: every tick's actions, rewards, tick_stats row and the scalars
    its obs carried (pre-step signal, outdoor temperature and cluster power; post-step signal)."""
    n, sh = env.n, env.shard
    out = {"acts": torch.full((T, n), 255, dtype=torch.uint8, device="cuda"),
           "rews": torch.full((T, n), float("nan"), dtype=torch.float64, device="cuda"),
           "rows": torch.full((T, 16), -7.0, dtype=torch.float64, device="cuda"),
           "s_prev": [], "od": [], "p_prev": [], "s_post": []}
    for t in range(T):
        out["s_prev"].append(float(env.power_grid.current_signal))
        out["od"].append(float(env.current_od_temp))
        out["p_prev"].append(env._cluster_power())
        a = env.greedy_actions(out=out["acts"][t])
        r = env.step_tensor(a, rewards=out["rews"][t], ctrl="greedy_keys")
        sh.tick_stats(r, out["rows"][t])
        out["s_post"].append(float(env.power_grid.current_signal))
    out["facts"] = facts(env)
    return out


def twin(torch, key, make, T):
    """The loop's record for a configuration: computed once, shared by the cases that need it."""
    if key not in _TWINS:
        _TWINS[key] = twin_loop(torch, make(), T)
    return _TWINS[key]


def run_with_rows(torch, env, T, dims, stats=None):
    from mdr_amd.services import RolloutStats

    n = env.n
    stats = stats or RolloutStats(env, T)
    acts = torch.full((T, n) if dims == 2 else (n,), 255, dtype=torch.uint8, device="cuda")
    rews = torch.full((T, n) if dims == 2 else (n,), float("nan"), dtype=torch.float64, device="cuda")
    a, r = env.greedy_rollout(T, actions=acts, rewards=rews, stats=stats)
    assert a.data_ptr() == acts.data_ptr() and r.data_ptr() == rews.data_ptr()
    return acts, rews, stats


def assert_is_the_loop(torch, env, acts, rews, stats, B, T, dims, row0=0, what=""):
    rows = stats.stats[row0:row0 + T]
    bad = (rows != B["rows"][:T]).nonzero().tolist()
    assert torch.equal(rows, B["rows"][:T]), f"{what}: rows differ at (tick, slot) {bad[:8]}"
    assert bool((rows[:, 4] != 0).all()), f"{what}: a reward slot is zero"
    assert bool((rows[:, 13:] == 0).all())
    if dims == 2:
        assert torch.equal(acts, B["acts"][:T]) and torch.equal(rews, B["rews"][:T]), what
    else:
        assert torch.equal(acts, B["acts"][T - 1]) and torch.equal(rews, B["rews"][T - 1]), what


# ------------------------------------------------------------------ 1. rows are tick_stats' rows
@pytest.mark.parametrize("dims", [2, 1])
@pytest.mark.parametrize("n,T", SHAPES)
def test_rows_are_the_per_tick_loops(torch_gpu, n, T, dims):
    torch = torch_gpu
    B = twin(torch, ("ind", n, T), lambda: make_env(n), T)
    env = make_env(n)
    acts, rews, stats = run_with_rows(torch, env, T, dims)
    assert stats.rows == T
    assert_is_the_loop(torch, env, acts, rews, stats, B, T, dims, what=f"n={n} T={T} dims={dims}")
    assert_same_facts(torch, facts(env), B["facts"], f"n={n} T={T}")  # state, tick, clock, P, od, signal, RNG


# ------------------------------------------------------------------ 2. rows do not perturb the rollout
def test_rows_do_not_perturb_the_rollout(torch_gpu):
    from mdr_amd.services import RolloutStats

    torch = torch_gpu
    n, T = 1030, 42
    B = twin(torch, ("ind", n, T), lambda: make_env(n), T)
    plain, rowed = make_env(n), make_env(n)
    pa, pr = plain.greedy_rollout(T, actions=torch.empty((T, n), dtype=torch.uint8, device="cuda"))
    ra, rr, _ = run_with_rows(torch, rowed, T, 2)
    assert torch.equal(pa, ra) and torch.equal(pr, rr)
    assert_same_facts(torch, facts(plain), facts(rowed), "with and without rows")
    # two calls into one RolloutStats: rows 0-4, then 5-41 (a batch of 32 and one of 5), as one loop's
    env = make_env(n)
    stats = RolloutStats(env, T)
    run_with_rows(torch, env, 5, 1, stats)
    assert stats.rows == 5
    acts, rews, _ = run_with_rows(torch, env, 37, 1, stats)
    assert stats.rows == T
    assert_is_the_loop(torch, env, acts, rews, stats, B, T, 1, what="5 + 37 ticks")
    assert_same_facts(torch, facts(env), B["facts"], "5 + 37 ticks")
    host, prev = stats.host(), stats.prev()
    assert np.array_equal(host, B["rows"].cpu().numpy())
    assert prev["cluster_hvac_power"].tolist() == B["p_prev"]  # (rows 0 and 5 from record_power, the rest slot 12)
    assert prev["reg_signal"].tolist() == B["s_prev"] and prev["OD_temp"].tolist() == B["od"]
    assert prev["signal_post"].tolist() == B["s_post"]


# ------------------------------------------------------------------ 3. forms and modes
@pytest.mark.parametrize("form,pmode,signal,T", [("fused", "individual_L2", "sinusoidals", 40),
                                                 ("band", "individual_L2", "regular_steps", 40),
                                                 ("band", "common_L2", "sinusoidals", 20),
                                                 ("band", "mixture", "sinusoidals", 20)])
def test_forms_and_modes(torch_gpu, form, pmode, signal, T):
    torch = torch_gpu
    n = FORM_N
    B = twin(torch, (pmode, signal, n, T), lambda: make_env(n, pmode, signal), T)
    env = make_env(n, pmode, signal)
    env.shard.set_option("gq_fused", 1 if form == "fused" else 0)
    acts, rews, stats = run_with_rows(torch, env, T, 2)
    assert_is_the_loop(torch, env, acts, rews, stats, B, T, 2, what=f"{form} {pmode} {signal}")
    assert_same_facts(torch, facts(env), B["facts"], f"{form} {pmode} {signal}")
    if form == "fused":
        fd = env.shard.greedy_fused_diag()
        assert fd["calls"] == T, fd  # (every tick took k_gq_decide2 + the fused step)
    else:
        print(pmode, signal, "band record", env.shard.greedy_band())


# ------------------------------------------------------------------ 4. the per-tick Python fallback
def test_python_fallback_rows(torch_gpu):
    """random_sample draws the neighbours every tick, so there is no link table and greedy_rollout
    steps from Python: its rows are shard.tick_stats' after each step_tensor."""
    torch = torch_gpu
    n, T = 130, 9
    extra = {"cluster_prop.agents_comm_prop.mode": "random_sample"}
    B = twin(torch, ("random_sample", n, T), lambda: make_env(n, extra=extra), T)
    env = make_env(n, extra=extra)
    assert env._links is None
    acts, rews, stats = run_with_rows(torch, env, T, 2)
    assert stats.rows == T
    assert_is_the_loop(torch, env, acts, rews, stats, B, T, 2, what="fallback")
    assert_same_facts(torch, facts(env), B["facts"], "fallback")
    assert stats.prev()["cluster_hvac_power"].tolist() == B["p_prev"]
    assert stats.prev()["signal_post"].tolist() == B["s_post"]


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_everything_where_it_was(torch_gpu):
    from mdr_amd import _lib
    from mdr_amd.services import RolloutStats

    torch = torch_gpu
    n = 300
    env, other = make_env(n), make_env(n)
    env.greedy_rollout(3)  # (an env that has moved on from its reset, its keys and band state live)
    stats = RolloutStats(env, 8)
    before = facts(env)
    with pytest.raises(ValueError, match="another environment"):
        env.greedy_rollout(4, stats=RolloutStats(other, 8))
    run_with_rows(torch, env, 5, 1, stats)
    mid, filled = facts(env), stats.stats.clone()
    assert mid[1][0] == before[1][0] + 5 and stats.rows == 5
    with pytest.raises(ValueError, match="overflow"):
        env.greedy_rollout(4, stats=stats)
    assert_same_facts(torch, facts(env), mid, "overflow")
    assert stats.rows == 5 and torch.equal(stats.stats, filled)

    # the C call with a negative first row
    sh = env.shard
    ticks = (_lib.mdr_tick * 2)(*(_lib.mdr_tick(t_od_prev=30.0, solar=0.0, s_prev=4.0e5, tick=env._tick + t)
                                  for t in range(2)))  # (made by hand: nobody's drivers advance)
    acts = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    rew = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    rows = torch.full((4, 16), -7.0, dtype=torch.float64, device="cuda")

    def c_call(shard, row0):
        return shard.lib.mdr_greedy_rollout_stats(shard.ctx, 2, ticks, _lib.ptr(acts), 0, _lib.ptr(rew), 0,
                                                  _lib.ptr(shard.p_dev), _lib.ptr(rows), row0, shard.stream())

    with pytest.raises(_lib.MdrError, match="MDR_EARG.*row0"):
        _lib.check(c_call(sh, -1), "mdr_greedy_rollout_stats")
    assert_same_facts(torch, facts(env), mid, "row0 < 0")
    assert float(rows.min()) == -7.0 == float(rows.max()) and float(rew.max()) == -7.0 and int(acts.min()) == 255

    # a context with a host communicator attached: the C call, then the Python call
    osh = other.shard
    keep = (_lib.HOST_ALLREDUCE_FN(lambda *a: 0), _lib.HOST_SENDRECV_FN(lambda *a: 0))
    _lib.check(osh.lib.mdr_comm_host(osh.ctx, 1, 0, keep[0], keep[1], None), "mdr_comm_host")
    o_before = facts(other)
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE.*single-shard"):
        _lib.check(c_call(osh, 0), "mdr_greedy_rollout_stats")
    ostats = RolloutStats(other, 8)
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        other.greedy_rollout(4, stats=ostats)
    assert_same_facts(torch, facts(other), o_before, "communicator")  # (drivers, tick and RNG included)
    assert ostats.rows == 0 and float(rows.min()) == -7.0 == float(rows.max())
    # the refused env still runs: its next rollout is the untouched twin's
    a1, r1, _ = run_with_rows(torch, env, 3, 1, stats)
    assert stats.rows == 8 and bool((stats.stats[5:8, 4] != 0).all())


# ------------------------------------------------------------------ 6. the reference's Metrics
def test_server_loop_chunks_feed_reference_metrics(torch_gpu):
    """services_greedy.npz's run (the reference's GreedyMyopic controllers, reference population)
    through ServerLoop(controller="greedy", rollout_ticks=32): chunks of 32, 32, 32, 24 ticks; after
    each, every accumulator against the golden at that step."""
    from mdr_amd.environment import Environment
    from mdr_amd.services import ServerLoop

    d = gu.load("services_greedy.npz")
    meta = json.loads(bytes(d["meta_json"]).decode())
    N, T = meta["N"], meta["T"]
    assert (N, T) == (50, 120)
    props = gu.props_from_overrides({"cluster_prop.nb_agents": N,
                                     "power_grid_prop.signal_properties.mode": meta["signal"]})
    env = Environment(props, rng=random.Random(meta["seed"]))
    env.reset(return_obs=False)
    env.reset(return_obs=False)
    loop = ServerLoop(env, controller="greedy", start_stats_from=meta["start_stats_from"], nb_time_steps=T,
                      rollout_ticks=32)
    final = None
    for k, done in ((32, 32), (32, 64), (32, 96), (24, 120)):
        final = loop.run(32)
        assert loop.current_time_step == done
        m = loop.metrics
        for f in m.FIELDS:
            print(f"step {done - 1} {f}: {getattr(m, f)!r} golden {d[f'metrics_{f}'][done - 1]!r}")
            np.testing.assert_allclose(getattr(m, f), d[f"metrics_{f}"][done - 1], rtol=1e-12, atol=1e-9,
                                       err_msg=f"{f} after step {done - 1}")
    assert sorted(loop.ui.description) == [0, 32, 64, 96]  # one UI update per chunk, at its start
    np.testing.assert_allclose([final["RMSE signal per agent"], final["RMSE temperature"],
                                final["RMS Max Error temperature"]], d["rms"], rtol=1e-12)


# ------------------------------------------------------------------ 7. evaluate_controller
def test_evaluate_controller_greedy_is_the_references_test(torch_gpu):
    from mdr_amd.services import ROLLOUT_CONTROLLERS, evaluate_controller

    torch = torch_gpu
    assert ROLLOUT_CONTROLLERS == ("bangbang", "deadband_bangbang", "greedy")
    n, T = 300, 37
    env_a, env_b = make_env(n), make_env(n)
    for e in (env_a, env_b):  # an env that has moved on from its reset
        e.greedy_rollout(3)
    before = facts(env_a)
    got = evaluate_controller(env_a, "greedy", T)
    assert sorted(got) == ["Mean test return", "Test mean signal error", "Test mean temperature error"]

    # B: TrainingManager.test by hand (training_manager.py:265-295) over the per-tick greedy loop
    ev = copy.deepcopy(env_b)
    ev.reset(return_obs=False)
    tg = ev.shard.target.cpu().numpy()
    ret = temp = sig = 0.0
    for _ in range(T):
        r = ev.step_tensor(ev.greedy_actions(), ctrl="greedy_keys").cpu().numpy()
        Tair = ev.shard.t_air.cpu().numpy()
        P, s = ev._cluster_power(), ev.power_grid.current_signal
        ret += float(np.sum(r / n))
        temp += float(np.sum(np.abs(Tair - tg) / n))
        sig += float(np.abs(s - P) / n ** 2) * n
    want = {"Mean test return": ret / T, "Test mean temperature error": temp / T, "Test mean signal error": sig / T}
    for k in want:
        print(f"greedy {k}: evaluate_controller {got[k]!r} manual {want[k]!r}")
        assert want[k] != 0.0 and got[k] != 0.0
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)

    # the caller's env is where it was (the shared RNG aside, which reset advances as in the reference)
    after = facts(env_a)
    for k, v in before[0].items():
        assert torch.equal(v, after[0][k]), k
    assert before[1][:5] == after[1][:5]

    # a caller-kept twin: its context and its row, action and reward buffers are reused
    tw = copy.deepcopy(env_a)
    o1 = evaluate_controller(env_a, "greedy", T, twin=tw)
    kept = dict(tw._eval_kept)
    o2 = evaluate_controller(env_a, "greedy", T, twin=tw)
    assert all(tw._eval_kept[k] is kept[k] for k in ("stats", "rewards", "actions"))
    assert all(np.isfinite(v) and v != 0.0 for v in list(o1.values()) + list(o2.values()))
    assert facts(env_a)[1][:5] == before[1][:5]
    with pytest.raises(ValueError, match="not the env itself"):
        evaluate_controller(env_a, "greedy", T, twin=env_a)
    with pytest.raises(ValueError, match="controller must be"):
        evaluate_controller(env_a, "random", T)
