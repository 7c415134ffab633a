"""Stats rows from the closed-loop bang-bang rollouts: ``Environment.rollout(action_mode="bangbang" |
"deadband_bangbang", stats=RolloutStats)`` (mdr_rollout_stats: k_step_closed<..., STATS> forms every
tick's block partials in the window kernel, k_closed_stats finishes the rows), its per-tick fallback,
``services.evaluate_controller`` and ``ServerLoop(rollout_ticks=K)``.

Reference: Metrics.update (server/app/services/metrics_service.py:108-157) and TrainingManager.test
(server/app/services/training_manager.py:265-295) for the two baseline controllers
(bangbang_controllers.py:25-65).

What is compared with what.  The twin of every run is the per-tick loop ``step_tensor(None,
action_mode=c, lookahead=c)`` + ``Shard.tick_stats``, whose state a rollout reproduces bit for bit
(tests/test_bangbang_rollout_gpu.py).
  * The rollout itself (rewards, t_air, t_mass, FSM words, P) with and without rows: ==.
  * Row slots 2 (a max), 10, 11 (counts) and 12 (P, from integer counts): == the twin's rows; 13-15: 0.
  * Sum slots 0, 1, 3, 5-9: against math.fsum of the float64 terms formed on the host from the
    twin's downloaded per-tick state (bit-equal state, so the kernel's terms), within
    n * 2^-52 * fsum(|terms|) — tests/test_tick_stats_gpu.py's bound: the first-order bound of any
    summation order, doubled.
  * Slot 4 = -((alpha_temp * sum pen [/ norm_temp] + n * sig) / N) against fsum(reward_i / N) over the
    2-D run's finalised rewards, within (n + 8) * 2^-52 * (|alpha_temp| * fsum(pen) / norm_temp +
    n * |sig|) / N: n - 1 roundings of the partial sums, at most 8 more from the factored form and
    the per-house roundings of the terms compared against.  The same bits with a 1-D reward buffer.
  * Every variant (2-D / 1-D rewards, direct / graph, first call / replay) writes the same bits: the
    reduction order is fixed.
  * The per-tick fallback's rows (window off, a common penalty mode): == the twin's rows.
  * ServerLoop(rollout_ticks=32) against the reference's Metrics golden, evaluate_controller against
    the reference's formulas in numpy: tests/test_tick_stats_gpu.py's tolerances (rtol 1e-12).
"""
import copy
import json
import math
import random

import numpy as np
import pytest

import golden_util as gu
from bangbang_inputs import CTRLS, DEADBAND, SEED, SHAPES, overrides

pytestmark = pytest.mark.gpu

STATS_SHAPES = SHAPES + [(300, 37, 32)]  # + a ragged last block
SUM_SLOTS = (0, 1, 3, 5, 6, 7, 8, 9)
EXACT_SLOTS = (2, 10, 11, 12)
HOUSE_SUMS = ("cumul_avg_reward", "cumul_temp_offset", "cumul_temp_error", "cumul_squared_error_temp")
VARIANTS = [("direct", 2), ("direct", 1), ("graph", 2), ("graph", 1)]
_SCEN = {}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def make_env(n, pmode="individual_L2", seed=SEED):
    from mdr_amd.environment import Environment

    return Environment(gu.props_from_overrides(overrides(n, pmode)), rng=random.Random(seed))


def state_of(torch, env):
    sh = env.shard
    return {"t_air": sh.t_air.clone(), "t_mass": sh.t_mass.clone(), "hvac": sh.hvac.clone(),
            "P": sh.p_dev.clone()}


def twin_loop(torch, env, ticks, ctrl):
    """The per-tick loop with tick_stats rows; per tick the downloaded post-step state, rewards and
    the signal the tick's reward compared P with."""
    sh = env.shard
    rows = torch.full((ticks, 16), -7.0, dtype=torch.float64, device="cuda")
    out = {"T": [], "Tm": [], "reward": [], "s_prev": []}
    for t in range(ticks):
        out["s_prev"].append(float(env.power_grid.current_signal))
        r = env.step_tensor(None, action_mode=ctrl, lookahead=ctrl)
        sh.tick_stats(r, rows[t])
        out["T"].append(sh.t_air.cpu().numpy())
        out["Tm"].append(sh.t_mass.cpu().numpy())
        out["reward"].append(r.cpu().numpy().copy())
    out["rows_dev"] = rows
    out["rows"] = rows.cpu().numpy()
    out["target"] = sh.target.cpu().numpy()
    out["final"] = state_of(torch, env)
    return out


def scenario(torch, n, ticks, win, ctrl):
    """Twins over 2 x ticks ticks: the per-tick loop B; a rollout without rows; and per variant a
    rollout with rows, called twice (graph: capture, then a replay with row0 unchanged)."""
    key = (n, ticks, win, ctrl)
    if key in _SCEN:
        return _SCEN[key]
    from mdr_amd.environment import ACTION_MODES
    from mdr_amd.services import RolloutStats

    s = {"B": twin_loop(torch, make_env(n), 2 * ticks, ctrl)}
    plain = make_env(n)
    plain.shard.set_rollout_window(win)
    s["plain"] = {"rewards": [plain.rollout(ticks, action_mode=ctrl).clone() for _ in range(2)],
                  "final": state_of(torch, plain)}
    for how, dims in VARIANTS:
        env = make_env(n)
        env.shard.set_rollout_window(win)
        assert env.shard.rollout_stats_path(ACTION_MODES[ctrl]) == 1  # the closed-loop windows write the rows
        stats = RolloutStats(env, ticks)
        rew = torch.full((ticks, n) if dims == 2 else (n,), float("nan"), dtype=torch.float64, device="cuda")
        g0 = env.shard.graph_info()
        v = {"rows": [], "rewards": [], "host": [], "prev": []}
        for call in range(2):
            stats.clear()
            out = env.rollout(ticks, action_mode=ctrl, rewards=rew, use_graph=(how == "graph"), stats=stats)
            assert out.data_ptr() == rew.data_ptr() and stats.rows == ticks
            v["rows"].append(stats.stats.clone())
            v["rewards"].append(rew.clone())
            v["host"].append(stats.host().copy())
            v["prev"].append({k: x.copy() for k, x in stats.prev().items()})
        v["final"] = state_of(torch, env)
        g1 = env.shard.graph_info()
        v["graphs"] = (g1["rollout_graphs"] - g0["rollout_graphs"], g1["rollout_launches"] - g0["rollout_launches"],
                       g1["guarded"] - g0["guarded"])
        v["cfg"] = env.shard.cfg
        s[(how, dims)] = v
    _SCEN[key] = s
    return s


def shape_params():
    return [pytest.param(n, t, w, c, id=f"{n}-{t}-{w}-{c}") for (n, t, w) in STATS_SHAPES for c in CTRLS]


# ------------------------------------------------------------------ 1. the rows do not perturb the rollout
@pytest.mark.parametrize("n,ticks,win,ctrl", shape_params())
def test_rows_do_not_perturb_the_rollout(torch_gpu, n, ticks, win, ctrl):
    torch = torch_gpu
    s = scenario(torch, n, ticks, win, ctrl)
    B, plain = s["B"], s["plain"]
    loop_rewards = [torch.from_numpy(np.stack(B["reward"][c * ticks:(c + 1) * ticks])).to("cuda") for c in range(2)]
    for call in range(2):  # (the rollout without rows is the loop: tests/test_bangbang_rollout_gpu.py)
        assert torch.equal(plain["rewards"][call], loop_rewards[call]), call
    for how, dims in VARIANTS:
        v = s[(how, dims)]
        for call in range(2):
            want = plain["rewards"][call] if dims == 2 else plain["rewards"][call][ticks - 1]
            assert torch.equal(v["rewards"][call], want), (how, dims, call)
        for k in ("t_air", "t_mass", "hvac", "P"):
            assert torch.equal(v["final"][k], plain["final"][k]), (how, dims, k)
            assert torch.equal(v["final"][k], B["final"][k]), (how, dims, k)
        if how == "graph":  # one capture (kernels only: the memset guard walked it), two launches
            assert v["graphs"] == (1, 2, 1), v["graphs"]
        else:
            assert v["graphs"] == (0, 0, 0), v["graphs"]


# ------------------------------------------------------------------ 2-4. the rows
def check_rows(rows, B, t0, ticks, n, rewards2d, cfg, tag):
    """rows [ticks, 16] of ticks t0 .. t0 + ticks - 1 against the twin loop B."""
    N = float(n)
    tg = B["target"]
    for j in range(ticks):
        t = t0 + j
        row, ref = rows[j], B["rows"][t]
        for k in EXACT_SLOTS:
            assert row[k] == ref[k], (tag, t, k, row[k], ref[k])
        assert list(row[13:]) == [0.0, 0.0, 0.0], (tag, t)
        T, Tm = B["T"][t], B["Tm"][t]
        e, d = T - tg / N, T - tg
        terms = {0: e, 1: np.abs(e), 3: e * e, 5: T, 6: d, 7: np.abs(d), 8: Tm, 9: tg}
        for k in SUM_SLOTS:
            want = math.fsum(terms[k])
            bound = n * 2.0 ** -52 * math.fsum(np.abs(terms[k]))
            err = abs(float(row[k]) - want)
            if j in (0, ticks - 1):
                print(f"{tag} t={t} slot {k}: got {row[k]!r} want {want!r} |err| {err:.3g} bound {bound:.3g}")
            assert err <= bound, (tag, t, k, row[k], want, err, bound)
        # slot 4: the factored reward sum against the finalised rewards of the 2-D run
        hi, lo = tg + DEADBAND / 2.0, tg - DEADBAND / 2.0
        pen = np.where(hi < T, (T - hi) ** 2, np.where(lo > T, (lo - T) ** 2, 0.0))
        x = (ref[12] - B["s_prev"][t]) / N
        sig = cfg.alpha_sig * (x * x) / cfg.norm_sig
        want4 = math.fsum(rewards2d[j] / N)
        bound4 = (n + 8) * 2.0 ** -52 * (abs(cfg.alpha_temp) * math.fsum(pen) / cfg.norm_temp + n * abs(sig)) / N
        err4 = abs(float(row[4]) - want4)
        if j in (0, ticks - 1):
            print(f"{tag} t={t} slot 4: got {row[4]!r} want {want4!r} |err| {err4:.3g} bound {bound4:.3g}")
        assert want4 != 0.0 and err4 <= bound4, (tag, t, row[4], want4, err4, bound4)


@pytest.mark.parametrize("n,ticks,win,ctrl", shape_params())
def test_rows_against_the_per_tick_loop(torch_gpu, n, ticks, win, ctrl):
    torch = torch_gpu
    s = scenario(torch, n, ticks, win, ctrl)
    B = s["B"]
    first = s[("direct", 2)]
    for call in range(2):
        rew = first["rewards"][call].cpu().numpy()
        check_rows(first["rows"][call].cpu().numpy(), B, call * ticks, ticks, n, rew, first["cfg"],
                   f"n={n} {ctrl} call {call}")
    # every variant writes the same bits (1-D rewards: slot 4 too; graph capture and replay)
    for how, dims in VARIANTS[1:]:
        for call in range(2):
            assert torch.equal(s[(how, dims)]["rows"][call], first["rows"][call]), (how, dims, call)
    # the host's side: the scalars tick t's obs carried, the post-step signal, the pre-step power
    assert first["host"][0].shape == (ticks, 16)
    for call in range(2):
        prev = first["prev"][call]
        sl = slice(call * ticks, (call + 1) * ticks)
        assert list(prev["reg_signal"]) == B["s_prev"][sl]
        assert list(prev["signal_post"][:-1]) == B["s_prev"][sl][1:]
        assert list(prev["cluster_hvac_power"][1:]) == list(B["rows"][sl][:-1, 12])
    if ticks > 1:
        assert first["prev"][1]["cluster_hvac_power"][0] == B["rows"][ticks - 1, 12]  # record_power: the env's P


@pytest.mark.parametrize("ctrl", CTRLS)
def test_two_window_sizes_on_one_context(torch_gpu, ctrl):
    """Two calls with different window sizes on one context (the partial rows are sized for the grid,
    not the window): the rows of both calls are right."""
    from mdr_amd.services import RolloutStats

    torch = torch_gpu
    n, ticks = 4099, 65
    s = scenario(torch, n, ticks, 32, ctrl)
    env = make_env(n)
    stats = RolloutStats(env, 2 * ticks)
    rew = torch.empty((2 * ticks, n), dtype=torch.float64, device="cuda")
    env.shard.set_rollout_window(32)
    env.rollout(ticks, action_mode=ctrl, rewards=rew[:ticks], stats=stats)
    env.shard.set_rollout_window(7)
    env.rollout(ticks, action_mode=ctrl, rewards=rew[ticks:], stats=stats)
    assert stats.rows == 2 * ticks
    rows = stats.host()
    check_rows(rows, s["B"], 0, 2 * ticks, n, rew.cpu().numpy(), env.shard.cfg, f"n={n} {ctrl} windows 32, 7")
    # the first call is the scenario's first call; the second one sums its windows' blocks alike
    assert np.array_equal(rows[:ticks], s[("direct", 2)]["host"][0])
    assert np.array_equal(rows[ticks:], s[("direct", 2)]["host"][1])


# ------------------------------------------------------------------ 5. the per-tick fallback
@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("case", ["window_off", "common_L2"])
def test_fallback_rows_are_tick_stats(torch_gpu, case, ctrl):
    from mdr_amd.environment import ACTION_MODES
    from mdr_amd.services import RolloutStats

    torch = torch_gpu
    n, ticks = 300, 37
    pmode = "common_L2" if case == "common_L2" else "individual_L2"
    B = twin_loop(torch, make_env(n, pmode), ticks, ctrl)
    for dims, use_graph in ((2, False), (1, True)):
        env = make_env(n, pmode)
        if case == "window_off":
            env.shard.set_rollout_window(0)
        assert env.shard.rollout_stats_path(ACTION_MODES[ctrl]) == 2  # mdr_tick_stats' kernels per tick
        stats = RolloutStats(env, ticks)
        rew = torch.empty((ticks, n) if dims == 2 else (n,), dtype=torch.float64, device="cuda")
        env.rollout(ticks, action_mode=ctrl, rewards=rew, use_graph=use_graph, stats=stats)
        assert torch.equal(stats.stats, B["rows_dev"]), (case, dims)
        assert float(B["rows_dev"][:, 4].abs().min()) > 0
        want = np.stack(B["reward"]) if dims == 2 else B["reward"][-1]
        assert np.array_equal(rew.cpu().numpy(), want)
        for k, x in state_of(torch, env).items():
            assert torch.equal(x, B["final"][k]), k


# ------------------------------------------------------------------ 6. the reference's Metrics
def test_server_loop_chunks_feed_reference_metrics(torch_gpu):
    """services.npz's run (tests/test_services_gpu.py) through ServerLoop(rollout_ticks=32): chunks of
    32, 32, 32, 24 ticks; after each, every accumulator against the golden at that step."""
    from mdr_amd.environment import Environment
    from mdr_amd.services import ServerLoop

    d = gu.load("services.npz")
    meta = json.loads(bytes(d["meta_json"]).decode())
    N, T = meta["N"], meta["T"]
    assert (N, T) == (50, 120)
    props = gu.props_from_overrides({"cluster_prop.nb_agents": N,
                                     "power_grid_prop.signal_properties.mode": meta["signal"]})
    env = Environment(props, rng=random.Random(meta["seed"]))
    env.reset(return_obs=False)
    env.reset(return_obs=False)
    loop = ServerLoop(env, controller="deadband_bangbang", start_stats_from=meta["start_stats_from"], nb_time_steps=T,
                      rollout_ticks=32)
    final = None
    for k, done in ((32, 32), (32, 64), (32, 96), (24, 120)):
        final = loop.run(32)
        assert loop.current_time_step == done
        m = loop.metrics
        for f in m.FIELDS:
            np.testing.assert_allclose(getattr(m, f), d[f"metrics_{f}"][done - 1], rtol=1e-12, atol=1e-9,
                                       err_msg=f"{f} after step {done - 1}")
    assert sorted(loop.ui.description) == [0, 32, 64, 96]  # one UI update per chunk, at its start
    np.testing.assert_allclose([final["RMSE signal per agent"], final["RMSE temperature"],
                                final["RMS Max Error temperature"]], d["rms"], rtol=1e-12)


def test_server_loop_chunks_cut_at_episodes_and_logs(torch_gpu):
    """Chunks end at episode ends, log boundaries and n_steps; the accumulators are the per-tick loop's."""
    from mdr_amd.services import ServerLoop

    n = 300
    kw = dict(controller="bangbang", start_stats_from=3, nb_time_steps=40, time_steps_per_episode=25,
              time_steps_train_log=10)
    a = ServerLoop(make_env(n), rollout_ticks=8, **kw)
    b = ServerLoop(make_env(n), **kw)
    assert a.run(17) is None and b.run(17) is None
    assert sorted(a.ui.description) == [0, 8, 10]  # chunks 0-7, 8-9 (a log boundary), 10-16 (n_steps)
    ra, rb = a.run(), b.run()
    assert a.current_time_step == b.current_time_step == 40
    # 17-19 (log), 20-24 (the episode's end), 25-29 (log), 30-37 (8 ticks), 38-39 (nb_time_steps)
    assert sorted(a.ui.description) == [0, 8, 10, 17, 20, 25, 30, 38]
    assert len(a.logs) == len(b.logs) == 4
    for la, lb in zip(a.logs, b.logs):
        assert la.keys() == lb.keys()
        for k in la:
            np.testing.assert_allclose(la[k], lb[k], rtol=1e-12, atol=0, err_msg=k)
    for f in a.metrics.FIELDS:
        got, want = getattr(a.metrics, f), getattr(b.metrics, f)
        if f in HOUSE_SUMS:
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f)
        else:
            assert got == want, f
    np.testing.assert_allclose(list(ra.values()), list(rb.values()), rtol=1e-12)
    assert a.env._tick == b.env._tick and a.env.date_time == b.env.date_time


# ------------------------------------------------------------------ 7. evaluate_controller
def _env_facts(torch, env):
    return (state_of(torch, env), env._tick, env.date_time, env._cluster_power(), env.current_od_temp,
            env.power_grid.current_signal)


@pytest.mark.parametrize("ctrl", CTRLS)
def test_evaluate_controller_is_the_references_test(torch_gpu, ctrl):
    from mdr_amd.services import evaluate_controller

    torch = torch_gpu
    n, T = 300, 37
    env_a, env_b = make_env(n, seed=11), make_env(n, seed=11)
    for e in (env_a, env_b):  # an env that has moved on from its reset
        e.rollout(3, action_mode=ctrl)
    before = _env_facts(torch, env_a)
    got = evaluate_controller(env_a, ctrl, T)
    assert sorted(got) == ["Mean test return", "Test mean signal error", "Test mean temperature error"]

    # B: TrainingManager.test by hand (training_manager.py:265-295) over the per-tick loop
    ev = copy.deepcopy(env_b)
    ev.reset(return_obs=False)
    tg = ev.shard.target.cpu().numpy()
    ret = temp = sig = 0.0
    for _ in range(T):
        r = ev.step_tensor(None, action_mode=ctrl, lookahead=ctrl).cpu().numpy()
        Tair = ev.shard.t_air.cpu().numpy()
        P, s = ev._cluster_power(), ev.power_grid.current_signal
        ret += float(np.sum(r / n))
        temp += float(np.sum(np.abs(Tair - tg) / n))
        sig += float(np.abs(s - P) / n ** 2) * n
    want = {"Mean test return": ret / T, "Test mean temperature error": temp / T, "Test mean signal error": sig / T}
    for k in want:
        print(f"{ctrl} {k}: evaluate_controller {got[k]!r} manual {want[k]!r}")
        assert want[k] != 0.0
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)

    # the caller's env is where it was
    after = _env_facts(torch, env_a)
    for k, v in before[0].items():
        assert torch.equal(v, after[0][k]), k
    assert before[1:] == after[1:]

    # a caller-kept twin: its context, buffers and graph are reused
    twin = copy.deepcopy(env_a)
    o1 = evaluate_controller(env_a, ctrl, T, twin=twin)
    g1 = twin.shard.graph_info()
    o2 = evaluate_controller(env_a, ctrl, T, twin=twin)
    g2 = twin.shard.graph_info()
    assert g1["rollout_graphs"] == g2["rollout_graphs"] == 1 and g2["rollout_launches"] == g1["rollout_launches"] + 1
    assert all(np.isfinite(v) for v in list(o1.values()) + list(o2.values()))
    assert _env_facts(torch, env_a)[1:] == before[1:]
    with pytest.raises(ValueError, match="not the env itself"):
        evaluate_controller(env_a, ctrl, T, twin=env_a)
    with pytest.raises(ValueError, match="controller must be"):
        evaluate_controller(env_a, "random", T)


# ------------------------------------------------------------------ 8. refusals
def test_refusals(torch_gpu):
    from mdr_amd import _lib
    from mdr_amd.services import RolloutStats, ServerLoop

    torch = torch_gpu
    n = 300
    env, other = make_env(n), make_env(n)
    stats = RolloutStats(env, 8)
    before = _env_facts(torch, env)
    with pytest.raises(NotImplementedError, match="open-loop window"):
        env.rollout(4, action_mode="random", stats=stats)
    with pytest.raises(ValueError, match="another environment"):
        env.rollout(4, action_mode="bangbang", stats=RolloutStats(other, 8))
    env.rollout(5, action_mode="bangbang", stats=stats)
    mid = _env_facts(torch, env)
    assert stats.rows == 5 and mid[1] == before[1] + 5
    filled = stats.stats.clone()
    with pytest.raises(ValueError, match="overflow"):
        env.rollout(4, action_mode="bangbang", stats=stats)
    after = _env_facts(torch, env)  # (nothing ran)
    assert stats.rows == 5 and after[1:] == mid[1:] and torch.equal(stats.stats, filled)
    for k, v in mid[0].items():
        assert torch.equal(v, after[0][k]), k
    # an open-loop source with the window off runs per tick: rows, no refusal
    env.shard.set_rollout_window(0)
    env.rollout(3, action_mode="random", stats=stats)
    assert stats.rows == 8
    # the C call: rows outside the buffer, a context with a communicator
    ticks = env.driver_window(2)
    rew = torch.empty((2, n), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="outside"):
        env.shard.rollout_stats(ticks, None, 0, _lib.ACT_BANGBANG, rew, n, stats.stats, 7)
    keep = (_lib.HOST_ALLREDUCE_FN(lambda *a: 0), _lib.HOST_SENDRECV_FN(lambda *a: 0))
    _lib.check(other.shard.lib.mdr_comm_host(other.shard.ctx, 1, 0, keep[0], keep[1], None), "mdr_comm_host")
    rows = torch.full((4, 16), -7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        other.shard.rollout_stats(other.driver_window(2), None, 0, _lib.ACT_BANGBANG, rew, n, rows, 0)
    assert float(rows.min()) == -7.0
    with pytest.raises(ValueError, match="rollout_ticks needs"):
        ServerLoop(make_env(8), controller="random", rollout_ticks=4)
