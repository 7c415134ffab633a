"""Closed-loop bang-bang windows under the common penalty modes (common_L2, common_max_error,
mixture): Environment.rollout(action_mode="bangbang" | "deadband_bangbang") runs k_step_closed<...,
COMMON> per window, then k_win_reduce, k_win_pen_reduce and k_closed_reward_common.

Exactness: the cluster's {sum pen_i / N, max pen_i} of a tick enter the reward only, so the state
trajectory is the individual_L2 window's, and the window adds the terms pen_i / N in the order of
k_step_t's block partial + k_pen_reduce (mdr_kernels.hip, k_step_closed's COMMON comment).  So a
rollout is BIT FOR BIT the loop of step_tensor(None, action_mode=c, lookahead=c): every comparison
with the loop or with a directly launched twin is ==.  tests/test_bangbang_common_cpu.py asserts
under the oracle that == on these inputs discriminates the summation order (the per-tick order and
k_step_window's differ in bits on several ticks of every shape with n >= 129).

Inputs: tests/bangbang_inputs.py (random.Random(8), sinusoidal signal, deadband 0.05 degC); mixture
with alpha_common_max = 0.5 so the max enters the reward.
"""
import random

import numpy as np
import pytest

import golden_util as gu
from bangbang_inputs import CTRLS, SEED, SHAPES, overrides

pytestmark = pytest.mark.gpu

PMODES = ["common_L2", "common_max_error", "mixture"]
TEMP_RTOL = 1e-10  # tests/test_env_parity_gpu.py
CHUNK = 37


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _props(n, pmode):
    o = overrides(n, pmode)
    if pmode == "mixture":
        o["reward_prop.penalty_props.alpha_common_max"] = 0.5
    return gu.props_from_overrides(o)


def _pair(n, pmode, **kw):
    from mdr_amd.environment import Environment

    props = _props(n, pmode)
    return (Environment(props, rng=random.Random(SEED), **kw), Environment(props, rng=random.Random(SEED), **kw))


def _same_state(torch, e1, e2):
    torch.cuda.synchronize()
    s1, s2 = e1.shard.host_state(), e2.shard.host_state()
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k], err_msg=k)
    assert e1._cluster_power() == e2._cluster_power()


def _loop(env, ticks, ctrl, lookahead=True):
    """The per-tick path: [ticks, N] rewards of a loop of step_tensor."""
    rows = []
    for _ in range(ticks):
        r = env.step_tensor(None, action_mode=ctrl, lookahead=ctrl if lookahead else None)
        rows.append(r.cpu().numpy().copy())
    return np.stack(rows)


# ------------------------------------------------------------------ 1. window == loop
@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("pmode", PMODES)
@pytest.mark.parametrize("n,ticks,win", SHAPES)
def test_window_equals_per_tick_loop(torch_gpu, n, ticks, win, pmode, ctrl):
    """Two rollouts in a row against the twin's step_tensor loop, ==: one lane, both slots of a
    lane, a second tile holding one house, a second block, three windows with a ragged last tile."""
    torch = torch_gpu
    e1, e2 = _pair(n, pmode)
    e1.shard.set_rollout_window(win)
    for rep in range(2):
        r1 = e1.rollout(ticks, action_mode=ctrl).cpu().numpy()
        assert r1.shape == (ticks, n)
        r2 = _loop(e2, ticks, ctrl)
        np.testing.assert_array_equal(r1, r2, err_msg=f"rollout {rep}")
        _same_state(torch, e1, e2)


def test_window_equals_loop_258_blocks(torch_gpu):
    """131,585 synthetic houses = 257 blocks of 512 and one block of ONE house: k_win_pen_reduce's
    threads 0 and 1 take a second block each.  mixture / deadband form, 33 ticks (two windows)."""
    torch = torch_gpu
    n, ticks, ctrl = 131585, 33, "deadband_bangbang"
    e1, e2 = _pair(n, "mixture", population="synthetic")
    for rep in range(2):
        r1 = e1.rollout(ticks, action_mode=ctrl)
        r2 = torch.stack([e2.step_tensor(None, action_mode=ctrl, lookahead=ctrl).clone() for _ in range(ticks)])
        assert torch.equal(r1, r2), f"rollout {rep}"
        sh1, sh2 = e1.shard, e2.shard
        assert torch.equal(sh1.t_air, sh2.t_air) and torch.equal(sh1.t_mass, sh2.t_mass)
        assert torch.equal(sh1.hvac, sh2.hvac)
        assert e1._cluster_power() == e2._cluster_power()


# ------------------------------------------------------------------ 2. the blocked path is taken
@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("pmode", PMODES)
def test_blocked_path_is_taken(torch_gpu, pmode, ctrl):
    """65 ticks are 3 step launches at window 32; the same state and rewards as the rollout."""
    torch = torch_gpu
    from mdr_amd.environment import ACTION_MODES

    n, T = 4099, 65
    e1, e2 = _pair(n, pmode)
    r1 = torch.empty((T, n), dtype=torch.float64, device="cuda")
    ms1, l1 = e1.shard.time_step_kernels(e1.driver_window(T), None, 0, ACTION_MODES[ctrl], r1, n)
    assert l1 == 3 and ms1 > 0.0
    e2.shard.set_rollout_window(0)
    r2 = torch.empty_like(r1)
    _ms2, l2 = e2.shard.time_step_kernels(e2.driver_window(T), None, 0, ACTION_MODES[ctrl], r2, n)
    assert l2 == T
    torch.cuda.synchronize()
    s1, s2 = e1.shard.host_state(), e2.shard.host_state()
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k], err_msg=k)
    assert torch.equal(r1, r2)


@pytest.mark.parametrize("dims,nodes", [(2, 4 * 6), (1, 2 * 6 + 2)])
@pytest.mark.parametrize("pmode", PMODES)
def test_captured_sequence(torch_gpu, pmode, dims, nodes):
    """257 houses, 40 ticks at window 7 (6 windows): the first use_graph=True call captures
    k_step_closed + k_win_reduce + k_win_pen_reduce + k_closed_reward_common per window (4 nw), or,
    with one shared reward row, the two finish kernels behind the last window only (2 nw + 2).
    Kernels only: the capture guard admits no memset node."""
    torch = torch_gpu
    n, ticks, win = 257, 40, 7
    from mdr_amd.environment import Environment

    env = Environment(_props(n, pmode), rng=random.Random(SEED))
    env.shard.set_rollout_window(win)
    rew = torch.empty((ticks, n) if dims == 2 else (n,), dtype=torch.float64, device="cuda")
    g0 = env.shard.graph_info()
    env.rollout(ticks, action_mode="deadband_bangbang", rewards=rew, use_graph=True)
    g1 = env.shard.graph_info()
    assert g1["rollout_graphs"] == g0["rollout_graphs"] + 1 and g1["guarded"] == g0["guarded"] + 1, (g0, g1)
    assert g1["guarded_nodes"] - g0["guarded_nodes"] == nodes, (g0, g1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. variants against the twin's direct rollout
@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("pmode", PMODES)
def test_one_row_rewards(torch_gpu, pmode, ctrl):
    """A 1-D [N] reward buffer holds the last tick's finalised rewards (two windows: the first
    one's rows are never finalised)."""
    torch = torch_gpu
    n, ticks = 513, 40
    e1, e2 = _pair(n, pmode)
    row = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    out = e1.rollout(ticks, action_mode=ctrl, rewards=row)
    assert out.data_ptr() == row.data_ptr()
    r2 = e2.rollout(ticks, action_mode=ctrl)
    assert torch.equal(row, r2[ticks - 1])
    _same_state(torch, e1, e2)


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("pmode", PMODES)
def test_graph_replay_equals_direct(torch_gpu, pmode, ctrl):
    """use_graph=True three times (one capture, then two replays) against the directly launched twin."""
    torch = torch_gpu
    n, ticks = 4099, 65
    e1, e2 = _pair(n, pmode)
    buf = torch.empty((ticks, n), dtype=torch.float64, device="cuda")
    g0 = e1.shard.graph_info()
    for rep in range(3):
        r1 = e1.rollout(ticks, action_mode=ctrl, rewards=buf, use_graph=True)
        r2 = e2.rollout(ticks, action_mode=ctrl)
        assert torch.equal(r1, r2), f"call {rep}"
        _same_state(torch, e1, e2)
    g1 = e1.shard.graph_info()
    assert g1["rollout_graphs"] - g0["rollout_graphs"] == 1 and g1["rollout_launches"] - g0["rollout_launches"] == 3


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("pmode", PMODES)
def test_window_off_equals_windows(torch_gpu, pmode, ctrl):
    """set_rollout_window(0): one launch per tick inside the call, the same bits."""
    torch = torch_gpu
    n, ticks = 513, 40
    e1, e2 = _pair(n, pmode)
    e1.shard.set_rollout_window(0)
    assert torch.equal(e1.rollout(ticks, action_mode=ctrl), e2.rollout(ticks, action_mode=ctrl))
    _same_state(torch, e1, e2)


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("pmode", PMODES)
def test_interleaved_with_steps_and_random_rollouts(torch_gpu, pmode, ctrl):
    """rollout -> step_tensor(bang-bang) -> rollout(random) -> rollout(bang-bang) against a twin that
    runs the bang-bang ticks one by one.  The random rollout is the same windowed call on both (the
    open-loop windows only bound their summation order against the one-tick kernels),
    from the same state: what is compared is that the closed-loop windows leave and find the count
    slots, the staged drivers and the penalty partial rows as every other path expects them."""
    torch = torch_gpu
    from mdr_amd import _lib as L

    n = 4099
    e1, e2 = _pair(n, pmode)
    for e in (e1, e2):
        e.shard.set_option("window_thermal", L.THERMAL_EXACT)
    got = [e1.rollout(33, action_mode=ctrl).cpu().numpy(), _loop(e1, 2, ctrl),
           e1.rollout(10, action_mode="random").cpu().numpy(), e1.rollout(40, action_mode=ctrl).cpu().numpy()]
    want = [_loop(e2, 33, ctrl), _loop(e2, 2, ctrl), e2.rollout(10, action_mode="random").cpu().numpy(),
            _loop(e2, 40, ctrl)]
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"part {i}")
    _same_state(torch, e1, e2)


# ------------------------------------------------------------------ 4. the reference's mixture trajectory
def _make_env(props, seed, resets):
    """tests/test_env_parity_gpu.py make_env: the goldens were recorded after `resets` resets."""
    from mdr_amd.environment import Environment

    env = Environment(props, rng=random.Random(seed))
    for _ in range(resets - 1):
        env.reset()
    return env


def test_reference_mixture_golden_as_rollouts(torch_gpu):
    """n64_mixture_2d (mixture, deadband form) as rollouts in chunks of 37 ticks at window 7: every
    reward row, and at each chunk's end the FSM state, temperatures and cluster power."""
    d, meta = gu.traj("n64_mixture_2d")
    assert meta["controller"] == "deadband_bbc"
    props = gu.props_from_overrides(meta["overrides"])
    env = _make_env(props, meta["seed"], meta["resets"])
    env.shard.set_rollout_window(7)
    T = meta["T"]
    t0 = 0
    while t0 < T:
        k = min(CHUNK, T - t0)
        R = env.rollout(k, action_mode="deadband_bangbang").cpu().numpy()
        for j in range(k):
            np.testing.assert_allclose(R[j], d["traj_reward"][t0 + j], rtol=1e-9, atol=1e-12, err_msg=f"t={t0 + j}")
        t0 += k
        st = env.shard.host_state()
        np.testing.assert_array_equal(st["on"], d["traj_on"][t0 - 1].astype(bool), err_msg=f"on t={t0 - 1}")
        np.testing.assert_array_equal(st["lock"], d["traj_lock"][t0 - 1].astype(bool), err_msg=f"lock t={t0 - 1}")
        np.testing.assert_array_equal(st["sso"], d["traj_sso"][t0 - 1], err_msg=f"sso t={t0 - 1}")
        np.testing.assert_allclose(st["T"], d["traj_T"][t0 - 1], rtol=TEMP_RTOL, atol=0)
        np.testing.assert_allclose(st["Tm"], d["traj_Tm"][t0 - 1], rtol=TEMP_RTOL, atol=0)
        assert env.cluster.current_power_consumption == float(d["traj_P"][t0 - 1])


# ------------------------------------------------------------------ 5. stats keep the per-tick path
@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("pmode", PMODES)
def test_stats_keep_the_per_tick_path(torch_gpu, pmode, ctrl):
    """With stats rows a common mode stays on the per-tick sequence (rollout_stats_path == 2); its
    rewards and state == the windowed rollout without rows."""
    torch = torch_gpu
    from mdr_amd.environment import ACTION_MODES
    from mdr_amd.services import RolloutStats

    n, ticks = 513, 40
    e1, e2 = _pair(n, pmode)
    assert e1.shard.rollout_stats_path(ACTION_MODES[ctrl]) == 2
    stats = RolloutStats(e1, ticks)
    r1 = e1.rollout(ticks, action_mode=ctrl, stats=stats)
    assert stats.rows == ticks
    r2 = e2.rollout(ticks, action_mode=ctrl)
    assert torch.equal(r1, r2)
    _same_state(torch, e1, e2)
