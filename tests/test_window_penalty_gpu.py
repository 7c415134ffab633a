"""Temporally blocked rollouts under the common penalty modes (common_L2, common_max_error,
mixture; rewards_calculator.py:46-181): k_step_window's COMMON variant writes per-tick, per-wave
{sum pen_i / N, max pen_i} partials, k_win_pen_reduce and k_win_reward_common finish each window.

The comparison is the per-tick path (a loop of step_tensor: k_step_t, k_pen_reduce,
k_reward_finalize), which test_env_parity_gpu.py pins to the oracle and test_oracle_golden.py to
the reference.  With the EXACT thermal form the two paths run the same operations on the same bits
except for the ORDER in which the n non-negative terms pen_i / N are added, so:
* state (FSM words, temperatures) and cluster power: equal;
* common_max_error rewards: equal (a max does not depend on the order);
* common_L2 / mixture rewards: each order is within (n - 1) 2^-53 relative of the exact sum, and
  the remaining operations add non-negative terms to operands that agree to that error:
  rtol = 2 n 2^-53 + 2^-50, atol = 0.  Derived, not measured.
"""
import random

import numpy as np
import pytest

import golden_util as gu
from oracle import env_np as O

pytestmark = pytest.mark.gpu

MODES = ["common_L2", "common_max_error", "mixture"]
AFFINE_T_RTOL = 1e-10                        # tests/test_window_gpu.py
AFFINE_R_RTOL, AFFINE_R_ATOL = 1e-9, 1e-10


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _overrides(n, pmode, signal="sinusoidals"):
    return {"cluster_prop.nb_agents": n,
            "power_grid_prop.signal_properties.mode": signal,
            "reward_prop.penalty_props.mode": pmode,
            "reward_prop.penalty_props.alpha_common_max": 0.5,
            "cluster_prop.house_prop.deadband": 0.4}


def _pair(n, pmode, seed=3, thermal=None):
    from mdr_amd import _lib as L
    from mdr_amd.environment import Environment

    props = gu.props_from_overrides(_overrides(n, pmode))
    e1 = Environment(props, rng=random.Random(seed), population="synthetic", seed=77)
    e2 = Environment(props, rng=random.Random(seed), population="synthetic", seed=77)
    if thermal is not None:
        for e in (e1, e2):
            e.shard.set_option("window_thermal", {"exact": L.THERMAL_EXACT, "affine": L.THERMAL_AFFINE}[thermal])
    return e1, e2


def _same_state(torch, e1, e2):
    torch.cuda.synchronize()
    s1, s2 = e1.shard.host_state(), e2.shard.host_state()
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k], err_msg=k)
    assert e1._cluster_power() == e2._cluster_power()


def _close_state(torch, e1, e2, rtol):
    torch.cuda.synchronize()
    s1, s2 = e1.shard.host_state(), e2.shard.host_state()
    for k in ("on", "lock", "sso"):
        np.testing.assert_array_equal(s1[k], s2[k], err_msg=k)
    for k in ("T", "Tm"):
        np.testing.assert_allclose(s1[k], s2[k], rtol=rtol, atol=0, err_msg=k)
    assert e1._cluster_power() == e2._cluster_power()


def _actions(torch, ticks, n, action_mode, seed):
    if action_mode != "buffer":
        return None
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((ticks, n), device="cuda", generator=g) < 0.5).to(torch.uint8)


def _step_loop(env, ticks, action_mode, acts):
    """The per-tick path: [ticks, N] rewards of a loop of step_tensor."""
    rows = []
    for t in range(ticks):
        r = env.step_tensor(None if acts is None else acts[t], action_mode=action_mode)
        rows.append(r.cpu().numpy().copy())
    return np.stack(rows)


def _order_rtol(n):
    return 2 * n * 2.0 ** -53 + 2.0 ** -50


def _check_rewards_exact_form(pmode, n, got, want):
    if pmode == "common_max_error":
        np.testing.assert_array_equal(got, want)
    else:
        np.testing.assert_allclose(got, want, rtol=_order_rtol(n), atol=0)


@pytest.mark.parametrize("n,ticks,win", [(1, 5, 32), (2, 33, 32), (129, 40, 7), (513, 33, 32), (4099, 65, 32),
                                         (20011, 64, 16)])
@pytest.mark.parametrize("pmode", MODES)
@pytest.mark.parametrize("action_mode", ["random", "buffer"])
def test_window_vs_per_tick_exact(torch_gpu, n, ticks, win, pmode, action_mode):
    """EXACT thermal form, two rollouts in a row against the same ticks of the step_tensor loop:
    one lane, both houses of a lane, a second tile / block with one house, three windows, a short
    window, 16-tick windows."""
    torch = torch_gpu
    e1, e2 = _pair(n, pmode, thermal="exact")
    e1.shard.set_rollout_window(win)
    for rep in range(2):
        acts = _actions(torch, ticks, n, action_mode, 1000 * rep + n)
        r1 = e1.rollout(ticks, actions=acts, action_mode=action_mode).cpu().numpy()
        r2 = _step_loop(e2, ticks, action_mode, acts)
        _same_state(torch, e1, e2)
        _check_rewards_exact_form(pmode, n, r1, r2)


@pytest.mark.parametrize("n,ticks,win", [(257, 40, 7), (4099, 65, 32)])
@pytest.mark.parametrize("pmode", MODES)
def test_window_vs_per_tick_affine(torch_gpu, n, ticks, win, pmode):
    """The default AFFINE form: integer state and P equal, temperatures and rewards within the
    project's affine-form bounds of the per-tick path."""
    torch = torch_gpu
    e1, e2 = _pair(n, pmode)
    e1.shard.set_rollout_window(win)
    r1 = e1.rollout(ticks, action_mode="random").cpu().numpy()
    r2 = _step_loop(e2, ticks, "random", None)
    _close_state(torch, e1, e2, AFFINE_T_RTOL)
    np.testing.assert_allclose(r1, r2, rtol=AFFINE_R_RTOL, atol=AFFINE_R_ATOL)


@pytest.mark.parametrize("pmode", MODES)
def test_window_vs_oracle(torch_gpu, pmode):
    """Every reward row of a buffer-action rollout (default thermal form) against OracleEnv.step."""
    torch = torch_gpu
    from mdr_amd.environment import Environment

    n, T = 3001, 40
    props = gu.props_from_overrides(_overrides(n, pmode, signal="flat"))
    env = Environment(props, rng=random.Random(12))
    ora = O.OracleEnv(props, random.Random(12))
    acts = np.random.RandomState(0).randint(0, 2, (T, n)).astype(np.uint8)
    R = env.rollout(T, actions=torch.from_numpy(acts).cuda(), action_mode="buffer").cpu().numpy()
    for t in range(T):
        o, rr = ora.step(acts[t].astype(bool))
        np.testing.assert_allclose(R[t], rr, rtol=1e-9, atol=1e-12, err_msg=f"t={t}")
    st = env.shard.host_state()
    np.testing.assert_array_equal(st["sso"], o["sso"])
    np.testing.assert_allclose(st["T"], o["T"], rtol=1e-10, atol=0)


@pytest.mark.parametrize("pmode", MODES)
def test_window_off_equals_per_tick(torch_gpu, pmode):
    """set_rollout_window(0): the rollout's one-tick fallback runs step_tensor's kernels."""
    torch = torch_gpu
    n, ticks = 777, 20
    e1, e2 = _pair(n, pmode)
    e1.shard.set_rollout_window(0)
    r1 = e1.rollout(ticks, action_mode="random").cpu().numpy()
    r2 = _step_loop(e2, ticks, "random", None)
    np.testing.assert_array_equal(r1, r2)
    _same_state(torch, e1, e2)


def test_graph_replay_equals_direct(torch_gpu):
    """use_graph=True (the second call replays the captured sequence, which holds no memset node)
    against the direct-launch rollout of a twin."""
    torch = torch_gpu
    n, ticks = 4099, 65
    e1, e2 = _pair(n, "mixture")
    for rep in range(2):
        r1 = e1.rollout(ticks, action_mode="random", use_graph=True).cpu().numpy()
        r2 = e2.rollout(ticks, action_mode="random").cpu().numpy()
        np.testing.assert_array_equal(r1, r2)
        _same_state(torch, e1, e2)


@pytest.mark.parametrize("pmode", MODES)
def test_one_row_rewards(torch_gpu, pmode):
    """A 1-D [N] reward buffer that every tick overwrites holds the last tick's finalised rewards."""
    torch = torch_gpu
    n, ticks = 3000, 40
    e1, e2 = _pair(n, pmode)
    row = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    out = e1.rollout(ticks, action_mode="random", rewards=row)
    assert out.data_ptr() == row.data_ptr()
    r2 = e2.rollout(ticks, action_mode="random").cpu().numpy()
    np.testing.assert_array_equal(row.cpu().numpy(), r2[ticks - 1])
    _same_state(torch, e1, e2)


def test_rollout_then_steps(torch_gpu):
    """step_tensor ticks behind a rollout continue from its state: ticks 40..44 of the twin's loop."""
    torch = torch_gpu
    n, ticks, more = 3000, 40, 5
    e1, e2 = _pair(n, "mixture", thermal="exact")
    e1.rollout(ticks, action_mode="random")
    r1 = _step_loop(e1, more, "random", None)
    r2 = _step_loop(e2, ticks + more, "random", None)[ticks:]
    _same_state(torch, e1, e2)
    _check_rewards_exact_form("mixture", n, r1, r2)
