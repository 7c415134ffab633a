"""Closed-loop windowed rollouts of the bang-bang controllers (BangBangController /
DeadbandBangBangController, bangbang_controllers.py:25-65): Environment.rollout(action_mode=
"bangbang" | "deadband_bangbang").

Under individual_L2 with <= 4 capacity classes a window of up to 32 ticks is one k_step_closed
launch (controller -> lockout FSM -> thermal update in registers), k_win_reduce and k_closed_reward
behind it; everything else of these sources runs one step launch per tick inside the C call.

Exactness: a rollout is BIT FOR BIT the loop of step_tensor(None, action_mode=c, lookahead=c) —
rewards, t_air, t_mass, FSM words, cluster power.  Per house the window runs the one-tick kernels'
operations in their order (the per-window thermal coefficients are the one-tick expressions), P is
a sum of exact integer counts, and -(x + -nsig) with nsig the exact negation of the signal penalty
is -(x + sig).  The per-tick form launches step_tensor's own kernels (the common penalty modes:
the same k_pen_reduce).  So every comparison with the loop is ==, not a tolerance.

Inputs: the default host-drawn population from random.Random(8), a sinusoidal signal and a
deadband of 0.05 degC — tests/test_bangbang_rollout_cpu.py asserts that with them both controllers
switch houses both ways, are refused by the lockout and (deadband form) hold inside the band at
every shape used here.
"""
import random

import numpy as np
import pytest

import golden_util as gu
from bangbang_inputs import CTRLS, SEED, SHAPES, overrides

pytestmark = pytest.mark.gpu

TEMP_RTOL = 1e-10  # tests/test_env_parity_gpu.py
CHUNK = 37


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _pair(n, pmode="individual_L2", extra=None):
    from mdr_amd.environment import Environment

    o = overrides(n, pmode)
    o.update(extra or {})
    props = gu.props_from_overrides(o)
    return Environment(props, rng=random.Random(SEED)), Environment(props, rng=random.Random(SEED))


def _make_env(props, seed, resets):
    """tests/test_env_parity_gpu.py make_env: the goldens were recorded after `resets` resets."""
    from mdr_amd.environment import Environment

    env = Environment(props, rng=random.Random(seed))
    for _ in range(resets - 1):
        env.reset()
    return env


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


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("n,ticks,win", SHAPES)
def test_window_equals_per_tick_loop(torch_gpu, n, ticks, win, ctrl):
    """Two rollouts in a row against the twin's step_tensor loop, ==: one lane, both slots of a
    lane, a second tile holding one house, a second block, three windows with a ragged last tile,
    short windows.  Default options (window_thermal = AFFINE): the option does not apply."""
    torch = torch_gpu
    e1, e2 = _pair(n)
    e1.shard.set_rollout_window(win)
    for rep in range(2):
        r1 = e1.rollout(ticks, action_mode=ctrl).cpu().numpy()
        assert r1.shape == (ticks, n)
        r2 = _loop(e2, ticks, ctrl)
        np.testing.assert_array_equal(r1, r2, err_msg=f"rollout {rep}")
        _same_state(torch, e1, e2)


@pytest.mark.parametrize("ctrl", CTRLS)
def test_blocked_path_is_taken(torch_gpu, ctrl):
    """65 ticks are 3 step launches at window 32 and 65 with the window off; the same state and
    rewards either way."""
    torch = torch_gpu
    from mdr_amd.environment import ACTION_MODES

    n, T = 4099, 65
    e1, e2 = _pair(n)
    e2.shard.set_rollout_window(0)
    r1 = torch.empty((T, n), dtype=torch.float64, device="cuda")
    r2 = torch.empty_like(r1)
    ms1, l1 = e1.shard.time_step_kernels(e1.driver_window(T), None, 0, ACTION_MODES[ctrl], r1, n)
    ms2, l2 = e2.shard.time_step_kernels(e2.driver_window(T), None, 0, ACTION_MODES[ctrl], r2, n)
    assert (l1, l2) == (3, T) and ms1 > 0.0 and ms2 > 0.0
    torch.cuda.synchronize()
    s1, s2 = e1.shard.host_state(), e2.shard.host_state()
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k], err_msg=k)
    assert torch.equal(r1, r2)


@pytest.mark.parametrize("name,ctrl", [("c1_sin_dbbc", "deadband_bangbang"), ("fixed_steps_bbc", "bangbang")])
def test_reference_goldens_as_rollouts(torch_gpu, name, ctrl):
    """The reference's bang-bang trajectories as rollouts in chunks of 37 ticks: every reward row,
    and at each chunk's end the FSM state, temperatures and cluster power."""
    d, meta = gu.traj(name)
    assert meta["controller"] == {"deadband_bangbang": "deadband_bbc", "bangbang": "bbc"}[ctrl]
    props = gu.props_from_overrides(meta["overrides"])
    env = _make_env(props, meta["seed"], meta["resets"])
    T = meta["T"]
    t0 = 0
    while t0 < T:
        k = min(CHUNK, T - t0)
        R = env.rollout(k, action_mode=ctrl).cpu().numpy()
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


def test_fallback_mixture_golden_config(torch_gpu):
    """n64_mixture_2d's configuration (mixture penalty, deadband form): the per-tick form inside
    the call == the twin's loop."""
    torch = torch_gpu
    d, meta = gu.traj("n64_mixture_2d")
    props = gu.props_from_overrides(meta["overrides"])
    e1 = _make_env(props, meta["seed"], meta["resets"])
    e2 = _make_env(props, meta["seed"], meta["resets"])
    r1 = e1.rollout(meta["T"], action_mode="deadband_bangbang").cpu().numpy()
    r2 = _loop(e2, meta["T"], "deadband_bangbang")
    np.testing.assert_array_equal(r1, r2)
    _same_state(torch, e1, e2)
    np.testing.assert_allclose(r1, d["traj_reward"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("pmode,ctrl", [("common_L2", "deadband_bangbang"), ("common_max_error", "bangbang")])
def test_fallback_common_penalties(torch_gpu, pmode, ctrl):
    torch = torch_gpu
    n, ticks = 513, 33
    e1, e2 = _pair(n, pmode)
    for rep in range(2):
        r1 = e1.rollout(ticks, action_mode=ctrl).cpu().numpy()
        r2 = _loop(e2, ticks, ctrl)
        np.testing.assert_array_equal(r1, r2, err_msg=f"rollout {rep}")
        _same_state(torch, e1, e2)


@pytest.mark.parametrize("ctrl", CTRLS)
def test_fallback_five_capacity_classes(torch_gpu, ctrl):
    """More capacity classes than the window kernels hold: one step launch per tick."""
    torch = torch_gpu
    from mdr_amd.environment import ACTION_MODES

    n, ticks = 513, 33
    caps = {"cluster_prop.house_prop.hvac_prop.noise_prop.cooling_capacity_list": [10000, 12500, 15000, 17500, 20000]}
    e1, e2 = _pair(n, extra=caps)
    assert len(np.unique(e1.shard.host_params()["cap_idx"])) == 5
    r1 = e1.rollout(ticks, action_mode=ctrl).cpu().numpy()
    r2 = _loop(e2, ticks, ctrl)
    np.testing.assert_array_equal(r1, r2)
    _same_state(torch, e1, e2)
    rw = torch.empty((ticks, n), dtype=torch.float64, device="cuda")
    _ms, launches = e1.shard.time_step_kernels(e1.driver_window(ticks), None, 0, ACTION_MODES[ctrl], rw, n)
    assert launches == ticks
    np.testing.assert_array_equal(rw.cpu().numpy(), _loop(e2, ticks, ctrl))


@pytest.mark.parametrize("ctrl", CTRLS)
def test_one_row_rewards(torch_gpu, ctrl):
    """A 1-D [N] reward buffer that every tick overwrites holds the last tick's rewards (two
    windows: the first one's rows are never finalised)."""
    torch = torch_gpu
    n, ticks = 513, 40
    e1, e2 = _pair(n)
    row = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    out = e1.rollout(ticks, action_mode=ctrl, rewards=row)
    assert out.data_ptr() == row.data_ptr()
    r2 = _loop(e2, ticks, ctrl)
    np.testing.assert_array_equal(row.cpu().numpy(), r2[ticks - 1])
    _same_state(torch, e1, e2)


@pytest.mark.parametrize("ctrl", CTRLS)
def test_interleaved_with_steps_and_random_rollouts(torch_gpu, ctrl):
    """rollout -> step_tensor(bang-bang) -> rollout(random) -> rollout(bang-bang) against a twin
    doing the same ticks one by one (the random rollout in the exact thermal form, which is the
    one-tick kernels' bit for bit)."""
    torch = torch_gpu
    from mdr_amd import _lib as L

    n = 4099
    e1, e2 = _pair(n)
    e1.shard.set_option("window_thermal", L.THERMAL_EXACT)
    got = [e1.rollout(33, action_mode=ctrl).cpu().numpy(), _loop(e1, 2, ctrl),
           e1.rollout(10, action_mode="random").cpu().numpy(), e1.rollout(40, action_mode=ctrl).cpu().numpy()]
    want = [_loop(e2, 33, ctrl), _loop(e2, 2, ctrl), _loop(e2, 10, "random", lookahead=False), _loop(e2, 40, ctrl)]
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"part {i}")
    _same_state(torch, e1, e2)


@pytest.mark.parametrize("ctrl", CTRLS)
def test_graph_replay_equals_direct(torch_gpu, ctrl):
    """use_graph=True three times (one capture, then replays; the capture guard admits no memset
    node) against the directly launched twin."""
    torch = torch_gpu
    n, ticks = 4099, 65
    e1, e2 = _pair(n)
    buf = torch.empty((ticks, n), dtype=torch.float64, device="cuda")
    g0 = e1.shard.graph_info()
    for rep in range(3):
        r1 = e1.rollout(ticks, action_mode=ctrl, rewards=buf, use_graph=True).cpu().numpy()
        r2 = e2.rollout(ticks, action_mode=ctrl).cpu().numpy()
        np.testing.assert_array_equal(r1, r2, err_msg=f"call {rep}")
        _same_state(torch, e1, e2)
    g1 = e1.shard.graph_info()
    assert g1["rollout_graphs"] - g0["rollout_graphs"] == 1 and g1["rollout_launches"] - g0["rollout_launches"] == 3
