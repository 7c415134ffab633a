"""``Environment.rollout_returns`` (mdr_rollout_returns) against a twin environment
from the same seed that runs ``rollout`` into 2-D reward rows with the same calls.

After every stage t_air, t_mass, the FSM words, P, tick and date are ``==`` the twin's.  The returns:
* open-loop sources and the one-launch-per-tick sequence: ``==`` the NumPy row form
  ``ret = ret + w[t] * rows[t]`` over the twin's rows (tests/returns_np.py);
* closed-loop windows: within ``2 (T + 8) 2^-53 |ret_rows|`` per house after T accumulated ticks
  (derived in returns_np.py; shown on the oracle alone in test_returns_cpu.py), and two runs ``==``.

Sizes: 1 house (one lane), 129 (a ragged second tile), 257 (two tiles and one house), 2,085 (five
blocks, the last ragged).  Script per case, ``returns`` pre-filled with non-zero values of the
rewards' sign and ``weight0`` carried from call to call: 70 ticks at window 32 (the KA window, then a
group of two), 37 at window 7 (KA, a group of four, one more), 5 ticks, 1 tick."""
import random

import numpy as np
import pytest

import golden_util as gu
import returns_np as RN
from bangbang_inputs import CTRLS, SEED, overrides

pytestmark = pytest.mark.gpu

SIZES = [1, 129, 257, 2085]
SCRIPT = [(70, 32), (37, 7), (5, 7), (1, 7)]  # (ticks, rollout window)
GENERAL = {"cluster_prop.house_prop.deadband": 0.5, "reward_prop.norm_temp": 2.0}  # not the SIMPLE reward


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _envs(n, k=2, extra=None, thermal=None, group=None, synthetic=True, seed=SEED):
    from mdr_amd import _lib as L
    from mdr_amd.environment import Environment

    ov = {"cluster_prop.nb_agents": n, "power_grid_prop.signal_properties.mode": "sinusoidals"}
    ov.update(extra or {})
    props = gu.props_from_overrides(ov)
    pop = {"population": "synthetic", "seed": 77} if synthetic else {}
    out = [Environment(props, rng=random.Random(seed), **pop) for _ in range(k)]
    for e in out:
        if thermal is not None:
            e.shard.set_option("window_thermal", {"exact": L.THERMAL_EXACT, "affine": L.THERMAL_AFFINE}[thermal])
        if group is not None:
            e.shard.set_option("window_group", group)
    return out


def _same_state(torch, e1, e2, what=""):
    torch.cuda.synchronize()
    s1, s2 = e1.shard.host_state(), e2.shard.host_state()
    for k in s1:
        assert np.array_equal(s1[k], s2[k], equal_nan=True), (what, k)
    assert torch.equal(e1.shard.hvac, e2.shard.hvac), what
    p1, p2 = e1._cluster_power(), e2._cluster_power()
    assert p1 == p2 or (p1 != p1 and p2 != p2), what
    assert e1._tick == e2._tick and e1.date_time == e2.date_time, what


def _prefill(torch, n):
    return -(1.0 + 0.001 * torch.arange(n, dtype=torch.float64, device="cuda"))


def _actions(torch, ticks, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((ticks, n), device="cuda", generator=g) < 0.5).to(torch.uint8)


def _run_script(torch, env, twin, mode, gamma, check=None, script=SCRIPT, windows=True):
    """The script on env (rollout_returns) and twin (rollout into rows).  Returns the device
    returns, the NumPy row form over the twin's rows and the ticks accumulated; ``check(ret, ref,
    T)`` after every stage."""
    n = env.n_local
    ret = _prefill(torch, n)
    ref = ret.cpu().numpy().copy()
    w0, done = 0.75, 0
    for ticks, win in script:
        if windows:
            env.shard.set_rollout_window(win), twin.shard.set_rollout_window(win)
        acts = _actions(torch, ticks, n, 100 + done) if mode == "buffer" else None
        w = RN.weights(w0, gamma, ticks)
        rows = twin.rollout(ticks, actions=acts, action_mode=mode)
        w_next = env.rollout_returns(ticks, ret, gamma=gamma, weight0=w0, actions=acts, action_mode=mode)
        assert w_next == w[ticks]
        ref = RN.row_form(ref, w, rows.cpu().numpy())
        done += ticks
        _same_state(torch, env, twin, (mode, ticks, win))
        if check is not None:
            check(ret.cpu().numpy(), ref, done)
        w0 = w_next
    return ret, ref, done


def _equal(ret, ref, T):
    assert np.array_equal(ret, ref, equal_nan=True), (T, np.flatnonzero(ret != ref)[:8])


@pytest.mark.parametrize("gamma", [1.0, 0.99])
@pytest.mark.parametrize("general", [False, True], ids=["simple", "general"])
@pytest.mark.parametrize("thermal", ["affine", "exact"])
@pytest.mark.parametrize("mode", ["random", "always_on", "buffer"])
def test_open_loop_returns_are_the_row_form(torch_gpu, mode, thermal, general, gamma):
    """k_step_group_ret: returns == the NumPy loop over the twin's rows, bit for bit, at every size."""
    from mdr_amd import _lib as L

    for n in SIZES:
        env, twin = _envs(n, extra=GENERAL if general else None, thermal=thermal)
        assert env.shard.rollout_returns_path(L.ACT_RANDOM) == 0
        _run_script(torch_gpu, env, twin, mode, gamma, check=_equal)


@pytest.mark.parametrize("mode", ["random", "buffer"])
def test_exact_form_is_independent_of_window_group_and_fallback(torch_gpu, mode):
    """EXACT thermal form: the same returns, bit for bit, at window 32, 7 and 0 (one launch per tick)
    and under MDR_OPT_WINDOW_GROUP 0, 2 and 4."""
    torch = torch_gpu
    n = 257
    res = []
    for win, group in ((32, 4), (7, 4), (0, 4), (7, 0), (7, 2), (32, 0)):
        (env,) = _envs(n, k=1, thermal="exact", group=group)
        env.shard.set_rollout_window(win)
        ret = _prefill(torch, n)
        w0 = 1.0
        for ticks in (70, 37, 1):
            acts = _actions(torch, ticks, n, ticks) if mode == "buffer" else None
            w0 = env.rollout_returns(ticks, ret, gamma=0.99, weight0=w0, actions=acts, action_mode=mode)
        torch.cuda.synchronize()
        res.append(((win, group), ret.cpu().numpy(), env.shard.host_state()))
    for what, ret, st in res[1:]:
        assert np.array_equal(ret, res[0][1]), what
        for k in st:
            assert np.array_equal(st[k], res[0][2][k]), (what, k)


@pytest.mark.parametrize("deadband", [0.0, 0.5])
@pytest.mark.parametrize("thermal", ["exact", "affine"])
def test_returns_off_the_fast_range(torch_gpu, thermal, deadband):
    """test_division_gpu's case — Ua = 1e-9 (params_ok false: IEEE division) and a house at 3e6 degC —
    through both thermal forms: returns == the row form of the twin's rows (equal_nan)."""
    torch = torch_gpu
    n = 257
    env, twin = _envs(n, extra={"cluster_prop.house_prop.deadband": deadband}, thermal=thermal, seed=2)
    for e in (env, twin):
        e.shard.ua[17] = 1e-9
        e.shard.t_air[130] = 3.0e6
        e.shard.params_changed()
    _run_script(torch, env, twin, "random", 0.99, check=_equal, script=[(40, 7), (5, 7)])


@pytest.mark.parametrize("gamma", [1.0, 0.99])
@pytest.mark.parametrize("ctrl", CTRLS)
def test_closed_loop_returns_within_the_bound(torch_gpu, ctrl, gamma):
    """k_step_closed's ClosedRet form + k_closed_return: state == the twin's; returns within
    2 (T + 8) 2^-53 |ret_rows| per house after every stage; a second run gives the same bits."""
    from mdr_amd import _lib as L

    torch = torch_gpu
    for n in SIZES:
        worst = [0.0]

        def bounded(ret, ref, T):
            assert np.all(ref < 0)
            err, lim = np.abs(ret - ref), RN.bound(T, ref)
            worst[0] = max(worst[0], float(np.max(err / lim)))
            print(f"{ctrl} gamma={gamma} n={n} T={T}: max err / bound = {np.max(err / lim):.3f}")
            assert np.all(err <= lim), (T, np.flatnonzero(err > lim)[:8])

        env, twin = _envs(n, extra=overrides(n), synthetic=False)
        assert env.shard.rollout_returns_path(L.ACT_BANGBANG) == 1
        ret1, _, _ = _run_script(torch, env, twin, ctrl, gamma, check=bounded)
        env2, twin2 = _envs(n, extra=overrides(n), synthetic=False)
        ret2, _, _ = _run_script(torch, env2, twin2, ctrl, gamma)
        assert torch.equal(ret1, ret2)


@pytest.mark.parametrize("case", ["common_L2_bangbang", "common_L2_random_window_0", "five_classes", "window_0_bangbang"])
def test_per_tick_sequence_is_the_row_form(torch_gpu, case):
    """Path 2 (k_return_acc behind each tick's final reward): a common penalty mode, five capacity
    classes, the window off.  returns == the row form of the twin's rows."""
    from mdr_amd.environment import ACTION_MODES

    torch = torch_gpu
    caps = {"cluster_prop.house_prop.hvac_prop.noise_prop.cooling_capacity_list": [10000, 12500, 15000, 17500, 20000]}
    extra, mode, win0, windows = {
        "common_L2_bangbang": (overrides(0, "common_L2"), "bangbang", False, True),
        "common_L2_random_window_0": ({"reward_prop.penalty_props.mode": "common_L2"}, "random", True, False),
        "five_classes": (caps, "random", False, False),  # (no window with more than four classes)
        "window_0_bangbang": (overrides(0), "deadband_bangbang", True, False),
    }[case]
    for n in (129, 2085):
        ov = dict(extra)
        ov["cluster_prop.nb_agents"] = n
        env, twin = _envs(n, extra=ov, synthetic=False)
        if win0:
            env.shard.set_rollout_window(0), twin.shard.set_rollout_window(0)
        assert env.shard.rollout_returns_path(ACTION_MODES[mode]) == 2
        _run_script(torch, env, twin, mode, 0.99, check=_equal, script=[(9, 7), (1, 7)], windows=windows)


def test_paths(torch_gpu):
    from mdr_amd import _lib as L

    (env,) = _envs(129, k=1)
    sh = env.shard
    assert [sh.rollout_returns_path(m) for m in (L.ACT_RANDOM, L.ACT_ALWAYS_ON, L.ACT_BUFFER)] == [0, 0, 0]
    assert [sh.rollout_returns_path(m) for m in (L.ACT_BANGBANG, L.ACT_DEADBAND_BANGBANG)] == [1, 1]
    sh.set_rollout_window(0)
    assert [sh.rollout_returns_path(m) for m in (L.ACT_RANDOM, L.ACT_BANGBANG)] == [2, 2]
    (env,) = _envs(129, k=1, extra={"reward_prop.penalty_props.mode": "mixture"})
    assert [env.shard.rollout_returns_path(m) for m in (L.ACT_RANDOM, L.ACT_BANGBANG)] == [2, 2]
    with pytest.raises(L.MdrError, match="MDR_EARG"):
        env.shard.rollout_returns_path(99)


def test_context_with_a_communicator_is_refused(torch_gpu):
    """mdr_comm_host attached: MDR_ESTATE naming the entry point; state and returns unchanged."""
    from mdr_amd import _lib as L

    torch = torch_gpu
    (env,) = _envs(129, k=1)
    sh = env.shard
    keep = (L.HOST_ALLREDUCE_FN(lambda *a: 0), L.HOST_SENDRECV_FN(lambda *a: 0))
    L.check(sh.lib.mdr_comm_host(sh.ctx, 1, 0, keep[0], keep[1], None), "mdr_comm_host")
    ticks = env.driver_window(3)
    ret = _prefill(torch, 129)
    before = (sh.t_air.clone(), sh.t_mass.clone(), sh.hvac.clone(), ret.clone())
    with pytest.raises(L.MdrError, match="MDR_ESTATE") as ei:
        sh.rollout_returns(ticks, None, 0, L.ACT_RANDOM, np.ones(3), ret)
    assert "mdr_rollout_returns" in str(ei.value)
    torch.cuda.synchronize()
    for a, b in zip(before, (sh.t_air, sh.t_mass, sh.hvac, ret)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("controller", ["random", "deadband_bangbang"])
def test_controller_returns_equals_a_hand_run_twin(torch_gpu, controller):
    import copy

    from mdr_amd import services

    torch = torch_gpu
    n, ticks = 257, 40
    env, other = _envs(n, k=2, extra=overrides(n), synthetic=False)  # (the same seed: the same RNG draws)
    hand = copy.deepcopy(other)
    facts = (env.shard.t_air.clone(), env._tick, env.date_time)
    returns, means = services.controller_returns(env, controller, ticks, gamma=1.0)
    hand.reset(return_obs=False)
    ret = torch.zeros(n, dtype=torch.float64, device="cuda")
    hand.rollout_returns(ticks, ret, action_mode=controller)
    assert torch.equal(returns, ret)
    assert means == {"Mean test return": float(ret.mean().item()) / ticks}
    assert torch.equal(env.shard.t_air, facts[0]) and (env._tick, env.date_time) == facts[1:]  # env untouched
