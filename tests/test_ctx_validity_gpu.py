"""The host library's beliefs about derived device state (counts, greedy keys, histogram,
key maps, fused products, window slots, an early first-window count) across interleavings of entry
points on ONE environment, against a twin that a stale belief cannot fool:

* greedy cases (3,001 houses): the twin runs the same calls with the ``greedy_sort`` option set, the
  full-sort form, which has no keys, histogram or maps;
* count and window cases (257 houses: two 128-house window tiles, the second ragged): the twin steps
  ``step_tensor`` with the counts recomputed every tick (``lookahead=None``), or, for an early count
  (``shard.rollout_begin``), makes the same calls without ever beginning.

Rewards, actions, P and the final state are compared with ==.  Each case first asserts that it is not
degenerate: mixed actions (for an in-kernel source: a mixed ON mask), for the greedy cases at least
one house whose decision changes across the interleaving, and on the CPU the oracle's controller
(greedy, bang-bang) on the twin's input state decides a mixed vector.  The interleavings other tests
drive already are named in DESIGN §7.2 instead."""
import random

import numpy as np
import pytest

import golden_util as gu
from oracle import env_np as O

pytestmark = pytest.mark.gpu

N_WIN, N_GREEDY = 257, 3001


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _env(n, seed, **over):
    from mdr_amd.environment import Environment

    ov = {"cluster_prop.nb_agents": n, "power_grid_prop.signal_properties.mode": "sinusoidals"}
    ov.update(over)
    return Environment(gu.props_from_overrides(ov), rng=random.Random(seed), population="synthetic", seed=seed)


def _greedy_tick(env, out):
    """greedy_actions -> step_tensor(ctrl='greedy_keys'); the decisions and rewards appended to out."""
    g = env.greedy_actions()
    r = env.step_tensor(g, ctrl="greedy_keys")
    out += [g.clone(), r.clone()]


def _end(env, out):
    out.append(env.cluster.current_power_consumption)
    return out, env.shard.host_state()


def _mixed(t):
    s = int(t.sum())
    return 0 < s < t.numel()


def _same(torch, a, b):
    (oa, sa), (ob, sb) = a, b
    assert len(oa) == len(ob)
    for i, (x, y) in enumerate(zip(oa, ob)):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y), i
        else:
            assert x == y, i
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)


def _oracle_greedy_mixed(env):
    """The inputs, on the CPU: the oracle's greedy decision on the environment's current state and signal
    switches some houses on and leaves some off."""
    st, prm = env.shard.host_state(), env.shard.host_params()
    caps = np.array(env._cap_values, np.float64)[prm["cap_idx"]]
    ref = O.greedy(st["T"], prm["target"], caps, env.init_props.cluster_prop.house_prop.hvac_prop.cop, st["lock"],
                   float(env.power_grid.current_signal))
    assert 0 < int(ref.sum()) < ref.size, "the oracle's greedy decision on this state is all on or all off"


def _greedy_not_degenerate(acts):
    """acts: the twin's uint8 decision vectors in call order."""
    assert all(_mixed(a) for a in acts)
    assert any(bool((a != acts[0]).any()) for a in acts[1:]), "no house ever changes its decision"


def _greedy_twins(seed, **over):
    a, b = _env(N_GREEDY, seed, **over), _env(N_GREEDY, seed, **over)
    b.shard.set_option("greedy_sort", 1)
    _oracle_greedy_mixed(b)
    return a, b


def _decisions(torch, out):
    return [x for x in out if isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and x.dim() == 1]


def test_keys_do_not_survive_a_rollout(torch_gpu):
    """greedy_actions -> step(ctrl='greedy_keys') x 3, rollout(5, 'random') at window 7, then greedy
    again: the keys the third step's epilogue wrote belong to a state the rollout replaced."""
    torch = torch_gpu
    res = []
    for e in _greedy_twins(5):
        e.shard.set_rollout_window(7)
        out = []
        for _ in range(3):
            _greedy_tick(e, out)
        out.append(e.rollout(5, action_mode="random").clone())
        _greedy_tick(e, out)
        res.append(_end(e, out))
    _greedy_not_degenerate(_decisions(torch, res[1][0]))
    _same(torch, *res)


def test_lookahead_counts_then_closed_rollout_then_buffer_step(torch_gpu):
    """step_tensor(lookahead='random') leaves counts ready; rollout(9, 'bangbang') (closed-loop windows
    of 5 + 4 ticks) replaces the state; the buffer step after it must count its own actions."""
    torch = torch_gpu
    a, b = _env(N_WIN, 7), _env(N_WIN, 7)
    a.shard.set_rollout_window(7)
    act = (torch.rand(N_WIN, device="cuda", generator=torch.Generator("cuda").manual_seed(3)) < 0.5).to(torch.uint8)
    assert _mixed(act)
    oa = [a.step_tensor(None, action_mode="random", lookahead="random").clone()]
    oa.append(a.rollout(9, action_mode="bangbang").clone())
    oa.append(a.step_tensor(act).clone())
    ob = [b.step_tensor(None, action_mode="random").clone()]
    ref = O.bangbang(b.shard.host_state()["T"], b.shard.host_params()["target"])  # (the inputs, on the CPU)
    assert 0 < int(ref.sum()) < ref.size, "the oracle's bang-bang decision on this state is all on or all off"
    ob.append(torch.stack([b.step_tensor(None, action_mode="bangbang").clone() for _ in range(9)]))
    mid = torch.from_numpy(b.shard.host_state()["on"])
    assert _mixed(mid), "the bang-bang ticks left every house in one state"
    ob.append(b.step_tensor(act).clone())
    _same(torch, _end(a, oa), _end(b, ob))


@pytest.mark.parametrize("follow", ["consumed", "mismatch", "step", "set_window"])
def test_early_count_then(torch_gpu, follow):
    """shard.rollout_begin for 9 ticks, then: the rollout it was begun for, a rollout of 8 ticks, a
    step, or set_rollout_window(5) and the rollout — and one more rollout behind each, which reads the
    window slots whatever the first call left in them.  The twin never began."""
    torch = torch_gpu
    from mdr_amd.environment import ACTION_MODES

    mode = ACTION_MODES["random"]

    def direct(e, k):  # the shard's call, without Environment.rollout's own early count
        ticks = e.driver_window(k)
        rew = torch.empty((k, N_WIN), dtype=torch.float64, device="cuda")
        e.shard.rollout(ticks, None, 0, mode, rew, N_WIN, False)
        e._P_dev_valid, e._counts_ready = True, 0
        return rew

    res = []
    for began in (True, False):
        e = _env(N_WIN, 11)
        e.shard.set_rollout_window(7)
        out = [e.step_tensor(None, action_mode="random").clone()]
        if began:
            e.shard.rollout_begin(9, e._tick, None, 0, mode)
        if follow == "consumed":
            out.append(direct(e, 9))
        elif follow == "mismatch":
            out.append(direct(e, 8))
        elif follow == "step":
            out.append(e.step_tensor(None, action_mode="random").clone())
        else:
            e.shard.set_rollout_window(5)
            out.append(direct(e, 9))
        out.append(e.rollout(9, action_mode="random").clone())
        res.append(_end(e, out))
    assert _mixed(torch.from_numpy(res[1][1]["on"]))
    _same(torch, *res)


def test_state_write_refits_the_maps(torch_gpu):
    """Greedy ticks, the state rewritten through the shard's tensors + params_changed() (air 9 K above
    target: keys far outside the fitted maps), greedy ticks again."""
    torch = torch_gpu
    from mdr_amd.shard import encode_hvac

    res = []
    for e in _greedy_twins(13):
        out = []
        for _ in range(3):
            _greedy_tick(e, out)
        sh = e.shard
        rs = np.random.RandomState(13)
        T = sh.host_params()["target"] + 9.0 + rs.normal(0.0, 1.0, N_GREEDY)
        lock = rs.rand(N_GREEDY) < 0.3
        sh.t_air.copy_(torch.from_numpy(T).cuda())
        sh.hvac.copy_(torch.from_numpy(encode_hvac(~lock & (rs.rand(N_GREEDY) < 0.5), lock,
                                                   rs.randint(0, 60, N_GREEDY))).cuda())
        sh.params_changed()
        _oracle_greedy_mixed(e)  # (the written state too)
        for _ in range(3):
            _greedy_tick(e, out)
        res.append(_end(e, out))
    _greedy_not_degenerate(_decisions(torch, res[1][0]))
    _same(torch, *res)


def test_fused_and_per_tick_forms_interleaved(torch_gpu):
    """gq_fused = 1: greedy_rollout(4), two per-tick greedy ticks, greedy_rollout(4); gq_fused = 0 and
    two more ticks: the fused products, the keys and the two forms' maps each belong to one state."""
    torch = torch_gpu
    res = []
    for k, e in enumerate(_greedy_twins(17)):
        if k == 0:
            e.shard.set_option("gq_fused", 1)
        out = []

        def roll():
            acts = torch.empty((4, N_GREEDY), dtype=torch.uint8, device="cuda")
            out.append(e.greedy_rollout(4, actions=acts)[1].clone())
            out.extend(acts[t].clone() for t in range(4))

        roll()
        for _ in range(2):
            _greedy_tick(e, out)
        roll()
        if k == 0:
            e.shard.set_option("gq_fused", 0)
        for _ in range(2):
            _greedy_tick(e, out)
        res.append(_end(e, out))
    _greedy_not_degenerate(_decisions(torch, res[1][0]))
    _same(torch, *res)


def test_greedy_stats_rollout_after_a_random_rollout(torch_gpu):
    """common_L2: rollout(6, 'random'), then greedy_rollout(6, stats=...) directly behind it."""
    torch = torch_gpu
    from mdr_amd.services import RolloutStats

    res = []
    for e in _greedy_twins(19, **{"reward_prop.penalty_props.mode": "common_L2"}):
        out = [e.rollout(6, action_mode="random").clone()]
        acts = torch.empty((6, N_GREEDY), dtype=torch.uint8, device="cuda")
        stats = RolloutStats(e, 6)
        out.append(e.greedy_rollout(6, actions=acts, stats=stats)[1].clone())
        out.extend(acts[t].clone() for t in range(6))
        res.append(_end(e, out))
    _greedy_not_degenerate(_decisions(torch, res[1][0]))
    _same(torch, *res)
