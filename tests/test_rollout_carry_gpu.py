"""Direct rollouts whose last step launch counts the next call's first group of windows (mdr.h
MDR_OPT_ROLLOUT_CARRY): twin environments from the same seed, A with the option on, B
with it off (every call counts its own first window), and a third whose calls replay the captured
graph.  Every comparison is `==` on bits after every call: rewards, the state (T, Tm, on, lock, sso),
the last P.  The counters (Shard.carry_info) are asserted, so the carried path really ran.
"""
import random

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

CALLS = 6
# A's counters behind six equal consecutive calls: the second call is the first that continues one, so
# calls 2..6 count ahead and calls 3..6 start from such a count
SIX = {"speculated": 5, "consumed": 4, "dropped": 0}
NONE = {"speculated": 0, "consumed": 0, "dropped": 0}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _envs(n, carries, thermal="affine", window=7, group=4, seed=3):
    """One environment per carry option value, all from the same seed."""
    from mdr_amd import _lib as L
    from mdr_amd.environment import Environment

    props = gu.props_from_overrides({"cluster_prop.nb_agents": n, "power_grid_prop.signal_properties.mode": "sinusoidals"})
    out = []
    for carry in carries:
        e = Environment(props, rng=random.Random(seed), population="synthetic", seed=77)
        e.shard.set_option("window_thermal", {"exact": L.THERMAL_EXACT, "affine": L.THERMAL_AFFINE}[thermal])
        e.shard.set_option("window_group", group)
        e.shard.set_option("rollout_carry", carry)
        e.shard.set_rollout_window(window)
        out.append(e)
    return out


def _results(torch, e, r):
    torch.cuda.synchronize()
    out = dict(e.shard.host_state())
    out["reward"] = r.cpu().numpy()
    out["P"] = np.float64(e.shard.p_dev.item())
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _counters(e):
    c = e.shard.carry_info()
    return {k: c[k] for k in ("speculated", "consumed", "dropped")}


def _call(torch, e, ticks, mode="random", one_row=False, **kw):
    rew = torch.empty(e.shard.n, dtype=torch.float64, device=e.shard.device) if one_row else None
    return _results(torch, e, e.rollout(ticks, action_mode=mode, rewards=rew, **kw))


def _six_calls(torch, n, ticks, window, mode, thermal, one_row=False, prepare=None):
    a, b, g = _envs(n, (1, 0, 1), thermal, window)
    for e in (a, b, g):
        if prepare:
            prepare(e)
    for call in range(CALLS):
        ra = _call(torch, a, ticks, mode, one_row)
        rb = _call(torch, b, ticks, mode, one_row)
        rg = _call(torch, g, ticks, mode, one_row, use_graph=True)
        _assert_same(ra, rb, ("carry 1 against 0", call))
        _assert_same(ra, rg, ("carry 1 against the graph", call))
    assert _counters(a) == SIX
    assert _counters(b) == NONE
    assert _counters(g) == NONE  # (a replayed graph never carries)
    return ra


@pytest.mark.parametrize("thermal", ["affine", "exact"])
@pytest.mark.parametrize("mode", ["random", "always_on"])
@pytest.mark.parametrize("n", [1, 129, 257])
def test_carry_equals_no_carry(torch_gpu, n, mode, thermal):
    """40 ticks at window 7: six windows (7, 7, 7, 7, 6, 6) in groups 4 + 2, the next call's first four
    counted by the {w4, w5} launch, so the slots run on across the call boundary (6 windows in 8
    slots).  n = 1, 129, 257: a ragged last tile, one and two blocks' tiles."""
    _six_calls(torch_gpu, n, 40, 7, mode, thermal)


@pytest.mark.parametrize("thermal", ["affine", "exact"])
@pytest.mark.parametrize("mode", ["random", "always_on"])
@pytest.mark.parametrize("ticks,window", [(7, 7), (20, 32)])
def test_carry_single_window_calls(torch_gpu, ticks, window, mode, thermal):
    """One window per call: the first speculating launch is the KA launch itself, and every carried
    call is one reduce and one staged group launch of a single window."""
    _six_calls(torch_gpu, 257, ticks, window, mode, thermal)


@pytest.mark.parametrize("thermal", ["affine", "exact"])
@pytest.mark.parametrize("mode", ["random", "always_on"])
def test_carry_one_reward_row(torch_gpu, mode, thermal):
    """A 1-D rewards buffer that every tick overwrites (rew_stride 0)."""
    _six_calls(torch_gpu, 257, 40, 7, mode, thermal, one_row=True)


def _break_n(torch, e):
    return _call(torch, e, 23)


def _break_buffer(torch, e):
    g = torch.Generator(device="cuda").manual_seed(11)
    acts = (torch.rand((40, e.shard.n), device="cuda", generator=g) < 0.5).to(torch.uint8)
    return _results(torch, e, e.rollout(40, actions=acts, action_mode="buffer"))


def _break_state_write(torch, e):
    e.load_state_dict(e.state_dict())


def _break_step(torch, e):
    e.step_tensor(None, action_mode="random")


def _break_returns(torch, e):
    ret = torch.zeros(e.shard.n, dtype=torch.float64, device=e.shard.device)
    e.rollout_returns(40, ret, gamma=0.99)
    return {"returns": ret.cpu().numpy()}


BREAKS = {
    "n 40 -> 23 -> 40": _break_n,
    "source random -> always_on": lambda torch, e: None,  # (the calls behind it run always_on)
    "one buffer call": _break_buffer,
    "set_rollout_window(5)": lambda torch, e: e.shard.set_rollout_window(5),
    "window group 2": lambda torch, e: e.shard.set_option("window_group", 2),
    "load_state_dict": _break_state_write,
    "one step_tensor tick": _break_step,
    "one rollout_returns call": _break_returns,
    "one use_graph call": lambda torch, e: _call(torch, e, 40, use_graph=True),
    "reset": lambda torch, e: e.reset(return_obs=False),
}


@pytest.mark.parametrize("what", list(BREAKS))
def test_carry_dropped_by(torch_gpu, what):
    """Three carried calls, then something that invalidates the count call 3 made for call 4, on both
    twins: the count is dropped once and the rest of the sequence still equals B bit for bit."""
    torch = torch_gpu
    a, b = _envs(257, (1, 0))
    for call in range(3):
        _assert_same(_call(torch, a, 40), _call(torch, b, 40), (what, call))
    assert _counters(a) == {"speculated": 2, "consumed": 1, "dropped": 0}
    ra, rb = BREAKS[what](torch, a), BREAKS[what](torch, b)
    if ra is not None:
        _assert_same(ra, rb, (what, "the break itself"))
    mode = "always_on" if what.startswith("source") else "random"
    for call in range(3, CALLS):
        _assert_same(_call(torch, a, 40, mode), _call(torch, b, 40, mode), (what, call))
    ca = _counters(a)
    assert ca["dropped"] == 1, (what, ca)
    assert ca["consumed"] >= 1 and ca["speculated"] >= ca["consumed"] + ca["dropped"], (what, ca)
    assert _counters(b) == NONE


@pytest.mark.parametrize("thermal", ["affine", "exact"])
def test_carry_non_finite_house(torch_gpu, thermal):
    """One house at T = inf: its wave takes the slow path in every window of every carried call."""
    def prepare(e):
        e.shard.t_air[130] = float("inf")

    last = _six_calls(torch_gpu, 257, 40, 7, "random", thermal, prepare=prepare)
    assert not np.isfinite(last["T"][130])
    assert np.isfinite(np.delete(last["T"], 130)).all()


@pytest.mark.parametrize("thermal", ["affine", "exact"])
def test_carry_off_the_fast_range(torch_gpu, thermal):
    """Ua = 1e-9 (params_ok false for the whole context: IEEE division in the window kernels) and one
    house at 3e6 degC, across carried calls."""
    def prepare(e):
        e.shard.ua[17] = 1e-9
        e.shard.t_air[130] = 3.0e6
        e.shard.params_changed()

    _six_calls(torch_gpu, 257, 40, 7, "random", thermal, prepare=prepare)
