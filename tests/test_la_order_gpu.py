"""Which blocks of a k_step_group launch run their FSM lookahead before their ticks (mdr.h
MDR_OPT_GROUP_LA_ORDER) must not move a bit: twin environments from one seed, one with
the option at 0 (every block counts last, the order before the option existed), one per pattern, and
one whose calls replay the captured graph (the k_step_window sequence, which the option does not
touch).  Six consecutive calls; after every call rewards, state (T, Tm, on, lock, sso) and the last P
are compared with `==` on bits.  The carry counters are asserted, so the carried path (where the half
of the group mask rows travels across the call boundary) really ran.
"""
import random

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

CALLS = 6
TICKS = 70  # window 32: one group of 24 / 23 / 23; window 8: nine windows, groups of 4, 4, 1 (the halves alternate)
SIX = {"speculated": 5, "consumed": 4, "dropped": 0}
NONE = {"speculated": 0, "consumed": 0, "dropped": 0}
# 1,500 houses: three blocks of 512, the last partial with a ragged last tile; blocks 0 and 2 count last
# and block 1 first under ALT1; a threshold of 1 or 2 blocks (value >> 8) splits the launch too
N = 1500


def _patterns():
    from mdr_amd import _lib as L

    return {"alt1": L.LA_ALT1, "before": L.LA_BEFORE, "alt1+tail": L.LA_ALT1 | L.LA_TAIL_BEFORE,
            "from block 1": 1 << 8, "from block 2": 2 << 8}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _env(n, order, thermal="affine", window=32, group=4, seed=3):
    from mdr_amd import _lib as L
    from mdr_amd.environment import Environment

    props = gu.props_from_overrides({"cluster_prop.nb_agents": n, "power_grid_prop.signal_properties.mode": "sinusoidals"})
    e = Environment(props, rng=random.Random(seed), population="synthetic", seed=77)
    e.shard.set_option("window_thermal", {"exact": L.THERMAL_EXACT, "affine": L.THERMAL_AFFINE}[thermal])
    e.shard.set_option("window_group", group)
    e.shard.set_option("group_la_order", order)
    e.shard.set_rollout_window(window)
    return e


def _bits(torch, x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x


def _results(torch, e, r):
    """Rewards stay on the device (compared there, on bits); the state and P come to the host."""
    torch.cuda.synchronize()
    out = dict(e.shard.host_state())
    out["P"] = np.float64(e.shard.p_dev.item())
    return out, r


def _assert_same(torch, a, b, what):
    (sa, ra), (sb, rb) = a, b
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), (what, k)
    assert ra.shape == rb.shape and torch.equal(_bits(torch, ra), _bits(torch, rb)), (what, "reward")


def _counters(e):
    c = e.shard.carry_info()
    return {k: c[k] for k in ("speculated", "consumed", "dropped")}


def _call(torch, e, ticks=TICKS, mode="random", acts=None, **kw):
    if mode == "buffer":
        return _results(torch, e, e.rollout(ticks, actions=acts[:ticks], action_mode="buffer", **kw))
    return _results(torch, e, e.rollout(ticks, action_mode=mode, **kw))


def _actions(torch, n, ticks=TICKS):
    g = torch.Generator(device="cuda").manual_seed(11)
    return (torch.rand((ticks, n), device="cuda", generator=g) < 0.5).to(torch.uint8)


def _six_calls(torch, n, orders, window, mode, thermal, group, prepare=None):
    """`orders`: the option values next to 0; every twin against option 0 after every call."""
    base, graph = _env(n, 0, thermal, window, group), _env(n, 0, thermal, window, group)
    twins = {k: _env(n, v, thermal, window, group) for k, v in orders.items()}
    acts = _actions(torch, n) if mode == "buffer" else None
    for e in [base, graph, *twins.values()]:
        if prepare:
            prepare(e)
    for call in range(CALLS):
        r0 = _call(torch, base, TICKS, mode, acts)
        _assert_same(torch, r0, _call(torch, graph, TICKS, mode, acts, use_graph=True), ("the graph", call))
        for k, e in twins.items():
            _assert_same(torch, r0, _call(torch, e, TICKS, mode, acts), (k, call))
    want = NONE if mode == "buffer" else SIX  # (a buffer source never carries: the next call's rows are unknown)
    for e in [base, *twins.values()]:
        assert _counters(e) == want
    assert _counters(graph) == NONE
    return r0


@pytest.mark.parametrize("group", [4, 3])
@pytest.mark.parametrize("thermal", ["affine", "exact"])
@pytest.mark.parametrize("mode", ["random", "always_on", "buffer"])
@pytest.mark.parametrize("window", [32, 8])
def test_orders_equal(torch_gpu, window, mode, thermal, group):
    _six_calls(torch_gpu, N, _patterns(), window, mode, thermal, group)


@pytest.mark.parametrize("n,order", [(4396, "LA_ALT8"), (131700, "LA_ALT256")])
@pytest.mark.parametrize("window", [32, 8])
def test_coarse_grains_equal(torch_gpu, n, order, window):
    """The smallest clusters at which both orders occur in one launch: runs of 8 blocks need 9 blocks
    (4,396 houses), runs of 256 need 257 (131,700); the last tile is ragged in both."""
    from mdr_amd import _lib as L

    _six_calls(torch_gpu, n, {order: getattr(L, order)}, window, "random", "affine", 4)


def _break_buffer(torch, e):
    return _call(torch, e, 40, "buffer", _actions(torch, e.shard.n, 40))


def _break_returns(torch, e):
    ret = torch.zeros(e.shard.n, dtype=torch.float64, device=e.shard.device)
    e.rollout_returns(40, ret, gamma=0.99)
    torch.cuda.synchronize()
    return {"returns": ret.cpu().numpy()}, ret


def _break_step(torch, e):
    e.step_tensor(None, action_mode="random")


def _break_reset(torch, e):
    e.reset(return_obs=False)


BREAKS = {
    "n 70 -> 23 -> 70": lambda torch, e: _call(torch, e, 23),
    "source random -> always_on": lambda torch, e: None,  # (the calls behind it run always_on)
    "one buffer call": _break_buffer,
    "set_rollout_window(5)": lambda torch, e: e.shard.set_rollout_window(5),
    "window group 2": lambda torch, e: e.shard.set_option("window_group", 2),
    "load_state_dict": lambda torch, e: e.load_state_dict(e.state_dict()),
    "one step_tensor tick": _break_step,
    "one rollout_returns call": _break_returns,
    "one use_graph call": lambda torch, e: _call(torch, e, TICKS, use_graph=True),
    "reset": _break_reset,
}


@pytest.mark.parametrize("what", list(BREAKS))
def test_half_reset_by(torch_gpu, what):
    """Window 8: a carried call makes three group launches, so the carried half is 1 behind the second
    call and keeps alternating.  Something between calls 3 and 4 drops the carried count on both twins;
    the calls behind it start from half 0 again and still equal option 0 bit for bit."""
    torch = torch_gpu
    from mdr_amd import _lib as L

    a, b = _env(N, L.LA_ALT1, window=8), _env(N, 0, window=8)
    for call in range(3):
        _assert_same(torch, _call(torch, a), _call(torch, b), (what, call))
    assert _counters(a) == {"speculated": 2, "consumed": 1, "dropped": 0}
    ra, rb = BREAKS[what](torch, a), BREAKS[what](torch, b)
    if ra is not None:
        _assert_same(torch, ra, rb, (what, "the break itself"))
    mode = "always_on" if what.startswith("source") else "random"
    for call in range(3, CALLS):
        _assert_same(torch, _call(torch, a, TICKS, mode), _call(torch, b, TICKS, mode), (what, call))
    ca = _counters(a)
    assert ca["dropped"] == 1, (what, ca)
    assert ca["consumed"] >= 1 and ca["speculated"] >= ca["consumed"] + ca["dropped"], (what, ca)
    assert _counters(b) == ca  # (option 0 carries the same way)


def test_option_change_drops_the_carry(torch_gpu):
    """A change of the option between two calls discards the carried count, like every other option."""
    torch = torch_gpu
    from mdr_amd import _lib as L

    a, b = _env(N, 0, window=8), _env(N, 0, window=8)
    for call in range(3):
        _assert_same(torch, _call(torch, a), _call(torch, b), call)
    a.shard.set_option("group_la_order", L.LA_ALT1)
    assert _counters(a)["dropped"] == 1 and a.shard.carry_info()["outstanding"] == 0
    for call in range(3, CALLS):
        _assert_same(torch, _call(torch, a), _call(torch, b), call)


def test_unknown_pattern_is_refused(torch_gpu):
    from mdr_amd._lib import MdrError

    e = _env(N, 0)
    for v in (5, 15, 32, 64, 128, -1):
        with pytest.raises(MdrError):
            e.shard.set_option("group_la_order", v)


@pytest.mark.parametrize("order", ["LA_ALT1", "LA_BEFORE"])
def test_returns_equal(torch_gpu, order):
    """k_step_group_ret shares the body (it keeps the one order: no reward rows to overlap with) and
    reads and writes the same two halves."""
    torch = torch_gpu
    from mdr_amd import _lib as L

    a, b = _env(N, getattr(L, order), window=8), _env(N, 0, window=8)
    for call in range(3):
        ra, rb = _break_returns(torch, a), _break_returns(torch, b)
        assert np.array_equal(ra[0]["returns"], rb[0]["returns"]), call
        _assert_same(torch, _call(torch, a), _call(torch, b), call)


@pytest.mark.parametrize("thermal", ["affine", "exact"])
def test_non_finite_house(torch_gpu, thermal):
    """One house at T = inf: its wave takes the slow path in every window, in both orders."""
    def prepare(e):
        e.shard.t_air[130] = float("inf")

    last, _ = _six_calls(torch_gpu, N, _patterns(), 32, "random", thermal, 4, prepare=prepare)
    assert not np.isfinite(last["T"][130])
    assert np.isfinite(np.delete(last["T"], 130)).all()
