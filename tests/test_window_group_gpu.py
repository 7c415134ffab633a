"""Directly launched window rollouts in groups (k_step_group, mdr.h MDR_OPT_WINDOW_GROUP: up to four
windows per step launch, state and coefficients loaded and formed once per group) against one
k_step_window launch per window (option 0) and against the captured graph's staged sequence.
Every comparison is `==` on bits: rewards [ticks, n], the state (T, Tm, on, lock, sso), the last P.
"""
import random

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

# (ticks, window): six windows of unequal sizes (7, 7, 7, 7, 6, 6) = groups {w0}, {w1..w4}, {w5} at
# option 4; four windows of 32 = {w0}, {w1..w3}; one window
SHAPES = [(40, 7), (128, 32), (20, 32)]


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _envs(n, options, thermal="affine", deadband=0.0, seed=3):
    """One environment per option value, all from the same seed."""
    from mdr_amd import _lib as L
    from mdr_amd.environment import Environment

    props = gu.props_from_overrides({"cluster_prop.nb_agents": n, "power_grid_prop.signal_properties.mode": "sinusoidals",
                                     "cluster_prop.house_prop.deadband": deadband})
    out = []
    for g in options:
        e = Environment(props, rng=random.Random(seed), population="synthetic", seed=77)
        e.shard.set_option("window_thermal", {"exact": L.THERMAL_EXACT, "affine": L.THERMAL_AFFINE}[thermal])
        e.shard.set_option("window_group", g)
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


def _actions(torch, mode, ticks, n):
    if mode != "buffer":
        return None
    g = torch.Generator(device="cuda").manual_seed(1000 * ticks + n)
    return (torch.rand((ticks, n), device="cuda", generator=g) < 0.5).to(torch.uint8)


@pytest.mark.parametrize("deadband", [0.0, 0.5])
@pytest.mark.parametrize("thermal", ["affine", "exact"])
@pytest.mark.parametrize("mode", ["random", "buffer", "always_on"])
@pytest.mark.parametrize("n", [1, 129, 257])
def test_group_equals_no_group(torch_gpu, n, mode, thermal, deadband):
    """Options 4, 3 and 2 against option 0 from the same seed, two consecutive calls per shape (the
    second starts from carried state), the shapes back to back on the same environments: a full
    group, a remainder group and unequal window sizes inside a group (40 ticks at window 7), four
    windows of 32, a single window.  n = 1, 129, 257: a ragged last tile, one and two blocks' tiles.
    Deadband 0 runs the SIMPLE reward, 0.5 the general one."""
    torch = torch_gpu
    opts = (0, 4, 3, 2)
    envs = _envs(n, opts, thermal, deadband)
    for ticks, win in SHAPES:
        acts = _actions(torch, mode, ticks, n)
        for e in envs:
            e.shard.set_rollout_window(win)
        for call in range(2):
            res = [_results(torch, e, e.rollout(ticks, actions=acts, action_mode=mode)) for e in envs]
            for g, r in zip(opts[1:], res[1:]):
                _assert_same(r, res[0], (ticks, win, call, g))


@pytest.mark.parametrize("thermal", ["affine", "exact"])
@pytest.mark.parametrize("mode", ["random", "buffer", "always_on"])
def test_group_equals_graph(torch_gpu, mode, thermal):
    """The grouped direct sequence against the captured graph (the unchanged staged sequence:
    k_count_window, then k_win_reduce + k_step_window per window), 257 houses x 40 ticks at window 7."""
    torch = torch_gpu
    n, ticks = 257, 40
    e1, e2 = _envs(n, (4, 4), thermal)
    acts = _actions(torch, mode, ticks, n)
    for e in (e1, e2):
        e.shard.set_rollout_window(7)
    for call in range(2):
        a = _results(torch, e1, e1.rollout(ticks, actions=acts, action_mode=mode))
        b = _results(torch, e2, e2.rollout(ticks, actions=acts, action_mode=mode, use_graph=True))
        _assert_same(a, b, call)


@pytest.mark.parametrize("thermal", ["affine", "exact"])
def test_group_window_boundary_non_finite(torch_gpu, thermal):
    """One house starts at T = inf: its wave takes the slow path (plain arithmetic) and keeps
    non-finite temperatures across every window boundary, where k_step_group forms win_finite again
    as each k_step_window launch does.  Option 4 and option 0 agree bit for bit (NaNs as equal)."""
    torch = torch_gpu
    n, ticks = 257, 40
    e4, e0 = _envs(n, (4, 0), thermal)
    for e in (e4, e0):
        e.shard.set_rollout_window(7)
        e.shard.t_air[130] = float("inf")
    for call in range(2):
        a = _results(torch, e4, e4.rollout(ticks, action_mode="random"))
        b = _results(torch, e0, e0.rollout(ticks, action_mode="random"))
        assert not np.isfinite(a["T"][130])
        assert np.isfinite(np.delete(a["T"], 130)).all()
        _assert_same(a, b, call)
