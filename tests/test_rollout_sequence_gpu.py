"""What each rollout launch sequencer of the host library issues, pinned through the numbers the
library already reports: the node count of the graph a first ``use_graph=True`` call captures (the
``guarded_nodes`` delta of ``Shard.graph_info()``) and the ``launches`` of ``Shard.time_step_kernels``.

257 houses (two tiles, the second ragged), 40 ticks at window 7: nw = 6 windows of 7, 7, 7, 7, 6, 6
ticks.  The documented sequences (DESIGN §"Launch sequence"):

* open-loop windows (window_launches): the first window's k_count_window, then per window
  k_win_reduce + k_step_window: 1 + 2 nw nodes; a common penalty mode adds k_win_pen_reduce +
  k_win_reward_common per finished window (every window with a row per tick: 1 + 4 nw; one shared
  reward row: the last window only, 1 + 2 nw + 2);
* closed-loop windows (closed_launches): per window k_step_closed + k_win_reduce + k_closed_reward
  (3 nw; one shared row finalises the last window only: 2 nw + 1), + k_closed_stats with stats rows
  (4 nw);
* window 0: one step launch per tick behind the slabs' zeroing kernel and the first tick's
  k_power_counts.

Sharded sequences (per-window allreduce, count-ahead pipeline, begun single window) need a process
group: tests/test_distributed_gpu.py compares them bit for bit.
"""
import random

import pytest

import golden_util as gu
from bangbang_inputs import SEED, overrides

pytestmark = pytest.mark.gpu

N, TICKS, WIN = 257, 40, 7
NW = 6  # ceil(40 / 7)

# (case id, penalty mode, action source, reward dims, stats rows, window, graph nodes, step launches or None)
CASES = [
    ("random_2d", "individual_L2", "random", 2, False, WIN, 1 + 2 * NW, NW),
    ("common_2d", "common_L2", "random", 2, False, WIN, 1 + 4 * NW, None),
    ("common_1d", "common_L2", "random", 1, False, WIN, 1 + 2 * NW + 2, None),
    ("bangbang_2d", "individual_L2", "bangbang", 2, False, WIN, 3 * NW, NW),
    ("bangbang_1d", "individual_L2", "bangbang", 1, False, WIN, 2 * NW + 1, None),
    ("bangbang_stats", "individual_L2", "bangbang", 2, True, WIN, 4 * NW, None),
    # window 0: k_zero_u64, tick 0's k_power_counts (the lookahead counts every later tick), 40 steps;
    # the node count is what this test measured on the commit before the sequencers were split
    ("window0_random", "individual_L2", "random", 2, False, 0, 2 + TICKS, TICKS),
]


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _env(pmode):
    from mdr_amd.environment import Environment

    return Environment(gu.props_from_overrides(overrides(N, pmode)), rng=random.Random(SEED))


@pytest.mark.parametrize("case,pmode,ctrl,dims,with_stats,win,nodes,launches", CASES, ids=[c[0] for c in CASES])
def test_sequence_counts(torch_gpu, case, pmode, ctrl, dims, with_stats, win, nodes, launches):
    torch = torch_gpu
    from mdr_amd.environment import ACTION_MODES
    from mdr_amd.services import RolloutStats

    env = _env(pmode)
    env.shard.set_rollout_window(win)
    rew = torch.empty((TICKS, N) if dims == 2 else (N,), dtype=torch.float64, device="cuda")
    stats = RolloutStats(env, TICKS) if with_stats else None
    g0 = env.shard.graph_info()
    env.rollout(TICKS, action_mode=ctrl, rewards=rew, use_graph=True, stats=stats)
    g1 = env.shard.graph_info()
    print(f"{case}: captured graph of {g1['guarded_nodes'] - g0['guarded_nodes']} nodes")
    assert g1["rollout_graphs"] == g0["rollout_graphs"] + 1 and g1["guarded"] == g0["guarded"] + 1, (g0, g1)
    assert g1["guarded_nodes"] - g0["guarded_nodes"] == nodes, (case, g0, g1)
    assert g1["rollout_launches"] == g0["rollout_launches"] + 1, (g0, g1)
    # the same call again replays the cached graph
    if stats is not None:
        stats.clear()
    env.rollout(TICKS, action_mode=ctrl, rewards=rew, use_graph=True, stats=stats)
    g2 = env.shard.graph_info()
    assert g2["rollout_graphs"] == g1["rollout_graphs"] and g2["guarded_nodes"] == g1["guarded_nodes"], (g1, g2)
    assert g2["rollout_launches"] == g1["rollout_launches"] + 1, (g1, g2)
    if launches is not None:
        _ms, got = env.shard.time_step_kernels(env.driver_window(TICKS), None, 0, ACTION_MODES[ctrl], rew,
                                               N if dims == 2 else 0)
        print(f"{case}: {got} step launches")
        assert got == launches, case
    torch.cuda.synchronize()
