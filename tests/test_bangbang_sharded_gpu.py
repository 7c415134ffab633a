"""Sharded closed-loop windows: Environment.rollout(action_mode="bangbang" | "deadband_bangbang") on
an environment with a communicator, against the single-process run of the same
cluster — rewards, t_air, t_mass, FSM words and the cluster power P, all ==.

Per rank the window is k_step_closed on its own houses (its trajectory never reads P); the rank's
per-tick class totals (k_win_shard_sum) are allreduced behind the window, and k_closed_reward_sharded
forms P (win_power over exact integer totals) and the signal term (win_nsig, every division by the
cluster's N) per block — the single-process expressions on the single-process operands.

The pattern is tests/test_distributed_gpu.py's: spawned ranks all on cuda:0, one process group per
case, world <= 3; `host` = the library's C sequencers with torch.distributed callbacks as the
communicator (mdr_comm_host), `rccl` = its own RCCL communicator (world 1), `torch` = one step per
tick from Python.  Every rank draws the whole reference population from random.Random(SEED) and
slices it.  Both controllers run inside one worker, on two environments.

tests/test_bangbang_sharded_cpu.py asserts under the oracle that with these inputs a rank-local P
differs from the cluster's at every tick of the first rollout.
"""
import datetime
import os
import random
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import golden_util as gu
from bangbang_inputs import CTRLS, SEED, overrides

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PER_TICK = ("serial", "overlap")  # <comm>-serial / <comm>-overlap: the per-tick C loops (window 0)


def _script(env, ctrl, torch, form=""):
    """70 ticks as three windows (2-D rewards); window 7: 37 ticks as six windows into one shared
    row (one finalised); one window of 5; three per-tick steps; 20 ticks (three windows of 7, 7, 6:
    the slots and the step path's counts were left clean).  The per-tick forms keep the window off."""
    nl = env.n_local
    rows, power = [], []

    def keep(r):
        rows.extend(np.atleast_2d(r.cpu().numpy().copy()))
        power.append(env._cluster_power())

    keep(env.rollout(70, action_mode=ctrl))
    if form not in PER_TICK:
        env.shard.set_rollout_window(7)
    row = torch.full((nl,), float("nan"), dtype=torch.float64, device=env.shard.device)
    keep(env.rollout(37, action_mode=ctrl, rewards=row))
    keep(env.rollout(5, action_mode=ctrl))
    for _ in range(3):
        keep(env.step_tensor(None, action_mode=ctrl, lookahead=ctrl))
    keep(env.rollout(20, action_mode=ctrl))
    torch.cuda.synchronize()
    st = env.shard.host_state()
    out = {k: st[k] for k in ("T", "Tm", "on", "lock", "sso")}
    out.update(rewards=np.stack(rows), P=np.array(power))
    return out


def _variant(env, form):
    if form == "winserial":
        env.shard.set_option("window_pipeline", 0)
    elif form in PER_TICK:
        env.shard.set_rollout_window(0)
        env.shard.set_option("sharded_overlap", form == "overlap")


def _worker(rank, world, port, backend, kind, n, out_dir):
    sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "marl-demandresponse_amd"), os.path.dirname(HERE)]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    kw = {"device_id": dev} if backend == "nccl" else {}
    # (a mismatched collective order between the ranks fails after a minute instead of hanging)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60), **kw)
    import golden_util as g

    from mdr_amd.distributed import make_comm
    from mdr_amd.environment import Environment

    comm_kind, _, form = kind.partition("-")
    res = {}
    for ctrl in CTRLS:
        env = Environment(g.props_from_overrides(overrides(n)), device=dev, rng=random.Random(SEED),
                          population="reference", rank=rank, world=world, comm=make_comm(comm_kind))
        _variant(env, form)
        if comm_kind != "torch":  # the C sequencer the case names is the one that runs
            pl = env._comm.pipeline(env.shard)
            if form in PER_TICK:
                assert pl["one_tick"].startswith("overlapped" if form == "overlap" else "serial"), pl
            else:
                assert pl["window"].startswith("one stream" if form == "winserial" else "count-ahead"), pl
        res.update({f"{ctrl}.{k}": v for k, v in _script(env, ctrl, torch, form).items()})
        res["lo"] = env._offset
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    torch.cuda.synchronize()
    dist.destroy_process_group()


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def single():
    """The single-process run of the script per (n, controller), computed once."""
    import torch

    from mdr_amd.environment import Environment

    cache = {}

    def get(n, ctrl):
        if (n, ctrl) not in cache:
            env = Environment(gu.props_from_overrides(overrides(n)), device=torch.device("cuda", 0),
                              rng=random.Random(SEED), population="reference")
            cache[n, ctrl] = _script(env, ctrl, torch)
        return cache[n, ctrl]

    return get


@pytest.mark.parametrize("backend,kind,world,n", [
    ("gloo", "host", 2, 130),              # 65 houses a rank: one full wave plus one lane
    ("gloo", "host", 3, 3001),             # shards 1000 / 1000 / 1001: two blocks, ragged last tile, uneven
    ("gloo", "host-winserial", 3, 3001),   # the one-stream form
    ("gloo", "host-serial", 3, 3001),      # per-tick C loop, serial
    ("gloo", "host-overlap", 3, 3001),     # per-tick C loop, overlapped (reward one launch later)
    ("gloo", "torch", 2, 3001),            # one step per tick from Python
    ("nccl", "rccl", 1, 3001),             # the library's communicator and comm stream
    ("nccl", "rccl-winserial", 1, 3001),   # the same, one stream
])
def test_sharded_rollout_equals_single(tmp_path, single, backend, kind, world, n):
    mp.start_processes(_worker, args=(world, _free_port(), backend, kind, n, str(tmp_path)),
                       nprocs=world, join=True, start_method="spawn")
    parts = sorted((np.load(tmp_path / f"rank{r}.npz") for r in range(world)), key=lambda p: int(p["lo"]))
    for ctrl in CTRLS:
        ref = single(n, ctrl)
        assert ref["rewards"].shape == (70 + 1 + 5 + 3 + 20, n)
        for key in ("on", "lock", "sso", "T", "Tm"):
            np.testing.assert_array_equal(np.concatenate([p[f"{ctrl}.{key}"] for p in parts]), ref[key],
                                          err_msg=f"{ctrl} {key}")
        got = np.concatenate([p[f"{ctrl}.rewards"] for p in parts], axis=1)
        np.testing.assert_array_equal(got, ref["rewards"], err_msg=ctrl)
        for p in parts:
            np.testing.assert_array_equal(p[f"{ctrl}.P"], ref["P"], err_msg=f"{ctrl} P")


def test_sharded_refusals_stay():
    """What stays refused on a sharded environment: a common penalty mode (Python and C level) and
    stats rows."""
    import torch

    from mdr_amd import _lib
    from mdr_amd.environment import ACTION_MODES, Environment
    from mdr_amd.services import RolloutStats

    n, dev = 300, torch.device("cuda", 0)
    keep = (_lib.HOST_ALLREDUCE_FN(lambda *a: 0), _lib.HOST_SENDRECV_FN(lambda *a: 0))

    def sharded_env(pmode):  # rank 0 of 2 (150 houses); its context gets host collectives
        env = Environment(gu.props_from_overrides(overrides(n, pmode)), device=dev, rng=random.Random(SEED),
                          population="reference", rank=0, world=2, comm=object())
        _lib.check(env.shard.lib.mdr_comm_host(env.shard.ctx, 2, 0, keep[0], keep[1], None), "mdr_comm_host")
        return env

    env = sharded_env("common_L2")
    state = env.shard.t_air.clone()
    for ctrl in CTRLS:
        with pytest.raises(NotImplementedError, match="individual_L2"):
            env.rollout(5, action_mode=ctrl)
        rew = torch.empty((5, env.n_local), dtype=torch.float64, device=dev)
        with pytest.raises(_lib.MdrError, match="MDR_EARG.*common penalty"):
            _lib.check(env.shard.lib.mdr_rollout_sharded(env.shard.ctx, 5, env.driver_window(5).ptr(), None, 0,
                                                         ACTION_MODES[ctrl], _lib.ptr(rew), env.n_local,
                                                         _lib.ptr(env.shard.p_dev), env.shard.stream()),
                       "mdr_rollout_sharded")
    assert torch.equal(env.shard.t_air, state)

    env = sharded_env("individual_L2")
    state = env.shard.t_air.clone()
    with pytest.raises(ValueError, match="sharded"):
        RolloutStats(env, 8)
    single_env = Environment(gu.props_from_overrides(overrides(n)), device=dev, rng=random.Random(SEED),
                             population="reference")
    for ctrl in CTRLS:
        with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
            env.shard.rollout_stats_path(ACTION_MODES[ctrl])
        with pytest.raises(ValueError):
            env.rollout(5, action_mode=ctrl, stats=RolloutStats(single_env, 8))
    assert torch.equal(env.shard.t_air, state)
