"""Stats rows of a house-sharded cluster on the GPU: ``ShardedRolloutStats`` rows from
``Environment.rollout``, ``DeviceActor.rollout``, ``DeviceMAPPO.collect`` / ``evaluate``,
``evaluate_controller`` and ``ServerLoop`` on an environment with a communicator, against the
single-process ``RolloutStats`` run of the same script.

The pattern is tests/test_bangbang_sharded_gpu.py's: spawned ranks all on cuda:0, one process group and
one spawn per (comm, world, form) case with every check of the case inside the worker, world <= 3, a
60-s collective timeout; `host` = the library's C sequencers with torch.distributed callbacks
(mdr_comm_host), `torch` = one step per tick from Python, `rccl` = the library's RCCL communicator
(world 1).

What is asserted of the rows: np.array_equal across the ranks; slots 2 (max), 10, 11 (exact integer
counts) and 12 (P) == the single process's; the sum slots within n * 2^-52 * A_k of it, A_k = sum of
the absolute values of the slot's terms, taken from the single-process row itself
(stats_sharded_np.sum_slot_bound: two groupings of the same n terms differ by at most
2 (n - 1) 2^-53 sum|t_i|); at RCCL world 1 every row == the unsharded one.  The single-process run
takes the launch form of the case (closed-loop windows, or one launch per tick for `host-serial` and
`torch`), so that the two rows sum the same terms.  tests/test_stats_sharded_cpu.py asserts under the
oracle that these inputs show a combine that drops a rank, sums slot 2 or takes the wrong rank's max.
"""
import datetime
import os
import random
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import golden_util as gu
import stats_sharded_np as X
from bangbang_inputs import CTRLS, SEED, overrides

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXACT = (2, 10, 11, 12)
CALLS = (70, 37, 5)


def _paths():
    sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "marl-demandresponse_amd"), os.path.dirname(HERE)]


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init_dist(rank, world, port, backend):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    kw = {"device_id": torch.device("cuda", 0)} if backend == "nccl" else {}
    # (a mismatched collective order between the ranks fails after a minute instead of hanging)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60), **kw)
    return torch, dist


def _spawn(fn, world, *args):
    mp.start_processes(fn, args=(world, _free_port()) + args, nprocs=world, join=True, start_method="spawn")


def _slab_zero(env, m):
    """The exchange slab of the m-row call that just returned is all zero again (sharded envs)."""
    if env._comm is None:
        return True
    return not bool(env.shard.stats_exchange_buffer(m).any())


# ------------------------------------------------------------------------------- 1. bang-bang rollouts
def _bb_variant(env, form):
    if form == "winserial":
        env.shard.set_option("window_pipeline", 0)
    elif form == "serial":
        env.shard.set_rollout_window(0)
        env.shard.set_option("sharded_overlap", 0)


def _bb_script(env, ctrl, torch, per_tick):
    """rollout(70) with 2-D rewards; window 7; rollout(37) into one shared row; rollout(5) — every call
    with stats rows (the per-tick forms keep the window off)."""
    from mdr_amd.services import RolloutStats, ShardedRolloutStats, rollout_stats_for

    stats = rollout_stats_for(env, sum(CALLS))
    assert type(stats) is (ShardedRolloutStats if env._comm is not None else RolloutStats)
    rows, power, zero = [], [], []

    def keep(r, m):
        rows.extend(np.atleast_2d(r.cpu().numpy().copy()))
        power.append(env._cluster_power())
        zero.append(_slab_zero(env, m))

    keep(env.rollout(70, action_mode=ctrl, stats=stats), 70)
    if not per_tick:
        env.shard.set_rollout_window(7)
    row = torch.full((env.n_local,), float("nan"), dtype=torch.float64, device=env.shard.device)
    keep(env.rollout(37, action_mode=ctrl, rewards=row, stats=stats), 37)
    keep(env.rollout(5, action_mode=ctrl, stats=stats), 5)
    torch.cuda.synchronize()
    assert stats.rows == sum(CALLS)
    st = env.shard.host_state()
    out = {k: st[k] for k in ("T", "Tm", "on", "lock", "sso")}
    out.update(rewards=np.stack(rows), P=np.array(power), stats=stats.host().copy(), slab_zero=np.array(zero),
               signal_post=stats.prev()["signal_post"], p_prev=stats.prev()["cluster_hvac_power"])
    return out


def _bb_worker(rank, world, port, backend, kind, n, out_dir):
    _paths()
    torch, dist = _init_dist(rank, world, port, backend)
    import golden_util as g

    from mdr_amd.distributed import make_comm
    from mdr_amd.environment import Environment

    comm_kind, _, form = kind.partition("-")
    res = {}
    for ctrl in CTRLS:
        env = Environment(g.props_from_overrides(overrides(n)), device=torch.device("cuda", 0),
                          rng=random.Random(SEED), population="reference", rank=rank, world=world,
                          comm=make_comm(comm_kind))
        _bb_variant(env, form)
        per_tick = form == "serial" or comm_kind == "torch"
        if comm_kind != "torch":  # the path the case names is the one that writes the rows
            assert env.shard.rollout_sharded_stats_path(16 if ctrl == "bangbang" else 17) == (2 if per_tick else 1)
            if form != "serial":
                pl = env._comm.pipeline(env.shard)
                assert pl["window"].startswith("one stream" if form == "winserial" else "count-ahead"), pl
        res.update({f"{ctrl}.{k}": v for k, v in _bb_script(env, ctrl, torch, per_tick).items()})
        res["lo"] = env._offset
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def bb_single():
    """The single-process RolloutStats run of the script per (n, controller, launch form), once."""
    import torch

    from mdr_amd.environment import Environment

    cache = {}

    def get(n, ctrl, per_tick):
        if (n, ctrl, per_tick) not in cache:
            env = Environment(gu.props_from_overrides(overrides(n)), device=torch.device("cuda", 0),
                              rng=random.Random(SEED), population="reference")
            if per_tick:
                env.shard.set_rollout_window(0)
            cache[n, ctrl, per_tick] = _bb_script(env, ctrl, torch, per_tick)
        return cache[n, ctrl, per_tick]

    return get


@pytest.fixture(scope="module")
def bb_runs(tmp_path_factory):
    """One spawn per sharded bang-bang case, shared by the tests that read it."""
    cache = {}

    def get(backend, kind, world, n):
        key = (backend, kind, world, n)
        if key not in cache:
            d = tmp_path_factory.mktemp("bb")
            _spawn(_bb_worker, world, backend, kind, n, str(d))
            cache[key] = sorted((dict(np.load(d / f"rank{r}.npz")) for r in range(world)), key=lambda p: int(p["lo"]))
        return cache[key]

    return get


def _assert_rows(got, ref, n, exact, what):
    """Stats rows against the single process's: EXACT slots ==, sum slots within their bound (printed
    first), 13..15 zero; ``exact``: every slot ==."""
    assert got.shape == ref.shape, what
    assert not got[:, 13:].any(), what
    for k in EXACT:
        assert np.array_equal(got[:, k], ref[:, k]), f"{what}: slot {k}"
    bound = X.sum_slot_bound(ref, n)
    err = np.abs(got[:, :X.N_STATS] - ref[:, :X.N_STATS])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)), axis=0)
    print(f"{what}: worst |sharded - single| / bound per slot {np.array2string(worst, precision=3)}")
    assert (err <= bound).all(), f"{what}: slots {sorted(set(np.argwhere(err > bound)[:, 1]))}"
    if exact:
        assert np.array_equal(got, ref), what


BB_CASES = [
    ("gloo", "host", 2, 130),             # 65 houses a rank; the two-stream closed-window form
    ("gloo", "host", 3, 3001),            # shards 1000 / 1000 / 1001: two blocks, ragged last tile, uneven
    ("gloo", "host-winserial", 3, 3001),  # the one-stream form
    ("gloo", "host-serial", 2, 130),      # window 0: partial rows per tick in the C loop
    ("gloo", "torch", 2, 130),            # one step per tick from Python, allreduce_sum of the slab
    ("nccl", "rccl", 1, 3001),            # the library's communicator, two streams
    ("nccl", "rccl-winserial", 1, 3001),  # ... and one
]


@pytest.mark.parametrize("backend,kind,world,n", BB_CASES)
def test_bangbang_rows(bb_runs, bb_single, backend, kind, world, n):
    parts = bb_runs(backend, kind, world, n)
    per_tick = kind in ("host-serial", "torch")
    for ctrl in CTRLS:
        ref = bb_single(n, ctrl, per_tick)
        assert ref["stats"].shape == (sum(CALLS), 16) and ref["rewards"].shape == (70 + 1 + 5, n)
        for p in parts:
            assert np.array_equal(p[f"{ctrl}.stats"], parts[0][f"{ctrl}.stats"]), f"{ctrl}: rows differ between ranks"
            assert p[f"{ctrl}.slab_zero"].all(), f"{ctrl}: the exchange slab is not zero after a call"
            for key in ("P", "signal_post", "p_prev"):
                np.testing.assert_array_equal(p[f"{ctrl}.{key}"], ref[key], err_msg=f"{ctrl} {key}")
        _assert_rows(parts[0][f"{ctrl}.stats"], ref["stats"], n, kind.startswith("rccl"), f"{kind} x{world} {ctrl}")
        # the rows perturb nothing: rewards, state, FSM words, P are still the single process's
        for key in ("on", "lock", "sso", "T", "Tm"):
            np.testing.assert_array_equal(np.concatenate([p[f"{ctrl}.{key}"] for p in parts]), ref[key],
                                          err_msg=f"{ctrl} {key}")
        np.testing.assert_array_equal(np.concatenate([p[f"{ctrl}.rewards"] for p in parts], axis=1), ref["rewards"],
                                      err_msg=ctrl)


def test_host_and_torch_rows_are_the_same_bits(bb_runs):
    """The per-tick partial rows, their exact exchange and the rank-order combine do not depend on who
    carries the collective: the library's C loop over host callbacks and the Python loop over
    torch.distributed write np.array_equal rows (world 2 x 130)."""
    host, tor = bb_runs("gloo", "host-serial", 2, 130), bb_runs("gloo", "torch", 2, 130)
    for ctrl in CTRLS:
        assert np.array_equal(host[0][f"{ctrl}.stats"], tor[0][f"{ctrl}.stats"]), ctrl


# ------------------------------------------------------------------------------- 2. the actor's rollouts
T_ACT, T_COL, T_EVAL = 6, 4, 6


def _actor_script(make_env, dist, torch, deep_copy):
    """On identical environments: DeviceActor.rollout(6) without rows; with rows; with rows and a
    (sharded) store; then DeviceMAPPO.collect(4, metrics=m) and evaluate(6) with a kept twin (and with
    the default deep copy)."""
    import copy

    from test_mappo_sharded_gpu import _agent

    from mdr_amd.services import DeviceMetrics, rollout_stats_for

    def outputs(env, r, a, p):
        torch.cuda.synchronize()
        st = env.shard.host_state()
        return [r.cpu().numpy(), a.cpu().numpy(), p.cpu().numpy(), st["T"], st["Tm"], st["on"], st["lock"], st["sso"],
                np.array(env._cluster_power())]

    res = {}
    outs = []
    for with_rows in (False, True):
        env = make_env()
        agent = _agent(env, dist, collect_ticks=T_ACT)
        nl = env.n_local
        a = torch.zeros((T_ACT, nl), dtype=torch.uint8, device="cuda")
        p = torch.zeros((T_ACT, nl), dtype=torch.float32, device="cuda")
        stats = rollout_stats_for(env, T_ACT) if with_rows else None
        r = agent.device_actor.rollout(T_ACT, actions=a, probs=p, stats=stats)
        outs.append(outputs(env, r, a, p))
        if with_rows:
            res["rows"] = stats.host().copy()
            res["slab_zero"] = np.array(_slab_zero(env, T_ACT))
    res["same_without_rows"] = np.array(all(np.array_equal(x, y) for x, y in zip(*outs)))
    res["rewards"], res["actions"] = outs[1][0], outs[1][1]
    res["lo"] = np.array(env._offset)

    env = make_env()  # ... with the store's snapshot (and halo) rows in the same loop
    agent = _agent(env, dist, collect_ticks=T_ACT)
    stats = rollout_stats_for(env, T_ACT)
    agent.device_actor.rollout(T_ACT, store=agent.store, stats=stats)
    res["rows_store"] = stats.host().copy()
    res["store_sharded"] = np.array(bool(agent.store.sharded))

    env = make_env()
    agent = _agent(env, dist, collect_ticks=T_COL)
    m = DeviceMetrics()
    m.initialize(env.n, 1, 100)
    agent.collect(T_COL, metrics=m)
    res["metrics"] = np.array([float(getattr(m, f)) for f in m.FIELDS])
    twin = copy.deepcopy(env)
    means = [agent.evaluate(T_EVAL, env=twin), agent.evaluate(T_EVAL, env=twin)]
    if deep_copy:
        means.append(agent.evaluate(T_EVAL))
    res["means"] = np.array([[v[k] for k in sorted(v)] for v in means])
    torch.cuda.synchronize()
    return res


def _actor_worker(rank, world, port, backend, kind, n, deep_copy, out_dir):
    _paths()
    torch, dist = _init_dist(rank, world, port, backend)
    from test_mappo_sharded_gpu import _make_env, _overrides

    from mdr_amd.distributed import make_comm

    res = _actor_script(lambda: _make_env(_overrides(n, 10), rank, world, make_comm(kind.partition("-")[0]), kind),
                        dist, torch, deep_copy)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def actor_single():
    """The single-process run of the actor script per cluster size, once."""
    import torch

    from test_mappo_sharded_gpu import _make_env, _overrides

    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = _actor_script(lambda: _make_env(_overrides(n, 10)), None, torch, True)
        return cache[n]

    return get


@pytest.mark.parametrize("backend,kind,world,n,deep_copy", [
    ("gloo", "host", 2, 303, True),                            # the halo rides in the count allreduce
    ("gloo", "host-twocoll", 2, 2 * 992, False),               # halo_in_counts off: the overlapped halo form
    ("gloo", "host-twocoll-serialhalo", 2, 2 * 992, False),    # ... and the plain one
    ("gloo", "host", 3, 301, False),                           # uneven shards 100 / 100 / 101
    ("gloo", "torch", 2, 303, False),                          # stepwise: partial rows from Python
    ("nccl", "rccl-force", 1, 303, False),                     # the library's communicator, halo to self
])
def test_actor_rows(tmp_path, actor_single, backend, kind, world, n, deep_copy):
    _spawn(_actor_worker, world, backend, kind, n, deep_copy, str(tmp_path))
    parts = sorted((np.load(tmp_path / f"rank{r}.npz") for r in range(world)), key=lambda p: int(p["lo"]))
    ref = actor_single(n)
    assert bool(ref["same_without_rows"]) and not bool(ref["store_sharded"])
    what = f"{kind} x{world}"
    for p in parts:
        assert bool(p["same_without_rows"]), "the rows changed the rollout's outputs or state"
        assert bool(p["slab_zero"]) and bool(p["store_sharded"])
        for key in ("rows", "rows_store", "means"):
            assert np.array_equal(p[key], parts[0][key]), f"{key} differs between ranks"
        assert np.array_equal(p["rows_store"], p["rows"]), "with and without a store"
        np.testing.assert_allclose(p["metrics"], ref["metrics"], rtol=1e-12, atol=1e-9)
        k = len(p["means"])
        np.testing.assert_allclose(p["means"], ref["means"][[0, 1, 2][:k]], rtol=1e-12, atol=0)
    _assert_rows(parts[0]["rows"], ref["rows"], n, kind.startswith("rccl"), what)
    for key in ("rewards", "actions"):
        np.testing.assert_array_equal(np.concatenate([p[key] for p in parts], axis=1), ref[key], err_msg=key)


# ------------------------------------------------------------------------------- 3. evaluation, server loop
CONTROLLERS = ("bangbang", "deadband_bangbang", "greedy")


def _eval_script(make_env):
    from mdr_amd.services import ServerLoop, evaluate_controller

    res = {}
    for c in CONTROLLERS:
        env = make_env()
        v = evaluate_controller(env, c, 40)
        res[f"eval.{c}"] = np.array([v[k] for k in sorted(v)])
        loop = ServerLoop(env, c, start_stats_from=5, nb_time_steps=40, time_steps_train_log=20, rollout_ticks=16)
        final = loop.run(40)
        m = loop.metrics
        res[f"loop.{c}"] = np.array([float(getattr(m, f)) for f in m.FIELDS] + [final[k] for k in sorted(final)])
        res[f"logs.{c}"] = np.array([[float(v) for k, v in sorted(lg.items()) if k != "Time (hour)"] for lg in loop.logs])
    return res


def _eval_worker(rank, world, port, n, out_dir):
    _paths()
    torch, dist = _init_dist(rank, world, port, "gloo")
    import golden_util as g

    from mdr_amd.distributed import make_comm
    from mdr_amd.environment import Environment

    res = _eval_script(lambda: Environment(g.props_from_overrides(overrides(n)), device=torch.device("cuda", 0),
                                           rng=random.Random(SEED), population="reference", rank=rank, world=world,
                                           comm=make_comm("host")))
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    torch.cuda.synchronize()
    dist.destroy_process_group()


def test_evaluation_and_server_loop(tmp_path):
    """evaluate_controller (the default deep copy) and ServerLoop(rollout_ticks=16) on a `host` world 2
    environment: equal across the ranks, and the single process's at test_services_gpu.py's and
    test_tick_stats_gpu.py's tolerances."""
    import torch

    from mdr_amd.environment import Environment

    n, world = 1000, 2
    _spawn(_eval_worker, world, n, str(tmp_path))
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    ref = _eval_script(lambda: Environment(gu.props_from_overrides(overrides(n)), device=torch.device("cuda", 0),
                                           rng=random.Random(SEED), population="reference"))
    for c in CONTROLLERS:
        for key in (f"eval.{c}", f"loop.{c}", f"logs.{c}"):
            assert np.array_equal(parts[0][key], parts[1][key]), f"{key} differs between ranks"
        np.testing.assert_allclose(parts[0][f"eval.{c}"], ref[f"eval.{c}"], rtol=1e-12, atol=0, err_msg=c)
        np.testing.assert_allclose(parts[0][f"loop.{c}"], ref[f"loop.{c}"], rtol=1e-12, atol=1e-9, err_msg=c)
        assert parts[0][f"logs.{c}"].shape == ref[f"logs.{c}"].shape == (2, ref[f"logs.{c}"].shape[1])
        np.testing.assert_allclose(parts[0][f"logs.{c}"], ref[f"logs.{c}"], rtol=1e-12, atol=1e-9, err_msg=c)


# ------------------------------------------------------------------------------- 4. refusals, in process
class _QuietComm:
    """A native communicator of world 2 whose collectives are never reached: every call below is
    refused before anything is exchanged.  The context gets host collectives (mdr_comm_host)."""

    native, world, rank = True, 2, 0

    def attach(self, shard):
        from mdr_amd import _lib

        shard._quiet_cbs = (_lib.HOST_ALLREDUCE_FN(lambda *a: -1), _lib.HOST_SENDRECV_FN(lambda *a: -1))
        _lib.check(shard.lib.mdr_comm_host(shard.ctx, 2, 0, shard._quiet_cbs[0], shard._quiet_cbs[1], None),
                   "mdr_comm_host")

    def allreduce_sum(self, shard, t):
        raise AssertionError("a refused call reached the exchange")

    def rollout(self, *a, **k):
        raise AssertionError("a refused call reached the rollout")


def test_refusals():
    import torch

    from mdr_amd import _lib
    from mdr_amd.environment import ACTION_MODES, Environment
    from mdr_amd.services import RolloutStats, ShardedRolloutStats, rollout_stats_for

    n, dev = 300, torch.device("cuda", 0)

    def make(pmode="individual_L2", comm=None, world=2):
        return Environment(gu.props_from_overrides(overrides(n, pmode)), device=dev, rng=random.Random(SEED),
                           population="reference", rank=0, world=world, comm=comm)

    # the pinned single-shard refusals still hold on a context with a communicator
    env = make(comm=_QuietComm())
    sh = env.shard
    with pytest.raises(ValueError, match="sharded"):
        RolloutStats(env, 8)
    out16 = torch.zeros(16, dtype=torch.float64, device=dev)
    for ctrl in CTRLS:
        with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
            sh.rollout_stats_path(ACTION_MODES[ctrl])
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        sh.tick_stats(None, out16)
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE.*single-shard"):
        sh.greedy_rollout_stats_check()
    one = make(comm=_QuietComm(), world=1)  # (world 1: a plain RolloutStats can be built over it)
    with pytest.raises(_lib.MdrError):
        one.greedy_rollout(4, stats=RolloutStats(one, 8))
    # a communicator without a callable allreduce_sum
    with pytest.raises(ValueError, match="sharded"):
        ShardedRolloutStats(make(comm=object()), 8)
    with pytest.raises(ValueError, match="sharded"):
        rollout_stats_for(make(comm=object()), 8)

    def untouched(env, stats, state):
        tick, rng, t_air = state
        return env._tick == tick and env.rng.getstate() == rng and torch.equal(env.shard.t_air, t_air) \
            and stats.rows == 0 and not bool(stats.stats.any())

    stats = ShardedRolloutStats(env, 8)
    state = (env._tick, env.rng.getstate(), sh.t_air.clone())
    # an open-loop source with the window on: no rows, before the drivers advance
    for mode in ("random", "always_on"):
        assert sh.lib.mdr_rollout_sharded_stats_path(sh.ctx, ACTION_MODES[mode]) == -1
        with pytest.raises(NotImplementedError, match="open-loop window"):
            env.rollout(5, action_mode=mode, stats=stats)
    # row overflow: ValueError before anything advances; the C call answers with the row range first
    with pytest.raises(ValueError, match="overflow"):
        env.rollout(9, action_mode="bangbang", stats=stats)
    rew = torch.empty((5, env.n_local), dtype=torch.float64, device=dev)
    with pytest.raises(_lib.MdrError, match="MDR_EARG.*stats_row0"):
        _lib.check(sh.lib.mdr_rollout_sharded_stats(sh.ctx, 5, None, None, 0, ACTION_MODES["bangbang"], _lib.ptr(rew),
                                                    env.n_local, _lib.ptr(sh.p_dev), _lib.ptr(stats.stats), 8, 4,
                                                    sh.stream()), "mdr_rollout_sharded_stats")
    with pytest.raises(_lib.MdrError, match="MDR_EARG.*row outside"):
        sh.tick_stats_sharded(None, 4, 4)
    assert untouched(env, stats, state)
    assert sh.rollout_sharded_stats_path(ACTION_MODES["bangbang"]) == 1
    sh.set_rollout_window(0)
    assert sh.rollout_sharded_stats_path(ACTION_MODES["random"]) == 2

    # a common penalty mode, as today: Python and C level
    env = make("common_L2", comm=_QuietComm())
    sh = env.shard
    stats = ShardedRolloutStats(env, 8)
    state = (env._tick, env.rng.getstate(), sh.t_air.clone())
    for ctrl in CTRLS:
        with pytest.raises(NotImplementedError, match="individual_L2"):
            env.rollout(5, action_mode=ctrl, stats=stats)
        with pytest.raises(_lib.MdrError, match="MDR_EARG.*common penalty"):
            sh.rollout_sharded_stats_path(ACTION_MODES[ctrl])
        with pytest.raises(_lib.MdrError, match="MDR_EARG.*common penalty"):
            _lib.check(sh.lib.mdr_rollout_sharded_stats(sh.ctx, 5, env.driver_window(5).ptr(), None, 0,
                                                        ACTION_MODES[ctrl], _lib.ptr(rew), env.n_local,
                                                        _lib.ptr(sh.p_dev), _lib.ptr(stats.stats), 8, 0, sh.stream()),
                       "mdr_rollout_sharded_stats")
    assert torch.equal(sh.t_air, state[2]) and stats.rows == 0 and not bool(stats.stats.any())

    # neither a communicator nor a shard: the sharded forms are MDR_ESTATE
    single = Environment(gu.props_from_overrides(overrides(n)), device=dev, rng=random.Random(SEED),
                         population="reference")
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        single.shard.tick_stats_sharded(None, 4, 0)
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        single.shard.stats_exchange_buffer(4)
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        single.shard.rollout_sharded_stats_path(ACTION_MODES["bangbang"])
