"""Sharded MA-PPO training on the GPU: ``DeviceMAPPO.collect`` / ``update`` on a house-sharded
``neighbours`` cluster (one process per rank, every rank on cuda:0 over gloo, or RCCL to self) against
the single-process run of the parent test process — code that existed before the sharded store.

* rows: every rank's ``store.states`` rows, concatenated along the house axis, are the single-process
  rows bit for bit, in all three forms of the C loop, the stepwise path and the common penalty mode;
* the library form: ``snap == NULL`` is ``mdr_actor_rollout_sharded``, NaN rows, the refusals;
* update: the ranks hold one set of weights, the single process's; the guards; the refusals.
"""
import os
import random
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import golden_util as gu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = 6
COMM = "cluster_prop.agents_comm_prop."
MSG11 = {"cluster_prop.message_prop.thermal": True, "cluster_prop.message_prop.hvac": True}


def _overrides(n, k, mode="individual_L2", msg11=False):
    o = {"cluster_prop.nb_agents": n, "power_grid_prop.signal_properties.mode": "sinusoidals",
         "reward_prop.penalty_props.mode": mode, COMM + "mode": "neighbours", COMM + "max_nb_agents_communication": k}
    if msg11:
        o.update(MSG11)
    return o


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _paths():
    sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "marl-demandresponse_amd"), os.path.dirname(HERE)]


def _make_env(ov, rank=0, world=1, comm=None, kind=""):
    import torch

    import golden_util as g
    from mdr_amd.environment import Environment

    env = Environment(g.props_from_overrides(ov), device=torch.device("cuda", 0), rng=random.Random(4),
                      population="synthetic", seed=77, rank=rank, world=world, comm=comm)
    if "-force" in kind:
        env.shard.set_option("force_halo", 1)
    if "-twocoll" in kind:  # MDR_OPT_HALO_IN_COUNTS off: a ring-halo send/recv + the count allreduce per tick
        env.shard.set_option("halo_in_counts", 0)
    if kind.endswith("-serialhalo"):  # MDR_OPT_HALO_OVERLAP off: halo, then one k_actor per tick
        env.shard.set_option("halo_overlap", 0)
    return env


def _agent(env, dist=None, cfg=None, returns="per_agent", collect_ticks=T):
    """DeviceMAPPO (torch seed 1) whose actor is golden_util's calibrated seed-1 actor: the scales are
    the cluster-wide feature maxima, identical on every rank."""
    import golden_util as g
    from mdr_amd.mappo import DeviceMAPPO, MAPPOConfig

    m = env.obs_tensor().abs().amax(0).double().contiguous()
    if dist is not None:
        dist.all_reduce(m, op=dist.ReduceOp.MAX)
    agent = DeviceMAPPO(env, cfg or MAPPOConfig(batch_size=64, ppo_update_time=2), seed=1, returns=returns,
                        collect_ticks=collect_ticks)
    cal = g.calibrated_actor(env.obs_spec().n_feat, m.cpu().numpy(), seed=1)
    agent.actor_net.load_state_dict(cal.state_dict())
    agent.device_actor.load_weights()
    return agent


def _collected(env, agent, torch):
    """collect(T), then everything the rows test compares (host arrays)."""
    agent.collect(T)
    st = agent.store
    nl = env.n_local
    idx = torch.arange(T * nl, device="cuda")
    rows = st.states(idx).cpu().numpy().reshape(T, nl, -1)
    out = {"rows": rows, "actions": st.actions[:T].cpu().numpy(), "probs": st.probs[:T].cpu().numpy(),
           "rewards": st.rewards[:T].cpu().numpy(), "lo": env._offset}
    if st.halo_rows is not None:  # the same gather with the halo slab zeroed
        kept = st.halo_rows.clone()
        st.halo_rows.zero_()
        out["rows_nohalo"] = st.states(idx).cpu().numpy().reshape(T, nl, -1)
        st.halo_rows.copy_(kept)
    torch.cuda.synchronize()
    hs = env.shard.host_state()
    out.update({"T": hs["T"], "Tm": hs["Tm"], "on": hs["on"], "lock": hs["lock"], "sso": hs["sso"]})
    return out


def _weights(agent):
    return {f"{tag}.{k}": v.detach().cpu().numpy() for tag, net in (("actor", agent.actor_net),
                                                                     ("critic", agent.critic_net))
            for k, v in net.state_dict().items()}


def _init_dist(rank, world, port, backend):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    kw = {"device_id": torch.device("cuda", 0)} if backend == "nccl" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    return torch, dist


# ---------------------------------------------------------------- 1. rows
def _rows_worker(rank, world, port, backend, kind, ov, out_dir):
    _paths()
    torch, dist = _init_dist(rank, world, port, backend)
    from mdr_amd.distributed import make_comm

    env = _make_env(ov, rank, world, make_comm(kind.partition("-")[0]), kind)
    agent = _agent(env, dist)
    assert agent.store.sharded and agent.store.halo_bytes_per_tick == 4 * agent.store.halo_rows.shape[1] <= 440
    res = _collected(env, agent, torch)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    torch.cuda.synchronize()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,kind,world,n,k,mode,msg11", [
    ("gloo", "host", 3, 3 * 101, 10, "individual_L2", True),   # four tiles, the last one holding hi houses; msg_w 11
    ("gloo", "host", 3, 3 * 994, 10, "individual_L2", False),  # a ragged last tile: the overlap must stay off
    ("gloo", "host-twocoll", 3, 3 * 994, 10, "individual_L2", False),
    ("gloo", "host-twocoll-serialhalo", 3, 3 * 994, 10, "individual_L2", False),
    ("gloo", "host-twocoll", 3, 3 * 992, 10, "individual_L2", False),  # overlap on, halo on the comm stream
    ("gloo", "host", 3, 3001, 10, "individual_L2", False),     # uneven shards
    ("gloo", "host", 3, 3001, 3, "individual_L2", False),      # lo = 1, hi = 2: a lo / hi swap shows
    ("nccl", "rccl-force", 1, 3001, 10, "individual_L2", False),  # the real RCCL path to self
    ("gloo", "torch", 2, 3001, 10, "individual_L2", False),    # the stepwise path
    ("gloo", "torch", 2, 2048, 10, "common_L2", False),        # ... with the penalty reduce
])
def test_sharded_rows_equal_single(tmp_path, backend, kind, world, n, k, mode, msg11):
    """Every rank's rebuilt obs rows, stored actions, probabilities, rewards and final state, side by
    side, are the single-process collect's, bit for bit (common_L2 rewards: 1e-12, the cluster
    penalty is reduced in another order per shard).  The halo is exercised: the rows of the houses
    that read it — each shard's first lo and last hi houses, every tick — differ from the same gather
    with the halo slab zeroed, every other row does not; hence so do the blocks of its first hi and
    last lo houses (the houses whose messages it holds)."""
    import torch

    ov = _overrides(n, k, mode, msg11)
    mp.start_processes(_rows_worker, args=(world, _free_port(), backend, kind, ov, str(tmp_path)), nprocs=world,
                       join=True, start_method="spawn")
    parts = sorted((np.load(tmp_path / f"rank{r}.npz") for r in range(world)), key=lambda p: int(p["lo"]))
    env = _make_env(ov)
    agent = _agent(env)
    assert not agent.store.sharded
    ref = _collected(env, agent, torch)
    assert (ref["rows"].shape[2] - env.obs_spec().n_feat, env.obs_spec().n_comm) == (0, k)
    np.testing.assert_array_equal(np.concatenate([p["rows"] for p in parts], axis=1), ref["rows"])
    for key in ("actions", "probs"):
        np.testing.assert_array_equal(np.concatenate([p[key] for p in parts], axis=1), ref[key], err_msg=key)
    got_r = np.concatenate([p["rewards"] for p in parts], axis=1)
    if mode == "individual_L2":
        np.testing.assert_array_equal(got_r, ref["rewards"])
    else:
        np.testing.assert_allclose(got_r, ref["rewards"], rtol=1e-12, atol=1e-15)
    for key in ("T", "Tm", "on", "lock", "sso"):
        np.testing.assert_array_equal(np.concatenate([p[key] for p in parts]), ref[key], err_msg=key)
    gu.assert_not_saturated(ref["probs"], ref["actions"])
    lo, hi = k // 2, (k + 1) // 2
    for p in parts:
        a, b = p["rows"], p["rows_nohalo"]
        nl = a.shape[1]
        differs = (a != b).any(axis=2)  # [T, n_local]
        assert differs[:, :lo].all() and differs[:, nl - hi:].all()
        assert not differs[:, lo:nl - hi].any()
        assert (a[:, :hi] != b[:, :hi]).any() and (a[:, nl - lo:] != b[:, nl - lo:]).any()


# ---------------------------------------------------------------- 2. the library form
def _lib_worker(rank, world, port, out_dir):
    _paths()
    torch, dist = _init_dist(rank, world, port, "gloo")
    import ctypes as C

    from mdr_amd import _lib
    from mdr_amd.actor import DeviceActor
    from mdr_amd.distributed import make_comm
    from mdr_amd.replay import RolloutStore

    ov = _overrides(3 * 101, 10)
    n_t = 4
    outs = []
    for snap_form in (False, True):  # two identical environments: the old entry point, the new one with snap == NULL
        env = _make_env(ov, rank, world, make_comm("host"))
        agent = _agent(env, dist)
        nl = env.n_local
        A = torch.zeros((n_t, nl), dtype=torch.uint8, device="cuda")
        Pr = torch.zeros((n_t, nl), dtype=torch.float32, device="cuda")
        R = torch.zeros((n_t, nl), dtype=torch.float64, device="cuda")
        ticks = env.driver_window(n_t)
        osc = np.zeros((n_t, 4))
        osc[:, 1], osc[:, 3] = ticks.s_prev, ticks.t_od_prev
        osc[0, 2], osc[1:, 2] = float(env._solar), ticks.solar[:-1]
        env.shard.p_dev.fill_(float(env._P_host))
        spec = env.obs_spec()
        if snap_form:
            env.shard.actor_rollout_sharded_snap(ticks, osc, spec, A, nl, Pr, nl, R, nl, None, None, 0)
        else:
            env.shard.actor_rollout_sharded(ticks, osc, spec, A, nl, Pr, nl, R, nl)
        torch.cuda.synchronize()
        env._P_dev_valid = True  # (the raw calls left the cluster power in p_dev)
        outs.append([x.cpu().numpy() for x in (A, Pr, R, env.shard.t_air, env.shard.t_mass, env.shard.hvac)])
    same = all(np.array_equal(a, b) for a, b in zip(*outs))

    # an index outside the stored rows is a NaN row; the ones inside are not
    st = RolloutStore(env, 4)
    DeviceActor(env, agent.actor_net).rollout(2, store=st)
    idx = torch.tensor([-1, 0, 2 * nl - 1, 2 * nl, 1 << 40], device="cuda")
    rows = st.states(idx).cpu().numpy()
    nan_ok = bool(np.isnan(rows[[0, 3, 4]]).all() and np.isfinite(rows[[1, 2]]).all())

    # refusals: MDR_EARG before anything is launched, the state and the graph counters as they were
    sh = env.shard
    ticks = env.driver_window(2)
    osc = np.zeros((2, 4))
    w = st.halo_rows.shape[1]
    before = (sh.graph_info(), sh.t_air.clone(), sh.t_mass.clone(), sh.hvac.clone(), st.halo_rows.clone(),
              st.t_air.clone())
    halo = lambda cap=4, stride=w, ptr=_lib.ptr(st.halo_rows): _lib.mdr_snap_halo(  # noqa: E731
        C.sizeof(_lib.mdr_snap_halo), cap, stride, ptr)
    snap_short = _lib.mdr_snap(C.sizeof(_lib.mdr_snap), 4, nl - 1, _lib.ptr(st.t_air), _lib.ptr(st.t_mass),
                               _lib.ptr(st.hvac), _lib.ptr(st.scalars))
    refused = {}
    for name, (snap, hl, row0) in {"rows past the snapshot": (st.snap, halo(), 3),
                                   "negative row": (st.snap, halo(), -1),
                                   "rows past the halo slab": (st.snap, halo(cap=3), 2),
                                   "short halo stride": (st.snap, halo(stride=w - 1), 0),
                                   "short snapshot stride": (snap_short, halo(), 0),
                                   "null halo slab": (st.snap, halo(ptr=0), 0),
                                   "no halo": (st.snap, None, 0)}.items():
        try:
            sh.actor_rollout_sharded_snap(ticks, osc, spec, A[:2], nl, Pr[:2], nl, R[:2], nl, snap, hl, row0)
            refused[name] = "accepted"
        except _lib.MdrError as e:
            refused[name] = "MDR_EARG" if "MDR_EARG" in str(e) else str(e)
    spec_h = env.obs_spec()
    spec_h.halo_msg = _lib.ptr(st.halo_rows)
    out = torch.empty((1, spec.n_feat), dtype=torch.float32, device="cuda")
    try:
        sh.obs_gather_sharded(spec_h, st.snap, st.halo, st.rows, idx[1:2], out)
        refused["gather with halo_msg"] = "accepted"
    except _lib.MdrError as e:
        refused["gather with halo_msg"] = "MDR_EARG" if "MDR_EARG" in str(e) else str(e)
    torch.cuda.synchronize()
    after = (sh.graph_info(), sh.t_air, sh.t_mass, sh.hvac, st.halo_rows, st.t_air)
    unchanged = before[0] == after[0] and all(torch.equal(a, b) for a, b in zip(before[1:], after[1:]))
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), same=same, nan_ok=nan_ok, unchanged=unchanged,
             refused=np.array([f"{k}={v}" for k, v in refused.items()]))
    dist.destroy_process_group()


def test_library_form(tmp_path):
    """snap == NULL: mdr_actor_rollout_sharded's outputs; NaN rows; the MDR_EARG cases on every rank
    with nothing launched; MDR_ESTATE without a communicator."""
    import ctypes as C

    import torch

    from mdr_amd import _lib
    from mdr_amd.replay import RolloutStore

    world = 3
    mp.start_processes(_lib_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    for r in range(world):
        p = np.load(tmp_path / f"rank{r}.npz")
        assert bool(p["same"]) and bool(p["nan_ok"]) and bool(p["unchanged"])
        for item in p["refused"]:
            assert str(item).endswith("=MDR_EARG"), str(item)

    # no communicator, not a shard: the sharded entry points are MDR_ESTATE, the state as it was
    env = _make_env(_overrides(3 * 101, 10))
    agent = _agent(env)
    st = RolloutStore(env, 4)
    sh, n = env.shard, env.n_local
    halo_rows = torch.zeros((4, 40), dtype=torch.float32, device="cuda")
    halo = _lib.mdr_snap_halo(C.sizeof(_lib.mdr_snap_halo), 4, 40, _lib.ptr(halo_rows))
    ticks = env.driver_window(2)
    spec = env.obs_spec()
    rew = torch.empty((2, n), dtype=torch.float64, device="cuda")
    g0, state = sh.graph_info(), sh.t_air.clone()
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        sh.actor_rollout_sharded_snap(ticks, np.zeros((2, 4)), spec, None, 0, None, 0, rew, n, st.snap, halo, 0)
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        sh.obs_gather_sharded(spec, st.snap, halo, 0, torch.zeros(1, dtype=torch.int64, device="cuda"),
                              torch.empty((1, spec.n_feat), dtype=torch.float32, device="cuda"))
    sc = _lib.mdr_obs_scalars(0.0, 0.0, 0.0, 0.0)
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        sh.snapshot_sharded(spec, st.snap, halo, 0, sc, halo_rows[0])
    assert sh.graph_info() == g0 and torch.equal(sh.t_air, state) and float(halo_rows.abs().max()) == 0.0
    assert agent.store.rows == 0


# ---------------------------------------------------------------- 3-5. update
def _update_worker(rank, world, port, returns, extra_draw, out_dir):
    _paths()
    torch, dist = _init_dist(rank, world, port, "gloo")
    from mdr_amd.distributed import make_comm

    env = _make_env(_overrides(3 * 101, 10), rank, world, make_comm("host"))
    agent = _agent(env, dist, returns=returns)
    agent.collect(T)
    if extra_draw and rank == 1:
        torch.rand(1)  # one number more from the torch CPU generator than the other ranks
    err = ""
    try:
        assert agent.update() is True
    except RuntimeError as e:
        err = str(e)
    res = _weights(agent)
    res["err"] = np.array(err)
    res["steps"] = agent.training_step
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    torch.cuda.synchronize()
    dist.destroy_process_group()


def _single_worker(rank, returns, out_dir):
    """The single-process collect + update (no torch.distributed), one fresh process per ``rank``."""
    _paths()
    import torch

    torch.cuda.set_device(0)
    env = _make_env(_overrides(3 * 101, 10))
    agent = _agent(env, returns=returns)
    agent.collect(T)
    assert agent.update() is True
    res = _weights(agent)
    res["steps"] = agent.training_step
    np.savez(os.path.join(out_dir, f"single{rank}.npz"), **res)
    torch.cuda.synchronize()


def _keys(p):
    return sorted(k for k in p.files if k.startswith(("actor.", "critic.")))


@pytest.mark.parametrize("returns", ["per_agent", "reference"])
def test_sharded_update_one_set_of_weights(tmp_path, returns):
    """World 3, 3 x 101 houses, T = 6, batch 64, two epochs.  The ranks' actor and critic weights are
    equal to each other bit for bit, always.  per_agent: equal to the single-process DeviceMAPPO's bit
    for bit, provided torch gives two fresh single processes on this GPU the same bits for the same
    update (measured here first; if it does not, rtol 2e-3 / atol 2e-4, test_mappo_gpu.py's tolerance
    against the reference).  reference: the cross-shard returns are another summation order
    (relative 1e-12 in float64), so rtol 2e-3 / atol 2e-4."""
    world = 3
    mp.start_processes(_single_worker, args=(returns, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    s0, s1 = np.load(tmp_path / "single0.npz"), np.load(tmp_path / "single1.npz")
    torch_repeats = all(np.array_equal(s0[k], s1[k]) for k in _keys(s0))
    print(f"single-process update, two fresh processes, bit-identical: {torch_repeats}")
    mp.start_processes(_update_worker, args=(world, _free_port(), returns, False, str(tmp_path)), nprocs=world,
                       join=True, start_method="spawn")
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    assert len(_keys(s0)) == 12
    for p in parts:
        assert str(p["err"]) == "" and int(p["steps"]) == int(s0["steps"]) == 2 * -(-T * 3 * 101 // 64)
    for k in _keys(s0):
        for p in parts[1:]:
            np.testing.assert_array_equal(p[k], parts[0][k], err_msg=f"ranks differ: {k}")
        if returns == "per_agent" and torch_repeats:
            np.testing.assert_array_equal(parts[0][k], s0[k], err_msg=k)
        else:
            np.testing.assert_allclose(parts[0][k], s0[k], rtol=2e-3, atol=2e-4, err_msg=k)


def test_permutation_guard(tmp_path):
    """A rank that drew one number more from the torch CPU generator holds another permutation:
    every rank raises, none trains on."""
    world = 3
    mp.start_processes(_update_worker, args=(world, _free_port(), "per_agent", True, str(tmp_path)), nprocs=world,
                       join=True, start_method="spawn")
    for r in range(world):
        p = np.load(tmp_path / f"rank{r}.npz")
        assert "minibatch permutations differ" in str(p["err"]), str(p["err"])
        assert int(p["steps"]) == 0


# ---------------------------------------------------------------- 6. refusals
def test_refusals():
    from mdr_amd.mappo import DeviceMAPPO, MAPPOConfig
    from mdr_amd.replay import ReplayStore, RolloutStore
    from mdr_amd.services import DeviceMetrics, RolloutStats

    n = 303
    for mode in ("closed_groups", "random_fixed"):
        ov = _overrides(n, 10)
        ov[COMM + "mode"] = mode
        tab = _make_env(ov, rank=0, world=2, comm=object())
        with pytest.raises(ValueError, match=mode):
            RolloutStore(tab, 4)
    ov = _overrides(n, 10)
    ov[COMM + "mode"] = "random_sample"
    with pytest.raises(ValueError, match="random_sample"):
        RolloutStore(_make_env(ov, rank=0, world=2, comm=object()), 4)
    with pytest.raises(ValueError, match="ring half-width"):
        RolloutStore(_make_env(_overrides(8, 7), rank=0, world=4, comm=object()), 4)
    half = _make_env(_overrides(n, 10), rank=0, world=2, comm=object())
    with pytest.raises(ValueError, match="sharded"):
        ReplayStore(half, 4)
    with pytest.raises(ValueError, match="sharded"):
        RolloutStats(half, 4)
    agent = DeviceMAPPO(half, MAPPOConfig(batch_size=16, ppo_update_time=1), collect_ticks=4)
    assert agent.store.sharded and agent.store.halo_bytes_per_tick == 10 * 4 * 4
    tick = half._tick
    with pytest.raises(ValueError, match="sharded"):
        agent.collect(2, metrics=DeviceMetrics())
    assert half._tick == tick and agent.store.rows == 0
