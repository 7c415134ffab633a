"""Training MA-PPO from the fused rollout: state snapshots (k_snap), the obs gather (k_obs_gather),
``RolloutStore`` and ``DeviceMAPPO.collect``.

Reference: TrainingManager.start stores the normalised state of every agent every tick
(server/app/services/training_manager.py:224-240, MAPPO.store_transition mappo.py:105-126); here a
transition keeps the 20 B of state its obs row depends on and the row is rebuilt on demand.

Bounds: gathered rows are BITWISE the rows ``obs_tensor`` produced at the snapshot's tick (the same
device functions assemble both), and within 2 float32 ulp of the reference's ``norm_state_dict``
(the bound of test_env_parity_gpu.test_golden_obs_vector).  ``collect`` reproduces the per-tick
training loop bitwise (actions, probabilities, rewards, states, final house state); the PPO update
from the store is compared with the update from the buffer within 4x the buffer path's own
run-to-run spread (plain equality when that path reproduces itself).
"""
import ctypes as C
import random

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

PROB_ATOL = {"fp32": 1e-6, "bf16x3": 1e-4}  # as tests/test_actor_gpu.py
SIN = {"power_grid_prop.signal_properties.mode": "sinusoidals"}  # every tick's scalars differ
COMM = "cluster_prop.agents_comm_prop."
WIDE = {"state_prop.hvac": True, "state_prop.solar_gain": True, "state_prop.thermal": True,
        "cluster_prop.message_prop.thermal": True, "cluster_prop.message_prop.hvac": True}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def make_env(overrides, seed=5, resets=1, **kw):
    from mdr_amd.environment import Environment

    env = Environment(gu.props_from_overrides(overrides), rng=random.Random(seed), **kw)
    for _ in range(resets - 1):
        env.reset(return_obs=False)
    return env


def snapshot_ticks(torch, env, store, ticks, seed=7):
    """Per tick: snapshot, keep obs_tensor, step with random actions.  Returns the stacked rows."""
    rs = np.random.RandomState(seed)
    rows = []
    for _ in range(ticks):
        env.snapshot(store)
        rows.append(env.obs_tensor().clone())
        env.step_tensor(torch.from_numpy(rs.randint(0, 2, env.n_local).astype(np.uint8)).to("cuda"))
    return torch.cat(rows)


# ------------------------------------------------------------------ 1. gather == obs_tensor
GATHER_CASES = {
    "ring_n13_k10_wraps": ({"cluster_prop.nb_agents": 13}, None),
    "ring_n77_ragged": ({"cluster_prop.nb_agents": 77}, None),
    "ring_n300_blocks": ({"cluster_prop.nb_agents": 300}, None),
    "closed_groups_n24": ({"cluster_prop.nb_agents": 24, COMM + "mode": "closed_groups"}, None),
    "random_fixed_n24": ({"cluster_prop.nb_agents": 24, COMM + "mode": "random_fixed"}, None),
    "wide_n77_msg11": (dict({"cluster_prop.nb_agents": 77}, **WIDE), 128),
}


@pytest.mark.parametrize("case", sorted(GATHER_CASES))
def test_gather_equals_obs_tensor(torch_gpu, case):
    from mdr_amd.replay import RolloutStore

    torch = torch_gpu
    ov, n_feat = GATHER_CASES[case]
    env = make_env(dict(ov, **SIN))
    n, T = env.n_local, 5
    spec = env.obs_spec()
    n_feat = n_feat or spec.n_feat
    assert spec.n_feat == n_feat
    if case.startswith("wide"):
        assert env.shard.lib.mdr_msg_width(C.byref(spec)) == 11
    store = RolloutStore(env, T)
    want = snapshot_ticks(torch, env, store, T)
    assert store.rows == T and len(store) == T * n and want.shape == (T * n, n_feat)
    g = torch.Generator().manual_seed(3)
    idx = torch.cat([torch.randperm(T * n, generator=g), torch.tensor([0, T * n - 1, n])]).to("cuda")
    got = store.states(idx)
    assert got.dtype == torch.float32 and got.shape == (T * n + 3, n_feat)
    assert torch.equal(got, want[idx])
    one = torch.tensor([2 * n + n // 2], device="cuda")  # m = 1
    assert torch.equal(store.states(one), want[one])
    assert torch.equal(store.states(torch.arange(T * n, device="cuda")), want)


# ------------------------------------------------------------------ 2. gather against the reference
@pytest.mark.parametrize("name", gu.TRAJ_NAMES)
def test_gather_golden_obs_vector(torch_gpu, name):
    from mdr_amd.replay import RolloutStore

    torch = torch_gpu
    d, meta = gu.traj(name)
    env = make_env(meta["overrides"], meta["seed"], meta["resets"])
    n = meta["N"]
    ticks = sorted(int(k[6:]) for k in d.keys() if k.startswith("norm_t"))
    store = RolloutStore(env, len(ticks))
    if 0 in ticks:
        env.snapshot(store)
    for t in range(max(ticks)):
        env.step_tensor(torch.from_numpy(d["actions"][t]).to("cuda"))
        if t + 1 in ticks:
            env.snapshot(store)
    assert store.rows == len(ticks)
    got = store.states(torch.arange(len(ticks) * n, device="cuda")).cpu().numpy().reshape(len(ticks), n, -1)
    for k, t in enumerate(ticks):
        np.testing.assert_array_max_ulp(got[k], d[f"norm_t{t}"].astype(np.float32), maxulp=2)


# ------------------------------------------------------------------ 3. out-of-range index
def test_gather_out_of_range_index_is_nan(torch_gpu):
    from mdr_amd.replay import RolloutStore

    torch = torch_gpu
    env = make_env(dict({"cluster_prop.nb_agents": 77}, **SIN))
    n = env.n_local
    store = RolloutStore(env, 8)
    want = snapshot_ticks(torch, env, store, 5)
    # row 5 is inside the allocation but not filled: never read, NaN out
    idx = torch.tensor([3, 5 * n + 3, 4 * n + 76, 5 * n, 6 * n - 1, -1, 0], device="cuda")
    got = store.states(idx)
    ok = torch.tensor([True, False, True, False, False, False, True], device="cuda")
    assert torch.isnan(got[~ok]).all()
    assert torch.equal(got[ok], want[idx[ok]])


# ------------------------------------------------------------------ 4 / 5. collect == the loop
COLLECT_CASES = [(77, "fp32"), (77, "bf16x3"), (4099, "fp32"), (4099, "bf16x3")]
T_COLLECT = 6
_SCEN = {}


def _agent(n, precision, collect_ticks=0):
    from mdr_amd.environment import Environment
    from mdr_amd.mappo import DeviceMAPPO, MAPPOConfig

    env = Environment(gu.props_from_overrides(dict({"cluster_prop.nb_agents": n}, **SIN)), rng=random.Random(2),
                      population="synthetic", seed=3)
    cfg = MAPPOConfig(batch_size=256 if n < 1000 else 4096, ppo_update_time=2)
    return env, DeviceMAPPO(env, cfg, precision=precision, collect_ticks=collect_ticks)


def _loop(torch, env, agent):
    """The loop of test_mappo_gpu.test_training_loop_runs_on_device."""
    obs = env.obs_tensor().clone()
    for t in range(T_COLLECT):
        a = agent.select_actions()
        r = env.step_tensor(a).clone()
        nxt = env.obs_tensor().clone()
        agent.store_transition(obs, nxt, r, done=(t == T_COLLECT - 1))
        obs = nxt


def _weights(agent):
    return {f"{tag}.{k}": v.detach().clone() for tag, net in (("actor", agent.actor_net), ("critic", agent.critic_net))
            for k, v in net.state_dict().items()}


def scenario(torch, n, precision):
    """Run once per case, shared by the collect and update tests: A1 / A2 the per-tick loop on fresh
    twins, B collect(); then one update each under the same torch seed; then B collects again."""
    key = (n, precision)
    if key in _SCEN:
        return _SCEN[key]
    s = {}
    env_a, a1 = _agent(n, precision)
    _loop(torch, env_a, a1)
    s["A"] = {"states": torch.cat([b[0] for b in a1.buffer]), "actions": torch.stack([b[1] for b in a1.buffer]),
              "probs": torch.stack([b[2] for b in a1.buffer]), "rewards": torch.stack([b[3] for b in a1.buffer]),
              "done": [b[4] for b in a1.buffer],
              "final": {k: getattr(env_a.shard, k).clone() for k in ("t_air", "t_mass", "hvac")}}
    env_b, b = _agent(n, precision, collect_ticks=8)
    g0 = env_b.shard.graph_info()
    r = b.collect(T_COLLECT)
    g1 = env_b.shard.graph_info()
    st = b.store
    s["B"] = {"states": st.states(torch.arange(T_COLLECT * n, device="cuda")), "actions": st.actions[:T_COLLECT].clone(),
              "probs": st.probs[:T_COLLECT].clone(), "rewards": st.rewards[:T_COLLECT].clone(), "done": list(st.done),
              "returned": r.clone(), "rows": st.rows, "len": len(b),
              "final": {k: getattr(env_b.shard, k).clone() for k in ("t_air", "t_mass", "hvac")}}
    env_a2, a2 = _agent(n, precision)
    _loop(torch, env_a2, a2)
    s["w0"] = _weights(b)
    s["init_equal"] = all(torch.equal(v, s["w0"][k]) for k, v in _weights(a1).items())
    for ag in (a1, a2, b):
        torch.manual_seed(123)
        assert ag.update()
    s["w"] = {"A1": _weights(a1), "A2": _weights(a2), "B": _weights(b)}
    s["len_after_update"] = (len(a1), len(b), b.store.rows)
    # the device actor follows the update (as test_actor_gpu checks select_actions against torch)
    F = env_b.obs_spec().n_feat
    probs = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    obs = torch.empty((n, F), dtype=torch.float32, device="cuda")
    b.device_actor.select_actions(probs=probs, obs_out=obs, count_next=False)
    with torch.no_grad():
        s["prob_err"] = float((probs - b.actor_net(obs)).abs().max())
    s["obs_eq"] = torch.equal(obs, env_b.obs_tensor())
    g2 = env_b.shard.graph_info()
    b.collect(T_COLLECT)
    g3 = env_b.shard.graph_info()
    s["graphs"] = (g0, g1, g2, g3)
    s["rows_second"] = b.store.rows
    _SCEN[key] = s
    return s


@pytest.mark.parametrize("n,precision", COLLECT_CASES)
def test_collect_equals_per_tick_loop(torch_gpu, n, precision):
    torch = torch_gpu
    s = scenario(torch, n, precision)
    A, B = s["A"], s["B"]
    assert B["rows"] == T_COLLECT and B["len"] == T_COLLECT * n
    for k in ("actions", "probs", "rewards", "states"):
        assert A[k].dtype == B[k].dtype and torch.equal(A[k], B[k]), k
    assert torch.equal(B["returned"], B["rewards"])
    assert A["done"] == B["done"] == [False] * (T_COLLECT - 1) + [True]
    for k in ("t_air", "t_mass", "hvac"):
        assert torch.equal(A["final"][k], B["final"][k]), k
    g0, g1, g2, g3 = s["graphs"]
    assert g1["actor_launches"] == g0["actor_launches"] + 1  # the graph path ran
    assert g1["actor_graphs"] == g0["actor_graphs"] + 1
    assert g3["actor_launches"] == g2["actor_launches"] + 1
    assert g3["actor_graphs"] == g2["actor_graphs"] == g1["actor_graphs"]  # the cached graph, replayed
    assert s["rows_second"] == T_COLLECT


@pytest.mark.parametrize("n,precision", COLLECT_CASES)
def test_update_from_store_equals_update_from_buffer(torch_gpu, n, precision):
    torch = torch_gpu
    s = scenario(torch, n, precision)
    assert s["init_equal"]
    assert s["len_after_update"] == (0, 0, 0)
    w = s["w"]
    for k in w["A1"]:
        spread = float((w["A2"][k] - w["A1"][k]).abs().max())
        err = float((w["B"][k] - w["A1"][k]).abs().max())
        print(f"n={n} {precision} {k}: |B - A1| = {err:.3g}, |A2 - A1| = {spread:.3g}")
        assert torch.isfinite(w["B"][k]).all()
        assert err <= 4.0 * spread, (k, err, spread)
    assert not torch.equal(w["B"]["actor.fc.0.weight"], s["w0"]["actor.fc.0.weight"])  # the update moved the policy
    assert not torch.equal(w["B"]["critic.fc.0.weight"], s["w0"]["critic.fc.0.weight"])
    print(f"n={n} {precision}: select_actions after update, max |p - p_torch| = {s['prob_err']:.3g}")
    assert s["obs_eq"]
    assert s["prob_err"] < PROB_ATOL[precision]


def test_rollout_windows_fill_consecutive_rows(torch_gpu):
    """rollout(3, store) then rollout(2, store) fill rows 0-4 and equal one rollout(5) on a twin."""
    from mdr_amd.actor import DeviceActor, make_actor
    from mdr_amd.replay import RolloutStore

    torch = torch_gpu
    n = 77
    ov = dict({"cluster_prop.nb_agents": n}, **SIN)
    env_a, env_b = make_env(ov, 8), make_env(ov, 8)
    actor = make_actor(env_a.obs_spec().n_feat, 2, [100, 100], seed=3).to("cuda")
    da, db = DeviceActor(env_a, actor), DeviceActor(env_b, actor)
    sa, sb = RolloutStore(env_a, 6), RolloutStore(env_b, 6)
    r3 = da.rollout(3, store=sa)
    assert sa.rows == 3 and r3.data_ptr() == sa.rewards.data_ptr()
    r2 = da.rollout(2, store=sa)
    assert sa.rows == 5 and r2.data_ptr() == sa.rewards[3].data_ptr()
    rew = torch.empty((5, n), dtype=torch.float64, device="cuda")
    acts = torch.empty((5, n), dtype=torch.uint8, device="cuda")
    probs = torch.empty((5, n), dtype=torch.float32, device="cuda")
    env_c = make_env(ov, 8)
    DeviceActor(env_c, actor).rollout(5, rewards=rew, actions=acts, probs=probs)  # the rollout without a store
    db.rollout(5, store=sb)
    for x, y, z in ((sa.actions, sb.actions, acts), (sa.probs, sb.probs, probs), (sa.rewards, sb.rewards, rew)):
        assert torch.equal(x[:5], y[:5]) and torch.equal(x[:5], z)
    for k in ("t_air", "t_mass", "hvac", "scalars"):
        assert torch.equal(getattr(sa, k)[:5], getattr(sb, k)[:5]), k
    ar = torch.arange(5 * n, device="cuda")
    assert torch.equal(sa.states(ar), sb.states(ar))
    for k in ("t_air", "t_mass", "hvac"):
        assert torch.equal(getattr(env_a.shard, k), getattr(env_b.shard, k)), k
        assert torch.equal(getattr(env_a.shard, k), getattr(env_c.shard, k)), k


# ------------------------------------------------------------------ 6. common penalty mode
def test_collect_common_penalty_mode_stepwise(torch_gpu):
    """common_L2 rollouts run tick by tick (_rollout_stepwise): env.snapshot before each
    select_actions; the stored states are the per-tick obs_tensor rows."""
    from mdr_amd.mappo import DeviceMAPPO, MAPPOConfig

    torch = torch_gpu
    n, T = 77, 4
    ov = dict({"cluster_prop.nb_agents": n, "reward_prop.penalty_props.mode": "common_L2"}, **SIN)
    env_a, env_b = make_env(ov, 4), make_env(ov, 4)
    a = DeviceMAPPO(env_a, MAPPOConfig(batch_size=256, ppo_update_time=1))
    b = DeviceMAPPO(env_b, MAPPOConfig(batch_size=256, ppo_update_time=1), collect_ticks=T)
    rows, acts, rews = [], [], []
    for _ in range(T):
        rows.append(env_a.obs_tensor().clone())
        acts.append(a.select_actions().clone())
        rews.append(env_a.step_tensor(acts[-1]).clone())
    g0 = env_b.shard.graph_info()
    b.collect(T)
    assert env_b.shard.graph_info()["actor_launches"] == g0["actor_launches"]  # no graph: stepwise
    assert b.store.rows == T and b.store.done == [False] * (T - 1) + [True]
    assert torch.equal(b.store.states(torch.arange(T * n, device="cuda")), torch.cat(rows))
    assert torch.equal(b.store.actions[:T], torch.stack(acts))
    assert torch.equal(b.store.rewards[:T], torch.stack(rews))


# ------------------------------------------------------------------ 7. refusals
def test_refusals(torch_gpu):
    from mdr_amd import _lib
    from mdr_amd.mappo import DeviceMAPPO, MAPPOConfig
    from mdr_amd.replay import RolloutStore

    torch = torch_gpu
    n = 24
    env_rs = make_env(dict({"cluster_prop.nb_agents": n, COMM + "mode": "random_sample"}, **SIN))
    with pytest.raises(ValueError, match="random_sample"):
        RolloutStore(env_rs, 4)
    with pytest.raises(ValueError, match="random_sample"):
        DeviceMAPPO(env_rs, MAPPOConfig(), collect_ticks=4)

    env = make_env(dict({"cluster_prop.nb_agents": n}, **SIN))
    agent = DeviceMAPPO(env, MAPPOConfig(batch_size=16, ppo_update_time=1), collect_ticks=4)
    with pytest.raises(ValueError, match="collect_ticks"):
        DeviceMAPPO(env, MAPPOConfig()).collect(2)
    agent.collect(3)
    with pytest.raises(ValueError, match="overflow"):
        agent.collect(2)
    assert agent.store.rows == 3  # (nothing appended by the refused call)
    # mixing the two buffers before one update
    obs = env.obs_tensor()
    agent.select_actions()
    with pytest.raises(ValueError, match="store_transition after collect"):
        agent.store_transition(obs, obs, env.shard.reward, False)
    # a reset re-draws targets, parameters and links: the stored rows cannot be rebuilt
    env.reset(return_obs=False)
    with pytest.raises(ValueError, match="reset"):
        agent.collect(1)
    with pytest.raises(ValueError, match="reset"):
        agent.store.states(torch.arange(4, device="cuda"))
    agent.store.clear()
    agent.collect(1)  # an empty store follows the reset
    assert agent.store.rows == 1
    agent.store.clear()
    agent.select_actions()
    agent.store_transition(obs, obs, env.shard.reward, False)
    with pytest.raises(ValueError, match="collect\\(\\) after store_transition"):
        agent.collect(1)

    # C level: row0 + n_ticks > cap_rows is MDR_EARG before anything launches
    st = agent.store
    ticks = env.driver_window(2)
    spec, _sc, _keep = env.bound_obs_spec()
    with pytest.raises(_lib.MdrError, match="MDR_EARG"):
        env.shard.actor_rollout_snap(ticks, np.zeros((2, 4)), spec, st.actions, n, st.probs, n, st.rewards, n,
                                     st.snap, 3, use_graph=False)
    with pytest.raises(_lib.MdrError, match="MDR_EARG"):
        env.shard.snapshot(st.snap, 4, _sc)
    with pytest.raises(_lib.MdrError, match="MDR_EARG"):
        env.shard.obs_gather(spec, st.snap, 5, torch.zeros(1, dtype=torch.int64, device="cuda"),
                             torch.empty((1, spec.n_feat), device="cuda"))
