"""Per-tick stats rows on the device (k_tick_stats + k_tick_stats_finish): ``Shard.tick_stats``,
``DeviceActor.rollout(stats=...)``, ``DeviceMetrics.update_rollout`` and ``DeviceMAPPO.evaluate``.

Reference: Metrics.update (server/app/services/metrics_service.py:108-157) walks the per-house obs
dicts every tick; TrainingManager.test (server/app/services/training_manager.py:265-295) runs the
policy on a reset deep copy of the env and logs three means (metrics_service.py:259-282).

Bounds.  A row's sum slots are compared with the exactly rounded sum (math.fsum) of the per-house
terms formed in float64 with the kernel's expressions: |got - want| <= n * 2^-52 * fsum(|terms|), the
first-order bound of any summation order, doubled (it covers a contracted e * e).  The max, the two
counts and P are compared with ==.  Rows written inside the rollout graph are the stand-alone
call's bits.  ``update_rollout`` against per-tick ``update`` and ``evaluate`` against the reference's
formulas in numpy: rtol 1e-12 (all terms of each sum have one sign, so the derived bound n * 2^-52 is
4.6e-13 at 2,085 houses); accumulators that hold no sum over houses are compared with ==.
"""
import copy
import json
import math
import random

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu

SIN = {"power_grid_prop.signal_properties.mode": "sinusoidals"}
SUM_SLOTS = (0, 1, 3, 4, 5, 6, 7, 8, 9)
# k_tick_stats' grid: at most kTickBlocks = 1,024 blocks of 256 lanes, 4 houses per lane and trip
# (csrc/mdr_kernels.h), i.e. 1,048,576 houses per trip of the grid-stride loop: lane 0 makes a second
# trip for the quad of houses 1,048,576..1,048,579 and three tail houses follow
TWO_TRIPS = 1024 * 256 * 4 + 7


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def make_env(n, extra=None, seed=5, **kw):
    from mdr_amd.environment import Environment

    ov = dict({"cluster_prop.nb_agents": n}, **SIN)
    ov.update(extra or {})
    return Environment(gu.props_from_overrides(ov), rng=random.Random(seed), **kw)


# ------------------------------------------------------------------ 1. the kernel against exact sums
def exact_row(env, reward):
    """Per slot (terms float64 [n] or None, exact value) from the downloaded state."""
    sh = env.shard
    st = sh.host_state()
    T, Tm = st["T"], st["Tm"]
    tg = sh.target.cpu().numpy()
    N = float(env.n)
    e = T - tg / N
    d = T - tg
    terms = {0: e, 1: np.abs(e), 3: e * e, 5: T, 6: d, 7: np.abs(d), 8: Tm, 9: tg}
    terms[4] = reward / N if reward is not None else np.zeros_like(T)
    exact = {2: max(0.0, float(e.max())), 10: float(st["lock"].sum()), 11: float(st["on"].sum())}
    return terms, exact


def check_row(row, env, reward, tag):
    n = env.n_local
    terms, exact = exact_row(env, reward)
    for k in SUM_SLOTS:
        want = math.fsum(terms[k])
        bound = n * 2.0 ** -52 * math.fsum(np.abs(terms[k]))
        err = abs(float(row[k]) - want)
        print(f"{tag} slot {k}: got {row[k]!r} want {want!r} |err| {err:.3g} bound {bound:.3g}")
        assert err <= bound, (tag, k, row[k], want, err, bound)
    for k, v in exact.items():
        assert float(row[k]) == v, (tag, k, row[k], v)
    assert float(row[12]) == float(env.shard.p_dev.item()), (tag, row[12])
    assert list(row[13:]) == [0.0, 0.0, 0.0], (tag, row[13:])


@pytest.mark.parametrize("n", [13, 77, 300, 4099, TWO_TRIPS])
def test_kernel_against_exact_sums(torch_gpu, n):
    torch = torch_gpu
    env = make_env(n, population="synthetic", seed=3)
    sh = env.shard
    rs = np.random.RandomState(n % 1000)
    rew2 = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    for t in range(3):
        a = torch.from_numpy(rs.randint(0, 2, n).astype(np.uint8)).to("cuda")
        env.step_tensor(a, rewards=rew2[t % 2])
    # ticks 0 and 2 wrote row 0, tick 1 row 1: the last tick's rewards are row 0, so step once more into row 1
    a = torch.from_numpy(rs.randint(0, 2, n).astype(np.uint8)).to("cuda")
    r1 = env.step_tensor(a, rewards=rew2[1])
    assert r1.data_ptr() == rew2.data_ptr() + 8 * n
    if n % 2:
        assert r1.data_ptr() % 16 == 8  # an odd row stride: row 1 is only 8-B aligned (the scalar reward path)
    rows = torch.full((3, 16), -7.0, dtype=torch.float64, device="cuda")
    sh.tick_stats(r1, rows[0])
    sh.tick_stats(None, rows[1])
    flat = r1.clone()
    assert flat.data_ptr() % 16 == 0
    sh.tick_stats(flat, rows[2])
    h = rows.cpu().numpy()
    rew = r1.cpu().numpy()
    assert np.abs(rew).sum() > 0
    check_row(h[0], env, rew, f"n={n} row 1 of [2, n]")
    check_row(h[1], env, None, f"n={n} no reward")
    assert h[1][4] == 0.0
    # the summation order does not depend on the reward row's alignment
    assert np.array_equal(h[0], h[2])
    # and the 12 values agree with mdr_cluster_stats' (another blocked order) within both bounds
    from mdr_amd.services import cluster_stats

    cs = cluster_stats(env, r1)
    terms, _ = exact_row(env, rew)
    for k in range(12):
        if k in SUM_SLOTS:
            assert abs(cs[k] - h[0][k]) <= 2 * n * 2.0 ** -52 * math.fsum(np.abs(terms[k])), k
        else:
            assert cs[k] == h[0][k], k


# ------------------------------------------------------------------ 2. against the reference's Metrics
def test_rows_feed_reference_metrics(torch_gpu):
    """test_services_gpu's services.npz loop with the rows feeding the accumulators, its tolerances."""
    from mdr_amd.services import DeviceMetrics, RolloutStats, observe

    d = gu.load("services.npz")
    meta = json.loads(bytes(d["meta_json"]).decode())
    N, T = meta["N"], meta["T"]
    env = make_env(N, {"power_grid_prop.signal_properties.mode": meta["signal"]}, seed=meta["seed"])
    env.reset(return_obs=False)
    env.reset(return_obs=False)
    m = DeviceMetrics()
    m.initialize(N, meta["start_stats_from"], T)
    stats = RolloutStats(env, T)
    c = "deadband_bangbang"
    for step in range(T):
        prev = observe(env)
        row = stats.begin_rows(1)
        stats.record_power(row)
        rewards = env.step_tensor(None, action_mode=c, lookahead=c)
        env.shard.tick_stats(rewards, stats.stats[row])
        stats.commit_rows([prev["reg_signal"]], [prev["OD_temp"]], [env.power_grid.current_signal], first=True)
        m.update_rollout(stats, step, row0=row)
        assert stats.prev()["cluster_hvac_power"][row] == prev["cluster_hvac_power"]
        for f in m.FIELDS:
            np.testing.assert_allclose(getattr(m, f), d[f"metrics_{f}"][step], rtol=1e-12, atol=1e-9,
                                       err_msg=f"{f} step {step}")
    m.update_rms(T)
    np.testing.assert_allclose([m.rmse_sig_per_ag, m.rmse_temp, m.rms_max_error_temp], d["rms"], rtol=1e-12)


# ------------------------------------------------------------------ 3 / 4. in-graph rows, update_rollout
T_ROLL = 6
VARIANTS = {
    "fused": ({}, [100, 100], False),
    "fused_store": ({}, [100, 100], True),
    "chain": ({}, [32], False),
    "common_L2": ({"reward_prop.penalty_props.mode": "common_L2"}, [100, 100], False),
}
HOUSE_SUMS = ("cumul_avg_reward", "cumul_temp_offset", "cumul_temp_error", "cumul_squared_error_temp")
_SCEN = {}


def scenario(torch, n, variant):
    """Twins: A runs rollout(6, stats=...) twice (capture, replay), B the per-tick loop of
    select_actions, step_tensor, tick_stats; both feed a DeviceMetrics (A by update_rollout)."""
    key = (n, variant)
    if key in _SCEN:
        return _SCEN[key]
    from mdr_amd.actor import DeviceActor, make_actor
    from mdr_amd.replay import RolloutStore
    from mdr_amd.services import DeviceMetrics, RolloutStats, observe

    extra, layers, with_store = VARIANTS[variant]
    env_a, env_b = make_env(n, extra, seed=8), make_env(n, extra, seed=8)
    actor = make_actor(env_a.obs_spec().n_feat, 2, layers, seed=3).to("cuda")
    da, db = DeviceActor(env_a, actor), DeviceActor(env_b, actor)
    s = {"fused": da.fused(), "stepwise": env_a.shard.penalty_mode != 0}
    ma, mb = DeviceMetrics(), DeviceMetrics()
    for m in (ma, mb):
        m.initialize(n, 4, 2 * T_ROLL)  # start_stats_from inside the first call
    stats = RolloutStats(env_a, T_ROLL)
    store = RolloutStore(env_a, T_ROLL) if with_store else None
    rew = None if with_store else torch.empty((T_ROLL, n), dtype=torch.float64, device="cuda")
    act = None if with_store else torch.empty((T_ROLL, n), dtype=torch.uint8, device="cuda")
    A = {"rows": [], "rewards": [], "actions": [], "graphs": [env_a.shard.graph_info()]}
    for call in range(2):
        stats.clear()
        if store is not None:
            store.clear()
        r = da.rollout(T_ROLL, rewards=rew, actions=act, store=store, stats=stats)
        assert stats.rows == T_ROLL
        A["graphs"].append(env_a.shard.graph_info())
        A["rows"].append(stats.stats.clone())
        A["rewards"].append(r.clone())
        A["actions"].append((store.actions if store is not None else act).clone())
        ma.update_rollout(stats, call * T_ROLL)
        if call == 0:
            A["host"], A["prev"] = stats.host().copy(), {k: v.copy() for k, v in stats.prev().items()}
    A["final"] = {k: getattr(env_a.shard, k).clone() for k in ("t_air", "t_mass", "hvac")}
    B = {"rows": torch.empty((2 * T_ROLL, 16), dtype=torch.float64, device="cuda"), "rewards": [], "actions": [],
         "prev": []}
    for t in range(2 * T_ROLL):
        prev = observe(env_b)
        a, _p = db.select_actions()
        r = env_b.step_tensor(a)
        env_b.shard.tick_stats(r, B["rows"][t])
        mb.update(prev, env_b, r, t)
        B["prev"].append(dict(prev, signal_post=env_b.power_grid.current_signal))
        B["rewards"].append(r.clone())
        B["actions"].append(a.clone())
    B["final"] = {k: getattr(env_b.shard, k).clone() for k in ("t_air", "t_mass", "hvac")}
    s.update(A=A, B=B, ma=ma, mb=mb)
    _SCEN[key] = s
    return s


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("n", [77, 2085])
def test_in_graph_rows_are_the_standalone_kernels(torch_gpu, n, variant):
    torch = torch_gpu
    s = scenario(torch, n, variant)
    A, B = s["A"], s["B"]
    assert s["fused"] == (variant != "chain")
    g0, g1, g2 = A["graphs"]
    if s["stepwise"]:
        assert g2["actor_launches"] == g0["actor_launches"]  # tick by tick: no graph
    else:
        assert g1["actor_graphs"] == g0["actor_graphs"] + 1 and g1["actor_launches"] == g0["actor_launches"] + 1
        assert g2["actor_graphs"] == g1["actor_graphs"] and g2["actor_launches"] == g1["actor_launches"] + 1  # replay
        assert g2["guarded"] == g2["rollout_graphs"] + g2["actor_graphs"]  # kernels only: the memset guard walked it
    for call in range(2):
        sl = slice(call * T_ROLL, (call + 1) * T_ROLL)
        assert torch.equal(A["rows"][call], B["rows"][sl]), call
        assert torch.equal(A["rewards"][call], torch.stack(B["rewards"][sl])), call
        assert torch.equal(A["actions"][call], torch.stack(B["actions"][sl])), call
    assert float(B["rows"][:, 4].abs().min()) > 0 and float(B["rows"][:, 12].min()) >= 0
    for k in ("t_air", "t_mass", "hvac"):
        assert torch.equal(A["final"][k], B["final"][k]), k
    # the host's side of the rows: the scalars tick t's obs carried, the post-step signal
    assert A["host"].shape == (T_ROLL, 16) and A["host"].dtype == np.float64
    assert np.array_equal(A["host"], B["rows"][:T_ROLL].cpu().numpy())
    for k in ("reg_signal", "OD_temp", "cluster_hvac_power", "signal_post"):
        assert list(A["prev"][k]) == [p[k] for p in B["prev"][:T_ROLL]], k


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("n", [77, 2085])
def test_update_rollout_equals_per_tick_update(torch_gpu, n, variant):
    s = scenario(torch_gpu, n, variant)
    ma, mb = s["ma"], s["mb"]
    for f in ma.FIELDS:
        got, want = getattr(ma, f), getattr(mb, f)
        print(f"n={n} {variant} {f}: update_rollout {got!r} update {want!r}")
        assert want != 0.0, f
        if f in HOUSE_SUMS:
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f)
        else:  # the max, and accumulators of per-tick scalars (signal, OD temperature, P): the same arithmetic
            assert got == want, f
    ma.update_rms(2 * T_ROLL)
    mb.update_rms(2 * T_ROLL)
    np.testing.assert_allclose([ma.rmse_sig_per_ag, ma.rmse_temp, ma.rms_max_error_temp],
                               [mb.rmse_sig_per_ag, mb.rmse_temp, mb.rms_max_error_temp], rtol=1e-12)


def test_collect_feeds_metrics(torch_gpu):
    """collect(n, metrics=...) == collect(n) on a twin + per-row update; the transitions are unchanged."""
    from mdr_amd.mappo import DeviceMAPPO, MAPPOConfig
    from mdr_amd.services import DeviceMetrics

    torch = torch_gpu
    n = 77
    env_a, env_b = make_env(n, seed=2), make_env(n, seed=2)
    cfg = MAPPOConfig(batch_size=64, ppo_update_time=1)
    a, b = DeviceMAPPO(env_a, cfg, collect_ticks=4), DeviceMAPPO(env_b, cfg, collect_ticks=4)
    m = DeviceMetrics()
    m.initialize(n, 0, 8)
    ret = sq = 0.0
    for call in range(2):
        a.store.clear()
        b.store.clear()
        a.collect(4, metrics=m)
        b.collect(4)
        assert a.stats.rows == 4 and torch.equal(a.store.rewards, b.store.rewards)
        assert torch.equal(a.store.actions, b.store.actions) and torch.equal(a.store.t_air, b.store.t_air)
        for t in range(4):  # time steps 4 * call + t, all >= start_stats_from
            ret += a.stats.host()[t, 4]
            sq += a.stats.host()[t, 3]
    assert a.collected_ticks == 8
    assert ret != 0.0 and m.cumul_avg_reward == ret and m.cumul_squared_error_temp == sq
    assert m.cumul_cons > 0 and m.cumul_squared_error_sig > 0


# ------------------------------------------------------------------ 5. evaluate
def _agent(n, seed):
    from mdr_amd.mappo import DeviceMAPPO, MAPPOConfig

    env = make_env(n, seed=seed)
    return env, DeviceMAPPO(env, MAPPOConfig(batch_size=64, ppo_update_time=1), precision="fp32", collect_ticks=4)


def _train_state(env):
    sh = env.shard
    return ({k: getattr(sh, k).clone() for k in ("t_air", "t_mass", "hvac", "target", "ua")}, env._tick, env.date_time,
            env._cluster_power(), env.current_od_temp, env.power_grid.current_signal, sh.graph_info())


@pytest.mark.parametrize("n", [77, 2085])
def test_evaluate_is_the_references_test(torch_gpu, n):
    from mdr_amd.actor import DeviceActor

    torch = torch_gpu
    T = 12
    env_a, a = _agent(n, 11)
    env_b, b = _agent(n, 11)
    for ag in (a, b):  # a training env that has moved on from its reset
        ag.collect(3)
        ag.store.clear()
    before = _train_state(env_a)
    got = a.evaluate(T)
    assert sorted(got) == ["Mean test return", "Test mean signal error", "Test mean temperature error"]

    # B: TrainingManager.test by hand (training_manager.py:265-295)
    ev = copy.deepcopy(env_b)
    ev.reset(return_obs=False)
    da = DeviceActor(ev, b.actor_net, precision="fp32")
    tg = ev.shard.target.cpu().numpy()
    ret = temp = sig = 0.0
    for _ in range(T):
        act, _p = da.select_actions()
        r = ev.step_tensor(act).cpu().numpy()
        Tair = ev.shard.t_air.cpu().numpy()
        P, s = ev._cluster_power(), ev.power_grid.current_signal
        for i in range(0, n, 1 if n < 100 else n):  # (house by house at 77; vectorised terms at 2,085)
            sl = slice(i, i + 1) if n < 100 else slice(None)
            ret += float(np.sum(r[sl] / n))
            temp += float(np.sum(np.abs(Tair[sl] - tg[sl]) / n))
            sig += float(np.abs(s - P) / n ** 2) * (1 if n < 100 else n)
    want = {"Mean test return": ret / T, "Test mean temperature error": temp / T, "Test mean signal error": sig / T}
    for k in want:
        print(f"n={n} {k}: evaluate {got[k]!r} manual {want[k]!r}")
        assert want[k] != 0.0
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)

    # the training env is where it was
    after = _train_state(env_a)
    for k, v in before[0].items():
        assert torch.equal(v, after[0][k]), k
    assert before[1:] == after[1:]
    # the shared RNG advanced alike on both sides: the twins go on collecting the same transitions
    ra, rb = a.collect(4).clone(), b.collect(4).clone()
    assert torch.equal(ra, rb) and torch.equal(a.store.actions, b.store.actions)
    assert torch.equal(a.store.probs, b.store.probs)
    for k in ("t_air", "t_mass", "hvac"):
        assert torch.equal(getattr(env_a.shard, k), getattr(env_b.shard, k)), k

    # a caller-kept twin: its context and graph are reused
    twin = copy.deepcopy(env_a)
    o1 = a.evaluate(T, env=twin)
    g1 = twin.shard.graph_info()
    o2 = a.evaluate(T, env=twin)
    g2 = twin.shard.graph_info()
    assert g2["actor_graphs"] == g1["actor_graphs"] == 1 and g2["actor_launches"] == g1["actor_launches"] + 1
    assert all(np.isfinite(v) for v in list(o1.values()) + list(o2.values()))
    o3, acts = a.evaluate(T, env=twin, return_actions=True)
    assert acts.shape == (T, n) and acts.dtype == torch.uint8 and int(acts.max()) <= 1
    assert sorted(o3) == sorted(got)
    with pytest.raises(ValueError, match="training env"):
        a.evaluate(T, env=env_a)


# ------------------------------------------------------------------ 6. refusals
def test_refusals(torch_gpu):
    from mdr_amd import _lib
    from mdr_amd.actor import DeviceActor, make_actor
    from mdr_amd.services import RolloutStats

    torch = torch_gpu
    n = 24
    env, other = make_env(n), make_env(n)
    da = DeviceActor(env, make_actor(env.obs_spec().n_feat, 2, [100, 100], seed=3).to("cuda"))
    with pytest.raises(ValueError, match="capacity"):
        RolloutStats(env, 0)
    stats = RolloutStats(env, 4)
    da.rollout(3, stats=stats)
    tick = env._tick
    with pytest.raises(ValueError, match="overflow"):
        da.rollout(2, stats=stats)
    assert stats.rows == 3 and env._tick == tick  # (nothing ran)
    with pytest.raises(ValueError, match="another environment"):
        da.rollout(1, stats=RolloutStats(other, 4))
    assert env._tick == tick

    # C level: stats_row0 + n_ticks past the rows is MDR_EARG with nothing launched
    g0 = env.shard.graph_info()
    state = env.shard.t_air.clone()
    ticks = env.driver_window(2)
    spec, _sc, _keep = env.bound_obs_spec()
    rew = torch.empty((2, n), dtype=torch.float64, device="cuda")
    filled = stats.stats.clone()
    with pytest.raises(_lib.MdrError, match="MDR_EARG.*stats_row0"):
        env.shard.actor_rollout_stats(ticks, np.zeros((2, 4)), spec, None, 0, None, 0, rew, n, None, 0, stats.stats, 3)
    assert env.shard.graph_info() == g0 and torch.equal(env.shard.t_air, state) and torch.equal(stats.stats, filled)

    # a sharded env: the Python store, and the C calls of a context with a communicator
    half = make_env(n, rank=0, world=2, comm=object())
    with pytest.raises(ValueError, match="sharded"):
        RolloutStats(half, 4)
    keep = (_lib.HOST_ALLREDUCE_FN(lambda *a: 0), _lib.HOST_SENDRECV_FN(lambda *a: 0))
    _lib.check(other.shard.lib.mdr_comm_host(other.shard.ctx, 1, 0, keep[0], keep[1], None), "mdr_comm_host")
    out = torch.full((16,), -7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        other.shard.tick_stats(None, out)
    spec_o, _sc, _keep = other.bound_obs_spec()
    with pytest.raises(_lib.MdrError, match="MDR_ESTATE"):
        other.shard.actor_rollout_stats(other.driver_window(1), np.zeros((1, 4)), spec_o, None, 0, None, 0, rew, n,
                                        None, 0, torch.zeros((4, 16), dtype=torch.float64, device="cuda"), 0)
    assert float(out.min()) == -7.0


# ------------------------------------------------------------------ 7. actor graph keys partition the calls
def test_actor_graph_keys_partition_the_calls(torch_gpu):
    """One graph per (snapshot rows?, stats rows?) form of the same call, each replayed by its repeat:
    a snapshot and a stats buffer are part of the key, ``row0`` only with a snapshot.  96 houses: three
    full 32-house actor tiles."""
    import ctypes as C

    from mdr_amd import _lib as L
    from mdr_amd.actor import DeviceActor, make_actor
    from mdr_amd.replay import RolloutStore
    from mdr_amd.services import RolloutStats

    torch = torch_gpu
    n, T = 96, 2
    env = make_env(n, seed=8)
    sh = env.shard
    da = DeviceActor(env, make_actor(env.obs_spec().n_feat, 2, [100, 100], seed=3).to("cuda"))
    assert da.fused()
    da.rollout(1)  # (off the reset state; its own graph is cached before the counts below)
    store, stats = RolloutStore(env, 8), RolloutStats(env, 8)
    spec, _sc, _keep = env.bound_obs_spec()
    sh.p_dev.fill_(float(env._P_host))
    solar0 = float(env._solar)
    ticks = env.driver_window(T)
    osc = np.zeros((T, 4), np.float64)
    osc[:, 1], osc[0, 2], osc[1:, 2], osc[:, 3] = ticks.s_prev, solar0, ticks.solar[:-1], ticks.t_od_prev
    rew = torch.empty((T, n), dtype=torch.float64, device="cuda")
    act = torch.empty((T, n), dtype=torch.uint8, device="cuda")
    state = {k: getattr(sh, k).clone() for k in ("t_air", "t_mass", "hvac", "p_dev")}
    snap_bufs = (store.t_air, store.t_mass, store.hvac, store.scalars)

    def call(form, row0=0):
        """The same two ticks from the same state; returns what the call wrote."""
        for k, v in state.items():
            getattr(sh, k).copy_(v)
        for b in (rew, act, stats.stats) + snap_bufs:
            b.zero_()
        a = (ticks, osc, spec, act, n, None, 0, rew, n)
        if form == "plain":
            sh.actor_rollout(*a)
        elif form == "plain_by_snap":  # (the C entry point itself: snap == NULL, row0 ignored)
            L.check(sh.lib.mdr_actor_rollout_snap(sh.ctx, T, ticks.ptr(), osc.ctypes.data, C.byref(spec), L.ptr(act), n,
                                                  0, 0, L.ptr(rew), n, L.ptr(sh.p_dev), 1, None, row0, sh.stream()),
                    "mdr_actor_rollout_snap")
        elif form == "snap":
            sh.actor_rollout_snap(*a, store.snap, row0)
        elif form == "stats":
            sh.actor_rollout_stats(*a, None, 0, stats.stats, 0)
        else:
            sh.actor_rollout_stats(*a, store.snap, row0, stats.stats, 0)
        return [x.clone() for x in (rew, act, stats.stats) + snap_bufs] + [getattr(sh, k).clone() for k in state]

    forms = ("plain", "snap", "stats", "both")
    g0 = sh.graph_info()
    first = {f: call(f) for f in forms}
    g1 = sh.graph_info()
    assert g1["actor_graphs"] == g0["actor_graphs"] + 4 and g1["actor_launches"] == g0["actor_launches"] + 4
    again = {f: call(f) for f in forms}
    g2 = sh.graph_info()
    assert g2["actor_graphs"] == g1["actor_graphs"] and g2["actor_launches"] == g1["actor_launches"] + 4
    for f in forms:
        for i, (x, y) in enumerate(zip(first[f], again[f])):
            assert torch.equal(x, y), (f, i)
    # the forms ran the same ticks, and each wrote exactly its own rows
    for f in forms[1:]:
        assert torch.equal(first[f][0], first["plain"][0]) and torch.equal(first[f][1], first["plain"][1]), f
    assert float(first["plain"][0].abs().max()) > 0
    for f in forms:
        assert bool(first[f][2][:T].any()) == (f in ("stats", "both")), f
        assert bool(first[f][3][:T].any()) == (f in ("snap", "both")), f
    assert torch.equal(first["both"][2], first["stats"][2])
    for i in range(3, 7):
        assert torch.equal(first["both"][i], first["snap"][i]), i

    # without a snapshot row0 is no part of the key; with one it is
    out = call("plain_by_snap", row0=5)
    g3 = sh.graph_info()
    assert g3["actor_graphs"] == g2["actor_graphs"] and g3["actor_launches"] == g2["actor_launches"] + 1
    for i, (x, y) in enumerate(zip(first["plain"], out)):
        assert torch.equal(x, y), i
    out = call("snap", row0=5)
    g4 = sh.graph_info()
    assert g4["actor_graphs"] == g3["actor_graphs"] + 1 and g4["actor_launches"] == g3["actor_launches"] + 1
    assert torch.equal(out[0], first["snap"][0]) and torch.equal(out[3][5:5 + T], first["snap"][3][:T])
    assert not bool(out[3][:T].any())
