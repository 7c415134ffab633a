"""``EnvBatch``: E independent clusters in one context, a rollout call in one launch
(mdr_batch_set / mdr_batch_rollout / mdr_batch_obs; k_batch_rollout, k_batch_obs).

Every comparison is with stand-alone ``Environment``s of the same seeds stepped through the per-tick
path, ``step_tensor(None, action_mode=c, lookahead=c)``, never with the batch itself, and every
comparison is ==: a block of k_batch_rollout runs the one-tick kernels' own device functions on its
cluster's view of the context (the cluster's size in the signal penalty, its seed and house ids in the
Philox counter), the cluster power is a sum of exact integer counts times the same table entries in the
same class order, and the host drivers of a member are ``driver_window`` of the same RNG.

Shapes (tests/batch_inputs.py): one house; both slots of a lane; config C1 (one ragged wave, the
barrier-free form); a second tile holding one house; the reference's 1,000 agents (8 waves, ragged last
tile); the full 1,024.  tests/test_env_batch_cpu.py asserts under the oracle that the clusters' powers
differ on nearly every tick, so mixed-up counts or drivers cannot pass, and that the lockout acts.
"""
import ctypes as C
import random

import numpy as np
import pytest

import batch_inputs as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def twin(n, seed, extra=None):
    from mdr_amd.environment import Environment

    return Environment(B.props(n, extra), rng=random.Random(seed), seed=seed, population="reference")


def batch(n_envs, n, extra=None):
    from mdr_amd.batch import EnvBatch

    return EnvBatch(B.props(n, extra), n_envs, seeds=B.seeds(n_envs))


def action_matrix(ticks, n_envs, n):
    return np.random.default_rng(B.ACTION_SEED).integers(0, 2, size=(ticks, n_envs, n), dtype=np.uint8)


def loop(torch, env, ticks, source, acts=None):
    """[ticks, n] rewards of the per-tick path on a stand-alone environment."""
    rows = []
    for t in range(ticks):
        if source == "buffer":
            r = env.step_tensor(torch.from_numpy(acts[t]).to(env.shard.device), action_mode="buffer")
        else:
            r = env.step_tensor(None, action_mode=source, lookahead=source)
        rows.append(r.cpu().numpy().copy())
    return np.stack(rows)


def state_of(env):
    sh = env.shard
    return sh.t_air.cpu().numpy(), sh.t_mass.cpu().numpy(), sh.hvac.cpu().numpy(), env._cluster_power()


_REF = {}


def reference(torch, n_envs, n, ticks, source):
    """The stand-alone twins' run of a shape and source, computed once: per member (rewards, t_air, t_mass,
    hvac words, P)."""
    key = (n_envs, n, ticks, source)
    if key not in _REF:
        acts = action_matrix(ticks, n_envs, n) if source == "buffer" else None
        out = []
        for e, s in enumerate(B.seeds(n_envs)):
            env = twin(n, s)
            r = loop(torch, env, ticks, source, None if acts is None else acts[:, e])
            out.append((r,) + state_of(env))
            env.shard.close()
        _REF[key] = out
    return _REF[key]


def fill_pads(torch, b, *views):
    """NaN / all-ones into every pad element of the state and of the given reward / action views."""
    n = b.n
    for v in (b.t_air, b.t_mass) + tuple(x for x in views if x.dtype == torch.float64):
        b.padded(v)[..., n:] = float("nan")
    b.padded(b.hvac)[..., n:] = -1
    for v in views:
        if v.dtype == torch.uint8:
            b.padded(v)[..., n:] = 0xFF


def assert_pads(torch, b, *views):
    n = b.n
    if b.stride == n:
        return
    for v in (b.t_air, b.t_mass) + tuple(x for x in views if x.dtype == torch.float64):
        assert bool(torch.isnan(b.padded(v)[..., n:]).all())
    assert bool((b.padded(b.hvac)[..., n:] == -1).all())
    for v in views:
        if v.dtype == torch.uint8:
            assert bool((b.padded(v)[..., n:] == 0xFF).all())


def assert_members(torch, b, ref, rewards=None):
    torch.cuda.synchronize()
    T, Tm, w, P = (x.cpu().numpy() for x in (b.t_air, b.t_mass, b.hvac, b.cluster_power()))
    for e, (r, t_air, t_mass, hvac, p) in enumerate(ref):
        if rewards is not None:
            np.testing.assert_array_equal(rewards[:, e], r, err_msg=f"rewards of member {e}")
        np.testing.assert_array_equal(T[e], t_air, err_msg=f"t_air of member {e}")
        np.testing.assert_array_equal(Tm[e], t_mass, err_msg=f"t_mass of member {e}")
        np.testing.assert_array_equal(w[e], hvac, err_msg=f"hvac words of member {e}")
        assert P[e] == p, f"cluster power of member {e}"


@pytest.mark.parametrize("source", B.SOURCES)
@pytest.mark.parametrize("n_envs,n,ticks", B.SHAPES)
def test_members_equal_standalone(torch_gpu, n_envs, n, ticks, source):
    """One rollout call of the batch against every member's stand-alone twin: every tick's reward row, the
    final t_air / t_mass / FSM words and the cluster power, ==; the pad elements untouched."""
    torch = torch_gpu
    ref = reference(torch, n_envs, n, ticks, source)
    b = batch(n_envs, n)
    assert (b.n_envs, b.n) == (n_envs, n) and tuple(b.t_air.shape) == (n_envs, n)
    rew = b.empty_rewards(ticks)
    acts = None
    if source == "buffer":
        acts = b.empty_actions(ticks)
        fill_pads(torch, b, rew, acts)
        acts.copy_(torch.from_numpy(action_matrix(ticks, n_envs, n)).to(b.device))
    else:
        fill_pads(torch, b, rew)
    out = b.rollout(ticks, action_mode=source, actions=acts, rewards=rew)
    assert out is rew and tuple(out.shape) == (ticks, n_envs, n)
    assert_members(torch, b, ref, out.cpu().numpy())
    assert_pads(torch, b, rew, *(() if acts is None else (acts,)))
    b.close()


@pytest.mark.parametrize("source", ["bangbang", "random"])
def test_calls_chain(torch_gpu, source):
    """Two rollouts in a row, and rollout -> step_tensor -> rollout, equal one call of the summed length;
    a stride-0 reward buffer holds the last tick's row."""
    torch = torch_gpu
    n_envs, n, ticks = 3, 129, 45
    ref = reference(torch, n_envs, n, ticks, source)
    b = batch(n_envs, n)
    r = np.concatenate([b.rollout(20, action_mode=source).cpu().numpy(),
                        b.rollout(25, action_mode=source).cpu().numpy()])
    assert_members(torch, b, ref, r)
    b.close()
    b = batch(n_envs, n)
    last = b.empty_rewards(None)
    fill_pads(torch, b, last)
    r0 = b.rollout(20, action_mode=source).cpu().numpy()
    r1 = b.step_tensor(action_mode=source).cpu().numpy()
    assert r1.shape == (n_envs, n)
    out = b.rollout(24, action_mode=source, rewards=last)
    assert out is last
    assert_members(torch, b, ref)
    for e in range(n_envs):
        np.testing.assert_array_equal(r0[:, e], ref[e][0][:20])
        np.testing.assert_array_equal(r1[e], ref[e][0][20])
        np.testing.assert_array_equal(last[e].cpu().numpy(), ref[e][0][44])
    assert_pads(torch, b, last)
    b.close()


def test_reset_of_one_member(torch_gpu):
    """reset([1]) in the middle of a run: members 0 and 2 continue == their twins, member 1 equals a twin
    reset at the same point."""
    torch = torch_gpu
    n_envs, n, source = 3, 50, "deadband_bangbang"
    b = batch(n_envs, n)
    twins = [twin(n, s) for s in B.seeds(n_envs)]
    r0 = b.rollout(17, action_mode=source).cpu().numpy()
    t0 = [loop(torch, tw, 17, source) for tw in twins]
    b.reset([1])
    twins[1].reset(return_obs=False)
    assert [m._tick for m in b.members] == [17, 0, 17]
    r1 = b.rollout(23, action_mode=source).cpu().numpy()
    t1 = [loop(torch, tw, 23, source) for tw in twins]
    ref = [(np.concatenate([t0[e], t1[e]]),) + state_of(twins[e]) for e in range(n_envs)]
    assert_members(torch, b, ref, np.concatenate([r0, r1]))
    for tw in twins:
        tw.shard.close()
    b.close()


@pytest.mark.parametrize("n_envs,n,extra", [(e, n, None) for e, n in B.OBS_SHAPES] + [
    (3, 129, {"cluster_prop.message_prop.thermal": True, "cluster_prop.message_prop.hvac": True})])
def test_obs_equals_standalone(torch_gpu, n_envs, n, extra):
    """obs_tensor() after a reset and after a rollout == every twin's obs_tensor(): the ring wraps inside
    the cluster and the uniform features are the cluster's own."""
    torch = torch_gpu
    b = batch(n_envs, n, extra)
    twins = [twin(n, s, extra) for s in B.seeds(n_envs)]
    for ticks in (0, 9):
        if ticks:
            b.rollout(ticks, action_mode="random")
            for tw in twins:
                loop(torch, tw, ticks, "random")
        obs = b.obs_tensor()
        torch.cuda.synchronize()
        o = obs.cpu().numpy()
        assert o.dtype == np.float32 and o.shape[:2] == (n_envs, n)
        for e, tw in enumerate(twins):
            np.testing.assert_array_equal(o[e], tw.obs_tensor().cpu().numpy(), err_msg=f"member {e}, {ticks} ticks")
    for tw in twins:
        tw.shard.close()
    b.close()


def test_python_refusals_touch_nothing(torch_gpu):
    """A refused rollout leaves every member's RNG, tick counter and date, and the device state, as they were."""
    torch = torch_gpu
    b = batch(3, 50)
    b.rollout(3, action_mode="bangbang")
    torch.cuda.synchronize()

    def snap():
        return ([m.rng.getstate() for m in b.members], [(m._tick, m.date_time, float(m.current_od_temp)) for m in b.members],
                [x.clone() for x in (b._store.t_air, b._store.t_mass, b._store.hvac, b.cluster_power())])

    before = snap()
    plain_r = torch.empty((4, 3, 50), dtype=torch.float64, device=b.device)
    plain_a = torch.zeros((4, 3, 50), dtype=torch.uint8, device=b.device)
    bad = [dict(n_ticks=0), dict(n_ticks=4, action_mode="greedy"), dict(n_ticks=4, action_mode="buffer"),
           dict(n_ticks=4, action_mode="buffer", actions=plain_a), dict(n_ticks=4, rewards=plain_r),
           dict(n_ticks=4, rewards=b.empty_rewards(5)), dict(n_ticks=4, action_mode="random", actions=b.empty_actions(4)),
           dict(n_ticks=4, rewards=b.empty_rewards(4).to(torch.float32))]
    for kw in bad:
        with pytest.raises(ValueError):
            b.rollout(**kw)
    with pytest.raises(ValueError):
        b.reset([3])
    torch.cuda.synchronize()
    after = snap()
    assert before[0] == after[0] and before[1] == after[1]
    for x, y in zip(before[2], after[2]):
        assert torch.equal(x, y)
    b.close()


def test_c_abi_refusals(torch_gpu):
    """mdr_batch_set refuses a cluster of 1,025 houses and a common penalty mode with MDR_EARG; after it the
    single-cluster entry points answer MDR_ESTATE; the batch entry points without it do too."""
    from mdr_amd import _lib as L
    from mdr_amd import population as popmod
    from mdr_amd.shard import HipShard

    def ctx_of(p, total):
        table, _ = popmod.cap_table(p.cluster_prop.house_prop.hvac_prop, ())
        return HipShard(p, total, 0, total, "cuda", table)

    seeds = (C.c_uint64 * 2)(8, 9)
    sh = ctx_of(B.props(50), 2 * 1152)
    lib = sh.lib
    assert lib.mdr_batch_set(sh.ctx, 2, 1025, seeds) == -1 and b"1024" in lib.mdr_last_error()
    assert lib.mdr_batch_set(sh.ctx, 2, 50, seeds) == -1  # (2 * 128 houses expected)
    assert lib.mdr_batch_set(sh.ctx, 0, 50, seeds) == -1
    assert lib.mdr_batch_set(sh.ctx, 2, 50, None) == -1
    tick = L.mdr_tick(20.0, 0.0, 1000.0, 0)
    assert lib.mdr_batch_rollout(sh.ctx, 1, C.byref(tick), None, 0, L.ACT_RANDOM, L.ptr(sh.reward), 0, L.ptr(sh.p_dev),
                                 sh.stream()) == -5
    assert lib.mdr_batch_set(sh.ctx, 2, 1100, seeds) == -1  # (the right context size, a cluster too long)
    sh.close()
    sh = ctx_of(B.props(50, {"reward_prop.penalty_props.mode": "common_L2"}), 256)
    assert lib.mdr_batch_set(sh.ctx, 2, 50, seeds) == -1 and b"common" in lib.mdr_last_error()
    sh.close()
    sh = ctx_of(B.props(50), 256)
    assert lib.mdr_batch_set(sh.ctx, 2, 50, seeds) == 0, lib.mdr_last_error()
    assert lib.mdr_step(sh.ctx, None, L.ACT_RANDOM, C.byref(tick), L.ptr(sh.reward), 0, 0, None, None, sh.stream()) == -5
    assert b"batch" in lib.mdr_last_error()
    assert lib.mdr_power_counts(sh.ctx, None, L.ACT_RANDOM, 0, sh.stream()) == -5
    assert lib.mdr_rollout(sh.ctx, 1, C.byref(tick), None, 0, L.ACT_RANDOM, L.ptr(sh.reward), 0, None, 0, sh.stream()) == -5
    assert lib.mdr_cluster_stats(sh.ctx, None, L.ptr(sh.reward), sh.stream()) == -5
    # argument errors of the batch entry points come before anything is staged or launched
    assert lib.mdr_batch_rollout(sh.ctx, 0, C.byref(tick), None, 0, L.ACT_RANDOM, L.ptr(sh.reward), 0, L.ptr(sh.p_dev),
                                 sh.stream()) == -1
    assert lib.mdr_batch_rollout(sh.ctx, 1, C.byref(tick), None, 0, L.ACT_BUFFER, L.ptr(sh.reward), 0, L.ptr(sh.p_dev),
                                 sh.stream()) == -1
    assert lib.mdr_batch_rollout(sh.ctx, 1, C.byref(tick), None, 0, 5, L.ptr(sh.reward), 0, L.ptr(sh.p_dev),
                                 sh.stream()) == -1
    sh.close()
