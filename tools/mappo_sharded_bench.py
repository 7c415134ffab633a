"""What recording training transitions costs the sharded MA-PPO rollout, and what the sharded update's
allreduce costs a minibatch.

    python tools/mappo_sharded_bench.py [--houses 131072 1048576] [--ticks 20] [--rounds 7]
                                        [--out profiles/r16_mappo_sharded.json]

One process, RCCL world 1 (the library's own communicator, every exchange to self) with
MDR_OPT_FORCE_HALO, so the ring halo is exchanged, recorded and read back as on a real shard.  Config
C5 (bench.py's env_props, the reference actor init), fp32 actor precision, synthetic houses.  Per size
three legs, each producing [ticks, N] actions, probabilities and rewards, alternating --rounds times
after a warm-up of the same shapes, device events around each leg:
* collect        — DeviceActor.rollout(ticks, store=RolloutStore): mdr_actor_rollout_sharded_snap, one
                   k_snap_halo per tick (40 B per house + the halo row);
* rollout        — mdr_actor_rollout_sharded, the same C loop without a store;
* per_tick_loop  — the only sharded training path before the sharded store: per tick select_actions,
                   step_tensor, obs_tensor().clone() and store_transition.
Then, at --update-houses, one PPO epoch of DeviceMAPPO.update() after collect(--update-ticks) on the
sharded environment (each minibatch: owned rows, one integer allreduce) and on a single-process one,
alternating, as us per minibatch.

One JSON line (also written to --out): per leg the median and the spread (min, max).  RCCL at
world > 1 is not measured here.
"""
import argparse
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-demandresponse_amd")]

STEP_TBPS = 5.3  # the step kernel's achieved HBM rate: the snapshot's derived time uses it
UNSHARDED_STORE_US_1M = 6.0  # profiles/r08_collect.json: rollout_store - rollout at 1,048,576 houses


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "samples": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--houses", type=int, nargs="+", default=[131072, 1048576])
    ap.add_argument("--ticks", type=int, default=20, help="ticks per rollout call")
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the legs")
    ap.add_argument("--update-houses", type=int, default=131072)
    ap.add_argument("--update-ticks", type=int, default=2)
    ap.add_argument("--update-rounds", type=int, default=3)
    ap.add_argument("--port", type=int, default=29533)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_mappo_sharded.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import torch.distributed as dist

    from bench import env_props
    from mdr_amd import _lib
    from mdr_amd.actor import DeviceActor, make_actor
    from mdr_amd.distributed import make_comm
    from mdr_amd.environment import Environment
    from mdr_amd.mappo import DeviceMAPPO, MAPPOConfig
    from mdr_amd.replay import RolloutStore

    if not torch.cuda.is_available():
        raise SystemExit("no ROCm GPU visible: nothing is measured without one")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(a.port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch creates the HIP events on the first record(): not inside a timing)
    e1.record()
    T = a.ticks

    def make(n, sharded=True):
        env = Environment(env_props(n), device=dev, rng=random.Random(1), population="synthetic", seed=5,
                          comm=make_comm("rccl") if sharded else None)
        if sharded:
            env.shard.set_option("force_halo", 1)
        return env

    def timed(fn, per):
        torch.cuda.synchronize()
        e0.record()
        keep = fn()
        e1.record()
        e1.synchronize()
        del keep
        return e0.elapsed_time(e1) * 1e3 / per

    res = {"bench": "mappo_sharded", "comm": "rccl, world 1, force_halo", "ticks_per_rollout": T, "precision": "fp32",
           "unit": "us per tick", "sizes": {}}
    for n in a.houses:
        rew = torch.empty((T, n), dtype=torch.float64, device=dev)
        acts = torch.empty((T, n), dtype=torch.uint8, device=dev)
        probs = torch.empty((T, n), dtype=torch.float32, device=dev)
        envs = [make(n) for _ in range(3)]
        nets = [make_actor(e.obs_spec().n_feat, 2, [100, 100], seed=1) for e in envs]
        da, db = (DeviceActor(e, m, precision="fp32") for e, m in zip(envs[:2], nets[:2]))
        agent = DeviceMAPPO(envs[2], MAPPOConfig(), precision="fp32")
        store = RolloutStore(envs[0], T)
        assert store.sharded

        def collect():
            store.clear()
            da.rollout(T, store=store)

        def rollout():  # DeviceActor.rollout's window, handed to the C loop without a store
            env = envs[1]
            solar0 = float(env._solar)
            ticks = env.driver_window(T)
            assert len(ticks) == T
            osc = np.zeros((T, 4))
            osc[:, 1], osc[:, 3] = ticks.s_prev, ticks.t_od_prev
            osc[0, 2], osc[1:, 2] = solar0, ticks.solar[:-1]
            if not env._P_dev_valid:
                env.shard.p_dev.fill_(float(env._P_host))
            env.shard.actor_rollout_sharded(ticks, osc, env.obs_spec(), acts, n, probs, n, rew, n)
            env._P_dev_valid = True
            env.finish_grid_step()

        def per_tick_loop():
            env = envs[2]
            obs = env.obs_tensor().clone()
            for t in range(T):
                act = agent.select_actions()
                r = env.step_tensor(act, rewards=rew[t])
                nxt = env.obs_tensor().clone()
                agent.store_transition(obs, nxt, r, t == T - 1)
                obs = nxt
            del agent.buffer[:]

        legs = (("collect", collect), ("rollout", rollout), ("per_tick_loop", per_tick_loop))
        for _ in range(3):  # warm-up: allocator, host drivers and the communicator in steady state
            for _name, fn in legs:
                fn()
        torch.cuda.synchronize()
        samples = {}
        for _ in range(a.rounds):
            for name, fn in legs:
                samples.setdefault(name, []).append(timed(fn, T))
        out = {"legs": {k: stats(v) for k, v in samples.items()}, "obs_features": envs[0].obs_spec().n_feat,
               "halo_bytes_per_tick": store.halo_bytes_per_tick}
        L = out["legs"]
        out["collect_range_wholly_below_per_tick_loop"] = L["collect"]["max"] < L["per_tick_loop"]["min"]
        derived = (2 * 20 * n + 2 * store.halo_bytes_per_tick) / (STEP_TBPS * 1e12) * 1e6
        out["store_cost"] = {"us_per_tick_measured": L["collect"]["median"] - L["rollout"]["median"],
                             "us_per_tick_derived": derived,
                             "derived_from": f"40 B per house + the halo row, at the step kernel's {STEP_TBPS} TB/s",
                             "unsharded_at_1048576_us": UNSHARDED_STORE_US_1M}
        res["sizes"][str(n)] = out
        del envs, da, db, agent, store

    # one PPO epoch, per minibatch: sharded (owned rows + one integer allreduce) against single-process
    n, Tu = a.update_houses, a.update_ticks
    cfg = MAPPOConfig(ppo_update_time=1)
    ag_s = DeviceMAPPO(make(n), cfg, precision="fp32", returns="per_agent", collect_ticks=Tu)
    ag_1 = DeviceMAPPO(make(n, sharded=False), cfg, precision="fp32", returns="per_agent", collect_ticks=Tu)
    assert ag_s.store.sharded and not ag_1.store.sharded
    n_mb = -(-Tu * n // cfg.batch_size)

    def upd(agent):
        def run():
            assert agent.update()
        agent.collect(Tu)
        return run

    for ag in (ag_s, ag_1):
        upd(ag)()
    torch.cuda.synchronize()
    us = {"sharded": [], "single_process": []}
    for _ in range(a.update_rounds):
        for name, ag in (("sharded", ag_s), ("single_process", ag_1)):
            us[name].append(timed(upd(ag), n_mb))
    res["update"] = {"houses": n, "ticks": Tu, "batch_size": cfg.batch_size, "minibatches_per_epoch": n_mb,
                     "unit": "us per minibatch (one epoch of update(), returns and guards included)",
                     "minibatch_bytes": 4 * cfg.batch_size * (ag_s.num_state + 4),
                     "legs": {k: stats(v) for k, v in us.items()}}
    res["update"]["allreduce_cost_us_per_minibatch"] = (res["update"]["legs"]["sharded"]["median"]
                                                        - res["update"]["legs"]["single_process"]["median"])
    res["not_measured"] = "RCCL at world > 1"
    res["build"] = _lib.build_id()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
