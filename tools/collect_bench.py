"""What recording training transitions costs the fused MA-PPO rollout, against the per-tick loop.

    python tools/collect_bench.py [--houses 1048576] [--ticks 20] [--rounds 7] [--out profiles/r08_collect.json]

Config C5 (bench.py's env_props, sinusoidal signal, individual_L2, the reference actor init), fp32
actor precision, synthetic houses.  Three legs, each producing one [ticks, N] block of actions,
probabilities and rewards, alternating --rounds times after a warm-up of the same shapes, device
events around each leg:
* rollout        — DeviceActor.rollout(ticks): one captured graph, k_actor + step per tick;
* rollout_store  — DeviceActor.rollout(ticks, store=RolloutStore): the same graph with one k_snap
                   node per tick (40 B read + 40 B written per house);
* per_tick_loop  — what training needed before: per tick select_actions, step_tensor and
                   obs_tensor().clone() (the float32 obs rows MAPPO.store_transition keeps).
Then RolloutStore.states(idx) (k_obs_gather) for random idx of m = 256 and m = 2^20 transitions.

One JSON line (also written to --out): per leg the median and the spread (min, max) of us per
tick; k_snap's share = rollout_store - rollout, beside the figure derived from its traffic.
"""
import argparse
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-demandresponse_amd")]

STEP_TBPS = 5.3  # the step kernel's achieved HBM rate: k_snap's derived time uses it


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "samples": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--houses", type=int, default=1048576)
    ap.add_argument("--ticks", type=int, default=20, help="ticks per rollout call (one graph)")
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the legs")
    ap.add_argument("--gather-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_collect.json"))
    a = ap.parse_args()

    import torch

    from bench import env_props
    from mdr_amd import _lib
    from mdr_amd.actor import DeviceActor, make_actor
    from mdr_amd.environment import Environment
    from mdr_amd.replay import RolloutStore

    n, T = a.houses, a.ticks
    dev = "cuda:0"
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch creates the HIP events on the first record(): not inside a timing)
    e1.record()

    def make():
        env = Environment(env_props(n), device=dev, rng=random.Random(1), population="synthetic", seed=5)
        actor = make_actor(env.obs_spec().n_feat, 2, [100, 100], seed=1)
        return env, DeviceActor(env, actor, precision="fp32")

    rew = torch.empty((T, n), dtype=torch.float64, device=dev)
    acts = torch.empty((T, n), dtype=torch.uint8, device=dev)
    probs = torch.empty((T, n), dtype=torch.float32, device=dev)
    env_a, da = make()
    env_b, db = make()
    env_c, dc = make()
    store = RolloutStore(env_b, T)

    def rollout():
        da.rollout(T, rewards=rew, actions=acts, probs=probs)

    def rollout_store():
        store.clear()
        db.rollout(T, store=store)

    def per_tick_loop():
        kept = []
        for t in range(T):
            act, _ = dc.select_actions(action=acts[t], prob=probs[t], count_next=True)
            env_c.step_tensor(act, rewards=rew[t])
            kept.append(env_c.obs_tensor().clone())
        return kept

    legs = (("rollout", rollout), ("rollout_store", rollout_store), ("per_tick_loop", per_tick_loop))

    def timed(fn):
        torch.cuda.synchronize()
        e0.record()
        keep = fn()
        e1.record()
        e1.synchronize()
        del keep
        return e0.elapsed_time(e1) * 1e3 / T  # us per tick

    for _ in range(3):  # warm-up: graph capture, allocator, host drivers in steady state
        for _name, fn in legs:
            fn()
    torch.cuda.synchronize()
    samples = {}
    for _ in range(a.rounds):
        for name, fn in legs:
            samples.setdefault(name, []).append(timed(fn))
    g = env_b.shard.graph_info()

    # the gather: random transitions of the last stored rollout
    gather = {}
    gen = torch.Generator(device=dev).manual_seed(1)
    for m in (256, 1 << 20):
        idx = torch.randint(0, store.rows * n, (m,), generator=gen, device=dev)
        store.states(idx)
        v = []
        for _ in range(a.gather_reps):
            torch.cuda.synchronize()
            e0.record()
            out = store.states(idx)
            e1.record()
            e1.synchronize()
            v.append(e0.elapsed_time(e1) * 1e3)
            del out
        gather[f"m_{m}"] = dict(stats(v), unit="us per states(idx) call")

    res = {"bench": "collect", "houses": n, "ticks_per_rollout": T, "precision": "fp32", "unit": "us per tick",
           "legs": {k: stats(v) for k, v in samples.items()},
           "obs_features": env_a.obs_spec().n_feat,
           "bytes_per_house_tick": {"store": RolloutStore.nbytes_per_house_tick,
                                    "obs_rows": 4 * env_a.obs_spec().n_feat + 13},
           "actor_graphs_cached": g["actor_graphs"], "obs_gather": gather, "build": _lib.build_id()}
    med = {k: v["median"] for k, v in res["legs"].items()}
    derived = 2 * 20 * n / (STEP_TBPS * 1e12) * 1e6  # 20 B read + 20 B written per house
    res["k_snap"] = {"us_per_tick_measured": med["rollout_store"] - med["rollout"], "us_per_tick_derived": derived,
                     "derived_from": f"40 B per house at the step kernel's {STEP_TBPS} TB/s",
                     "within_twice_derived": med["rollout_store"] - med["rollout"] <= 2 * derived}
    res["store_rollout_below_per_tick_loop"] = med["rollout_store"] < med["per_tick_loop"]
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
