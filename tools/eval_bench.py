"""What per-tick stats rows cost the fused MA-PPO rollout, against the per-tick loop with cluster_stats.

    python tools/eval_bench.py [--houses 1048576] [--ticks 20] [--rounds 7] [--out profiles/r09_eval.json]

Config C5 (bench.py's env_props, sinusoidal signal, individual_L2, the reference actor init), fp32
actor precision, synthetic houses.  Three legs, each running --ticks ticks of select_actions ->
step, alternating --rounds times after a warm-up of the same shapes, device events around each leg:
* rollout         — DeviceActor.rollout(ticks): one captured graph, k_actor + step per tick;
* rollout_stats   — DeviceActor.rollout(ticks, stats=RolloutStats): the same graph with the two stats
                    nodes per tick (k_tick_stats reads 36 B per house, k_tick_stats_finish one block),
                    then RolloutStats.host(): one download for the whole call;
* per_tick_stats  — the only way to metrics before: per tick select_actions, step_tensor and
                    services.cluster_stats (two launches and a .cpu() every tick).
DeviceMAPPO.evaluate on a kept twin is timed too (reset + rollout_stats + the host pass).

One JSON line (also written to --out): per leg the median and the spread (min, max) of us per
tick; the stats nodes' share = rollout_stats - rollout, beside the figure derived from their traffic.
"""
import argparse
import copy
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-demandresponse_amd")]

STEP_TBPS = 5.3  # the step kernel's achieved HBM rate: the derived time uses it
STATS_BYTES = 8 + 8 + 8 + 4 + 8  # t_air, t_mass, target, hvac, reward


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "samples": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--houses", type=int, default=1048576)
    ap.add_argument("--ticks", type=int, default=20, help="ticks per rollout call (one graph)")
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the legs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_eval.json"))
    a = ap.parse_args()

    import torch

    from bench import env_props
    from mdr_amd import _lib
    from mdr_amd.actor import DeviceActor, make_actor
    from mdr_amd.environment import Environment
    from mdr_amd.mappo import DeviceMAPPO
    from mdr_amd.services import RolloutStats, cluster_stats

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
    rows = RolloutStats(env_b, T)

    def rollout():
        da.rollout(T, rewards=rew, actions=acts, probs=probs)

    def rollout_stats():
        rows.clear()
        db.rollout(T, rewards=rew, actions=acts, probs=probs, stats=rows)
        return rows.host()

    def per_tick_stats():
        kept = []
        for t in range(T):
            act, _ = dc.select_actions(action=acts[t], prob=probs[t], count_next=True)
            r = env_c.step_tensor(act, rewards=rew[t])
            kept.append(cluster_stats(env_c, r))
        return kept

    legs = (("rollout", rollout), ("rollout_stats", rollout_stats), ("per_tick_stats", per_tick_stats))

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

    # evaluate on a kept twin: wall time per call (reset of the synthetic population included)
    agent = DeviceMAPPO(env_a, precision="fp32")
    twin = copy.deepcopy(env_a)
    ev = []
    out = None
    for k in range(1 + a.rounds):  # (the first call captures the twin's graph: not kept)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = agent.evaluate(T, env=twin)
        if k:
            ev.append((time.perf_counter() - t0) * 1e6 / T)
    gt = twin.shard.graph_info()

    res = {"bench": "eval", "houses": n, "ticks_per_rollout": T, "precision": "fp32", "unit": "us per tick",
           "legs": {k: stats(v) for k, v in samples.items()},
           "evaluate_twin": dict(stats(ev), unit="wall us per tick, reset included", graphs=gt["actor_graphs"],
                                 launches=gt["actor_launches"], result=out),
           "actor_graphs_cached": g["actor_graphs"], "build": _lib.build_id()}
    med = {k: v["median"] for k, v in res["legs"].items()}
    derived = STATS_BYTES * n / (STEP_TBPS * 1e12) * 1e6
    inc = med["rollout_stats"] - med["rollout"]
    res["stats_nodes"] = {"us_per_tick_measured": inc, "us_per_tick_derived": derived,
                          "derived_from": f"{STATS_BYTES} B per house at the step kernel's {STEP_TBPS} TB/s",
                          "within_twice_derived": inc <= 2 * derived}
    res["stats_rollout_below_per_tick_stats"] = med["rollout_stats"] < med["per_tick_stats"]
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
