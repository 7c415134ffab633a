"""A/B of MDR_OPT_GROUP_LA_ORDER on bench.py's default workload (one process, interleaved rounds).

    python tools/la_order_ab.py [--houses 1048576] [--steps 2000] [--chunk 128] [--window 32]
                                [--rounds 6] [--orders 0,1,2,3,4,17,18,19,16] [--out profiles/rNN_la_order_ab.json]

One environment per option value (bench.py's env_props and seeds), every round runs each of them
over --steps ticks in rollout calls of --chunk ticks (direct launches, random actions, every reward
row kept) and times it as bench.py does: wall clock from the first call to the stream's
synchronisation.  One JSON line: per option value the median, min and max of house-steps/s.
Values (mdr.h): 0 every block counts last, 1 / 2 / 3 blocks alternate in runs of 1 / 8 / 256, 4 every
block counts first, + 16 the blocks past the first resident round count first.
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-demandresponse_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--houses", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--orders", default="0,1,2,3,4,16,17,18,19")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from bench import env_props
    from mdr_amd.environment import Environment

    n, chunk = a.houses, min(a.chunk, a.steps)
    chunks = [chunk] * (a.steps // chunk) + ([a.steps % chunk] if a.steps % chunk else [])
    rew = torch.empty((chunk, n), dtype=torch.float64, device="cuda:0")
    envs = {}
    for order in [int(v) for v in a.orders.split(",")]:
        env = Environment(env_props(n), device="cuda:0", rng=random.Random(4), population="synthetic", seed=1234)
        env.shard.set_rollout_window(a.window)
        env.shard.set_option("group_la_order", order)
        envs[order] = env

    def run(env):
        for c in chunks:
            env.rollout(c, action_mode="random", rewards=rew if c == chunk else rew[:c])

    for env in envs.values():  # warm-up: every call size once, then a full pass
        run(env)
    torch.cuda.synchronize()
    vals = {g: [] for g in envs}
    for r in range(a.rounds):
        order = list(envs) if r % 2 == 0 else list(envs)[::-1]
        for g in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(envs[g])
            torch.cuda.synchronize()
            vals[g].append(n * a.steps / (time.perf_counter() - t0))
    out = {"what": f"MDR_OPT_GROUP_LA_ORDER A/B: {n} houses, {a.steps} ticks in calls of {chunk}, window {a.window}, "
                   f"{a.rounds} interleaved rounds, house-steps/s",
           "order": {str(g): {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "samples": len(v)}
                     for g, v in vals.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
