"""Stats rows from the greedy-myopic rollout against the per-tick loop that wrote them before.

    python tools/greedy_stats_bench.py --parent-tree PATH [--houses 1048576] [--ticks 512] [--out FILE]

Synthetic houses, the sinusoidal signal, individual_L2; ``--ticks`` ticks per sample in
``greedy_rollout(--chunk)`` calls into 1-D action and reward buffers, device events:
* loop_stats     — (a) the parent commit's only way to the rows: per tick ``greedy_actions`` ->
                   ``step_tensor(ctrl="greedy_keys")`` -> ``Shard.tick_stats``, one download per chunk;
* rollout        — (b) ``greedy_rollout(chunk)`` without rows (parent commit and this tree:
                   mdr_greedy_rollout's launches must not have moved);
* rollout_stats  — (c) ``greedy_rollout(chunk, stats=RolloutStats)`` and its ``host()`` download
                   after every call.

The baseline is never taken from this tree: --parent-tree names a built checkout of the parent
commit, whose legs run in child processes alternating with this tree's (fresh processes: each
initialises the GPU itself).  Inside a process the legs alternate --rounds times after a warm-up of
the same shapes.  One JSON line (also written to --out): per leg the median and the spread (min, max)
of house-steps/s over every sample, (c)/(b), (c)/(a), whether (c)'s [min, max] lies wholly above
(a)'s, and whether (b)'s ranges of parent and tree overlap.

``--child --legs rollout_stats --rounds 1`` is leg (c) alone in this process: what a kernel trace of
the rows rollout is taken over.
"""
import argparse
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PARENT_LEGS = ("loop_stats", "rollout")
TREE_LEGS = ("rollout", "rollout_stats")


def child(a):
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "marl-demandresponse_amd")]
    import torch

    from bench import env_props
    from mdr_amd.environment import Environment
    from mdr_amd.services import RolloutStats

    n, chunk = a.houses, a.chunk
    calls = -(-a.ticks // chunk)
    ticks = calls * chunk  # every leg runs the same number of ticks per sample
    legs = a.legs.split(",")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch creates the HIP events on the first record(): not inside a timing)
    e1.record()

    def make():
        env = Environment(env_props(n), device="cuda:0", rng=random.Random(1), population="synthetic", seed=5)
        env._act = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        env._rew = torch.empty(n, dtype=torch.float64, device="cuda:0")
        return env

    def rollout(env):
        for _ in range(calls):
            env.greedy_rollout(chunk, actions=env._act, rewards=env._rew)

    def rollout_stats(env):
        for _ in range(calls):
            env._rows.clear()
            env.greedy_rollout(chunk, actions=env._act, rewards=env._rew, stats=env._rows)
            env._rows.host()

    def loop_stats(env):
        rows, sh = env._rows, env.shard
        for _ in range(calls):
            rows.clear()
            for t in range(chunk):
                act = env.greedy_actions(out=env._act)
                r = env.step_tensor(act, rewards=env._rew, ctrl="greedy_keys")
                sh.tick_stats(r, rows.stats[t])
            rows.rows = chunk  # (the rows' host scalars are not part of the measurement)
            rows._first = [True] + [False] * (chunk - 1)
            rows.host()

    def timed(fn, env):
        torch.cuda.synchronize()
        e0.record()
        fn(env)
        e1.record()
        e1.synchronize()
        return n * ticks / (e0.elapsed_time(e1) * 1e-3)

    fns = {"loop_stats": loop_stats, "rollout": rollout, "rollout_stats": rollout_stats}
    out, jobs = {}, []
    for leg, fn in fns.items():
        if leg not in legs:
            continue
        env = make()
        if leg != "rollout":
            env._rows = RolloutStats(env, chunk)
        fn(env)  # warm-up: the same shapes
        jobs.append((leg, fn, env))
    for _ in range(a.rounds):
        for leg, fn, env in jobs:
            out.setdefault(leg, []).append(timed(fn, env))
    print("CHILD " + json.dumps(out), flush=True)


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "samples": len(s)}


def overlap(x, y):
    return x["min"] <= y["max"] and y["min"] <= x["max"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (the baseline)")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--houses", type=int, default=1048576)
    ap.add_argument("--ticks", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=128, help="ticks per greedy_rollout call")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the legs inside a process")
    ap.add_argument("--alternations", type=int, default=2, help="parent / this-tree process pairs")
    ap.add_argument("--legs", default="")
    ap.add_argument("--out", help="also write the JSON result here")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree: the baseline comes from a checkout of the parent commit")
    samples = {}
    for _ in range(a.alternations):
        for who, tree, names in (("parent", a.parent_tree, PARENT_LEGS), ("tree", a.tree, TREE_LEGS)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--legs", ",".join(names),
                   "--houses", str(a.houses), "--ticks", str(a.ticks), "--chunk", str(a.chunk),
                   "--rounds", str(a.rounds)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{who} child failed ({r.returncode})")
            for k, v in json.loads(line[-1][6:]).items():
                samples.setdefault((who, k), []).extend(v)
    calls = -(-a.ticks // a.chunk)
    loop = stats(samples[("parent", "loop_stats")])
    pb, tb = stats(samples[("parent", "rollout")]), stats(samples[("tree", "rollout")])
    c = stats(samples[("tree", "rollout_stats")])
    res = {"bench": "greedy_stats", "houses": a.houses, "ticks_per_sample": calls * a.chunk, "rollout_chunk": a.chunk,
           "unit": "house-steps/s", "samples_per_leg": a.rounds * a.alternations,
           "a_loop_stats_parent": loop, "b_rollout_parent": pb, "b_rollout": tb, "c_rollout_stats": c,
           "c_over_b": c["median"] / tb["median"], "c_over_a": c["median"] / loop["median"],
           "us_per_tick": {"a": a.houses / loop["median"] * 1e6, "b": a.houses / tb["median"] * 1e6,
                           "c": a.houses / c["median"] * 1e6},
           "c_range_above_a": c["min"] > loop["max"], "b_parent_tree_overlap": overlap(pb, tb)}
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
