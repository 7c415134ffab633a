"""Stats rows from the closed-loop bang-bang rollouts against the per-tick loop that wrote them before.

    python tools/bangbang_stats_bench.py --parent-tree PATH [--houses 1048576] [--ticks 2048] [--out FILE]

For the plain and the deadband controller, synthetic houses (deadband 0.05 degC, so both controllers
keep switching), ``--ticks`` ticks per sample in ``rollout(--chunk)`` calls, device events:
* rollout1d        — Environment.rollout(chunk, action_mode=c) into a 1-D [N] reward buffer, no rows
                     (parent commit and this tree: k_step_closed<..., STATS = false> must not have moved);
* rollout1d_stats  — the same with stats=RolloutStats and its host() download after every call
                     (k_step_closed<..., STATS = true> + k_closed_stats per window);
* rollout2d_stats  — the same into a [chunk, N] reward buffer;
* per_tick_stats   — the parent commit's only way to the rows: a loop of step_tensor(None,
                     action_mode=c, lookahead=c) + Shard.tick_stats, one download per chunk.

The baseline is never taken from this tree: --parent-tree names a built checkout of the parent
commit, whose legs run in child processes alternating with this tree's (fresh processes: each
initialises the GPU itself).  Inside a process the legs alternate --rounds times after a warm-up of
the same shapes.  One JSON line (also written to --out): per leg the median and the spread (min, max)
of house-steps/s over every sample; per controller the with-rows / without-rows ratio, the
rows-rollout / parent-loop ratio, whether the rows rollout's [min, max] lies wholly above the parent
loop's, and whether the no-rows legs of parent and tree overlap.
"""
import argparse
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CTRLS = ["bangbang", "deadband_bangbang"]
DEADBAND = 0.05
PARENT_LEGS = ("rollout1d", "per_tick_stats")
TREE_LEGS = ("rollout1d", "rollout1d_stats", "rollout2d_stats")


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
        p = env_props(n)
        p.cluster_prop.house_prop.deadband = DEADBAND
        return Environment(p, device="cuda:0", rng=random.Random(1), population="synthetic", seed=5)

    def rollout(env, ctrl):
        for _ in range(calls):
            env.rollout(chunk, action_mode=ctrl, rewards=env._rew)

    def rollout_stats(env, ctrl):
        for _ in range(calls):
            env._rows.clear()
            env.rollout(chunk, action_mode=ctrl, rewards=env._rew, stats=env._rows)
            env._rows.host()

    def per_tick_stats(env, ctrl):
        rows, sh = env._rows, env.shard
        for _ in range(calls):
            rows.clear()
            for t in range(chunk):
                r = env.step_tensor(None, action_mode=ctrl, lookahead=ctrl, rewards=env._rew)
                sh.tick_stats(r, rows.stats[t])
            rows.rows = chunk  # (the rows' host scalars are not part of the measurement)
            rows._first = [True] + [False] * (chunk - 1)
            rows.host()

    def timed(fn, env, ctrl):
        torch.cuda.synchronize()
        e0.record()
        fn(env, ctrl)
        e1.record()
        e1.synchronize()
        return n * ticks / (e0.elapsed_time(e1) * 1e-3)

    fns = {"rollout1d": rollout, "rollout1d_stats": rollout_stats, "rollout2d_stats": rollout_stats,
           "per_tick_stats": per_tick_stats}
    out, jobs, rew2d = {}, [], None
    for ctrl in CTRLS:
        for leg, fn in fns.items():
            if f"{ctrl}:{leg}" not in legs:
                continue
            env = make()
            if leg == "rollout2d_stats":  # (one [chunk, N] buffer serves both controllers)
                if rew2d is None:
                    rew2d = torch.empty((chunk, n), dtype=torch.float64, device="cuda:0")
                env._rew = rew2d
            else:
                env._rew = torch.empty(n, dtype=torch.float64, device="cuda:0")
            if leg != "rollout1d":
                env._rows = RolloutStats(env, chunk)
            fn(env, ctrl)  # warm-up: the same shapes
            jobs.append((f"{ctrl}:{leg}", fn, env, ctrl))
    for _ in range(a.rounds):
        for key, fn, env, ctrl in jobs:
            out.setdefault(key, []).append(timed(fn, env, ctrl))
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
    ap.add_argument("--ticks", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=128, help="ticks per rollout call")
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
            legs = [f"{c}:{leg}" for c in CTRLS for leg in names]
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--legs", ",".join(legs),
                   "--houses", str(a.houses), "--ticks", str(a.ticks), "--chunk", str(a.chunk),
                   "--rounds", str(a.rounds)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{who} child failed ({r.returncode})")
            for k, v in json.loads(line[-1][6:]).items():
                samples.setdefault((who, k), []).extend(v)
    calls = -(-a.ticks // a.chunk)
    res = {"bench": "bangbang_stats", "houses": a.houses, "ticks_per_sample": calls * a.chunk,
           "rollout_chunk": a.chunk, "deadband": DEADBAND, "unit": "house-steps/s",
           "samples_per_leg": a.rounds * a.alternations, "controllers": {}}
    for c in CTRLS:
        loop = stats(samples[("parent", f"{c}:per_tick_stats")])
        p1 = stats(samples[("parent", f"{c}:rollout1d")])
        t1 = stats(samples[("tree", f"{c}:rollout1d")])
        s1, s2 = stats(samples[("tree", f"{c}:rollout1d_stats")]), stats(samples[("tree", f"{c}:rollout2d_stats")])
        res["controllers"][c] = {
            "per_tick_stats_parent": loop, "rollout_1d_parent": p1, "rollout_1d": t1,
            "rollout_1d_stats": s1, "rollout_2d_stats": s2,
            "stats_over_no_stats_1d": s1["median"] / t1["median"],
            "rollout_1d_stats_over_parent_loop": s1["median"] / loop["median"],
            "rollout_2d_stats_over_parent_loop": s2["median"] / loop["median"],
            "stats_ranges_above_parent_loop": min(s1["min"], s2["min"]) > loop["max"],
            "no_stats_parent_tree_overlap": overlap(p1, t1)}
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
