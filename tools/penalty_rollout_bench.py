"""Rollouts under the common penalty modes against the per-tick loop they replace.

    python tools/penalty_rollout_bench.py --parent-tree PATH [--houses 1048576] [--ticks 2000] [--rounds 3]

For common_L2, common_max_error and mixture, synthetic houses and random actions, two legs:
* per_tick — a loop of step_tensor(None, action_mode="random", lookahead="random"): three launches
  per tick (k_step_*, k_pen_reduce, k_reward_finalize), the only way before windowed rollouts
  accepted these modes;
* rollout  — Environment.rollout(chunk, action_mode="random") into a 1-D reward buffer.
plus an individual_L2 rollout leg (the headline path, which must not move).

The baseline is never taken from this tree alone: --parent-tree names a built checkout of the
parent commit, whose per_tick and individual_L2 legs run in child processes alternating with this
tree's (fresh processes: each initialises the GPU itself).  Inside a process the legs alternate
--rounds times after a warm-up of the same shapes; device events time each leg (>= --ticks ticks).
One JSON line: per leg the median and the spread (min, max) of house-steps/s over every sample, and
each mode's rollout / parent per_tick ratio.

A child run (--child) measures the legs of --legs from the tree in --tree and prints its samples.
"""
import argparse
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ["common_L2", "common_max_error", "mixture"]


def child(a):
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "marl-demandresponse_amd")]
    import torch

    from bench import env_props
    from mdr_amd.environment import Environment

    n, ticks, chunk = a.houses, a.ticks, a.chunk
    legs = a.legs.split(",")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch creates the HIP events on the first record(): not inside a timing)
    e1.record()

    def make(mode):
        p = env_props(n)
        p.reward_prop.penalty_props.mode = mode
        return Environment(p, device="cuda:0", rng=random.Random(1), population="synthetic", seed=5)

    def per_tick(env, k):
        for _ in range(k):
            env.step_tensor(None, action_mode="random", lookahead="random")

    def rollout(env, k):
        for _ in range(k // chunk):
            env.rollout(chunk, action_mode="random", rewards=env._row)

    def timed(fn, env, k):
        torch.cuda.synchronize()
        e0.record()
        fn(env, k)
        e1.record()
        e1.synchronize()
        return n * (k // chunk * chunk if fn is rollout else k) / (e0.elapsed_time(e1) * 1e-3)

    out = {}
    jobs = []  # (key, fn, env)
    for mode in MODES + ["individual_L2"]:
        for leg, fn in (("per_tick", per_tick), ("rollout", rollout)):
            if f"{mode}:{leg}" not in legs:
                continue
            env = make(mode)
            env._row = torch.empty(n, dtype=torch.float64, device="cuda:0")
            fn(env, ticks)  # warm-up: the same shapes
            jobs.append((f"{mode}:{leg}", fn, env))
    for _ in range(a.rounds):
        for key, fn, env in jobs:
            out.setdefault(key, []).append(timed(fn, env, ticks))
    print("CHILD " + json.dumps(out), flush=True)


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "samples": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (the baseline)")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--houses", type=int, default=1048576)
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=500, help="ticks per rollout call")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the legs inside a process")
    ap.add_argument("--alternations", type=int, default=2, help="parent / this-tree process pairs")
    ap.add_argument("--legs", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree: the baseline comes from a checkout of the parent commit")
    parent_legs = [f"{m}:per_tick" for m in MODES] + ["individual_L2:rollout"]
    own_legs = [f"{m}:{leg}" for m in MODES for leg in ("per_tick", "rollout")] + ["individual_L2:rollout"]
    samples = {}
    for _ in range(a.alternations):
        for who, tree, legs in (("parent", a.parent_tree, parent_legs), ("tree", a.tree, own_legs)):
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
    res = {"bench": "penalty_rollout", "houses": a.houses, "ticks": a.ticks, "rollout_chunk": a.chunk,
           "unit": "house-steps/s", "samples_per_leg": a.rounds * a.alternations, "modes": {}}
    for m in MODES:
        base = stats(samples[("parent", f"{m}:per_tick")])
        ro = stats(samples[("tree", f"{m}:rollout")])
        res["modes"][m] = {"per_tick_parent": base, "per_tick": stats(samples[("tree", f"{m}:per_tick")]),
                           "rollout": ro, "rollout_over_parent_per_tick": ro["median"] / base["median"]}
    res["individual_L2"] = {"rollout_parent": stats(samples[("parent", "individual_L2:rollout")]),
                            "rollout": stats(samples[("tree", "individual_L2:rollout")])}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
