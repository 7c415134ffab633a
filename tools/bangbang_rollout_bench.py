"""Closed-loop windowed rollouts of the bang-bang controllers against the per-tick loop they replace.

    python tools/bangbang_rollout_bench.py --parent-tree PATH [--houses 1048576] [--ticks 2000] [--out FILE]

For the plain and the deadband controller, synthetic houses (deadband 0.05 degC, so both controllers
keep switching), three legs:
* per_tick  — a loop of step_tensor(None, action_mode=c, lookahead=c): one k_step_* launch per tick
  and a Python round trip, the only way before rollouts accepted these sources;
* rollout2d — Environment.rollout(chunk, action_mode=c) into a [chunk, N] reward buffer
  (k_step_closed, k_win_reduce, k_closed_reward per window of 32 ticks);
* rollout1d — the same into a 1-D [N] buffer (only the last tick's rewards are finalised).

The baseline is never taken from this tree: --parent-tree names a built checkout of the parent
commit, whose per_tick legs run in child processes alternating with this tree's (fresh processes:
each initialises the GPU itself).  Inside a process the legs alternate --rounds times after a
warm-up of the same shapes; device events time each leg (>= --ticks ticks per sample).  One JSON
line (also written to --out): per leg the median and the spread (min, max) of house-steps/s over
every sample, each controller's rollout / parent per_tick ratio, and whether the 2-D rollout's
range lies wholly above the parent loop's.

A child run (--child) measures the legs of --legs from the tree in --tree and prints its samples
(one leg alone under a kernel trace shows how a window's time splits over its three launches).
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


def child(a):
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "marl-demandresponse_amd")]
    import torch

    from bench import env_props
    from mdr_amd.environment import Environment

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

    def per_tick(env, ctrl):
        for _ in range(ticks):
            env.step_tensor(None, action_mode=ctrl, lookahead=ctrl)

    def rollout(env, ctrl):
        for _ in range(calls):
            env.rollout(chunk, action_mode=ctrl, rewards=env._rew)

    def timed(fn, env, ctrl):
        torch.cuda.synchronize()
        e0.record()
        fn(env, ctrl)
        e1.record()
        e1.synchronize()
        return n * ticks / (e0.elapsed_time(e1) * 1e-3)

    out = {}
    jobs = []  # (key, fn, env, ctrl)
    rew2d = None
    for ctrl in CTRLS:
        for leg, fn in (("per_tick", per_tick), ("rollout2d", rollout), ("rollout1d", rollout)):
            if f"{ctrl}:{leg}" not in legs:
                continue
            env = make()
            if leg == "rollout2d":  # (one [chunk, N] buffer serves both controllers)
                if rew2d is None:
                    rew2d = torch.empty((chunk, n), dtype=torch.float64, device="cuda:0")
                env._rew = rew2d
            else:
                env._rew = torch.empty(n, dtype=torch.float64, device="cuda:0")
            fn(env, ctrl)  # warm-up: the same shapes
            jobs.append((f"{ctrl}:{leg}", fn, env, ctrl))
    for _ in range(a.rounds):
        for key, fn, env, ctrl in jobs:
            out.setdefault(key, []).append(timed(fn, env, ctrl))
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
    parent_legs = [f"{c}:per_tick" for c in CTRLS]
    own_legs = [f"{c}:{leg}" for c in CTRLS for leg in ("per_tick", "rollout2d", "rollout1d")]
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
    calls = -(-a.ticks // a.chunk)
    res = {"bench": "bangbang_rollout", "houses": a.houses, "ticks_per_sample": calls * a.chunk,
           "rollout_chunk": a.chunk, "deadband": DEADBAND, "unit": "house-steps/s",
           "samples_per_leg": a.rounds * a.alternations, "controllers": {}}
    for c in CTRLS:
        base = stats(samples[("parent", f"{c}:per_tick")])
        r2, r1 = stats(samples[("tree", f"{c}:rollout2d")]), stats(samples[("tree", f"{c}:rollout1d")])
        res["controllers"][c] = {"per_tick_parent": base, "per_tick": stats(samples[("tree", f"{c}:per_tick")]),
                                 "rollout_2d": r2, "rollout_1d": r1,
                                 "rollout_2d_over_parent_per_tick": r2["median"] / base["median"],
                                 "rollout_1d_over_parent_per_tick": r1["median"] / base["median"],
                                 "rollout_2d_range_above_parent": r2["min"] > base["max"]}
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
