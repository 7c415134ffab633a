"""Closed-loop bang-bang rollouts under the common penalty modes against the parent commit's, where
the same call ran one step launch per tick (+ k_pen_reduce and k_reward_finalize_dev) inside the C call.

    python tools/bangbang_common_bench.py --parent-tree PATH [--houses 1048576] [--ticks 2048] [--out FILE]

Legs: for common_L2, common_max_error and mixture (alpha_common_max 0.5) and both controllers,
Environment.rollout(chunk, action_mode=c) into a [chunk, N] reward buffer (2d) and into a 1-D [N]
buffer (1d), synthetic houses, deadband 0.05 degC; plus the same four legs under individual_L2, whose
kernels are the same instructions on both trees (a control: the two trees' ranges must overlap).

The baseline is never taken from this tree: --parent-tree names a built checkout of the parent
commit, and parent and this-tree child processes alternate (fresh processes: each initialises the
GPU itself).  Inside a process the legs alternate --rounds times after a warm-up of the same
shapes; device events time each sample (>= --ticks ticks).  One JSON line (also written to --out):
per leg and tree the median and the spread (min, max) of house-steps/s over every sample, the
ratio of the medians, and whether this tree's range lies wholly above the parent's.

A child run (--child) measures the legs of --legs from the tree in --tree and prints its samples
(the new legs alone under a kernel trace show how a window's time splits over its four launches).
"""
import argparse
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CTRLS = ["bangbang", "deadband_bangbang"]
COMMON = ["common_L2", "common_max_error", "mixture"]
CONTROL = "individual_L2"
DEADBAND = 0.05


def all_legs():
    return [f"{m}:{c}:{d}" for m in COMMON + [CONTROL] for c in CTRLS for d in ("2d", "1d")]


def child(a):
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "marl-demandresponse_amd")]
    import torch

    from bench import env_props
    from mdr_amd.environment import Environment

    n, chunk = a.houses, a.chunk
    calls = -(-a.ticks // chunk)
    ticks = calls * chunk  # every leg runs the same number of ticks per sample
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch creates the HIP events on the first record(): not inside a timing)
    e1.record()

    def make(pmode):
        p = env_props(n)
        p.cluster_prop.house_prop.deadband = DEADBAND
        p.reward_prop.penalty_props.mode = pmode
        if pmode == "mixture":
            p.reward_prop.penalty_props.alpha_common_max = 0.5
        return Environment(p, device="cuda:0", rng=random.Random(1), population="synthetic", seed=5)

    def rollout(env, ctrl, rew):
        for _ in range(calls):
            env.rollout(chunk, action_mode=ctrl, rewards=rew)

    def timed(env, ctrl, rew):
        torch.cuda.synchronize()
        e0.record()
        rollout(env, ctrl, rew)
        e1.record()
        e1.synchronize()
        return n * ticks / (e0.elapsed_time(e1) * 1e-3)

    rew = {"2d": torch.empty((chunk, n), dtype=torch.float64, device="cuda:0"),  # (one buffer serves every leg)
           "1d": torch.empty(n, dtype=torch.float64, device="cuda:0")}
    jobs = []
    for leg in a.legs.split(","):
        pmode, ctrl, dims = leg.split(":")
        env = make(pmode)
        rollout(env, ctrl, rew[dims])  # warm-up: the same shapes
        jobs.append((leg, env, ctrl, rew[dims]))
    out = {}
    for _ in range(a.rounds):
        for leg, env, ctrl, r in jobs:
            out.setdefault(leg, []).append(timed(env, ctrl, r))
    print("CHILD " + json.dumps(out), flush=True)


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "samples": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (the baseline)")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--houses", type=int, default=1048576)
    ap.add_argument("--ticks", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=128, help="ticks per rollout call")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the legs inside a process")
    ap.add_argument("--alternations", type=int, default=2, help="parent / this-tree process pairs")
    ap.add_argument("--legs", default="", help="comma-separated mode:controller:2d|1d (default: all)")
    ap.add_argument("--out", help="also write the JSON result here")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree: the baseline comes from a checkout of the parent commit")
    legs = a.legs.split(",") if a.legs else all_legs()
    samples = {}
    for _ in range(a.alternations):
        for who, tree in (("parent", a.parent_tree), ("tree", a.tree)):
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
            print(f"{who}: done", file=sys.stderr, flush=True)
    calls = -(-a.ticks // a.chunk)
    res = {"bench": "bangbang_common", "houses": a.houses, "ticks_per_sample": calls * a.chunk,
           "rollout_chunk": a.chunk, "deadband": DEADBAND, "unit": "house-steps/s",
           "samples_per_leg": a.rounds * a.alternations, "legs": {}}
    for leg in legs:
        p, t = stats(samples[("parent", leg)]), stats(samples[("tree", leg)])
        row = {"parent": p, "tree": t, "tree_over_parent": t["median"] / p["median"]}
        if leg.startswith(CONTROL + ":"):
            row["ranges_overlap"] = t["min"] <= p["max"] and p["min"] <= t["max"]
        else:
            row["tree_range_above_parent"] = t["min"] > p["max"]
        res["legs"][leg] = row
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
