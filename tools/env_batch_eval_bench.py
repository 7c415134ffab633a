"""Evaluating a baseline controller over E seeds: services.evaluate_batch (one launch: returns and stats
rows, no reward matrix) against the only two routes that exist on the parent commit, both run on the parent.

    python tools/env_batch_eval_bench.py --parent-tree PATH [--out profiles/r28_env_batch_eval.json]
                                         [--bench-control N]

Legs: (E, N_c, T) = (1024, 1000, 128) and (1024, 50, 128) x {deadband_bangbang, random}, the bench's
configuration with a deadband of 0.05 degC and host-drawn populations (seeds 8 + e).

  eval    this tree: evaluate_batch(batch, c, 128, stats=kept rows) — the members' reset, E driver windows,
          ONE k_batch_eval launch (returns + stats), one download, the means on the host.
  matrix  parent: batch.reset(), EnvBatch.rollout(128) into a full [128, E, N_c] reward matrix, torch
          reductions to every cluster's mean return, one download.  (No temperature error, lockout or ON
          counts: the parent cannot form them on a batch.)
  twins   parent, deadband_bangbang only (evaluate_controller takes no random controller): min(E,
          --twins-cap) stand-alone Environments through evaluate_controller(env, c, 128, twin=kept copy),
          looped from Python.  The loop is serial, so its time is scaled by E / cap (stated as `twins_envs`).

Parent and this-tree child processes alternate (fresh processes, each under its own timeout; the tool stops
at the first failure); inside a process the legs alternate --rounds times after a warm-up of the same shape.
Per sample: the wall time of the whole evaluation (its reset included), and separately its parts — a reset
alone (host, once per round), the E driver_window calls (host, perf_counter) and the device span of the
launch alone (device events around the launch, the drivers computed before; `matrix`: the launch and the
reductions).  One JSON line (also written to --out): per leg and route the median and [min, max] of each.

--bench-control N: bench.py and bench.py --steps 20, N runs each of parent and this tree, alternated; the
tree passes if its median lies inside the spread the parent shows against itself.  Recorded as `bench_control`.
"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
GRID = [(1024, 1000), (1024, 50)]
SOURCES = ["deadband_bangbang", "random"]
TICKS = 128
DEADBAND = 0.05
# bytes per house-tick the device moves beyond the state it keeps in registers: the
# expectation written before measuring
EXPECTED = {"matrix_reward_bytes_per_house_tick": 8, "eval_reward_bytes_per_house_tick": 0,
            "eval_returns_bytes_per_house_per_call": 16, "eval_stats_bytes_per_cluster_tick": 128}


def all_legs():
    return [f"{e}x{n}:{c}" for e, n in GRID for c in SOURCES]


def props_of(n):
    from bench import env_props

    p = env_props(n)
    p.cluster_prop.house_prop.deadband = DEADBAND
    return p


def child(a):
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "marl-demandresponse_amd")]
    import copy

    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch creates the HIP events on the first record(): not inside a timing)
    e1.record()
    legs = a.legs.split(",")
    shapes = list(dict.fromkeys(leg.split(":")[0] for leg in legs))
    out = {}

    def span(fn):
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def add(leg, **kw):
        r = out.setdefault(leg, {})
        for k, v in kw.items():
            r.setdefault(k, []).append(v)

    for shape in shapes:
        E, n = (int(x) for x in shape.split("x"))
        mine = [leg for leg in legs if leg.split(":")[0] == shape]
        if a.child in ("eval", "matrix"):
            from mdr_amd.batch import EnvBatch
            from mdr_amd.environment import ACTION_MODES

            t0 = time.perf_counter()
            b = EnvBatch(props_of(n), E, seeds=[8 + e for e in range(E)])
            out.setdefault("build_s", {})[shape] = time.perf_counter() - t0
        if a.child == "eval":
            from mdr_amd.environment import discount_weights
            from mdr_amd.services import BatchRolloutStats, evaluate_batch

            import numpy as np

            stats = BatchRolloutStats(b, TICKS)
            w = np.ascontiguousarray(np.stack([discount_weights(1.0, 1.0, TICKS)[:TICKS]] * E))
            for leg in mine:
                evaluate_batch(b, leg.split(":")[1], TICKS, stats=stats)
            for _ in range(a.rounds):
                r_s, _ = wall(b.reset)  # (E host resets: seconds at E = 1,024, so one sample per round)
                for leg in mine:
                    c = leg.split(":")[1]
                    s, res = wall(lambda: evaluate_batch(b, c, TICKS, stats=stats))
                    t0 = time.perf_counter()
                    ticks = b._driver_windows(TICKS)
                    host = time.perf_counter() - t0
                    stats.clear()
                    ret = b.empty_returns()
                    dev = span(lambda: b._launch(ticks, None, 0, ACTION_MODES[c], None, 0, weights=w, returns=ret,
                                                 stats=stats, srow0=0))
                    add(leg, wall_s=s, reset_s=r_s, host_drivers_s=host, device_s=dev,
                        mean_return=res["mean"]["Mean test return"])
            b.close()
        elif a.child == "matrix":
            rew = b.empty_rewards(TICKS)

            def reduce_():
                return (rew.sum(dim=(0, 2)) / (n * TICKS)).cpu().numpy()

            def run(c):
                b.reset()
                b.rollout(TICKS, action_mode=c, rewards=rew)
                return float(reduce_().mean())

            for leg in mine:
                run(leg.split(":")[1])
            for _ in range(a.rounds):
                r_s, _ = wall(b.reset)
                for leg in mine:
                    c = leg.split(":")[1]
                    s, res = wall(lambda: run(c))
                    t0 = time.perf_counter()
                    ticks = b._driver_windows(TICKS)
                    host = time.perf_counter() - t0

                    def launch():
                        b._launch(ticks, None, 0, ACTION_MODES[c], rew, b.n_envs * b.stride)
                        rew.sum(dim=(0, 2))

                    dev = span(launch)
                    add(leg, wall_s=s, reset_s=r_s, host_drivers_s=host, device_s=dev, mean_return=res)
            b.close()
        else:
            from mdr_amd.environment import Environment
            from mdr_amd.services import evaluate_controller

            cap = min(E, a.twins_cap)
            envs = [Environment(props_of(n), device="cuda:0", rng=random.Random(8 + e), seed=8 + e,
                                population="reference") for e in range(cap)]
            twins = [copy.deepcopy(env) for env in envs]

            def run(c):
                return [evaluate_controller(env, c, TICKS, twin=tw)["Mean test return"] for env, tw in zip(envs, twins)]

            mine = [leg for leg in mine if leg.split(":")[1] != "random"]
            for leg in mine:
                run(leg.split(":")[1])
            for _ in range(a.rounds):
                for leg in mine:
                    s, res = wall(lambda: run(leg.split(":")[1]))
                    add(leg, wall_s=s * E / cap, mean_return=sum(res) / len(res))
                    out[leg]["twins_envs"] = cap
            for env in envs + twins:
                env.shard.close()
        torch.cuda.empty_cache()
    print("CHILD " + json.dumps(out), flush=True)


def stats_of(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "samples": len(s)}


def run_child(cmd, limit, cwd=None):
    """One GPU step under its own time limit; the tool stops at the first failure."""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, cwd=cwd)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd[:4])} ... failed ({r.returncode}); nothing more is started")
    return r.stdout


def bench_control(a):
    """bench.py headline control: parent and this tree alternated, N runs each and per argument set."""
    res = {}
    for name, extra in (("default", []), ("steps20", ["--steps", "20"])):
        vals = {"parent": [], "tree": []}
        for _ in range(a.bench_control):
            for who, tree in (("parent", a.parent_tree), ("tree", a.tree)):
                text = run_child([sys.executable, "bench.py", "--gpus", "1"] + extra, a.step_timeout, cwd=tree)
                line = [ln for ln in text.splitlines() if ln.startswith("{")][-1]
                vals[who].append(json.loads(line)["value"])
        p, t = stats_of(vals["parent"]), stats_of(vals["tree"])
        res[name] = {"parent": p, "tree": t, "values": vals,
                     "tree_median_inside_parent_spread": p["min"] <= t["median"] <= p["max"],
                     "tree_median_over_parent_median": t["median"] / p["median"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (the baselines)")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the legs inside a process")
    ap.add_argument("--alternations", type=int, default=2, help="parent / this-tree process rounds")
    ap.add_argument("--twins-cap", type=int, default=32, help="stand-alone environments the twins route builds at most")
    ap.add_argument("--legs", default="", help="comma-separated ExN:source (default: all)")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds a child process may take")
    ap.add_argument("--bench-control", type=int, default=0, help="bench.py runs per tree and argument set (0: none)")
    ap.add_argument("--out", help="also write the JSON result here")
    ap.add_argument("--child", choices=["eval", "matrix", "twins"])
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree: the baselines come from a checkout of the parent commit")
    legs = a.legs.split(",") if a.legs else all_legs()
    samples, build = {}, {}
    for _ in range(a.alternations):
        for who, tree in (("matrix", a.parent_tree), ("eval", a.tree), ("twins", a.parent_tree)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", who, "--tree", tree, "--legs", ",".join(legs),
                   "--rounds", str(a.rounds), "--twins-cap", str(a.twins_cap)]
            text = run_child(cmd, a.step_timeout)
            got = json.loads([ln for ln in text.splitlines() if ln.startswith("CHILD ")][-1][6:])
            for shape, s in got.pop("build_s", {}).items():
                build.setdefault((who, shape), []).append(s)
            for leg, rec in got.items():
                for k, v in rec.items():
                    if isinstance(v, list):
                        samples.setdefault((who, leg, k), []).extend(v)
                    else:
                        samples[(who, leg, k)] = v
            print(f"{who}: done", file=sys.stderr, flush=True)
    res = {"bench": "env_batch_eval", "ticks_per_call": TICKS, "deadband": DEADBAND, "unit": "seconds per evaluation of E clusters",
           "samples_per_leg": a.rounds * a.alternations, "expected_bytes": EXPECTED,
           "routes": {"eval": "this tree: services.evaluate_batch (returns + stats, one launch)",
                      "matrix": "parent: EnvBatch.rollout into [T, E, N_c] + torch reductions to the clusters' mean return",
                      "twins": "parent: evaluate_controller(twin=...) over stand-alone Environments, a subset scaled to E"},
           "batch_build_s": {f"{w}:{s}": stats_of(v) for (w, s), v in build.items()}, "legs": {}}
    for leg in legs:
        rec = {}
        for who in ("eval", "matrix", "twins"):
            keys = [k for (w, l, k) in samples if w == who and l == leg]
            if keys:
                rec[who] = {k: (stats_of(samples[(who, leg, k)]) if isinstance(samples[(who, leg, k)], list)
                                else samples[(who, leg, k)]) for k in keys}
        rec["matrix_over_eval_wall"] = rec["matrix"]["wall_s"]["median"] / rec["eval"]["wall_s"]["median"]
        rec["matrix_over_eval_device"] = rec["matrix"]["device_s"]["median"] / rec["eval"]["device_s"]["median"]
        if "twins" in rec:
            rec["twins_over_eval_wall"] = rec["twins"]["wall_s"]["median"] / rec["eval"]["wall_s"]["median"]
        res["legs"][leg] = rec
    if a.bench_control:
        res["bench_control"] = bench_control(a)
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
