"""Batched small clusters (mdr_amd.EnvBatch: one launch per rollout call for E clusters) against the
only way to the same result on the parent commit: E stand-alone Environments, each calling
rollout(128, action_mode=c), one after another in a Python loop.

    python tools/env_batch_bench.py --parent-tree PATH [--out profiles/r27_env_batch.json]

Legs: (E, N_c) in {(1024, 1000), (256, 1000), (8192, 50), (64, 1000)} x {bangbang, random} x {2d: a
[128, E, N_c] reward buffer, 1d: the stride-0 [E, N_c] row}, 128 ticks per call, the bench's
configuration with a deadband of 0.05 degC and host-drawn populations (seeds 8 + e).

The baseline is never taken from this tree: --parent-tree names a built checkout of the parent commit;
parent and this-tree child processes alternate (fresh processes), and inside a process the legs
alternate --rounds times after a warm-up call of the same shape.  The baseline builds min(E,
--baseline-cap) environments and reports their rate: the loop is serial, so E environments take E / cap
times as long at the same house-steps/s (stated as `baseline_envs` per leg).

Per sample, device events around the whole call give house-steps/s (E N_c 128 / span: the host
drivers are inside the span).  The batch legs also report, separately, the host time of the E
driver_window calls (perf_counter) and the device time of the one launch (events around
mdr_batch_rollout alone, the drivers computed before).  One JSON line (also written to --out): per leg
and tree the median and [min, max], and whether the batch's range lies wholly above the baseline's.
"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
GRID = [(1024, 1000), (256, 1000), (8192, 50), (64, 1000)]
SOURCES = ["bangbang", "random"]
TICKS = 128
DEADBAND = 0.05


def all_legs():
    return [f"{e}x{n}:{c}:{d}" for e, n in GRID for c in SOURCES for d in ("2d", "1d")]


def props_of(n):
    from bench import env_props

    p = env_props(n)
    p.cluster_prop.house_prop.deadband = DEADBAND
    return p


def child(a):
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "marl-demandresponse_amd")]
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch creates the HIP events on the first record(): not inside a timing)
    e1.record()
    legs = a.legs.split(",")
    shapes = sorted({leg.split(":")[0] for leg in legs}, key=lambda s: legs.index(next(x for x in legs if x.startswith(s))))
    out = {}

    def span(fn):
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    for shape in shapes:
        E, n = (int(x) for x in shape.split("x"))
        mine = [leg for leg in legs if leg.split(":")[0] == shape]
        if a.child == "batch":
            from mdr_amd.batch import EnvBatch
            from mdr_amd.environment import ACTION_MODES

            t0 = time.perf_counter()
            b = EnvBatch(props_of(n), E, seeds=[8 + e for e in range(E)])
            out.setdefault("build_s", {})[shape] = time.perf_counter() - t0
            rew = {"2d": b.empty_rewards(TICKS), "1d": b.empty_rewards(None)}
            for leg in mine:  # warm-up: the same shapes
                b.rollout(TICKS, action_mode=leg.split(":")[1], rewards=rew[leg.split(":")[2]])
            for _ in range(a.rounds):
                for leg in mine:
                    _, c, d = leg.split(":")
                    s = span(lambda: b.rollout(TICKS, action_mode=c, rewards=rew[d]))
                    t0 = time.perf_counter()
                    ticks = b._driver_windows(TICKS)
                    host = time.perf_counter() - t0
                    stride = 0 if d == "1d" else b.n_envs * b.stride
                    dev = span(lambda: b._launch(ticks, None, 0, ACTION_MODES[c], rew[d], stride))
                    r = out.setdefault(leg, {"rate": [], "host_drivers_s": [], "device_launch_s": []})
                    r["rate"].append(E * n * TICKS / s)
                    r["host_drivers_s"].append(host)
                    r["device_launch_s"].append(dev)
            b.close()
            del b, rew
        else:
            from mdr_amd.environment import Environment

            cap = min(E, a.baseline_cap)
            envs = [Environment(props_of(n), device="cuda:0", rng=random.Random(8 + e), seed=8 + e,
                                population="reference") for e in range(cap)]
            rew = {"2d": torch.empty((TICKS, n), dtype=torch.float64, device="cuda:0"),
                   "1d": torch.empty(n, dtype=torch.float64, device="cuda:0")}

            def run(c, d):
                for env in envs:
                    env.rollout(TICKS, action_mode=c, rewards=rew[d])

            for leg in mine:
                run(*leg.split(":")[1:])
            for _ in range(a.rounds):
                for leg in mine:
                    _, c, d = leg.split(":")
                    s = span(lambda: run(c, d))
                    r = out.setdefault(leg, {"rate": [], "baseline_envs": cap})
                    r["rate"].append(cap * n * TICKS / s)
            for env in envs:
                env.shard.close()
            del envs
        torch.cuda.empty_cache()
    print("CHILD " + json.dumps(out), flush=True)


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "samples": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (the baseline)")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the legs inside a process")
    ap.add_argument("--alternations", type=int, default=2, help="parent / this-tree process pairs")
    ap.add_argument("--baseline-cap", type=int, default=64, help="stand-alone environments the baseline builds at most")
    ap.add_argument("--legs", default="", help="comma-separated ExN:source:2d|1d (default: all)")
    ap.add_argument("--out", help="also write the JSON result here")
    ap.add_argument("--child", choices=["batch", "baseline"])
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree: the baseline comes from a checkout of the parent commit")
    legs = a.legs.split(",") if a.legs else all_legs()
    samples, build = {}, {}
    for _ in range(a.alternations):
        for who, tree in (("baseline", a.parent_tree), ("batch", a.tree)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", who, "--tree", tree, "--legs", ",".join(legs),
                   "--rounds", str(a.rounds), "--baseline-cap", str(a.baseline_cap)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"{who} child failed ({r.returncode})")
            got = json.loads(line[-1][6:])
            for shape, s in got.pop("build_s", {}).items():
                build.setdefault(shape, []).append(s)
            for leg, rec in got.items():
                for k, v in rec.items():
                    if isinstance(v, list):
                        samples.setdefault((who, leg, k), []).extend(v)
                    else:
                        samples[(who, leg, k)] = v
            print(f"{who}: done", file=sys.stderr, flush=True)
    res = {"bench": "env_batch", "ticks_per_call": TICKS, "deadband": DEADBAND, "unit": "house-steps/s",
           "samples_per_leg": a.rounds * a.alternations, "baseline": "parent commit: stand-alone Environments, "
           "rollout(128) each, in a Python loop", "batch_build_s": {k: stats(v) for k, v in build.items()}, "legs": {}}
    for leg in legs:
        bt, bs = stats(samples[("batch", leg, "rate")]), stats(samples[("baseline", leg, "rate")])
        res["legs"][leg] = {"batch": bt, "baseline": bs, "baseline_envs": samples[("baseline", leg, "baseline_envs")],
                            "batch_over_baseline": bt["median"] / bs["median"],
                            "batch_range_above_baseline": bt["min"] > bs["max"],
                            "host_drivers_s": stats(samples[("batch", leg, "host_drivers_s")]),
                            "device_launch_s": stats(samples[("batch", leg, "device_launch_s")])}
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
