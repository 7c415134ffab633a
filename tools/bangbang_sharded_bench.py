"""Sharded closed-loop bang-bang rollouts against the only sharded form the parent
commit has for these sources: the per-tick step_tensor(None, action_mode=c, lookahead=c) loop.

    python tools/bangbang_sharded_bench.py --parent-tree PATH [--houses 1048576,131072] [--ticks 2048] [--out FILE]

One GPU, world 1 over the library's own RCCL communicator, synthetic houses, deadband 0.05 degC.
Legs, per controller c (bangbang, deadband_bangbang):

    loop:c               sharded env, the per-tick loop (both trees; the parent's samples are the baseline)
    sharded:c:2d:pipe    sharded env, rollout(chunk) into [chunk, N] rewards, two streams (the default)
    sharded:c:2d:serial  ... MDR_OPT_WINDOW_PIPELINE 0 (one stream)
    sharded:c:1d:pipe    ... into a 1-D [N] buffer (the library runs one shared row on one stream whatever the
    sharded:c:1d:serial      option says, so these two legs time the same sequence: a control)
    unsharded:c:2d       no communicator: the ceiling
    unsharded:c:1d

The baseline is never taken from this tree: --parent-tree names a built checkout of the parent
commit, and parent and this-tree child processes alternate (fresh processes: each initialises the
GPU itself).  Inside a process the legs alternate --rounds times after a warm-up of the same
shapes; device events on the caller's stream time each sample (>= --ticks ticks; the stream waits
for the comm stream's last finish, so the span covers it).  One JSON line (also written to --out):
per size and leg the median and the spread (min, max) of house-steps/s over every sample, whether
each sharded rollout leg's range lies wholly above the parent loop's, and its ratio to the unsharded leg.
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


def tree_legs():
    out = []
    for c in CTRLS:
        out.append(f"loop:{c}")
        out += [f"sharded:{c}:{d}:{f}" for d in ("2d", "1d") for f in ("pipe", "serial")]
        out += [f"unsharded:{c}:{d}" for d in ("2d", "1d")]
    return out


def child(a):
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "marl-demandresponse_amd")]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(a.port))
    import torch
    import torch.distributed as dist

    from bench import env_props
    from mdr_amd.distributed import make_comm
    from mdr_amd.environment import Environment

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    n, chunk = int(a.houses), a.chunk
    calls = -(-a.ticks // chunk)
    ticks = calls * chunk  # every leg runs the same number of ticks per sample
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch creates the HIP events on the first record(): not inside a timing)
    e1.record()

    def make(sharded):
        p = env_props(n)
        p.cluster_prop.house_prop.deadband = DEADBAND
        kw = {"rank": 0, "world": 1, "comm": make_comm("rccl")} if sharded else {}
        return Environment(p, device=dev, rng=random.Random(1), population="synthetic", seed=5, **kw)

    rew = {"2d": torch.empty((chunk, n), dtype=torch.float64, device=dev),  # (one buffer serves every leg)
           "1d": torch.empty(n, dtype=torch.float64, device=dev)}
    envs = {}

    def run(leg):
        kind, ctrl, *rest = leg.split(":")
        key = (kind != "unsharded", ctrl)
        if key not in envs:
            envs[key] = make(key[0])
        env = envs[key]
        if kind == "loop":
            for _ in range(ticks):
                env.step_tensor(None, action_mode=ctrl, lookahead=ctrl)
            return
        if kind == "sharded":
            env.shard.set_option("window_pipeline", rest[1] == "pipe")
        for _ in range(calls):
            env.rollout(chunk, action_mode=ctrl, rewards=rew[rest[0]])

    def timed(leg):
        torch.cuda.synchronize()
        e0.record()
        run(leg)
        e1.record()
        e1.synchronize()
        return n * ticks / (e0.elapsed_time(e1) * 1e-3)

    legs = a.legs.split(",")
    for leg in legs:
        run(leg)  # warm-up: the same shapes
    out = {}
    for _ in range(a.rounds):
        for leg in legs:
            out.setdefault(leg, []).append(timed(leg))
    print("CHILD " + json.dumps(out), flush=True)
    torch.cuda.synchronize()
    dist.destroy_process_group()


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "samples": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (the baseline)")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--houses", default="1048576,131072", help="comma-separated cluster sizes")
    ap.add_argument("--ticks", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=128, help="ticks per rollout call")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the legs inside a process")
    ap.add_argument("--alternations", type=int, default=2, help="parent / this-tree process pairs")
    ap.add_argument("--legs", default="", help="comma-separated legs of this tree's processes (default: all)")
    ap.add_argument("--port", type=int, default=29517)
    ap.add_argument("--out", help="also write the JSON result here")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree: the baseline comes from a checkout of the parent commit")
    legs = a.legs.split(",") if a.legs else tree_legs()
    parent_legs = [f"loop:{c}" for c in CTRLS]
    calls = -(-a.ticks // a.chunk)
    res = {"bench": "bangbang_sharded", "comm": "rccl", "world": 1, "ticks_per_sample": calls * a.chunk,
           "rollout_chunk": a.chunk, "deadband": DEADBAND, "unit": "house-steps/s",
           "samples_per_leg": a.rounds * a.alternations, "sizes": {}}
    for houses in a.houses.split(","):
        samples = {}
        for _ in range(a.alternations):
            for who, tree, lg in (("parent", a.parent_tree, parent_legs), ("tree", a.tree, legs)):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--legs", ",".join(lg),
                       "--houses", houses, "--ticks", str(a.ticks), "--chunk", str(a.chunk),
                       "--rounds", str(a.rounds), "--port", str(a.port)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout + r.stderr)
                    raise SystemExit(f"{who} child failed ({r.returncode})")
                for k, v in json.loads(line[-1][6:]).items():
                    samples.setdefault((who, k), []).extend(v)
                print(f"{houses} {who}: done", file=sys.stderr, flush=True)
        rows = {}
        for (who, leg), v in samples.items():
            rows.setdefault(leg, {})[who] = stats(v)
        for leg, row in rows.items():
            kind, ctrl, *rest = leg.split(":")
            if kind != "sharded":
                continue
            base = rows.get(f"loop:{ctrl}", {}).get("parent")
            ceil = rows.get(f"unsharded:{ctrl}:{rest[0]}", {}).get("tree")
            if base:
                row["range_above_parent_loop"] = row["tree"]["min"] > base["max"]
                row["over_parent_loop"] = row["tree"]["median"] / base["median"]
            if ceil:
                row["over_unsharded"] = row["tree"]["median"] / ceil["median"]
        res["sizes"][houses] = rows
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
