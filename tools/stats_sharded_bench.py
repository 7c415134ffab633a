"""Stats rows of a sharded cluster against the only sharded route to a row the parent
commit has: the per-tick Python loop around services.cluster_stats.

    python tools/stats_sharded_bench.py --parent-tree PATH [--houses 1048576,131072] [--out FILE]

The method of tools/bangbang_sharded_bench.py: one GPU, world 1 over the library's own RCCL
communicator, synthetic houses, deadband 0.05 degC, device events on the caller's stream, a warm-up of
the same shapes, --rounds samples per leg and process with the legs alternated, parent-commit and
this-tree processes alternated --alternations times (fresh processes).  Every leg reads its rows on the
host after every call (``host()``; the loop legs: cluster_stats' ``.cpu()`` every tick).

Legs per controller c (bangbang, deadband_bangbang), calls of --chunk = 128 ticks:

    a  loop:c       PARENT tree, sharded env: step_tensor(None, action_mode=c, lookahead=c) +
                    services.cluster_stats(env, r) per tick
    b  sharded:c    sharded env: rollout(128, c, rewards=row, stats=ShardedRolloutStats) + host()
    c  unsharded:c  no communicator: rollout(128, c, rewards=row, stats=RolloutStats) + host()
    d  norows:c     sharded env: rollout(128, c, rewards=row)

and for the actor (a 'neighbours' ring cluster, the default two-layer net), calls of --actor-chunk = 20:

    a  loop:actor       PARENT tree, sharded env: select_actions + step_tensor + cluster_stats per tick
    b  sharded:actor    sharded env: DeviceActor.rollout(20, rewards=row, stats=...) + host()
    c  unsharded:actor  no communicator: the same call (graph replay)

One JSON line (also written to --out): per size and leg the median and (min, max) of house-steps/s
over every sample; per source whether leg b's whole range lies above leg a's, and b/c, b/d.
"""
import argparse
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CTRLS = ["bangbang", "deadband_bangbang"]
SOURCES = CTRLS + ["actor"]
DEADBAND = 0.05


def child(a):
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "marl-demandresponse_amd")]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(a.port))
    import torch
    import torch.distributed as dist

    from bench import env_props
    from mdr_amd import services
    from mdr_amd.actor import DeviceActor, make_actor
    from mdr_amd.distributed import make_comm
    from mdr_amd.environment import Environment

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    n = int(a.houses)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()  # (torch creates the HIP events on the first record(): not inside a timing)
    e1.record()
    row = torch.empty(n, dtype=torch.float64, device=dev)
    envs = {}

    def make(sharded, actor):
        p = env_props(n)
        p.cluster_prop.house_prop.deadband = DEADBAND
        if actor:
            p.cluster_prop.agents_comm_prop.mode = "neighbours"
        kw = {"rank": 0, "world": 1, "comm": make_comm("rccl")} if sharded else {}
        env = Environment(p, device=dev, rng=random.Random(1), population="synthetic", seed=5, **kw)
        out = {"env": env}
        if actor:
            out["actor"] = DeviceActor(env, make_actor(env.obs_spec().n_feat).to(dev))
        return out

    def plan(leg):
        kind, src = leg.split(":")
        chunk = a.actor_chunk if src == "actor" else a.chunk
        ticks = a.actor_ticks if src == "actor" else (a.loop_ticks if kind == "loop" else a.ticks)
        calls = -(-ticks // chunk)
        return kind, src, chunk, calls

    def run(leg):
        kind, src, chunk, calls = plan(leg)
        key = (kind != "unsharded", src == "actor")
        if key not in envs:
            envs[key] = make(*key)
        e = envs[key]
        env = e["env"]
        if kind == "loop":  # the parent's only sharded route to a row
            for _ in range(calls * chunk):
                if src == "actor":
                    act, _p = e["actor"].select_actions()
                    r = env.step_tensor(act, rewards=row)
                else:
                    r = env.step_tensor(None, action_mode=src, lookahead=src, rewards=row)
                services.cluster_stats(env, r)
            return
        if kind != "norows" and "stats" not in e.setdefault(kind, {}):
            mk = getattr(services, "rollout_stats_for", None) or (lambda env_, cap: services.RolloutStats(env_, cap))
            e[kind]["stats"] = mk(env, chunk)
        for _ in range(calls):
            st = None if kind == "norows" else e[kind]["stats"]
            if st is not None:
                st.clear()
            if src == "actor":
                e["actor"].rollout(chunk, rewards=row, stats=st)
            else:
                env.rollout(chunk, action_mode=src, rewards=row, stats=st)
            if st is not None:
                st.host()

    def timed(leg):
        _kind, _src, chunk, calls = plan(leg)
        torch.cuda.synchronize()
        e0.record()
        run(leg)
        e1.record()
        e1.synchronize()
        return n * calls * chunk / (e0.elapsed_time(e1) * 1e-3)

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
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit (leg a)")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--houses", default="1048576,131072", help="comma-separated cluster sizes")
    ap.add_argument("--ticks", type=int, default=1024, help="ticks per sample of the rollout legs")
    ap.add_argument("--loop-ticks", type=int, default=256, help="ticks per sample of the per-tick loop legs")
    ap.add_argument("--actor-ticks", type=int, default=100, help="ticks per sample of the actor legs")
    ap.add_argument("--chunk", type=int, default=128, help="ticks per bang-bang rollout call")
    ap.add_argument("--actor-chunk", type=int, default=20, help="ticks per actor rollout call")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the legs inside a process")
    ap.add_argument("--alternations", type=int, default=2, help="parent / this-tree process pairs")
    ap.add_argument("--sources", default=",".join(SOURCES))
    ap.add_argument("--port", type=int, default=29519)
    ap.add_argument("--out", help="also write the JSON result here")
    ap.add_argument("--legs", default="")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree: leg a comes from a checkout of the parent commit")
    sources = a.sources.split(",")
    parent_legs = [f"loop:{s}" for s in sources]
    tree_legs = [f"{k}:{s}" for s in sources for k in ("sharded", "unsharded", "norows") if (k, s) != ("norows", "actor")]
    res = {"bench": "stats_sharded", "comm": "rccl", "world": 1, "rollout_chunk": a.chunk, "actor_chunk": a.actor_chunk,
           "ticks_per_sample": {"rollout": a.ticks, "loop": a.loop_ticks, "actor": a.actor_ticks}, "deadband": DEADBAND,
           "unit": "house-steps/s", "samples_per_leg": a.rounds * a.alternations, "sizes": {}}
    for houses in a.houses.split(","):
        samples = {}
        for _ in range(a.alternations):
            for who, tree, lg in (("parent", a.parent_tree, parent_legs), ("tree", a.tree, tree_legs)):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--legs", ",".join(lg),
                       "--houses", houses, "--ticks", str(a.ticks), "--loop-ticks", str(a.loop_ticks),
                       "--actor-ticks", str(a.actor_ticks), "--chunk", str(a.chunk), "--actor-chunk", str(a.actor_chunk),
                       "--rounds", str(a.rounds), "--port", str(a.port)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout + r.stderr)
                    raise SystemExit(f"{who} child failed ({r.returncode})")
                for k, v in json.loads(line[-1][6:]).items():
                    samples.setdefault(k, []).extend(v)
                print(f"{houses} {who}: done", file=sys.stderr, flush=True)
        rows = {leg: stats(v) for leg, v in samples.items()}
        verdict = {}
        for s in sources:
            la, lb, lc, ld = (rows.get(f"{k}:{s}") for k in ("loop", "sharded", "unsharded", "norows"))
            verdict[s] = {"b_range_above_a": lb["min"] > la["max"], "b_over_a": lb["median"] / la["median"],
                          "b_over_c": lb["median"] / lc["median"]}
            if ld:
                verdict[s]["b_over_d"] = lb["median"] / ld["median"]
        res["sizes"][houses] = {"legs": rows, "sources": verdict}
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
