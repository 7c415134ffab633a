"""Golden fixture of the reference's Metrics under GreedyMyopic controllers (config C3), written to
tests/golden/services_greedy.npz.  Run where the reference tree is present (the path and import
shims are ``make_golden``'s); nothing of the reference is copied here — only what its programs
compute.

Recipe: ``make_golden.gen_services``'s ControllerManager-style loop (controller_manager.py:104-187:
random.seed, three resets, then per tick the controllers' actions -> env.step ->
Metrics.update(obs, next_obs, rewards, step)) with one ``GreedyMyopic`` per house
(greedy_myopic_controller.py:9-104; ``global_myopic_memory`` cleared first), N = 50, T = 120,
seed 4, ``start_stats_from`` 30, the sinusoidal signal.  Recorded: Metrics' twelve accumulators after
every update (metrics_service.py:108-157), the three RMS values, every tick's N actions and the meta
JSON.

The reference sorts the houses' keys ``-(indoor_temp - target_temp)`` with pandas' default unstable
quicksort, so two equal keys would leave the order, and with it the fixture, to the implementation:
every tick asserts that the keys are pairwise distinct, and the smallest gap seen goes into the meta.
A seed that ties is passed over for the next one that does not (``seed_requested`` keeps the first).
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np

import make_golden as G  # the reference path and the sys.modules shims

OUT = G.OUT

FIELDS = ["cumul_avg_reward", "cumul_temp_offset", "cumul_temp_error", "cumul_signal_offset",
          "cumul_signal_error", "cumul_squared_error_temp", "max_temp_error", "cumul_OD_temp", "cumul_signal",
          "cumul_cons", "cumul_squared_error_sig", "cumul_squared_max_error_temp"]


class KeyTie(Exception):
    pass


def run(N: int, T: int, seed: int, start_stats_from: int):
    from app.services.metrics_service import Metrics

    props = G.make_props({"cluster_prop.nb_agents": N, "power_grid_prop.signal_properties.mode": "sinusoidals"})
    random.seed(seed)
    env = G.Environment(props)
    obs = env.reset()
    obs = env.reset()
    met = Metrics(sys.modules["app.services.wandb_service"].WandbManager())
    met.initialize(N, start_stats_from, T)
    G.greedy_mod.global_myopic_memory[0] = None
    G.greedy_mod.global_myopic_memory[1] = None
    ctl = [G.greedy_mod.GreedyMyopic({"id": i}, None) for i in range(N)]
    rec = {f: [] for f in FIELDS}
    actions, min_gap = [], float("inf")
    for step in range(T):
        key = np.sort([-(obs[i]["indoor_temp"] - obs[i]["target_temp"]) for i in range(N)])
        gap = float(np.diff(key).min())
        if not gap > 0.0:
            raise KeyTie(f"seed {seed}: two houses share a key at tick {step}")
        min_gap = min(min_gap, gap)
        acts = {i: int(ctl[i].act(obs)) for i in range(N)}
        actions.append([acts[i] for i in range(N)])
        nxt, rew = env.step(acts)
        met.update(obs, nxt, rew, step)
        for f in FIELDS:
            rec[f].append(float(getattr(met, f)))
        obs = nxt
    met.update_rms(T)
    out = {f"metrics_{f}": np.array(v, np.float64) for f, v in rec.items()}
    out["rms"] = np.array([met.rmse_sig_per_ag, met.rmse_temp, met.rms_max_error_temp], np.float64)
    out["actions"] = np.array(actions, np.uint8)
    return out, min_gap


def gen_services_greedy(N: int = 50, T: int = 120, seed: int = 4, start_stats_from: int = 30) -> None:
    requested = seed
    while True:
        try:
            out, min_gap = run(N, T, seed, start_stats_from)
            break
        except KeyTie as e:
            print(e, "- trying the next seed")
            seed += 1
    meta = {"N": N, "T": T, "seed": seed, "seed_requested": requested, "start_stats_from": start_stats_from,
            "resets": 3, "controller": "greedy_myopic", "signal": "sinusoidals", "min_key_gap": min_gap}
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(os.path.join(OUT, "services_greedy.npz"), **out)
    print("services_greedy.npz written:", meta, "ON per tick:", out["actions"].sum(1)[:12], "...")


if __name__ == "__main__":
    gen_services_greedy()
