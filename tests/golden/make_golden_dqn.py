"""Golden fixture of the reference DQN (server/app/core/agents/trainables/dqn.py:54-194), written to
tests/golden/dqn.npz.  Run where the reference tree is present (the path and import shims are
``make_golden``'s); nothing of the reference is copied here — only what its programs compute.

Recipe: ``DQN(DQNProperties(batch_size=16, buffer_capacity=64), num_state=14, seed=1)``; T = 40 ticks
of N = 2 agents of synthetic float32-exact states, actions and rewards from ``RandomState(5)`` pushed
through ``store_transition`` (80 pushes into a deque of 64: the drop-oldest rule is exercised);
``random.seed(7)`` then three ``update()`` calls.  Recorded: the initial policy weights, the inputs,
per update the sampled indices (``ReplayBuffer.sample`` is ``random.choices(memory, k)``, which draws
the same positions as ``random.choices(range(len(memory)), k)`` from the same seed), the loss (the
update's own expression on the drawn batch, evaluated before the step) and the policy / target
weights after it, the final epsilon, and ``select_actions`` at epsilon 0 on 64 recorded states (the
argmax actions and the Q rows).
"""
from __future__ import annotations

import json
import os
import random

import numpy as np

import make_golden as G  # the reference path and the sys.modules shims

OUT = G.OUT


def gen_dqn(num_state: int = 14, T: int = 40, batch_size: int = 16, capacity: int = 64, updates: int = 3) -> None:
    import torch
    from app.core.agents.trainables.buffer import Transition
    from app.core.agents.trainables.dqn import DQN, DQNProperties

    cfg = DQNProperties(batch_size=batch_size, buffer_capacity=capacity)
    agent = DQN(cfg, num_state=num_state, num_action=2, seed=1)
    sd = lambda net: {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}  # noqa: E731
    out = {f"init_policy_{k}": v for k, v in sd(agent.policy_net).items()}
    rs = np.random.RandomState(5)
    states = rs.normal(0, 1, (T + 1, 2, num_state)).astype(np.float32)
    actions = rs.randint(0, 2, (T, 2)).astype(np.int64)
    rewards = -rs.uniform(0, 2, (T, 2))
    for t in range(T):
        agent.last_actions = {0: bool(actions[t, 0]), 1: bool(actions[t, 1])}
        agent.store_transition([states[t, 0].astype(np.float64), states[t, 1].astype(np.float64)],
                               [states[t + 1, 0].astype(np.float64), states[t + 1, 1].astype(np.float64)],
                               {0: float(rewards[t, 0]), 1: float(rewards[t, 1])}, False)
    assert len(agent.buffer) == capacity
    # the indices the updates will draw: the same stream, replayed after the updates' own seed
    random.seed(7)
    idx = np.array([random.choices(range(capacity), k=batch_size) for _ in range(updates)], np.int64)
    random.seed(7)
    losses = []
    for u in range(updates):
        # the loss of this update's batch at the weights before its step (dqn.py:151-166 on the
        # recorded indices; the update below draws the same ones)
        batch = Transition(*zip(*[agent.buffer.memory[i] for i in idx[u]]))
        s, a, r, s2 = agent.convert_batch(batch)
        with torch.no_grad():
            q = agent.policy_net(s).gather(1, a)
            nq = agent.target_net(s2).max(1)[0]
            losses.append(float(torch.nn.SmoothL1Loss()(q, r + nq.unsqueeze(1) * agent.gamma)))
        agent.update()
        out.update({f"u{u}_policy_{k}": v for k, v in sd(agent.policy_net).items()})
        out.update({f"u{u}_target_{k}": v for k, v in sd(agent.target_net).items()})
    # the updates consumed exactly the recorded draws: the stream continues where the replay ends
    after_updates = random.random()
    random.seed(7)
    for _ in range(updates):
        random.choices(range(capacity), k=batch_size)
    after_replay = random.random()
    assert after_updates == after_replay
    # select_actions at epsilon 0 (the DQNController's rule) on 64 recorded states
    agent.epsilon_final = float(agent.epsilon)
    agent.epsilon = 0.0
    sel_states = rs.normal(0, 1, (64, num_state)).astype(np.float32)
    acts = agent.select_actions([x for x in sel_states])
    with torch.no_grad():
        q_rows = agent.policy_net(torch.from_numpy(sel_states)).numpy()
    out.update(states=states, actions=actions, rewards=rewards, indices=idx, losses=np.array(losses, np.float64),
               epsilon_final=np.float64(agent.epsilon_final), sel_states=sel_states,
               sel_actions=np.array([int(acts[i]) for i in range(64)], np.int64), sel_q=q_rows,
               after_replay=np.float64(after_replay))
    meta = {"num_state": num_state, "T": T, "N": 2, "batch_size": batch_size, "buffer_capacity": capacity,
            "updates": updates, "seed": 1, "update_seed": 7, "gamma": cfg.gamma, "tau": cfg.tau, "lr": cfg.lr,
            "epsilon_decay": cfg.epsilon_decay, "min_epsilon": cfg.min_epsilon}
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(os.path.join(OUT, "dqn.npz"), **out)
    print("dqn.npz written:", {k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items() if "policy" not in k
                               and "target" not in k})


if __name__ == "__main__":
    gen_dqn()
