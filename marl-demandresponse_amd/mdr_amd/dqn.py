"""DQN / DDQN on the device: epsilon-greedy rollouts from the fused Q head, replay, the update.

Reference: ``DQN`` / ``DDQN`` — server/app/core/agents/trainables/dqn.py:54-229 (properties:
``DQNProperties``, dqn.py:17-51; network: ``DQN_network``, network.py:84-103; memory:
``ReplayBuffer``, buffer.py:14-33), and the deployed ``DQNController``
(server/app/core/agents/controllers/rl_controllers.py:97-159), which is ``select_actions`` at
epsilon 0.

What is the same: the policy / target networks and their initialisation under
``torch.manual_seed(seed)`` (the target loaded from the policy), Adam, the replay memory's
drop-oldest rule, a batch drawn with replacement (``sampler="reference"``: the reference's own draws
from the global Python RNG, index for index), ``Q(s, a)`` by gather, ``r + gamma max_a' Q_target(s',
a')``, SmoothL1Loss, gradients clamped elementwise to [-1, 1], the soft target update by ``tau``, and
``decrease_epsilon`` — which in the reference sets ``epsilon = max(epsilon_decay, min_epsilon)``,
i.e. a constant after the first update (``epsilon_schedule="reference"``; "multiplicative" is
``max(epsilon * epsilon_decay, min_epsilon)``).  ``dqn_update`` is that arithmetic as a pure
function over tensors (tests/test_dqn_cpu.py pins it against the reference on the CPU).

What is changed, deliberately:
  * epsilon-greedy draws come from the device actor's Philox stream (mdr_amd.actor.DeviceActor, head
    "q": explore iff the house's 24-bit uniform < epsilon, random action = bit 0 of the same word),
    not from Python's ``random``;
  * ``collect`` keeps transitions as state snapshots (mdr_amd.replay.ReplayStore, 29 B each) and
    rebuilds the batch's ``s`` and ``s'`` rows on demand; ``store_transition`` keeps explicit rows
    like the reference;
  * ``double=True`` (the reference's ``DDQN``, dqn.py:196-229).  The reference's DDQN.update adds
    ``reward`` [B, 1] to ``next_q.unsqueeze(1)`` [B, 1, 1], which broadcasts to a B x B target that
    SmoothL1Loss then broadcasts against ``q_values`` (torch warns), and it never updates the target
    network.  Here the target is elementwise ``r_i + gamma Q_target(s'_i, argmax_a Q_policy(s'_i,
    a))`` and the target network follows by ``tau`` as in DQN.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from typing import List, Optional

from .actor import DeviceActor, make_qnet


def _torch():
    import torch

    return torch


@dataclass
class DQNConfig:
    """DQNProperties (dqn.py:17-51) defaults."""

    network_layers: List[int] = field(default_factory=lambda: [100, 100])
    gamma: float = 0.99
    tau: float = 0.001
    lr: float = 3e-3
    buffer_capacity: int = 524288
    batch_size: int = 256
    epsilon_decay: float = 0.99998
    min_epsilon: float = 0.01


def next_epsilon(epsilon: float, cfg: DQNConfig, schedule: str = "reference") -> float:
    """Epsilon after one update.  "reference": DQN.decrease_epsilon literally (dqn.py:179-181),
    ``max(epsilon_decay, min_epsilon)`` whatever epsilon was; "multiplicative":
    ``max(epsilon * epsilon_decay, min_epsilon)``."""
    if schedule == "reference":
        return float(max(cfg.epsilon_decay, cfg.min_epsilon))
    if schedule == "multiplicative":
        return float(max(epsilon * cfg.epsilon_decay, cfg.min_epsilon))
    raise ValueError("epsilon_schedule must be 'reference' or 'multiplicative'")


def reference_sample(length: int, batch: int) -> List[int]:
    """The positions ReplayBuffer.sample draws (buffer.py:28-30: ``random.choices(memory, k)``) in a
    memory of ``length`` transitions, oldest first, from the global Python RNG — with replacement."""
    return random.choices(range(length), k=batch)


def dqn_update(policy, target, optimizer, s, a, r, s2, cfg: DQNConfig, double: bool = False):
    """One DQN.update step (dqn.py:147-177) on a drawn batch: ``s`` / ``s2`` float32 [B, F], ``a``
    int64 [B], ``r`` float32 [B], on the networks' device (no env, no GPU needed).  Steps the policy
    through ``optimizer``, soft-updates ``target`` by ``cfg.tau``; returns the loss (0-d tensor,
    before the step).  ``double``: see the module docstring."""
    torch = _torch()
    q_values = policy(s).gather(1, a.view(-1, 1))
    with torch.no_grad():
        if double:
            next_action = policy(s2).argmax(dim=1, keepdim=True)
            next_q = target(s2).gather(1, next_action).squeeze(1)
        else:
            next_q = target(s2).max(1)[0]
        expected = r.view(-1, 1) + (next_q.unsqueeze(1) * cfg.gamma)
    loss = torch.nn.SmoothL1Loss()(q_values, expected)
    optimizer.zero_grad()
    loss.backward()
    for p in policy.parameters():
        p.grad.data.clamp_(-1, 1)
    optimizer.step()
    with torch.no_grad():  # update_target_network (dqn.py:139-145)
        new = policy.state_dict()
        params = target.state_dict()
        for k in params.keys():
            params[k] = (1 - cfg.tau) * params[k] + cfg.tau * new[k]
        target.load_state_dict(params)
    return loss.detach()


class DeviceDQN:
    """DQN (``double=True``: DDQN) with device Q-head rollouts, device replay and the update on the GPU."""

    def __init__(self, env, config: Optional[DQNConfig] = None, num_action: int = 2, seed: int = 1,
                 precision: str = "bf16x3", double: bool = False, sampler: str = "reference",
                 epsilon_schedule: str = "reference", collect_ticks: int = 0):
        """``sampler``: "reference" draws each batch's indices from the global Python RNG exactly as
        the reference does (256 int64 go to the device); "device" draws them with ``torch.randint``
        on the GPU.  ``epsilon_schedule``: see ``next_epsilon``.  ``collect_ticks`` > 0 allocates a
        ``ReplayStore`` of that many ticks (``self.store``): ``collect`` fills it from the
        graph-captured rollout and ``update`` trains from it; ``store_transition`` fills a ring of
        ``buffer_capacity`` explicit transitions instead.  One update trains from one of the two."""
        torch = _torch()
        if sampler not in ("reference", "device"):
            raise ValueError("sampler must be 'reference' or 'device'")
        next_epsilon(1.0, config or DQNConfig(), epsilon_schedule)  # (ValueError: unknown schedule)
        self.cfg = config or DQNConfig()
        self.env = env
        self.double = bool(double)
        self.sampler = sampler
        self.epsilon_schedule = epsilon_schedule
        self.epsilon = 1.0  # dqn.py:59
        num_state = env.obs_spec().n_feat
        self.num_state, self.num_action = num_state, num_action
        torch.manual_seed(seed)  # dqn.py:62-81: policy then target from this stream, then target <- policy
        self.policy_net = make_qnet(num_state, num_action, self.cfg.network_layers, seed=None)
        self.target_net = make_qnet(num_state, num_action, self.cfg.network_layers, seed=None)
        self.target_net.load_state_dict(self.policy_net.state_dict())
        dev = env.shard.device
        self.policy_net.to(dev)
        self.target_net.to(dev)
        self.policy_optimizer = torch.optim.Adam(self.policy_net.parameters(), self.cfg.lr)
        self.device_actor = DeviceActor(env, self.policy_net, precision=precision, head="q", epsilon=self.epsilon)
        self.store = None
        if collect_ticks > 0:
            from .replay import ReplayStore

            self.store = ReplayStore(env, collect_ticks)
        self._buf = None  # store_transition's ring: (s, a, r, s2) tensors of buffer_capacity rows
        self._pos = 0     # its next row
        self._len = 0     # its valid rows (the oldest is row (_pos - _len) % capacity)
        self.last_actions = None
        self.last_loss = None
        self.training_step = 0

    # ---------------------------------------------------------------- rollout
    def select_actions(self):
        """DQN.select_actions (dqn.py:93-105) for every local house from the env's current state: the
        device Q head at the current epsilon, one launch; the actions' ON counts are prepared for
        the next step."""
        self.device_actor.set_epsilon(self.epsilon)
        a, _q = self.device_actor.select_actions(count_next=True)
        self.last_actions = a
        return a

    def store_transition(self, observations, next_observations, rewards, done: bool = False) -> None:
        """dqn.py:107-123 for all houses at once: device tensors obs / next obs float32 [N, F], rewards
        float [N] (kept as float32, dqn.py:119), the last select_actions' actions.  ``done`` is
        accepted for the reference's signature; DQN.update never reads it."""
        torch = _torch()
        if self.store is not None and len(self.store):
            raise ValueError("store_transition after collect(): one update trains from one of the two buffers")
        cap = int(self.cfg.buffer_capacity)
        dev = self.env.shard.device
        s = observations.to(dev, torch.float32)
        s2 = next_observations.to(dev, torch.float32)
        r = rewards.to(dev, torch.float32).reshape(-1)
        a = self.last_actions.to(dev, torch.int64).reshape(-1)
        if self._buf is None:
            F = s.shape[1]
            self._buf = (torch.empty((cap, F), dtype=torch.float32, device=dev),
                         torch.empty(cap, dtype=torch.int64, device=dev),
                         torch.empty(cap, dtype=torch.float32, device=dev),
                         torch.empty((cap, F), dtype=torch.float32, device=dev))
        n = s.shape[0]
        if n > cap:  # (only the newest buffer_capacity pushes survive)
            s, a, r, s2 = (x[n - cap:] for x in (s, a, r, s2))
            self._pos = (self._pos + n - cap) % cap
            n = cap
        rows = (self._pos + torch.arange(n, device=dev)) % cap
        for dst, src in zip(self._buf, (s, a, r, s2)):
            dst[rows] = src
        self._pos = (self._pos + n) % cap
        self._len = min(self._len + n, cap)

    def collect(self, n_ticks: int):
        """n_ticks of select_actions -> env.step at the current epsilon as ``device_actor.rollout``
        runs them (one captured graph for individual_L2; two when the ticks cross the ring's end),
        stored in ``self.store`` with the trailing snapshot of the post-step state."""
        if self.store is None:
            raise ValueError("collect() needs DeviceDQN(..., collect_ticks=N)")
        if self._len:
            raise ValueError("collect() after store_transition: one update trains from one of the two buffers")
        self.device_actor.set_epsilon(self.epsilon)
        self.store.collect(self.device_actor, n_ticks)

    def __len__(self) -> int:
        if self.store is not None and len(self.store):
            return len(self.store)
        return self._len

    # ---------------------------------------------------------------- update
    def _sample(self, length: int):
        torch = _torch()
        dev = self.env.shard.device
        if self.sampler == "reference":
            return torch.tensor(reference_sample(length, self.cfg.batch_size), dtype=torch.int64, device=dev)
        return torch.randint(length, (self.cfg.batch_size,), dtype=torch.int64, device=dev)

    def update(self) -> bool:
        """DQN.update (dqn.py:147-177; ``dqn_update``) on one batch drawn with replacement, then the
        epsilon schedule; the fused kernel's packed weights and epsilon follow.  Returns False while
        the memory holds fewer than batch_size transitions."""
        L = len(self)
        if L < self.cfg.batch_size:
            return False
        idx = self._sample(L)
        st = self.store if self.store is not None and len(self.store) else None
        if st is not None:
            s, s2 = st.states(idx), st.next_states(idx)
            a, r = st.actions_at(idx), st.rewards_at(idx).float()
        else:
            cap = int(self.cfg.buffer_capacity)
            rows = (idx + (self._pos - self._len)) % cap  # logical (oldest first) -> ring row
            s, a, r, s2 = (x[rows] for x in self._buf)
        self.last_loss = dqn_update(self.policy_net, self.target_net, self.policy_optimizer, s, a, r, s2,
                                    self.cfg, self.double)
        self.epsilon = next_epsilon(self.epsilon, self.cfg, self.epsilon_schedule)
        self.training_step += 1
        self.device_actor.load_weights()
        self.device_actor.set_epsilon(self.epsilon)
        return True

    def save(self, path: str, t=None) -> None:
        """dqn.py:184-193: the policy network's state_dict as ``actor<t>.pth`` / ``actor.pth``."""
        import os

        torch = _torch()
        os.makedirs(path, exist_ok=True)
        torch.save(self.policy_net.state_dict(), os.path.join(path, "actor" + (str(t) if t else "") + ".pth"))
