"""MA-PPO on the device: rollout storage and the PPO update.

Reference: ``MAPPO`` — server/app/core/agents/trainables/mappo.py:37-217 (properties:
``PPOProperties``, ppo.py:20-70; networks: network.py:14-58), driven by TrainingManager.start
(server/app/services/training_manager.py:183-263, update every ``time_steps_per_epoch``).

What is the same: the actor / critic modules and their initialisation order under
``torch.manual_seed(seed)``; Adam optimisers; the discounted return over the buffer in the
reference's storage order (tick-major, house-minor — the reference's ``R`` runs across houses of a
tick; ``returns="per_agent"`` discounts each house over its own ticks instead); ``ppo_update_time``
epochs of ``BatchSampler(SubsetRandomSampler(range(L)), batch_size)`` minibatches drawn from the
global torch CPU generator exactly as the reference draws them; the clipped surrogate on the ratio of
new to stored action probabilities, ``clip_grad_norm_``, and the critic's MSE to the returns.

What is changed, deliberately:
  * ``store_transition`` is O(N) per tick on device tensors (the reference deep-copies the action
    dict per house: O(N^2));
  * the critic input.  The reference builds ``Critic(num_state + num_action - 1)`` but feeds it
    ``state ++ others_actions`` — N-1 extra columns — so it only runs at N = 2 (mappo.py:50-53,
    113-115, 172-174).  Here the extra column is the mean of the other houses' actions, which has
    the declared width and equals the reference's input at N = 2 (tests/test_mappo_gpu.py pins the
    update against the reference MAPPO at N = 2).
Actions are sampled by the fused device actor (mdr_amd.actor.DeviceActor, Philox), not by torch's
Categorical RNG.

On a house-sharded ``neighbours`` environment ``collect`` / ``update`` train one policy from the
cluster's buffer: every rank builds the agent with the same seed, stores its own houses' transitions
and ring halos, and per minibatch contributes the rows it owns to one integer allreduce, after which
every rank takes the identical optimiser step (``DeviceMAPPO.update``).  ``evaluate`` and
``collect(metrics=...)`` are collective calls there: their stats rows are
``services.ShardedRolloutStats``', combined over the ranks once per call.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .actor import DeviceActor, make_actor


def _torch():
    import torch

    return torch


@dataclass
class MAPPOConfig:
    """PPOProperties (ppo.py:20-70) defaults."""

    actor_layers: List[int] = field(default_factory=lambda: [100, 100])
    critic_layers: List[int] = field(default_factory=lambda: [100, 100])
    gamma: float = 0.99
    lr_critic: float = 3e-3
    lr_actor: float = 3e-3
    clip_param: float = 0.2
    max_grad_norm: float = 0.5
    ppo_update_time: int = 10
    batch_size: int = 256


def make_critic(num_state: int, layers=(100, 100)):
    """The reference Critic (network.py:36-51): Linear layers with ReLU, one output."""
    torch = _torch()
    nn = torch.nn

    class Critic(nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = [int(x) for x in layers]
            self.fc = nn.ModuleList([nn.Linear(num_state, self.layers[0])])
            self.fc.extend([nn.Linear(self.layers[i], self.layers[i + 1]) for i in range(len(self.layers) - 1)])
            self.fc.append(nn.Linear(self.layers[-1], 1))

        def forward(self, x):
            for i in range(len(self.layers)):
                x = torch.nn.functional.relu(self.fc[i](x))
            return self.fc[len(self.layers)](x)

    return Critic()


def _suffix_affine(r, c):
    """G_i = r_i + c_i * G_{i+1} with G_L = 0, over 1-D float64 tensors, without a host round trip:
    a reverse recurrence inside ~sqrt(L) blocks of ~sqrt(L), the blocks' carries by the same scan one
    level down (G entering block b is itself a suffix recurrence over the blocks), one fix-up pass."""
    torch = _torch()
    L = r.numel()
    if L <= 64:
        g = torch.empty_like(r)
        nxt = r.new_zeros(())
        for j in range(L - 1, -1, -1):
            nxt = r[j] + c[j] * nxt
            g[j] = nxt
        return g
    M = int(np.ceil(np.sqrt(L)))
    B = -(-L // M)
    pad = B * M - L  # (padding after the end: r = c = 0, so G stays 0 there)
    r2 = torch.cat([r, r.new_zeros(pad)]).view(B, M)
    c2 = torch.cat([c, c.new_zeros(pad)]).view(B, M)
    g = torch.empty_like(r2)
    nxt = r.new_zeros(B)
    for j in range(M - 1, -1, -1):  # local returns, each block as if it ended the buffer
        nxt = r2[:, j] + c2[:, j] * nxt
        g[:, j] = nxt
    suf = torch.flip(torch.cumprod(torch.flip(c2, [1]), 1), [1])  # prod_{k >= j} c_k within the block
    # carry[b] = G at the first element of block b + 1 = g[b+1, 0] + suf[b+1, 0] * carry[b+1]
    carry = torch.cat([_suffix_affine(g[1:, 0].contiguous(), suf[1:, 0].contiguous()), r.new_zeros(1)])
    return (g + suf * carry[:, None]).reshape(-1)[:L]


def discounted_returns(reward, done, gamma: float):
    """G_i = r_i + gamma * (0 if done_i else G_{i+1}) over a 1-D device tensor (the reference's
    reversed loop, mappo.py:135-140), as the blocked scan of _suffix_affine: float64, on the
    tensor's device, no host synchronisation."""
    torch = _torch()
    if reward.numel() == 0:
        return reward.double().clone()
    return _suffix_affine(reward.double(), gamma * (1.0 - done.double()))


def shard_owner(idx, n: int, world: int):
    """(rank, local index) of the global transition indices ``idx`` (tick * n + global house, the
    reference's buffer order) of a cluster of ``n`` houses sharded over ``world`` ranks as
    ``environment.shard_range`` cuts it: rank r owns houses [r * n // world, (r + 1) * n // world),
    so a house's rank is the largest r with r * n // world <= house, and its local index is
    tick * n_local(rank) + house - offset(rank).  ``idx``: an integer torch tensor or numpy array."""
    tick, house = idx // n, idx % n
    rank = ((house + 1) * world - 1) // n
    off = rank * n // world
    nl = (rank + 1) * n // world - off
    return rank, tick * nl + (house - off)


def sharded_reference_returns(reward, done, gamma: float, rank: int, world: int, all_gather):
    """``discounted_returns`` over the cluster's buffer (tick-major, house-minor over global house
    ids) from one rank's part of it: ``reward`` [T, n_local] (this rank's houses, a contiguous range
    of every tick), ``done`` [T].  The recurrence G_i = r_i + c_i G_{i+1} (c = gamma * (1 - done) of the
    element's tick) runs across the houses of a tick, hence across ranks: each rank's part of a tick
    is one block of the buffer, an affine map of the return entering it, G_first = C + A G_in with
    A = c_t ** n_local and C the block's return for G_in = 0.  ``all_gather`` takes this rank's
    [T, 2] float64 (A, C) rows and returns every rank's, [world, T, 2] in rank order — the only
    exchange; then every rank solves the T x world block recurrence and fixes its elements up:
    G[t, j] = G0[t, j] + c_t ** (n_local - j) * G_in[t].  Shards may be uneven.  float64 [T, n_local]."""
    torch = _torch()
    r = reward.double()
    T, nl = r.shape
    c = (gamma * (1.0 - done.double())).reshape(T)
    # G0: the suffix recurrence inside every (tick, rank) block, the chain cut after its last element
    cc = c[:, None].expand(T, nl).clone()
    cc[:, nl - 1] = 0.0
    g0 = _suffix_affine(r.reshape(-1).contiguous(), cc.reshape(-1)).view(T, nl)
    # suf[t, j] = c_t ** (n_local - j): the weight of the entering return at element j
    expo = torch.arange(nl, 0, -1, device=r.device, dtype=torch.float64)
    suf = torch.pow(c[:, None], expo[None, :])
    mine = torch.stack([suf[:, 0], g0[:, 0]], 1).contiguous()
    blocks = all_gather(mine).double().cpu()  # [world, T, 2]
    g_in = torch.zeros(T, dtype=torch.float64)
    nxt = 0.0  # the return entering the buffer's last block
    A, Cc = blocks[:, :, 0].tolist(), blocks[:, :, 1].tolist()
    for t in range(T - 1, -1, -1):
        for w in range(world - 1, -1, -1):
            if w == rank:
                g_in[t] = nxt
            nxt = Cc[w][t] + A[w][t] * nxt
    return g0 + suf * g_in.to(r.device)[:, None]


def _checksum53(t):
    """A 53-bit position-weighted checksum of an integer tensor's values (exact in a double, so a
    min- and a max-allreduce of it compare the ranks' tensors): device int64 scalar."""
    torch = _torch()
    v = t.reshape(-1).to(torch.int64)
    w = torch.arange(v.numel(), device=v.device, dtype=torch.int64) % 1021 + 1
    return (v * w).sum() & ((1 << 53) - 1)


class DeviceMAPPO:
    """MAPPO with device actor rollouts, device transition storage and the PPO update on the GPU."""

    def __init__(self, env, config: Optional[MAPPOConfig] = None, num_action: int = 2, seed: int = 1,
                 precision: str = "bf16x3", returns: str = "reference", sampler: str = "reference",
                 collect_ticks: int = 0):
        """``sampler``: the minibatch permutation of each PPO epoch — "reference" (default) draws it
        from the global torch CPU generator exactly as the reference's SubsetRandomSampler does, so
        reference-seeded runs keep the reference's minibatch order and later CPU draws at any size;
        "device" (explicit opt-in) draws it on the GPU (torch.randperm on the device generator: no
        L-element host permutation and copy per epoch at C5's N x T transitions; another order);
        "auto" = "reference" up to 2^20 transitions and "device" beyond.  ``last_sampler`` records
        which one the last update used.

        ``collect_ticks`` > 0 allocates a ``RolloutStore`` of that many ticks (``self.store``):
        ``collect`` then fills it from the graph-captured rollout and ``update`` trains from it."""
        torch = _torch()
        if returns not in ("reference", "per_agent"):
            raise ValueError("returns must be 'reference' (the reference's buffer order) or 'per_agent'")
        if sampler not in ("auto", "reference", "device"):
            raise ValueError("sampler must be 'auto', 'reference' or 'device'")
        self.sampler = sampler
        self.last_sampler = None
        self.cfg = config or MAPPOConfig()
        self.env = env
        self.returns = returns
        num_state = env.obs_spec().n_feat
        self.num_state, self.num_action = num_state, num_action
        torch.manual_seed(seed)  # mappo.py:41-42: actor then critic initialised from this stream
        self.actor_net = make_actor(num_state, num_action, self.cfg.actor_layers, seed=None)
        self.critic_net = make_critic(num_state + num_action - 1, self.cfg.critic_layers)
        dev = env.shard.device
        self.actor_net.to(dev)
        self.critic_net.to(dev)
        self.actor_optimizer = torch.optim.Adam(self.actor_net.parameters(), self.cfg.lr_actor)
        self.critic_net_optimizer = torch.optim.Adam(self.critic_net.parameters(), self.cfg.lr_critic)
        self.device_actor = DeviceActor(env, self.actor_net, precision=precision)
        self.buffer = []  # per tick: (state, action, prob, reward, done)
        self.store = None  # or the compact transitions of collect()
        if collect_ticks > 0:
            from .replay import RolloutStore

            self.store = RolloutStore(env, collect_ticks)
        self.stats = None  # collect(metrics=...): the ticks' stats rows (services.RolloutStats)
        self.collected_ticks = 0
        self._eval = {}  # evaluate(env=twin): the twin's actor binding, stats rows and outputs
        self.counter = 0
        self.training_step = 0
        self.last_actions = None
        self.last_probs = None

    # ---------------------------------------------------------------- rollout
    def select_actions(self):
        """MAPPO.select_actions for every local house from the env's current state (fused obs +
        actor + sampling, one launch); the actions' ON counts are prepared for the next step."""
        a, p = self.device_actor.select_actions(count_next=True)
        self.last_actions, self.last_probs = a, p
        return a

    def store_transition(self, observations, next_observations, rewards, done: bool) -> None:
        """mappo.py:105-126 for all houses at once: device tensors obs float32 [N, F], rewards float
        [N] (the last select_actions' actions and probabilities).  ``next_observations`` is accepted
        for the reference's signature but not kept: update never reads it (mappo.py:128-217)."""
        if self.store is not None and self.store.rows:
            raise ValueError("store_transition after collect(): one update trains from one of the two buffers")
        self.buffer.append((observations, self.last_actions.clone(), self.last_probs.clone(),
                            rewards.clone(), bool(done)))
        self.counter += observations.shape[0]

    def collect(self, n_ticks: int, done: bool = True, metrics=None, time_step0: Optional[int] = None):
        """n_ticks of select_actions -> env.step as ``device_actor.rollout`` runs them (one captured
        graph for individual_L2), stored as transitions: the state snapshots, actions, probabilities
        and rewards go to ``self.store``; the last tick is marked done (training_manager.py:224-240
        marks the epoch's last step).  Returns the ticks' reward rows (a view of the store).

        ``metrics`` (mdr_amd.services.DeviceMetrics): the ticks also feed it as
        ``metrics_service.update`` does every step (training_manager.py:242-245) — their stats rows
        are written inside the same graph (``self.stats``, ``rollout_stats_for`` the store's capacity)
        and accumulated by one ``update_rollout`` as time steps ``time_step0`` .. (default: the
        ticks collected so far)."""
        if self.store is None:
            raise ValueError("collect() needs DeviceMAPPO(..., collect_ticks=N)")
        if self.buffer:
            raise ValueError("collect() after store_transition: one update trains from one of the two buffers")
        stats = None
        if metrics is not None:
            if self.stats is None:
                from .services import rollout_stats_for

                self.stats = rollout_stats_for(self.env, self.store.capacity)
            stats = self.stats
            stats.clear()
        r = self.device_actor.rollout(n_ticks, store=self.store, stats=stats)
        if done:
            self.store.done[-1] = True
        self.counter += n_ticks * self.env.n_local
        if metrics is not None:
            metrics.update_rollout(stats, self.collected_ticks if time_step0 is None else time_step0)
        self.collected_ticks += n_ticks
        return r

    # ---------------------------------------------------------------- evaluation
    def evaluate(self, n_ticks: int, env=None, return_actions: bool = False):
        """TrainingManager.test (training_manager.py:265-295): the policy run for ``n_ticks`` on a
        reset copy of the env.  ``env`` None: ``copy.deepcopy(self.env)`` as the reference does; a
        caller-kept twin may be passed instead, whose context, actor binding and rollout graph are
        then reused by later calls.  The copy is ``reset`` (which advances the shared RNG, as in the
        reference), a ``DeviceActor`` over the same ``actor_net`` and precision runs
        ``rollout(n_ticks, stats=...)`` in the copy's context, and the three means the reference logs
        (metrics_service.py:259-282) are formed from the post-step rows:

          "Mean test return"             sum_t sum_i reward_i / N / T
          "Test mean temperature error"  sum_t sum_i |T_i - target_i| / N / T
          "Test mean signal error"       sum_t N |s_post - P_post| / N^2 / T

        The training env's device state, tick, date, P, graphs and packed weights are not touched.
        On a sharded env the call is collective and every rank returns the same means.
        ``return_actions``: also the ticks' actions, uint8 [n_ticks, n_local]."""
        import copy

        from .services import evaluation_means, rollout_stats_for

        torch = _torch()
        if n_ticks < 1:
            raise ValueError("n_ticks must be at least 1")
        ev = copy.deepcopy(self.env) if env is None else env
        if ev is self.env:
            raise ValueError("evaluate() resets its env: pass a copy, not the training env")
        ev.reset(return_obs=False)
        kept = self._eval.get(id(ev)) if env is not None else None
        if kept is None or kept["env"] is not ev or kept["stats"].capacity < n_ticks:
            kept = {"env": ev, "actor": DeviceActor(ev, self.actor_net, precision=self.device_actor.precision),
                    "stats": rollout_stats_for(ev, n_ticks),
                    "rewards": torch.empty(ev.n_local, dtype=torch.float64, device=ev.shard.device), "actions": None}
            if env is not None:
                self._eval[id(ev)] = kept
        else:
            kept["actor"].load_weights()  # (the policy may have been updated since the twin's last run)
        stats = kept["stats"]
        stats.clear()
        acts = None
        if return_actions:
            acts = kept["actions"]
            if acts is None or acts.shape[0] != n_ticks:
                acts = kept["actions"] = torch.empty((n_ticks, ev.n_local), dtype=torch.uint8, device=ev.shard.device)
        # (one reward row, overwritten every tick: tick t's stats nodes read it before tick t + 1's step)
        kept["actor"].rollout(n_ticks, rewards=kept["rewards"], actions=acts, stats=stats)
        out = evaluation_means(stats.host(), stats.prev()["signal_post"], ev.n, n_ticks)
        return (out, acts) if return_actions else out

    def __len__(self) -> int:
        if self.store is not None and self.store.rows:
            return len(self.store)
        return sum(b[0].shape[0] for b in self.buffer)

    # ---------------------------------------------------------------- update
    def _returns(self, reward, done_rows, n):
        if self.returns == "reference":
            return discounted_returns(reward.reshape(-1), done_rows.reshape(-1), self.cfg.gamma)
        # each house over its own ticks: the same recurrence along the tick axis, houses in parallel
        torch = _torch()
        T = reward.shape[0]
        g = torch.empty_like(reward, dtype=torch.float64)
        nxt = torch.zeros(n, dtype=torch.float64, device=reward.device)
        for t in range(T - 1, -1, -1):
            nxt = reward[t].double() + self.cfg.gamma * (1.0 - done_rows[t].double()) * nxt
            g[t] = nxt
        return g.reshape(-1)

    # ---------------------------------------------------------------- sharded update
    def _allgather_rows(self, mine):
        """Every rank's equal-shape device tensor, [world, ...] in rank order (one byte all-gather)."""
        torch = _torch()
        env = self.env
        raw = env._comm.allgather_bytes(env.shard, mine.contiguous().view(torch.uint8).reshape(-1))
        return raw.view(mine.dtype).view(env.world, *mine.shape)

    def _same_on_all_ranks(self, value, what: str) -> None:
        """RuntimeError on every rank unless every rank holds the same 53-bit ``value`` (a device
        int64 scalar): a min- and a max-allreduce of it as a double.  Synchronises."""
        torch = _torch()
        env = self.env
        lo = value.double().reshape(1).clone()
        hi = lo.clone()
        env._comm.allreduce_min(env.shard, lo)
        env._comm.allreduce_max(env.shard, hi)
        if float(lo.item()) != float(hi.item()):
            raise RuntimeError(f"DeviceMAPPO.update: the ranks' {what} differ (checksums {int(lo.item())} .. "
                               f"{int(hi.item())}): the replicas would drift apart")

    def _minibatch_sharded(self, st, idx, cols):
        """The minibatch of global transition indices ``idx`` on every rank, bit for bit: float32
        [B, F + 4] = the obs row, action, stored probability, return and the critic's others column.
        Each rank fills the rows of the transitions it owns (``shard_owner``; the obs rows rebuilt
        from its snapshot and halo rows) into a zeroed buffer at their positions, and one
        sum-allreduce of the buffer as 32-bit integer bit patterns (x + 0 is exact, as in
        k_halo_step_pack's rows) gives every rank every row."""
        torch = _torch()
        env = self.env
        rank, loc = shard_owner(idx, env.n, env.world)
        own = rank == env.rank
        loc = torch.where(own, loc, torch.full_like(loc, -1))
        rows = torch.cat([st.states(loc), cols[loc.clamp(min=0)]], 1)  # (not owned: a NaN row, masked below)
        buf = torch.where(own[:, None], rows, torch.zeros_like(rows)).contiguous()
        env._comm.allreduce_count32(env.shard, buf.view(torch.int32))
        return buf

    def update(self, t=None) -> bool:
        """mappo.py:128-217: returns, then ppo_update_time epochs of minibatch PPO steps.  Returns
        False (and keeps the buffer) while it holds fewer than batch_size transitions.

        After ``collect`` on a sharded environment the buffer is the cluster's T x N transitions in
        the reference's order (tick-major, house-minor over global house ids): every rank draws the
        same permutation of it (the ranks share the constructor's seed; a checksum guard per epoch),
        holds every minibatch after one integer allreduce (``_minibatch_sharded``) and runs the
        identical forward, backward, clip and Adam step — no gradient is exchanged — so the ranks
        keep one set of weights (a checksum guard at the end)."""
        torch = _torch()
        F = torch.nn.functional
        L = len(self)
        if self.store is not None and self.store.rows and self.store.sharded:
            L = self.store.rows * self.env.n  # the cluster's buffer
        if L < self.cfg.batch_size:
            return False
        cfg = self.cfg
        st = self.store if self.store is not None and self.store.rows else None
        if st is not None:
            # the collected rollout: each minibatch's obs rows are rebuilt from the state snapshots
            T, n = st.rows, st.n_local
            state = None
            act = st.actions[:T].reshape(-1).long().view(-1, 1)
            old_prob = st.probs[:T].reshape(-1).float().view(-1, 1)
            acts = st.actions[:T].double()  # [T, N]
            dev = st.rewards.device
        else:
            state = torch.cat([b[0] for b in self.buffer]).float()
            act = torch.cat([b[1] for b in self.buffer]).long().view(-1, 1)
            old_prob = torch.cat([b[2] for b in self.buffer]).float().view(-1, 1)
            n = self.buffer[0][0].shape[0]
            acts = torch.stack([b[1] for b in self.buffer]).double()  # [T, N]
            dev = state.device
        n_glob = self.env.n
        tot = acts.sum(1, keepdim=True)
        sharded = st is not None and st.sharded  # one policy from the cluster's buffer (see _minibatch_sharded)
        if self.env.world > 1 or sharded:
            self.env._comm.allreduce_sum(self.env.shard, tot)
        others = ((tot - acts) / max(n_glob - 1, 1)).float().reshape(-1, 1)  # mean of the other houses' actions
        reward = st.rewards[:T] if st is not None else torch.stack([b[3] for b in self.buffer])  # [T, N]
        done = torch.tensor(st.done if st is not None else [b[4] for b in self.buffer], dtype=torch.float64,
                            device=reward.device)
        done_rows = done[:, None].expand(-1, n)
        if sharded and self.returns == "reference":
            Gt = sharded_reference_returns(reward, done, cfg.gamma, self.env.rank, self.env.world,
                                           self._allgather_rows).reshape(-1).float()
        else:
            Gt = self._returns(reward, done_rows, n).float()
        critic_in = torch.cat([state, others], 1) if st is None else None
        if sharded:  # the local columns a minibatch row carries beside its obs row
            cols = torch.cat([act.float(), old_prob, Gt.view(-1, 1), others], 1).contiguous()
        on_device = self.sampler == "device" or (self.sampler == "auto" and L > (1 << 20))
        self.last_sampler = "device" if on_device else "reference"
        for _ in range(cfg.ppo_update_time):
            # SubsetRandomSampler + BatchSampler(drop_last=False): a permutation (the global CPU
            # generator's, or the device generator's — see sampler), cut in order into batch_size chunks
            perm = torch.randperm(L, device=dev) if on_device else torch.randperm(L).to(dev)
            if sharded:
                self._same_on_all_ranks(_checksum53(perm), "minibatch permutations")
            for k in range(0, L, cfg.batch_size):
                idx = perm[k:k + cfg.batch_size]
                if sharded:
                    mb = self._minibatch_sharded(st, idx, cols)
                    nf = self.num_state
                    state_idx = mb[:, :nf].contiguous()
                    act_idx, old_idx = mb[:, nf].long().view(-1, 1), mb[:, nf + 1].reshape(-1, 1).contiguous()
                    Gt_index = mb[:, nf + 2].reshape(-1, 1).contiguous()
                    critic_idx = torch.cat([state_idx, mb[:, nf + 3:nf + 4]], 1)
                else:
                    Gt_index = Gt[idx].view(-1, 1)
                    state_idx = state[idx] if st is None else st.states(idx)
                    critic_idx = critic_in[idx] if st is None else torch.cat([state_idx, others[idx]], 1)
                    act_idx, old_idx = act[idx], old_prob[idx]
                V = self.critic_net(critic_idx)
                advantage = (Gt_index - V).detach()
                action_prob = self.actor_net(state_idx).gather(1, act_idx)
                ratio = action_prob / old_idx
                clipped_ratio = torch.clamp(ratio, 1 - cfg.clip_param, 1 + cfg.clip_param)
                action_loss = -torch.min(ratio * advantage, clipped_ratio * advantage).mean()
                self.actor_optimizer.zero_grad()
                action_loss.backward()
                torch.nn.utils.clip_grad_norm_(self.actor_net.parameters(), cfg.max_grad_norm)
                self.actor_optimizer.step()
                value_loss = F.mse_loss(Gt_index, V)
                self.critic_net_optimizer.zero_grad()
                value_loss.backward()
                torch.nn.utils.clip_grad_norm_(self.critic_net.parameters(), cfg.max_grad_norm)
                self.critic_net_optimizer.step()
                self.training_step += 1
        del self.buffer[:]
        if st is not None:
            st.clear()
        if sharded:
            bits = torch.cat([p.detach().reshape(-1).view(torch.int32) for net in (self.actor_net, self.critic_net)
                              for p in net.parameters()])
            self._same_on_all_ranks(_checksum53(bits), "actor and critic weights after the update")
        self.device_actor.load_weights()  # the fused kernel's packed weights follow the update
        return True

    def save(self, path: str, time_step=None) -> None:
        import os

        torch = _torch()
        os.makedirs(path, exist_ok=True)
        name = "actor" + (str(time_step) if time_step else "") + ".pth"
        torch.save(self.actor_net.state_dict(), os.path.join(path, name))
