"""Compact transition storage for MA-PPO training from the fused rollout.

Reference: TrainingManager.start stores ``norm_state_dict`` of every agent every tick
(server/app/services/training_manager.py:224-240 -> MAPPO.store_transition,
server/app/core/agents/trainables/mappo.py:105-126): n_feat float32 per house-tick.

An observation row is a function of the house's and its neighbours' ``t_air`` / ``t_mass`` / hvac
word, the tick's four obs scalars, and parameters that stay fixed between resets.  ``RolloutStore``
keeps the first (8 + 8 + 4 B per house-tick) and second (one row per tick), written by ``k_snap``
inside the graph-captured rollout (``DeviceActor.rollout(store=...)``) or per tick
(``Environment.snapshot``); ``states(idx)`` rebuilds any minibatch's rows with ``k_obs_gather``, which
assembles them with the device functions ``k_obs`` and ``k_actor`` use, so they are bit-identical to
``obs_tensor()`` of their tick.  With the action, its probability and the reward a stored
transition is 33 B.

A house-sharded environment: with the ``neighbours`` ring a shard's rows read at most ``lo = K // 2``
houses before the shard and ``hi = (K + 1) // 2`` after it, and only their message features — the ring
halo the sharded actor reads every tick.  ``RolloutStore`` keeps that row beside the snapshot
(``k_snap_halo``: ``halo_bytes_per_tick`` <= 440 B), so ``states(idx)`` of local indices rebuilds every
local row on its own rank (``k_obs_gather_halo``), bit-identical to the single-process rows.

Limits: fixed links (the ``random_sample`` comm mode re-draws them every tick); on a sharded
environment the ``neighbours`` ring only (a table mode's neighbours live anywhere in the cluster)
and shards no smaller than the ring half-width; ``ReplayStore`` (DQN) is single-shard (its next
state is the ring-next slot's row, whose halo a trailing snapshot does not have).
``Environment.reset()`` re-draws targets,
parameters and links, so rows stored before it can no longer be rebuilt: a non-empty store then
refuses appends and gathers until ``clear()``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


class RolloutStore:
    """Fixed-capacity device storage of ``capacity_ticks`` ticks of transitions of ``env``'s houses.
    The tensors never move, so rollout graphs captured with their pointers are reused."""

    nbytes_per_house_tick = 8 + 8 + 4 + 1 + 4 + 8  # t_air, t_mass, hvac, action, prob, reward

    def __init__(self, env, capacity_ticks: int):
        import torch

        if capacity_ticks < 1:
            raise ValueError("capacity_ticks must be at least 1")
        self.env = env
        # a shard of a larger cluster, or a context with the library's own communicator (world 1
        # included): the sharded entry points and a ring-halo row per tick
        self.sharded = env.world > 1 or bool(getattr(env._comm, "native", False))
        self._check_supported()
        sh = env.shard
        dev = sh.device
        cap, n = int(capacity_ticks), env.n_local
        self.capacity, self.n_local = cap, n
        self.t_air = torch.empty((cap, n), dtype=torch.float64, device=dev)
        self.t_mass = torch.empty((cap, n), dtype=torch.float64, device=dev)
        self.hvac = torch.empty((cap, n), dtype=torch.int32, device=dev)
        self.scalars = torch.empty((cap, 4), dtype=torch.float64, device=dev)
        self.actions = torch.empty((cap, n), dtype=torch.uint8, device=dev)
        self.probs = torch.empty((cap, n), dtype=torch.float32, device=dev)
        self.rewards = torch.empty((cap, n), dtype=torch.float64, device=dev)
        self.snap = L.mdr_snap(C.sizeof(L.mdr_snap), cap, n, L.ptr(self.t_air), L.ptr(self.t_mass),
                               L.ptr(self.hvac), L.ptr(self.scalars))
        self.halo_rows, self.halo, self.halo_bytes_per_tick = None, None, 0
        if self.sharded:
            spec = env.obs_spec()
            w = spec.n_comm * sh.lib.mdr_msg_width(C.byref(spec))  # (lo + hi) rows of msg_w floats
            if w:
                self.halo_rows = torch.zeros((cap, w), dtype=torch.float32, device=dev)
                self.halo = L.mdr_snap_halo(C.sizeof(L.mdr_snap_halo), cap, w, L.ptr(self.halo_rows))
                self.halo_bytes_per_tick = 4 * w
        self.rows = 0
        self.done = []  # host: per stored tick
        self._epoch = None
        self._spec = None
        self._table = None

    # ---------------------------------------------------------------- validity
    def _check_supported(self):
        env = self.env
        if env._links is None:
            raise ValueError("RolloutStore: the random_sample comm mode re-draws its links every tick; "
                             "a state snapshot cannot reproduce its observations")
        if self.sharded:
            mode = env.init_props.cluster_prop.agents_comm_prop.mode
            spec = env.obs_spec()
            if spec.comm_mode != L.COMM_RING and spec.n_comm > 0:
                raise ValueError(f"RolloutStore: on a sharded environment only the 'neighbours' ring is supported, "
                                 f"not the {mode!r} comm mode (its neighbours live anywhere in the cluster)")
            if env.n_local < (spec.n_comm + 1) // 2:
                raise ValueError("RolloutStore: a shard smaller than the ring half-width")

    def _bind(self):
        """Remember the env's population epoch and links table (an empty store follows a reset)."""
        import torch

        env = self.env
        self._check_supported()
        if env.n_local != self.n_local:
            raise ValueError("RolloutStore: the environment's house count changed")
        spec = env.obs_spec()
        self._table = None
        if spec.comm_mode == L.COMM_TABLE and spec.n_comm > 0:
            links = np.ascontiguousarray(np.asarray(env._obs_links, np.int32))
            self._table = torch.from_numpy(links).to(env.shard.device)
            spec.comm_table = L.ptr(self._table)
        self._spec = spec
        self._epoch = env._pop_epoch

    def _check_epoch(self, what: str):
        if self.rows == 0:
            if self._epoch != self.env._pop_epoch:
                self._bind()
        elif self._epoch != self.env._pop_epoch:
            raise ValueError(f"RolloutStore: cannot {what}: the environment was reset since the stored rows "
                             "were taken (targets, parameters and links were re-drawn); clear() the store")

    # ---------------------------------------------------------------- rows
    def begin_rows(self, k: int) -> int:
        """The first of the next ``k`` rows, after checking that they fit and that the stored rows are
        still of the env's population; nothing is appended until ``commit_rows``."""
        self._check_epoch("append rows")
        if self.rows + k > self.capacity:
            raise ValueError(f"RolloutStore: {self.rows} + {k} ticks overflow the capacity of {self.capacity}")
        return self.rows

    def commit_rows(self, k: int) -> None:
        self.rows += k
        self.done.extend([False] * k)

    def clear(self) -> None:
        self.rows = 0
        del self.done[:]

    def __len__(self) -> int:
        return self.rows * self.n_local

    # ---------------------------------------------------------------- gather
    def states(self, idx):
        """float32 [len(idx), n_feat]: the obs rows of transitions ``idx`` (tick * n_local + house,
        the buffer's tick-major order), rebuilt from the snapshot rows.  An index outside the stored
        rows gives a NaN row."""
        import torch

        self._check_epoch("gather states")
        sh = self.env.shard
        idx = torch.as_tensor(idx, device=sh.device).to(torch.int64).reshape(-1).contiguous()
        out = torch.empty((idx.numel(), self._spec.n_feat), dtype=torch.float32, device=sh.device)
        if idx.numel():
            if self.sharded:  # local indices; the ring sources outside the shard from the halo rows
                sh.obs_gather_sharded(self._spec, self.snap, self.halo, self.rows, idx, out)
            else:
                sh.obs_gather(self._spec, self.snap, self.rows, idx, out)
        return out


class TickRing:
    """Slot arithmetic of ``ReplayStore``: a ring of ``capacity + 1`` tick slots, no device state.

    Slot s holds one tick's pre-step snapshot, actions and rewards; the slot after the newest tick
    (``head``) holds the trailing snapshot of the post-step state, which is the newest tick's next
    state — and, being written over the slot of the oldest tick once the ring is full, what drops
    that tick, like ``deque(maxlen)`` (buffer.py:14-33).  So at most ``capacity`` ticks are valid."""

    def __init__(self, capacity: int):
        if capacity < 1:
            raise ValueError("capacity_ticks must be at least 1")
        self.capacity = int(capacity)
        self.slots = self.capacity + 1
        self.head = 0   # the slot the next tick is written to (now: the trailing snapshot's)
        self.count = 0  # valid ticks

    def clear(self) -> None:
        self.head = self.count = 0

    def segments(self, k: int):
        """The runs of consecutive slots the next ``k`` ticks take: [(slot0, ticks)], one run, or two
        when they cross the ring's end."""
        if not 1 <= k <= self.capacity:
            raise ValueError(f"a collect takes 1 to {self.capacity} ticks (the ring's capacity), not {k}")
        first = min(k, self.slots - self.head)
        return [(self.head, first)] + ([(0, k - first)] if k > first else [])

    def commit(self, k: int) -> None:
        self.head = (self.head + k) % self.slots
        self.count = min(self.count + k, self.capacity)

    @property
    def oldest(self) -> int:
        return (self.head - self.count) % self.slots

    def valid_slots(self):
        """The slots of the valid ticks, oldest first."""
        return [(self.oldest + j) % self.slots for j in range(self.count)]

    def next_slot(self, s: int) -> int:
        return (s + 1) % self.slots


class ReplayStore:
    """Device replay memory of (s, a, r, s') for DQN from the fused rollout: ``RolloutStore``'s state
    snapshots in a ring (``TickRing``) of ``capacity_ticks + 1`` tick slots, no ``probs`` slab.  The
    next state of a transition is the same house's row in the ring-next slot, so a stored transition
    is 8 + 8 + 4 (snapshot) + 1 (action) + 8 (reward) = 29 B, against the reference's two float32
    state rows (buffer.py:14-33, dqn.py:107-123).

    Transitions are addressed by a logical index, oldest first: ``tick_rank * n_local + house`` with
    tick_rank 0 the oldest valid tick — the order of the reference's deque.  The same limits as
    ``RolloutStore`` (one shard, fixed links, refusal after ``reset()`` until ``clear()``); and the env
    may only be stepped by ``collect`` while the store holds ticks (the trailing snapshot is the next
    collect's first state)."""

    nbytes_per_house_tick = 8 + 8 + 4 + 1 + 8  # t_air, t_mass, hvac, action, reward

    def __init__(self, env, capacity_ticks: int):
        import torch

        self.ring = TickRing(capacity_ticks)
        self.env = env
        self._check_supported()
        dev = env.shard.device
        S, n = self.ring.slots, env.n_local
        self.capacity, self.n_local = self.ring.capacity, n
        self.t_air = torch.empty((S, n), dtype=torch.float64, device=dev)
        self.t_mass = torch.empty((S, n), dtype=torch.float64, device=dev)
        self.hvac = torch.empty((S, n), dtype=torch.int32, device=dev)
        self.scalars = torch.empty((S, 4), dtype=torch.float64, device=dev)
        self.actions = torch.empty((S, n), dtype=torch.uint8, device=dev)
        self.rewards = torch.empty((S, n), dtype=torch.float64, device=dev)
        self.probs = None  # (DeviceActor.rollout's store protocol: no probability rows)
        self.snap = L.mdr_snap(C.sizeof(L.mdr_snap), S, n, L.ptr(self.t_air), L.ptr(self.t_mass),
                               L.ptr(self.hvac), L.ptr(self.scalars))
        self._epoch = None
        self._spec = None
        self._table = None
        self._tick = None  # the env tick the trailing snapshot was taken at
        self._collecting = False

    # ---------------------------------------------------------------- validity (RolloutStore's rules)
    @property
    def rows(self) -> int:
        return self.ring.count

    sharded = False  # (RolloutStore's attribute: this store never takes the sharded entry points)

    def _check_supported(self):
        env = self.env
        if env.world > 1:
            raise ValueError("ReplayStore: sharded environments are not supported (a transition's next state "
                             "is the ring-next slot's row, and a neighbour's snapshot lives on another shard)")
        if env._links is None:
            raise ValueError("ReplayStore: the random_sample comm mode re-draws its links every tick; "
                             "a state snapshot cannot reproduce its observations")

    _bind = RolloutStore._bind
    _check_epoch = RolloutStore._check_epoch

    def clear(self) -> None:
        self.ring.clear()
        self._tick = None

    def __len__(self) -> int:
        return self.ring.count * self.n_local

    # ---------------------------------------------------------------- DeviceActor.rollout's store protocol
    def begin_rows(self, k: int) -> int:
        """The first of the next ``k`` slots, which must be consecutive (``collect`` splits a run that
        crosses the ring's end)."""
        self._check_epoch("append rows")
        if not self._collecting:
            raise ValueError("ReplayStore: rollouts fill it through collect() (ring segments, trailing snapshot)")
        if self.ring.head + k > self.ring.slots:
            raise ValueError("ReplayStore: rows of one rollout call must not cross the ring's end")
        return self.ring.head

    def commit_rows(self, k: int) -> None:
        self.ring.commit(k)

    # ---------------------------------------------------------------- collect
    def collect(self, device_actor, n_ticks: int, use_graph: bool = True):
        """``n_ticks`` of ``device_actor.rollout`` into the ring — two rollout calls when they cross
        its end, so that the rows of one call are consecutive — then the trailing snapshot of the
        post-step state (``mdr_snapshot``) into the slot after the newest tick."""
        if device_actor.env is not self.env:
            raise ValueError("the store belongs to another environment")
        self._check_epoch("append rows")
        if self.ring.count and self._tick != self.env._tick:
            raise ValueError("ReplayStore: the environment was stepped outside collect() since the trailing "
                             "snapshot was taken (it is the newest tick's next state); clear() the store")
        segs = self.ring.segments(n_ticks)
        self._collecting = True
        try:
            for _slot0, k in segs:
                device_actor.rollout(k, store=self, use_graph=use_graph)
        except Exception:
            self.clear()  # (a partial run has no trailing snapshot: nothing of it is kept)
            raise
        finally:
            self._collecting = False
        self._trailing_snapshot()

    def _trailing_snapshot(self) -> None:
        env = self.env
        sc = L.mdr_obs_scalars(float(env._P_host), float(env.power_grid.current_signal),
                               float(env._solar), float(env.current_od_temp))
        env.shard.snapshot(self.snap, self.ring.head, sc, use_p_dev=env._P_dev_valid)
        self._tick = env._tick

    # ---------------------------------------------------------------- sampling and gathers
    def sample_indices(self, batch: int, sampler: str = "reference"):
        """``batch`` logical transition indices drawn with replacement from the valid transitions:
        "reference" — ``random.choices(range(len), k=batch)`` of the global Python RNG, the draws of
        ReplayBuffer.sample (buffer.py:28-30) on a deque of the same length; "device" —
        ``torch.randint`` on the GPU.  Device int64."""
        import random

        import torch

        n = len(self)
        if n == 0:
            raise ValueError("ReplayStore: empty")
        dev = self.env.shard.device
        if sampler == "reference":
            return torch.tensor(random.choices(range(n), k=batch), dtype=torch.int64, device=dev)
        if sampler == "device":
            return torch.randint(n, (batch,), dtype=torch.int64, device=dev)
        raise ValueError("sampler must be 'reference' or 'device'")

    def _physical(self, idx, shift: int = 0):
        """slot * n_local + house of logical indices (``shift`` = 1: the ring-next slot, the next
        state's); an index outside the valid transitions maps to -1 (a NaN row, like RolloutStore)."""
        import torch

        dev = self.env.shard.device
        idx = torch.as_tensor(idx, device=dev).to(torch.int64).reshape(-1)
        n, S = self.n_local, self.ring.slots
        slot = (torch.div(idx, n, rounding_mode="floor") + (self.ring.oldest + shift)) % S
        phys = slot * n + idx % n
        return torch.where((idx >= 0) & (idx < len(self)), phys, torch.full_like(phys, -1)).contiguous()

    def _gather(self, phys):
        import torch

        self._check_epoch("gather states")
        sh = self.env.shard
        out = torch.empty((phys.numel(), self._spec.n_feat), dtype=torch.float32, device=sh.device)
        if phys.numel():
            sh.obs_gather(self._spec, self.snap, self.ring.slots, phys, out)
        return out

    def states(self, idx):
        """float32 [len(idx), n_feat]: the obs rows of the transitions' states (one k_obs_gather)."""
        return self._gather(self._physical(idx))

    def next_states(self, idx):
        """... of their next states: the same house in the ring-next slot (one k_obs_gather)."""
        return self._gather(self._physical(idx, 1))

    def actions_at(self, idx):
        """int64 [len(idx)]: the transitions' actions."""
        return self.actions.reshape(-1)[self._physical(idx)].long()

    def rewards_at(self, idx):
        """float64 [len(idx)]: the transitions' rewards."""
        return self.rewards.reshape(-1)[self._physical(idx)]
