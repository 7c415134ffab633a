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

Limits: one shard (a neighbour's snapshot would live on another shard) and fixed links (the
``random_sample`` comm mode re-draws them every tick).  ``Environment.reset()`` re-draws targets,
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
        self.rows = 0
        self.done = []  # host: per stored tick
        self._epoch = None
        self._spec = None
        self._table = None

    # ---------------------------------------------------------------- validity
    def _check_supported(self):
        env = self.env
        if env.world > 1:
            raise ValueError("RolloutStore: sharded environments are not supported (a neighbour's "
                             "snapshot lives on another shard)")
        if env._links is None:
            raise ValueError("RolloutStore: the random_sample comm mode re-draws its links every tick; "
                             "a state snapshot cannot reproduce its observations")

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
            sh.obs_gather(self._spec, self.snap, self.rows, idx, out)
        return out
