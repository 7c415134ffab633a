"""``EnvBatch``: E independent small clusters resident in one context, stepped by one launch.

The reference trains and evaluates on many short episodes of a small cluster (1,000 agents in
MARLconfig.json, 50 in config C1).  One ``Environment`` of that size is a latency chain: a tick costs
the same few launches whatever the cluster size.  A batch keeps E such clusters in ONE libmdr_hip
context (mdr_batch_set) and steps a whole rollout call of all of them with ONE kernel launch
(mdr_batch_rollout, k_batch_rollout: one workgroup per cluster, the cluster power behind one block
barrier, state and parameters in registers from the first tick to the last).

Members are host-side ``Environment`` objects — reset, RNG order, population draw, date
randomisation, ``GridSignal`` and ``driver_window`` are the existing code, per member — whose shard
is a slice view of the batch's tensors (``_MemberShard``, through ``Environment``'s ``_shard_factory``
hook).  Member ``e`` draws from ``random.Random(seeds[e])`` and its random controller from Philox
key ``seeds[e]``: it reproduces ``Environment(props, rng=random.Random(seeds[e]), seed=seeds[e])``
bit for bit (tests/test_env_batch_gpu.py).

Layout: cluster ``e`` is elements ``[e * S, e * S + N_c)`` of every per-house tensor, ``S = 128 *
ceil(N_c / 128)``; the public tensors are ``[E, N_c]`` strided views of that padded storage, and the
pad elements are never read into a result, written, counted or rewarded.
"""
from __future__ import annotations

import copy
import ctypes as C
import random as _random
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from . import config as cfgmod
from . import population as popmod
from .environment import ACTION_MODES, Environment, discount_weights
from .shard import HipShard, decode_hvac

MAX_LEN = 1024  # MDR_BATCH_MAX_LEN: a cluster is stepped by one workgroup


def batch_stride(n: int) -> int:
    """Houses between two clusters' first elements: 128 * ceil(n / 128) (mdr_batch_stride)."""
    return (int(n) + 127) // 128 * 128


def check_batch_props(props, n_envs: int, population: str = "reference", comm=None) -> None:
    """The configurations a batch refuses, each with its reason; needs no device and draws nothing."""
    cp = props.cluster_prop
    n = int(cp.nb_agents)
    if int(n_envs) < 1:
        raise ValueError("EnvBatch needs n_envs >= 1")
    if n > MAX_LEN:
        raise ValueError(f"EnvBatch steps a cluster with one workgroup: nb_agents = {n} > {MAX_LEN}; larger clusters "
                         "run as stand-alone Environments")
    if comm is not None:
        raise NotImplementedError("EnvBatch lives on one GPU: a batch has no communicator")
    if population != "reference":
        raise NotImplementedError("EnvBatch draws each member's population on the host (population='reference'): the "
                                  "synthetic population is keyed by a context-wide house id")
    pmode = props.reward_prop.penalty_props.mode
    if pmode != "individual_L2":
        raise NotImplementedError(f"EnvBatch supports the individual_L2 penalty; {pmode!r} needs a cluster-wide "
                                  "penalty reduction per tick (use stand-alone Environments)")
    cmode = cp.agents_comm_prop.mode
    if cmode == "random_sample":
        raise NotImplementedError("EnvBatch: the random_sample comm mode draws from the RNG every tick, so no "
                                  "driver window can run ahead of the device")
    if cmode != "neighbours":
        raise NotImplementedError(f"EnvBatch observations support the 'neighbours' (ring) comm mode; {cmode!r} "
                                  "needs a neighbour table per cluster")
    if props.power_grid_prop.base_power_props.mode == "interpolation":
        raise NotImplementedError("EnvBatch: the interpolation base power reads the house state in the middle of a "
                                  "driver window (its grid step), which a one-launch rollout cannot serve")


class _MemberShard:
    """What a member ``Environment`` asks of its shard, served from cluster ``e``'s slice of the
    batch's tensors.  It owns no context: every launch is the batch's."""

    penalty_mode = 0

    def __init__(self, batch: "EnvBatch", e: int, cap_values):
        if list(cap_values) != list(batch._cap_values):
            raise ValueError("a batch member's capacity table differs from the batch's")
        st = batch._store
        self.device = st.device
        self.n, self.offset, self.n_global = batch.n, 0, batch.n
        lo = e * batch.stride
        for k in ("t_air", "t_mass", "hvac", "ua", "ca", "cm", "hm", "target", "cap_idx"):
            setattr(self, k, getattr(st, k)[lo:lo + batch.n])
        self._batch, self._e = batch, e

    def upload(self, pop: dict, cap_idx, t_air, t_mass, hvac_words):
        import torch

        dev = self.device
        for name in ("ua", "ca", "cm", "hm", "target"):
            getattr(self, name).copy_(torch.from_numpy(np.ascontiguousarray(pop[name], np.float64)).to(dev))
        self.cap_idx.copy_(torch.from_numpy(np.ascontiguousarray(cap_idx, np.uint8)).to(dev))
        self.t_air.copy_(torch.from_numpy(np.ascontiguousarray(t_air, np.float64)).to(dev))
        self.t_mass.copy_(torch.from_numpy(np.ascontiguousarray(t_mass, np.float64)).to(dev))
        self.hvac.copy_(torch.from_numpy(np.ascontiguousarray(hvac_words, np.int32)).to(dev))
        self._batch._store.params_changed()

    def populate(self, hp, cap_values):
        raise NotImplementedError("a batch member's population is drawn on the host")

    def close(self):
        pass

    def host_state(self):
        import torch

        torch.cuda.current_stream(self.device).synchronize()
        on, lock, sso = decode_hvac(self.hvac.cpu().numpy())
        return {"T": self.t_air.cpu().numpy(), "Tm": self.t_mass.cpu().numpy(), "on": on, "lock": lock, "sso": sso}

    def host_params(self):
        return {k: getattr(self, k).cpu().numpy() for k in ("ua", "ca", "cm", "hm", "target", "cap_idx")}


class EnvBatch:
    """``n_envs`` independent clusters of ``env_props.cluster_prop.nb_agents`` (<= 1,024) houses each,
    same ``env_props``, own seed / population / start date / outdoor-temperature noise / regulation
    signal per cluster.  ``seeds``: one int per cluster (default ``range(n_envs)``)."""

    def __init__(self, env_props, n_envs: int, seeds: Optional[Sequence[int]] = None, device=None,
                 population: str = "reference", comm=None):
        props = copy.deepcopy(env_props)
        cfgmod.validate(props)
        check_batch_props(props, n_envs, population, comm)
        n_envs = int(n_envs)
        seeds = list(range(n_envs)) if seeds is None else [int(s) for s in seeds]
        if len(seeds) != n_envs:
            raise ValueError(f"{len(seeds)} seeds for {n_envs} clusters")
        import torch

        self.init_props = props
        self.n_envs = n_envs
        self.n = int(props.cluster_prop.nb_agents)
        self.stride = batch_stride(self.n)
        self.seeds = seeds
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cuda"
        # every member's capacity table is the configuration's own (population.cap_table: the noise list, then
        # the nominal capacity; a drawn capacity is an entry of the list), so the union is that table
        self._cap_values, _ = popmod.cap_table(props.cluster_prop.house_prop.hvac_prop, ())
        total = n_envs * self.stride
        self._store = HipShard(props, total, 0, total, device, self._cap_values, seed=0)
        st = self._store
        self.device = st.device
        for k in ("ua", "ca", "cm", "hm", "target", "t_air", "t_mass"):  # pads: finite, never used
            getattr(st, k).fill_(1.0)
        st.hvac.zero_()
        st.cap_idx.zero_()
        arr = (C.c_uint64 * n_envs)(*[s & 0xFFFFFFFFFFFFFFFF for s in seeds])
        L.check(st.lib.mdr_batch_set(st.ctx, n_envs, self.n, arr), "mdr_batch_set")
        self._p_dev = torch.zeros(n_envs, dtype=torch.float64, device=self.device)
        self.members = [Environment(props, device=self.device, rng=_random.Random(seeds[e]), population="reference",
                                    seed=seeds[e], _shard_factory=self._member_factory(e)) for e in range(n_envs)]
        self._sync_power(range(n_envs))

    def _member_factory(self, e: int):
        def factory(props, n_local, offset, n_global, dev, cap_values, seed=0):
            return _MemberShard(self, e, cap_values)
        return factory

    def _sync_power(self, ids):
        """A freshly reset member's cluster power is its host value (Cluster.reset) until a step writes it."""
        for e in ids:
            self._p_dev[e] = float(self.members[e]._P_host)

    # ------------------------------------------------------------------ tensors
    def _view(self, flat):
        """[.., E * S] padded storage -> its [.., E, N_c] view."""
        lead = flat.shape[:-1]
        return flat.view(*lead, self.n_envs, self.stride)[..., :self.n]

    @property
    def t_air(self):
        return self._view(self._store.t_air)

    @property
    def t_mass(self):
        return self._view(self._store.t_mass)

    @property
    def hvac(self):
        return self._view(self._store.hvac)

    def padded(self, view):
        """The ``[.., E, S]`` padded storage behind one of the batch's ``[.., E, N_c]`` views (state,
        ``empty_rewards``, ``empty_actions``): the houses and the pad elements between clusters."""
        import torch

        self._check_view(view, view.shape[0] if view.dim() == 3 else None, view.dtype, "padded")
        return torch.as_strided(view, tuple(view.shape[:-1]) + (self.stride,), view.stride(), view.storage_offset())

    def empty_rewards(self, n_ticks: Optional[int] = None):
        """float64 reward rows for ``rollout``: ``[n_ticks, E, N_c]``, or ``[E, N_c]`` (``None``: one row
        that every tick overwrites, so it keeps the last tick's).  A view of padded storage."""
        import torch

        lead = () if n_ticks is None else (int(n_ticks),)
        return self._view(torch.empty(lead + (self.n_envs * self.stride,), dtype=torch.float64, device=self.device))

    def empty_actions(self, n_ticks: Optional[int] = None):
        """uint8 action rows for ``action_mode='buffer'`` (non-zero = turn on): ``[n_ticks, E, N_c]``, or
        ``[E, N_c]`` for ``step_tensor``.  A view of padded storage, zero-filled."""
        import torch

        lead = () if n_ticks is None else (int(n_ticks),)
        return self._view(torch.zeros(lead + (self.n_envs * self.stride,), dtype=torch.uint8, device=self.device))

    def _check_view(self, t, n_ticks, dtype, what):
        import torch

        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device:
            raise ValueError(f"{what} must be a {dtype} tensor on {self.device} from EnvBatch.empty_{what}()")
        shape = (self.n_envs, self.n) if n_ticks is None else (n_ticks, self.n_envs, self.n)
        stride = (self.stride, 1) if n_ticks is None else (self.n_envs * self.stride, self.stride, 1)
        ok = tuple(t.shape) == shape and all(t.shape[i] == 1 or t.stride(i) == stride[i] for i in range(len(shape)))
        if not ok or t.data_ptr() % 16:
            raise ValueError(f"{what} must come from EnvBatch.empty_{what}() (shape {shape} over the padded cluster "
                             f"stride {self.stride}); got shape {tuple(t.shape)}, strides {tuple(t.stride())}")

    # ------------------------------------------------------------------ episodes
    def reset(self, env_ids: Optional[Sequence[int]] = None):
        """Re-draw every member (``None``) or the given ones — population, start date, drivers, tick
        counter, each from its own RNG as ``Environment.reset`` — and leave the others' state, drivers
        and ticks alone: episodes end independently."""
        ids = range(self.n_envs) if env_ids is None else [int(e) for e in env_ids]
        for e in ids:
            if not 0 <= e < self.n_envs:
                raise ValueError(f"env id {e} outside [0, {self.n_envs})")
        for e in ids:
            self.members[e].reset(return_obs=False)
        self._sync_power(ids)

    # ------------------------------------------------------------------ stepping
    def empty_returns(self):
        """Zero-filled float64 ``[E, N_c]`` returns for ``rollout_returns``.  A view of padded storage."""
        import torch

        return self._view(torch.zeros(self.n_envs * self.stride, dtype=torch.float64, device=self.device))

    def _check_source(self, n_ticks, action_mode: str, actions):
        """(n_ticks, mode, act_stride) of a rollout call's tick count and action source, checked."""
        import torch

        if int(n_ticks) != n_ticks or n_ticks < 1:
            raise ValueError("rollout needs n_ticks >= 1")
        n_ticks = int(n_ticks)
        if action_mode not in ACTION_MODES:
            raise ValueError(f"unknown action_mode {action_mode!r}")
        mode = ACTION_MODES[action_mode]
        act_stride = 0
        if mode == L.ACT_BUFFER:
            if actions is None:
                raise ValueError("action_mode='buffer' needs an actions tensor from empty_actions()")
            if actions.dim() == 2 and n_ticks == 1:
                self._check_view(actions, None, torch.uint8, "actions")
            else:
                self._check_view(actions, n_ticks, torch.uint8, "actions")
                act_stride = self.n_envs * self.stride
        elif actions is not None:
            raise ValueError(f"action_mode={action_mode!r} takes no actions tensor")
        return n_ticks, mode, act_stride

    def _check_stats(self, stats, n_ticks: int) -> int:
        """The first of the call's rows in ``stats`` (services.BatchRolloutStats), after checking that
        they are this batch's and that ``n_ticks`` more fit; nothing is appended."""
        if stats is None:
            return 0
        if getattr(stats, "batch", None) is not self:
            raise ValueError("the stats rows belong to another batch (services.BatchRolloutStats(batch, capacity))")
        return stats.begin_rows(n_ticks)  # (ValueError: overflow)

    def rollout(self, n_ticks: int, action_mode: str = "random", actions=None, rewards=None, stats=None):
        """``n_ticks`` steps of every cluster in one launch.  Returns the float64 rewards ``[n_ticks, E,
        N_c]`` (``rewards`` from ``empty_rewards(n_ticks)``, allocated if None); with a buffer from
        ``empty_rewards(None)`` the last tick's ``[E, N_c]``.  ``action_mode='buffer'``: ``actions`` from
        ``empty_actions(n_ticks)``.  Per cluster bit for bit the stand-alone ``step_tensor(None,
        action_mode=c, lookahead=c)`` loop.  ``stats`` (``services.BatchRolloutStats`` of this batch): the
        same launch also writes every cluster's ``mdr_tick_stats`` row of every tick (k_batch_eval).
        Every argument, the stats capacity included, is checked before any member's drivers advance.
        The host side is one ``driver_window`` call per member."""
        import torch

        n_ticks, mode, act_stride = self._check_source(n_ticks, action_mode, actions)
        srow0 = self._check_stats(stats, n_ticks)
        if rewards is None:
            rewards = self.empty_rewards(n_ticks)
        if rewards.dim() == 2:
            self._check_view(rewards, None, torch.float64, "rewards")
            rew_stride = 0
        else:
            self._check_view(rewards, n_ticks, torch.float64, "rewards")
            rew_stride = self.n_envs * self.stride
        ticks = self._driver_windows(n_ticks)
        self._launch(ticks, actions, act_stride, mode, rewards, rew_stride, stats=stats, srow0=srow0)
        return rewards

    def rollout_returns(self, n_ticks: int, returns, gamma: float = 1.0, weight0=1.0, actions=None,
                        action_mode: str = "random", stats=None):
        """``rollout`` that writes no reward row: every house's weighted rewards of the call's ticks are
        added to ``returns`` (from ``empty_returns()``, on top of its contents) in a register of the one
        launch,

            returns[e, i] += w[e][0] r_i(0) + w[e][1] r_i(1) + ...,   w[e] = discount_weights(weight0[e], gamma, n_ticks)

        the sum running left to right, one multiply and one add per tick: the bits of ``ret = ret +
        w[e][t] * rows[t]`` over ``rollout``'s rows, for every source.  ``weight0``: a scalar, or one value
        per cluster (members reset independently and sit at different points of their episodes).
        Returns the float64 ``[E]`` array of ``w[e][n_ticks]``, the ``weight0`` of the next call of a chain.
        State, FSM words, cluster power, ticks and dates advance exactly as under ``rollout``; ``stats``
        as there.  ``ValueError``: ``returns`` not from ``empty_returns()``, ``gamma`` outside (0, 1], a
        non-finite ``weight0`` or one of another length, ``n_ticks < 1``, stats rows of another batch or
        too few left — all before any member's drivers advance."""
        import torch

        n_ticks, mode, act_stride = self._check_source(n_ticks, action_mode, actions)
        if not (isinstance(gamma, (int, float)) and 0.0 < gamma <= 1.0):
            raise ValueError(f"gamma = {gamma!r} outside (0, 1]")
        w0 = np.asarray(weight0, np.float64)
        if w0.ndim == 0:
            w0 = np.full(self.n_envs, float(w0))
        if w0.shape != (self.n_envs,):
            raise ValueError(f"weight0: a scalar or one value per cluster ({self.n_envs}), not shape {w0.shape}")
        if not np.all(np.isfinite(w0)):
            raise ValueError(f"weight0 = {weight0!r} is not finite")
        self._check_view(returns, None, torch.float64, "returns")
        srow0 = self._check_stats(stats, n_ticks)
        w = np.stack([discount_weights(float(w0[e]), float(gamma), n_ticks) for e in range(self.n_envs)])
        ticks = self._driver_windows(n_ticks)
        self._launch(ticks, actions, act_stride, mode, None, 0, weights=np.ascontiguousarray(w[:, :n_ticks]),
                     returns=returns, stats=stats, srow0=srow0)
        return w[:, n_ticks].copy()

    def _driver_windows(self, n_ticks: int) -> np.ndarray:
        """Every member's host drivers ``n_ticks`` ahead (``Environment.driver_window``, one call per member)
        as one mdr_tick array [E, n_ticks, 4]."""
        ticks = np.empty((self.n_envs, n_ticks, 4), np.float64)
        for e, m in enumerate(self.members):
            w = m.driver_window(n_ticks)
            if len(w) != n_ticks:
                raise RuntimeError("a member's driver window ended early")
            ticks[e] = w.a
        return ticks

    def _launch(self, ticks: np.ndarray, actions, act_stride: int, mode: int, rewards, rew_stride: int,
                weights=None, returns=None, stats=None, srow0: int = 0) -> None:
        """mdr_batch_rollout of staged driver windows: the one launch of a rollout call
        (mdr_batch_rollout_eval when it also writes ``stats`` rows, or ``returns`` under the host
        ``weights`` [E, n_ticks] instead of reward rows)."""
        st = self._store
        if weights is None and stats is None:
            L.check(st.lib.mdr_batch_rollout(st.ctx, ticks.shape[1], ticks.ctypes.data, L.ptr(actions), act_stride, mode,
                                             L.ptr(rewards), rew_stride, L.ptr(self._p_dev), st.stream()),
                    "mdr_batch_rollout")
        else:
            if stats is not None:
                stats.record_power(srow0)  # (the pre-step P of the call's first tick, before the launch overwrites it)
            L.check(st.lib.mdr_batch_rollout_eval(
                st.ctx, ticks.shape[1], ticks.ctypes.data, L.ptr(actions), act_stride, mode, L.ptr(rewards), rew_stride,
                None if weights is None else weights.ctypes.data, L.ptr(returns),
                None if stats is None else L.ptr(stats.stats), 0 if stats is None else stats.capacity, srow0,
                L.ptr(self._p_dev), st.stream()), "mdr_batch_rollout_eval")
            if stats is not None:  # tick t's post-step signal is tick t + 1's s_prev; the last one's is the grid's
                stats.commit_rows(ticks, [float(m.power_grid.current_signal) for m in self.members])
        self._ticks_kept = ticks, weights  # (the host records outlive the call, whatever the copy's staging does)
        for m in self.members:
            m._P_dev_valid = False  # (the members' own p_dev is not written: the batch's [E] vector is)
            m._counts_ready = 0

    def step_tensor(self, actions=None, action_mode: str = "buffer", rewards=None):
        """One tick of every cluster: ``rollout(1, ...)`` into an ``[E, N_c]`` row (``rewards`` from
        ``empty_rewards(None)``, allocated if None; ``actions`` from ``empty_actions(None)``)."""
        if rewards is None:
            rewards = self.empty_rewards(None)
        return self.rollout(1, action_mode=action_mode, actions=actions, rewards=rewards)

    def cluster_power(self):
        """float64 ``[E]`` on device: every cluster's power of its last tick (after a reset: the
        member's ``Cluster.reset`` value)."""
        return self._p_dev

    # ------------------------------------------------------------------ observations
    def obs_tensor(self, out=None):
        """``norm_state_dict`` of every house as float32 ``[E, N_c, F]`` on device (k_batch_obs); the
        ring messages wrap inside each cluster, the uniform features are each cluster's own."""
        import torch

        spec = self.members[0].obs_spec()
        if spec.comm_mode != L.COMM_RING:
            raise NotImplementedError("EnvBatch observations support the 'neighbours' (ring) comm mode")
        shape = (self.n_envs, self.n, spec.n_feat)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on {self.device}")
        sc = np.empty((self.n_envs, 4), np.float64)
        for e, m in enumerate(self.members):
            sc[e] = (float(m._P_host), float(m.power_grid.current_signal), float(m._solar), float(m.current_od_temp))
        st = self._store
        L.check(st.lib.mdr_batch_obs(st.ctx, C.byref(spec), sc.ctypes.data, L.ptr(self._p_dev), L.ptr(out),
                                     st.stream()), "mdr_batch_obs")
        self._sc_kept = sc
        return out

    def close(self):
        self._store.close()
