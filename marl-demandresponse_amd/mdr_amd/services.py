"""The server's per-tick consumers of the environment, served from device reductions
(SURVEY §8(f) row 1).

The reference's services walk the N per-house observation dicts in Python every tick
(``Metrics.update`` loops over houses, ``ClientManagerService.update_data`` builds a pandas frame of
all of them).  Here every per-house quantity they need comes from ONE fused device reduction over
the state (``mdr_cluster_stats``, 12 sums/counts), so a tick costs O(1) host work at any N; the
per-house UI list is materialised only when read.

  DeviceMetrics  Metrics               server/app/services/metrics_service.py:71-257
  RolloutStats   (the obs dicts Metrics.update and TrainingManager.test read, as one device row per
                 tick written inside a rollout: ``mdr_tick_stats``)  training_manager.py:242-245,265-295
  ShardedRolloutStats  the same rows on a house-sharded env: the ranks' partial rows of a call, combined by one
                 exact exchange behind it (``rollout_stats_for(env, cap)`` picks the class)
  BatchRolloutStats  the same rows for every cluster of an ``EnvBatch``, written by the batch's one launch
  evaluate_batch  ``evaluate_controller`` + ``controller_returns`` for every cluster of a batch, one launch
  UISummary      ClientManagerService  server/app/services/client_manager_service.py:12-245
  ServerLoop     ControllerManager     server/app/services/controller_manager.py:93-260
  evaluate_controller  TrainingManager.test for the bang-bang and greedy-myopic baselines
                                                                 training_manager.py:265-295

Floating-point sums over houses are reduced in a fixed blocked order on the device, where the
reference adds house by house; they agree to rounding (tests/test_services_gpu.py: rtol 1e-12).
Reference quirks are kept: Metrics' ``indoor_temp - target_temp / nb_agents`` precedence, its
``cumul_squared_error_sig`` of the signal itself, ``cumul_squared_max_error_temp`` assigned (not
accumulated), the UI "Mass temperature" / "Target temperature" of house 0 only.
"""
from __future__ import annotations

from collections.abc import Sequence
from math import nan

import numpy as np

DESCRIPTION_KEYS = [
    "Number of HVAC",
    "Number of locked HVAC",
    "Outdoor temperature",
    "Average indoor temperature",
    "Average temperature difference",
    "Regulation signal",
    "Current consumption",
    "Consumption error (%)",
    "RMSE",
    "Mass temperature",
    "Target temperature",
    "Average temperature error",
]

# mdr_cluster_stats output slots (include/mdr.h)
S_TERR, S_ABS_TERR, S_MAX_TERR, S_SQ_TERR, S_REW, S_T, S_DIFF, S_ABS_DIFF, S_TM, S_TGT, S_LOCK, S_ON = range(12)


def cluster_stats(env, rewards=None) -> np.ndarray:
    """The 12 cluster statistics of the env's current state (+ ``rewards``, a device float64 [n_local]
    tensor, or None) as a host float64 array; sharded envs are reduced over ranks (sum, max)."""
    import torch

    sh = env.shard
    out = torch.empty(12, dtype=torch.float64, device=sh.device)
    sh.cluster_stats(rewards, out)
    if env.world > 1:
        comm = env._comm
        mx = out[S_MAX_TERR:S_MAX_TERR + 1].clone()
        out[S_MAX_TERR] = 0.0
        comm.allreduce_sum(sh, out)
        comm.allreduce_max(sh, mx)
        out[S_MAX_TERR] = mx[0]
    return out.cpu().numpy()


# mdr_tick_stats rows: the 12 slots above, the cluster power after the step, three zeros
S_POWER = 12
TICK_ROW = 16


class RolloutStats:
    """Fixed-capacity device storage of one ``mdr_tick_stats`` row per tick of ``env``, written
    inside a rollout's launch sequence (``DeviceActor.rollout(stats=...)``) and read by the host once
    per call (``host()``): what ``Metrics.update`` (metrics_service.py:108-157) and
    ``TrainingManager.test`` (training_manager.py:265-295) take from the per-house obs dicts.  The
    tensor never moves, so rollout graphs captured with its pointer are replayed.

    Per stored tick the host keeps the scalars that tick's obs carried and the driver window
    already knows — the pre-step ``reg_signal`` and ``OD_temp`` — and the post-step signal.  The
    pre-step cluster power of a call's first tick is copied on the device, without a
    synchronisation, from the env's ``P`` scalar; every later tick's is the previous row's slot 12.
    One shard only (a row sums the shard's own houses); a sharded environment: ``ShardedRolloutStats``."""

    def __init__(self, env, capacity_ticks: int):
        import torch

        if capacity_ticks < 1:
            raise ValueError("capacity_ticks must be at least 1")
        if env.world > 1:
            raise ValueError("RolloutStats: sharded environments are not supported (a row sums this "
                             "shard's houses only)")
        self._alloc(env, capacity_ticks)

    def _alloc(self, env, capacity_ticks: int) -> None:
        import torch

        self.env = env
        cap = self.capacity = int(capacity_ticks)
        # one allocation, one download: [cap, 16] rows, then the cap pre-step powers
        self._buf = torch.zeros(cap * (TICK_ROW + 1), dtype=torch.float64, device=env.shard.device)
        self.stats = self._buf[:cap * TICK_ROW].view(cap, TICK_ROW)
        self._p_first = self._buf[cap * TICK_ROW:]
        self.clear()

    def clear(self) -> None:
        self.rows = 0
        self.reg_signal, self.od_temp, self.signal_post, self._first = [], [], [], []
        self._host = None

    def begin_rows(self, k: int) -> int:
        """The first of the next ``k`` rows, after checking that they fit; nothing is appended until
        ``commit_rows``."""
        if self.rows + k > self.capacity:
            raise ValueError(f"RolloutStats: {self.rows} + {k} ticks overflow the capacity of {self.capacity}")
        return self.rows

    def record_power(self, row: int) -> None:
        """The cluster power before tick ``row`` (the first of a call) from the env's device scalar:
        an asynchronous device copy on the current stream, outside any graph."""
        env = self.env
        if env._P_dev_valid:
            self._p_first[row:row + 1].copy_(env.shard.p_dev, non_blocking=True)
        else:
            self._p_first[row:row + 1].fill_(float(env._P_host))

    def commit_rows(self, reg_signal, od_temp, signal_post, first: bool) -> None:
        """Append the host scalars of the ``len(reg_signal)`` ticks whose rows were just launched;
        ``first``: the first of them starts a call (its pre-step power is ``record_power``'s)."""
        k = len(reg_signal)
        self.reg_signal.extend(float(x) for x in reg_signal)
        self.od_temp.extend(float(x) for x in od_temp)
        self.signal_post.extend(float(x) for x in signal_post)
        self._first.extend([bool(first)] + [False] * (k - 1))
        self.rows += k
        self._host = None

    def host(self) -> np.ndarray:
        """The filled rows as float64 [rows, 16] on the host (one download, one synchronisation)."""
        if self._host is None:
            h = self._buf.cpu().numpy()
            cap = self.capacity
            rows = h[:cap * TICK_ROW].reshape(cap, TICK_ROW)[:self.rows].copy()
            p_prev = np.empty(self.rows, np.float64)
            p_prev[1:] = rows[:-1, S_POWER]
            first = np.asarray(self._first, bool)
            p_prev[first] = h[cap * TICK_ROW:][:self.rows][first]
            self._host = (rows, p_prev)
        return self._host[0]

    def prev(self) -> dict:
        """Per stored tick, float64 [rows] each: the pre-step obs scalars ``reg_signal``, ``OD_temp``
        and ``cluster_hvac_power`` (``observe(env)`` before the step) and the post-step ``signal_post``."""
        self.host()
        return {"reg_signal": np.asarray(self.reg_signal, np.float64), "OD_temp": np.asarray(self.od_temp, np.float64),
                "cluster_hvac_power": self._host[1], "signal_post": np.asarray(self.signal_post, np.float64)}


class ShardedRolloutStats(RolloutStats):
    """``RolloutStats`` of a house-sharded environment (``world > 1``, or any env with a communicator):
    the same ``[capacity, 16]`` tensor and host scalars, on every rank.  During a call of m ticks each
    rank writes PARTIAL rows — its own houses' sums with N = the cluster's size — into its part of the
    context's exchange slab X[world][m][16]; behind the call ONE double sum-allreduce of the slab (every
    element has exactly one non-zero contributor: exact whatever the collective does) and one combine
    kernel, adding the ranks in rank order (slot 2: max), write the rows.  They are bit-identical on
    every rank and between communicators, equal to ``RolloutStats``' at world 1, and differ from the
    single process at world > 1 only by that regrouping of the sum slots.

    Rollouts that take it: ``Environment.rollout`` / ``greedy_rollout``, ``DeviceActor.rollout``; every
    such call is collective.  ``rollout_stats_for(env, capacity)`` picks this class or ``RolloutStats``."""

    sharded = True  # (what the rollouts ask: partial rows and one exchange, not mdr_tick_stats' rows)

    def __init__(self, env, capacity_ticks: int):
        if capacity_ticks < 1:
            raise ValueError("capacity_ticks must be at least 1")
        comm = getattr(env, "_comm", None)
        if comm is None or not callable(getattr(comm, "allreduce_sum", None)):
            raise ValueError("ShardedRolloutStats: the rows of a sharded environment are summed over its ranks; "
                             "its communicator needs a callable allreduce_sum (mdr_amd.distributed.make_comm)")
        self._alloc(env, capacity_ticks)
        self._call = None  # (m, first row) of the per-tick call whose partial rows are being written

    # ---- calls stepped from Python: partial rows tick by tick, then one exchange
    def _native(self) -> bool:
        return bool(getattr(self.env._comm, "native", False))

    def begin_partial(self, m: int) -> int:
        """Start a call of ``m`` ticks whose partial rows ``partial_row`` writes one by one; returns the
        first row (``begin_rows``: ValueError before anything advances)."""
        row0 = self.begin_rows(m)
        sh, comm = self.env.shard, self.env._comm
        if not self._native():  # the context has no communicator of its own: tell it the slab's layout
            sh.stats_exchange_ranks(comm.world, comm.rank)
        self._call = (int(m), row0)
        return row0

    def partial_row(self, rewards, t: int) -> None:
        """This rank's partial row ``t`` of the call from the current (post-step) state, ``rewards``
        and the device P (mdr_tick_stats_sharded)."""
        self.env.shard.tick_stats_sharded(rewards, self._call[0], t)

    def exchange(self) -> None:
        """The call's one exchange and combine: the library's communicator (RCCL, host callbacks), or
        ``comm.allreduce_sum`` of the slab and mdr_stats_rows_combine."""
        (m, row0), self._call = self._call, None
        sh = self.env.shard
        if self._native():
            sh.stats_rows_exchange(m, self.stats, row0)
        else:
            self.env._comm.allreduce_sum(sh, sh.stats_exchange_buffer(m))
            sh.stats_rows_combine(m, self.stats, row0)

    def abort(self) -> None:
        """A call that failed between ``begin_partial`` and ``exchange``: the slab back to all zero."""
        if self._call is not None:
            m, self._call = self._call[0], None
            self.env.shard.stats_exchange_buffer(m).zero_()


class _MemberRows:
    """One cluster's rows of a ``BatchRolloutStats`` behind ``RolloutStats``' read interface (``rows``,
    ``host()``, ``prev()``): what ``DeviceMetrics.update_rollout`` and ``evaluation_means`` take."""

    def __init__(self, stats: "BatchRolloutStats", e: int):
        self._stats, self._e = stats, int(e)
        self.env = stats.batch.members[self._e]

    @property
    def rows(self) -> int:
        return self._stats.rows

    @property
    def capacity(self) -> int:
        return self._stats.capacity

    def host(self) -> np.ndarray:
        return self._stats.host()[self._e]

    def prev(self) -> dict:
        s, e = self._stats, self._e
        s.host()
        return {"reg_signal": np.asarray(s.reg_signal[e], np.float64), "OD_temp": np.asarray(s.od_temp[e], np.float64),
                "cluster_hvac_power": s._host[1][e], "signal_post": np.asarray(s.signal_post[e], np.float64)}


class BatchRolloutStats:
    """``RolloutStats`` for an ``EnvBatch``: fixed-capacity device storage of one ``mdr_tick_stats`` row
    per cluster and tick, ``[E, capacity, 16]``, written by the batch's one launch
    (``EnvBatch.rollout(stats=...)`` / ``rollout_returns(stats=...)``, k_batch_eval) and read by the host
    once (``host()``).  One allocation holds the rows and the ``[E, capacity]`` pre-step powers: the
    pre-step power of a call's first tick is copied on the device from ``batch.cluster_power()`` before
    the launch, without a synchronisation; every later tick's is the previous row's slot 12.

    Per member the host keeps what ``Environment.rollout`` commits from that member's driver window:
    the pre-step ``reg_signal`` (``s_prev``) and ``OD_temp`` (``t_od_prev``), and the post-step signal
    (``s_prev[1:]`` and the member's grid signal after the window).  ``member(e)`` is cluster ``e`` behind
    ``RolloutStats``' read interface.  ``clear()`` forgets every cluster's rows."""

    def __init__(self, batch, capacity_ticks: int):
        import torch

        if capacity_ticks < 1:
            raise ValueError("capacity_ticks must be at least 1")
        self.batch = batch
        cap = self.capacity = int(capacity_ticks)
        E = batch.n_envs
        self._buf = torch.zeros(E * cap * (TICK_ROW + 1), dtype=torch.float64, device=batch.device)
        self.stats = self._buf[:E * cap * TICK_ROW].view(E, cap, TICK_ROW)
        self._p_first = self._buf[E * cap * TICK_ROW:].view(E, cap)
        self.clear()

    def clear(self) -> None:
        E = self.batch.n_envs
        self.rows = 0
        self.reg_signal, self.od_temp, self.signal_post = ([[] for _ in range(E)] for _ in range(3))
        self._first = []
        self._host = None

    def begin_rows(self, k: int) -> int:
        """The first of the next ``k`` rows, after checking that they fit; nothing is appended until
        ``commit_rows``."""
        if self.rows + k > self.capacity:
            raise ValueError(f"BatchRolloutStats: {self.rows} + {k} ticks overflow the capacity of {self.capacity}")
        return self.rows

    def record_power(self, row: int) -> None:
        """Every cluster's power before tick ``row`` (the first of a call) from the batch's device
        vector: an asynchronous device copy on the current stream."""
        self._p_first[:, row].copy_(self.batch.cluster_power(), non_blocking=True)

    def commit_rows(self, ticks: np.ndarray, signal_after) -> None:
        """Append the host scalars of the call whose rows were just launched: ``ticks`` the members'
        driver windows ``[E, k, 4]`` (mdr_tick layout), ``signal_after[e]`` member e's grid signal
        behind its window."""
        k = ticks.shape[1]
        for e in range(self.batch.n_envs):
            s_prev = ticks[e, :, 2]
            self.reg_signal[e].extend(float(x) for x in s_prev)
            self.od_temp[e].extend(float(x) for x in ticks[e, :, 0])
            self.signal_post[e].extend([float(x) for x in s_prev[1:]] + [float(signal_after[e])])
        self._first.extend([True] + [False] * (k - 1))
        self.rows += k
        self._host = None

    def host(self) -> np.ndarray:
        """The filled rows as float64 [E, rows, 16] on the host (one download, one synchronisation)."""
        if self._host is None:
            h = self._buf.cpu().numpy()
            E, cap = self.batch.n_envs, self.capacity
            rows = h[:E * cap * TICK_ROW].reshape(E, cap, TICK_ROW)[:, :self.rows].copy()
            p_prev = np.empty((E, self.rows), np.float64)
            p_prev[:, 1:] = rows[:, :-1, S_POWER]
            first = np.asarray(self._first, bool)
            p_prev[:, first] = h[E * cap * TICK_ROW:].reshape(E, cap)[:, :self.rows][:, first]
            self._host = (rows, p_prev)
        return self._host[0]

    def member(self, e: int) -> _MemberRows:
        if not 0 <= int(e) < self.batch.n_envs:
            raise ValueError(f"env id {e} outside [0, {self.batch.n_envs})")
        return _MemberRows(self, e)


def rollout_stats_for(env, capacity_ticks: int):
    """The stats rows class for ``env``: ``ShardedRolloutStats`` for a sharded environment or one with
    a communicator, ``RolloutStats`` otherwise."""
    sharded = env.world > 1 or getattr(env, "_comm", None) is not None
    return (ShardedRolloutStats if sharded else RolloutStats)(env, capacity_ticks)


class DeviceMetrics:
    """``Metrics`` (metrics_service.py:71-257) fed by device reductions instead of a per-house loop."""

    FIELDS = ("cumul_avg_reward", "cumul_temp_offset", "cumul_temp_error", "cumul_signal_offset",
              "cumul_signal_error", "cumul_squared_error_temp", "max_temp_error", "cumul_OD_temp", "cumul_signal",
              "cumul_cons", "cumul_squared_error_sig", "cumul_squared_max_error_temp")

    def __init__(self, wandb_service=None):
        self.wandb_service = wandb_service

    def initialize(self, nb_agents: int, start_stats_from: int, nb_time_steps: int) -> None:
        self.nb_time_steps = nb_time_steps
        self.start_stats_from = start_stats_from
        self.nb_agents = nb_agents
        for f in self.FIELDS:
            setattr(self, f, 0.0)
        self.rmse_sig_per_ag = nan
        self.rmse_temp = nan
        self.rms_max_error_temp = nan
        if self.wandb_service is not None:
            self.wandb_service.initialize()

    def update(self, prev: dict, env, rewards, time_step: int) -> None:
        """Metrics.update(obs_dict, next_obs_dict, rewards_dict, time_step): ``prev`` holds the
        pre-step obs scalars {"reg_signal", "OD_temp", "cluster_hvac_power"} (observe(env) before
        the step); ``env`` is the post-step environment and ``rewards`` its device reward tensor."""
        st = cluster_stats(env, rewards)
        self._accumulate(st, prev["reg_signal"], prev["OD_temp"], prev["cluster_hvac_power"],
                         env.cluster.current_power_consumption, time_step)

    def update_rollout(self, stats: "RolloutStats", time_step0: int, row0: int = 0) -> None:
        """``update`` for the stored ticks ``row0 ..`` of ``stats`` (time steps ``time_step0``,
        ``time_step0 + 1``, ...): the same arithmetic in the same order, from the rows a rollout wrote
        on the device — one synchronisation and one host pass per call instead of one per tick."""
        rows, prev = stats.host(), stats.prev()
        for r in range(row0, stats.rows):
            st = rows[r]
            self._accumulate(st, float(prev["reg_signal"][r]), float(prev["OD_temp"][r]),
                             float(prev["cluster_hvac_power"][r]), float(st[S_POWER]), time_step0 + r - row0)

    def _accumulate(self, st, reg_signal, od_temp, cons_prev, cons_post, time_step: int) -> None:
        """One tick of Metrics.update (metrics_service.py:131-157) from its cluster statistics."""
        n = self.nb_agents
        prev = {"reg_signal": reg_signal, "OD_temp": od_temp, "cluster_hvac_power": cons_prev}
        self.cumul_temp_offset += st[S_TERR]
        self.cumul_temp_error += st[S_ABS_TERR]
        self.max_temp_error = max(self.max_temp_error, float(st[S_MAX_TERR]))
        self.cumul_avg_reward += st[S_REW]
        if time_step >= self.start_stats_from:
            self.cumul_squared_error_temp += st[S_SQ_TERR]
        # the same per-house signal error for every house (metrics_service.py:140-145)
        signal_error = (prev["reg_signal"] - cons_post) / (n ** 2)
        self.cumul_signal_offset += n * signal_error
        self.cumul_signal_error += n * np.abs(signal_error)
        self.cumul_OD_temp += prev["OD_temp"]
        self.cumul_signal += prev["reg_signal"]
        self.cumul_cons += prev["cluster_hvac_power"]
        if time_step >= self.start_stats_from:
            self.cumul_squared_error_sig += prev["reg_signal"] ** 2
            self.cumul_squared_max_error_temp = self.max_temp_error ** 2

    def log(self, time_step: int, time_steps_log: int, time) -> dict:
        """Metrics.log without the reference's stray breakpoint (metrics_service.py:159-195)."""
        if time_step >= self.start_stats_from:
            self.update_rms(time_step)
        else:
            self.rmse_sig_per_ag = self.rmse_temp = self.rms_max_error_temp = nan
        metrics = {
            "Mean train return": self.cumul_avg_reward / time_steps_log,
            "Mean temperature offset": self.cumul_temp_offset / time_steps_log,
            "Mean temperature error": self.cumul_temp_error / time_steps_log,
            "Mean signal error": self.cumul_signal_offset / time_steps_log,
            "Mean signal offset": self.cumul_signal_offset / time_steps_log,
            "Mean outside temperature": self.cumul_OD_temp / time_steps_log,
            "Mean signal": self.cumul_signal / time_steps_log,
            "Mean consumption": self.cumul_cons / time_steps_log,
            "Time (hour)": time.hour,
            "Time step": time_step,
        }
        if self.wandb_service is not None:
            self.wandb_service.log(metrics)
        return metrics

    def reset(self) -> None:
        for f in ("cumul_avg_reward", "cumul_temp_offset", "cumul_temp_error", "max_temp_error",
                  "cumul_signal_offset", "cumul_signal_error", "cumul_OD_temp", "cumul_signal", "cumul_cons"):
            setattr(self, f, 0)

    def update_rms(self, time_step: int) -> None:
        k = time_step - self.start_stats_from
        self.rmse_sig_per_ag = np.sqrt(self.cumul_squared_error_sig / k) / self.nb_agents
        self.rmse_temp = np.sqrt(self.cumul_squared_error_temp / (k * self.nb_agents))
        self.rms_max_error_temp = np.sqrt(self.cumul_squared_max_error_temp / k)

    def update_final(self) -> dict:
        self.update_rms(self.nb_time_steps)
        return {"RMSE signal per agent": self.rmse_sig_per_ag, "RMSE temperature": self.rmse_temp,
                "RMS Max Error temperature": self.rms_max_error_temp}


def evaluation_means(rows, signal_post, n: int, n_ticks: int) -> dict:
    """The three means TrainingManager.test logs (training_manager.py:265-295, metrics_service.py:
    259-282) from the first ``n_ticks`` post-step stats rows and post-step signals of a cluster of
    ``n`` houses:

      "Mean test return"             sum_t sum_i reward_i / N / T
      "Test mean temperature error"  sum_t sum_i |T_i - target_i| / N / T
      "Test mean signal error"       sum_t N |s_post - P_post| / N^2 / T
    """
    ret = temp = sig = 0.0
    for t in range(n_ticks):
        ret += rows[t, S_REW]
        temp += rows[t, S_ABS_DIFF] / n
        sig += n * (np.abs(signal_post[t] - rows[t, S_POWER]) / n ** 2)
    return {"Mean test return": float(ret / n_ticks), "Test mean temperature error": float(temp / n_ticks),
            "Test mean signal error": float(sig / n_ticks)}


BANGBANG_CONTROLLERS = ("bangbang", "deadband_bangbang")
# the controllers whose rollouts write their own stats rows: ``rollout(action_mode=c, stats=...)`` for the
# bang-bang pair, ``greedy_rollout(stats=...)`` for GreedyMyopic (config C3)
ROLLOUT_CONTROLLERS = BANGBANG_CONTROLLERS + ("greedy",)


def evaluate_controller(env, controller: str, n_ticks: int, twin=None) -> dict:
    """TrainingManager.test (training_manager.py:265-295) for a baseline controller, 'bangbang' or
    'deadband_bangbang' (bangbang_controllers.py:25-65): the controller run for ``n_ticks`` on a reset
    copy of ``env`` as ONE ``rollout(n_ticks, action_mode=controller, stats=...)`` — closed-loop windows
    writing their own stats rows where they apply — and ``evaluation_means`` of the rows, the values
    ``DeviceMAPPO.evaluate`` reports for a policy.  'greedy' (GreedyMyopic,
    greedy_myopic_controller.py:67-104): ONE ``greedy_rollout(n_ticks, stats=...)`` with one action
    and one reward row every tick overwrites.  ``twin`` None: ``copy.deepcopy(env)`` as the
    reference does; a caller-kept twin may be passed instead, whose context, row and reward buffers
    and rollout graph are then reused by later calls.  The copy is ``reset`` (which advances the
    shared RNG, as in the reference); ``env``'s device state, tick, date and P are not touched.
    On a sharded environment the call is collective (every rank makes it) and the rows are
    ``ShardedRolloutStats``': the same means on every rank."""
    import copy

    import torch

    if controller not in ROLLOUT_CONTROLLERS:
        raise ValueError(f"evaluate_controller: controller must be one of {ROLLOUT_CONTROLLERS}, not {controller!r}")
    if n_ticks < 1:
        raise ValueError("n_ticks must be at least 1")
    ev = copy.deepcopy(env) if twin is None else twin
    if ev is env:
        raise ValueError("evaluate_controller() resets its env: pass a copy as twin, not the env itself")
    ev.reset(return_obs=False)
    kept = getattr(ev, "_eval_kept", None) if twin is not None else None
    if kept is None or kept["stats"].capacity != n_ticks:  # (a graph is cached per rollout length anyway)
        kept = {"stats": rollout_stats_for(ev, n_ticks),
                "rewards": torch.empty(ev.n_local, dtype=torch.float64, device=ev.shard.device)}
        if twin is not None:
            ev._eval_kept = kept  # (Environment.__deepcopy__ leaves it behind)
    stats = kept["stats"]
    stats.clear()
    # (one reward row: the windows finalise only the last tick's rewards, the rows need none of them)
    if controller == "greedy":
        if "actions" not in kept:
            kept["actions"] = torch.empty(ev.n_local, dtype=torch.uint8, device=ev.shard.device)
        ev.greedy_rollout(n_ticks, actions=kept["actions"], rewards=kept["rewards"], stats=stats)
    else:
        ev.rollout(n_ticks, action_mode=controller, rewards=kept["rewards"], use_graph=twin is not None, stats=stats)
    return evaluation_means(stats.host(), stats.prev()["signal_post"], ev.n, n_ticks)


RETURNS_CONTROLLERS = ("random", "always_on", "bangbang", "deadband_bangbang")


def controller_returns(env, controller: str, n_ticks: int, gamma: float = 1.0, twin=None):
    """Every house's discounted return ``sum_t gamma**t r_i(t)`` (ppo.py:196-206) of a baseline run for
    ``n_ticks`` on a reset copy of ``env``, as ONE ``rollout_returns`` — no reward matrix.  The
    controllers: the open-loop baselines 'random' and 'always_on' and the two bang-bang controllers.
    The copy-and-reset protocol is ``evaluate_controller``'s (``twin`` None: ``copy.deepcopy(env)``;
    the copy is ``reset``; ``env`` is not touched).  Returns ``(returns, means)``: the float64 [N]
    device tensor and ``{"Mean test return": mean(returns) / n_ticks}``, which at gamma = 1 is
    TrainingManager.test's mean reward per house and tick (training_manager.py:265-295)."""
    import copy

    import torch

    if controller not in RETURNS_CONTROLLERS:
        raise ValueError(f"controller_returns: controller must be one of {RETURNS_CONTROLLERS}, not {controller!r}")
    if n_ticks < 1:
        raise ValueError("n_ticks must be at least 1")
    ev = copy.deepcopy(env) if twin is None else twin
    if ev is env:
        raise ValueError("controller_returns() resets its env: pass a copy as twin, not the env itself")
    ev.reset(return_obs=False)
    returns = torch.zeros(ev.n_local, dtype=torch.float64, device=ev.shard.device)
    ev.rollout_returns(n_ticks, returns, gamma=gamma, action_mode=controller)
    return returns, {"Mean test return": float(returns.mean().item()) / n_ticks}


EVALUATION_KEYS = ("Mean test return", "Test mean temperature error", "Test mean signal error")


def evaluate_batch(batch, controller: str, n_ticks: int, gamma: float = 1.0, stats=None) -> dict:
    """``evaluate_controller`` and ``controller_returns`` for every cluster of an ``EnvBatch`` at once:
    the batch is reset, then ONE ``rollout_returns(n_ticks, ..., action_mode=controller, stats=...)`` —
    one launch, no reward matrix — gives every house's discounted return and every cluster's stats
    rows.  ``controller``: one of ``RETURNS_CONTROLLERS``.  A batch has no deep copy, so unlike
    ``evaluate_controller`` this resets ``batch`` ITSELF (every member, each from its own RNG):
    evaluation batches are built for the purpose.  ``stats``: a ``BatchRolloutStats`` of ``batch``
    with room for ``n_ticks`` rows to reuse (cleared here), or None.

    Returns ``evaluation_means``' three keys as float64 ``[E]`` arrays (cluster e's value what
    ``evaluate_controller`` gives its stand-alone twin, the sums regrouped), ``"returns"``: the
    ``[E, N_c]`` device tensor, and ``"mean"``: the three keys averaged over the clusters."""
    if controller not in RETURNS_CONTROLLERS:
        raise ValueError(f"evaluate_batch: controller must be one of {RETURNS_CONTROLLERS}, not {controller!r}")
    if int(n_ticks) != n_ticks or n_ticks < 1:
        raise ValueError("n_ticks must be at least 1")
    if not (isinstance(gamma, (int, float)) and 0.0 < gamma <= 1.0):
        raise ValueError(f"gamma = {gamma!r} outside (0, 1]")
    if stats is None:
        stats = BatchRolloutStats(batch, n_ticks)
    elif getattr(stats, "batch", None) is not batch or stats.capacity < n_ticks:
        raise ValueError(f"evaluate_batch: stats must be a BatchRolloutStats of this batch with capacity >= {n_ticks}")
    batch.reset()
    stats.clear()
    returns = batch.empty_returns()
    batch.rollout_returns(n_ticks, returns, gamma=gamma, action_mode=controller, stats=stats)
    per = [evaluation_means(stats.member(e).host(), stats.member(e).prev()["signal_post"], batch.n, n_ticks)
           for e in range(batch.n_envs)]
    out = {k: np.array([m[k] for m in per], np.float64) for k in EVALUATION_KEYS}
    out["mean"] = {k: float(np.mean(out[k])) for k in EVALUATION_KEYS}
    out["returns"] = returns
    return out


def observe(env) -> dict:
    """The per-tick scalars every house's obs dict carries (environment.py:110-130)."""
    return {"reg_signal": env.power_grid.current_signal, "OD_temp": env.current_od_temp,
            "cluster_hvac_power": env.cluster.current_power_consumption}


class HouseList(Sequence):
    """ClientManagerService.update_houses_data's N-entry house list (client_manager_service.py:
    198-230) over a snapshot of the state: an entry is built when it is read.  The snapshot is a
    device copy until ``offload()`` moves it to host memory (UISummary keeps only the latest tick's
    list on the device, so a long server run grows host memory like the reference's list, not HBM)."""

    def __init__(self, env):
        sh = env.shard
        self._n = sh.n
        self._t, self._tg, self._hv = sh.t_air.clone(), sh.target.clone(), sh.hvac.clone()
        self._host = None
        self._lo = env._offset

    def _arrays(self):
        if self._host is None:
            from .shard import decode_hvac

            on, lock, sso = decode_hvac(self._hv.cpu().numpy())
            self._host = (self._t.cpu().numpy(), self._tg.cpu().numpy(), on, lock, sso)
            self._t = self._tg = self._hv = None  # (the device copies are no longer needed)
        return self._host

    def offload(self) -> None:
        """Move the snapshot to host memory now (one device->host copy) and free its device copy."""
        self._arrays()

    def __len__(self) -> int:
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        T, tg, on, lock, sso = self._arrays()
        i = int(i)
        if i < 0:
            i += len(self)
        d = {"id": self._lo + i}
        if on[i]:
            d["hvacStatus"] = "ON"
        else:
            d.update({"hvacStatus": "Lockout" if lock[i] else "OFF", "secondsSinceOff": int(sso[i])})
        d["indoorTemp"] = float(T[i])
        d["targetTemp"] = float(tg[i])
        d["tempDifference"] = float(T[i]) - float(tg[i])
        return d

    def status_counts(self):
        """(#ON, #Lockout, #OFF, sum of secondsSinceOff over the non-ON houses)."""
        _, _, on, lock, sso = self._arrays()
        off = ~on
        return int(on.sum()), int((off & lock).sum()), int((off & ~lock).sum()), int(sso[off].sum())


class UISummary:
    """ClientManagerService (client_manager_service.py:28-245) from device reductions: the 12
    summary strings, the graph series and the house list of every tick, without a pandas frame."""

    def __init__(self, socket_manager=None):
        self.socket_manager = socket_manager

    def initialize_data(self, interface: bool) -> None:
        self.interface = interface
        self.description = {}
        self.temp_diff = np.array([])
        self.temp_err = np.array([])
        self.air_temp = np.array([])
        self.mass_temp = np.array([])
        self.target_temp = np.array([])
        self.outdoor_temp = np.array([])
        self.signal = np.array([])
        self.consumption = np.array([])
        self.houses_data = {}

    def update_data(self, env, time_step: int) -> None:
        """update_data(obs_dict, time_step) for the env's current obs."""
        n = env.n
        st = cluster_stats(env)
        od, S, P = env.current_od_temp, env.power_grid.current_signal, env.cluster.current_power_consumption
        # update_graph_data (client_manager_service.py:177-196): per-tick means over the houses
        self.temp_diff = np.append(self.temp_diff, st[S_DIFF] / n)
        self.temp_err = np.append(self.temp_err, st[S_ABS_DIFF] / n)
        self.air_temp = np.append(self.air_temp, st[S_T] / n)
        self.mass_temp = np.append(self.mass_temp, st[S_TM] / n)
        self.target_temp = np.append(self.target_temp, st[S_TGT] / n)
        self.outdoor_temp = np.append(self.outdoor_temp, od)
        self.signal = np.append(self.signal, S)
        self.consumption = np.append(self.consumption, P)
        tm0, tg0 = self._house0(env)
        values = [
            str(n),
            str(int(st[S_LOCK])),
            str(round(od, 2)),
            str(round(st[S_T] / n, 2)),
            str(round(st[S_DIFF] / n, 2)),
            str(S),
            str(P),
            str((S - P) / S * 100),
            str(np.sqrt(np.mean((self.signal - self.consumption) ** 2))),
            str(round(tm0, 2)),
            str(round(tg0, 2)),
            str(np.mean(self.temp_err)),
        ]
        self.description[time_step] = dict(zip(DESCRIPTION_KEYS, values))
        if self.houses_data:  # the previous tick's snapshot leaves HBM
            self.houses_data[next(reversed(self.houses_data))].offload()
        self.houses_data[time_step] = HouseList(env)

    @staticmethod
    def _house0(env):
        """mass_temp / target_temp of house 0 (the reference reads data_frame[...][0])."""
        import torch

        sh = env.shard
        v = torch.stack([sh.t_mass[0], sh.target[0]]) if env._offset == 0 else \
            torch.zeros(2, dtype=torch.float64, device=sh.device)
        if env.world > 1:
            env._comm.allreduce_sum(sh, v)
        a, b = v.cpu().tolist()
        return a, b


class ServerLoop:
    """ControllerManager.start's tick loop (controller_manager.py:129-187) on the device env:
    UI summary of the current obs -> actions -> env.step -> Metrics.update -> episode reset ->
    periodic log.  ``controller``: 'deadband_bangbang' / 'bangbang' / 'always_on' / 'random' (fused
    in the step kernel), 'greedy' (device GreedyMyopic), or a callable env -> uint8 device actions.
    Per-house Python objects are only built on access (UISummary.houses_data).
    ``rollout_ticks`` = K > 0 (the two bang-bang controllers and 'greedy'): ``run`` advances in chunks
    of up to K ticks, each one rollout whose stats rows feed the Metrics, with one UI update per chunk."""

    def __init__(self, env, controller="deadband_bangbang", start_stats_from: int = 0, nb_time_steps: int = 1000,
                 time_steps_per_episode: int = 10 ** 9, time_steps_train_log: int = 10 ** 9, interface: bool = False,
                 metrics=None, ui=None, rollout_ticks: int = 0):
        if rollout_ticks < 0:
            raise ValueError("rollout_ticks must be >= 0")
        if rollout_ticks and controller not in ROLLOUT_CONTROLLERS:
            raise ValueError(f"rollout_ticks needs one of the controllers {ROLLOUT_CONTROLLERS}")
        self.rollout_ticks = int(rollout_ticks)
        self._rows = None  # RolloutStats of rollout_ticks rows + the chunks' one reward (greedy: and action) row
        self.env = env
        self.controller = controller
        self.metrics = metrics or DeviceMetrics()
        self.ui = ui or UISummary()
        self.metrics.initialize(env.n, start_stats_from, nb_time_steps)
        self.ui.initialize_data(interface)
        self.nb_time_steps = nb_time_steps
        self.time_steps_per_episode = time_steps_per_episode
        self.time_steps_train_log = time_steps_train_log
        self.current_time_step = 0
        self.logs = []

    def _step(self):
        env, c = self.env, self.controller
        if callable(c):
            return env.step_tensor(c(env))
        if c == "greedy":
            return env.step_tensor(env.greedy_actions())
        if c in ("deadband_bangbang", "bangbang", "always_on", "random"):
            # the launch also counts the next tick's power under the same source (one launch per tick)
            return env.step_tensor(None, action_mode=c, lookahead=c)
        raise ValueError(f"unknown controller {c!r}")

    def _run_chunks(self, end: int) -> None:
        """``run``'s loop for ``rollout_ticks`` = K > 0: chunks of up to K ticks as one
        ``env.rollout(k, action_mode=controller, stats=...)`` (``env.greedy_rollout(k, stats=...)``
        for 'greedy') each, cut at episode ends, log
        boundaries and ``end``; ``ui.update_data`` once at each chunk's start; Metrics from the
        chunk's rows (``DeviceMetrics.update_rollout``: the per-tick arithmetic in its order)."""
        import torch

        env = self.env
        if self._rows is None:
            self._rows = (rollout_stats_for(env, self.rollout_ticks),
                          torch.empty(env.n_local, dtype=torch.float64, device=env.shard.device),
                          torch.empty(env.n_local, dtype=torch.uint8, device=env.shard.device)
                          if self.controller == "greedy" else None)
        stats, rewards, actions = self._rows
        ep, lg = self.time_steps_per_episode, self.time_steps_train_log
        while self.current_time_step < end:
            step = self.current_time_step
            k = min(self.rollout_ticks, end - step, ep - step % ep, lg - step % lg)
            self.ui.update_data(env, step)
            stats.clear()
            if self.controller == "greedy":
                env.greedy_rollout(k, actions=actions, rewards=rewards, stats=stats)
            else:
                env.rollout(k, action_mode=self.controller, rewards=rewards, stats=stats)
            self.metrics.update_rollout(stats, step)
            last = step + k - 1
            if last % ep == ep - 1:
                env.reset(return_obs=False)
            if last % lg == lg - 1:
                self.logs.append(self.metrics.log(last, lg, env.date_time))
                self.metrics.reset()
            self.current_time_step += k

    def run(self, n_steps=None):
        end = self.nb_time_steps if n_steps is None else min(self.nb_time_steps, self.current_time_step + n_steps)
        if self.rollout_ticks:
            self._run_chunks(end)
            end = self.current_time_step  # (the per-tick loop below has nothing left)
        for step in range(self.current_time_step, end):
            self.ui.update_data(self.env, step)
            prev = observe(self.env)
            rewards = self._step()
            self.metrics.update(prev, self.env, rewards, step)
            if step % self.time_steps_per_episode == self.time_steps_per_episode - 1:
                self.env.reset(return_obs=False)
            if step % self.time_steps_train_log == self.time_steps_train_log - 1:
                self.logs.append(self.metrics.log(step, self.time_steps_train_log, self.env.date_time))
                self.metrics.reset()
            self.current_time_step += 1
        if self.current_time_step == self.nb_time_steps:
            return self.metrics.update_final()
        return None
