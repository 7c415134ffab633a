"""Stats rows and returns of an ``EnvBatch`` (mdr_batch_rollout_eval, k_batch_eval): what needs no GPU.

* the new entry point and the Python layer refuse bad arguments before any HIP call;
* the inputs of tests/test_env_batch_eval_gpu.py exercise the row's slots.  Under the oracle
  (oracle/env_np.OracleEnv, seeds 8, 9, ...), at every GPU shape with N_c >= 50 and both bang-bang
  controllers: on every tick of every cluster there are houses above and below their target (slots 0 and
  6 really cancel), at least one house in lockout, and an ON count strictly between 0 and N_c — measured
  with one exception, one tick of 45 at (3, 50), bang-bang, seed 8, so the assertion is >= 44 of 45 ticks
  (12 of 12 at 1,024); and the clusters' lockout counts are pairwise distinct on at least 3/5 of the ticks
  (measured 31-41 of 45, 11-12 of 12 at 1,024), so rows written to the wrong cluster cannot pass ==;
* the NumPy summation helper of the GPU test (tests/batch_eval_rows.py) is deterministic and differs from
  np.sum on the oracle's ticks: the "order" part of the GPU test's == tests something.
"""
import random

import numpy as np
import pytest

import batch_eval_rows as R
import batch_inputs as B
from bangbang_inputs import CTRLS
from oracle import env_np as O

_RUNS = {}


def oracle_ticks(n, seed, ticks, ctrl):
    """Per tick of one cluster under the oracle and the controller: (T, Tm, target, lock, on, rewards, P)."""
    key = (n, seed, ticks, ctrl)
    if key not in _RUNS:
        props = B.props(n)
        ora = O.OracleEnv(props, random.Random(seed))
        db = props.cluster_prop.house_prop.deadband
        tg = np.asarray(ora.pop["target"], np.float64)
        out = []
        for _ in range(ticks):
            a = O.bangbang(ora.T, tg) if ctrl == "bangbang" else O.deadband_bangbang(ora.T, tg, db, ora.on)
            o, rew = ora.step(a)
            out.append((o["T"], o["Tm"], tg, o["lock"], o["on"], np.asarray(rew, np.float64), o["P"]))
        _RUNS[key] = out
    return _RUNS[key]


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("n_envs,n,ticks", [s for s in B.SHAPES if s[1] >= 50])
def test_inputs_exercise_the_slots(n_envs, n, ticks, ctrl):
    runs = [oracle_ticks(n, s, ticks, ctrl) for s in B.seeds(n_envs)]
    need = ticks if ticks < 45 else ticks - 1
    for e, run in enumerate(runs):
        both = sum(bool((T > tg).any() and (T < tg).any()) for T, _, tg, _, _, _, _ in run)
        locked = sum(bool(np.any(lock)) for _, _, _, lock, _, _, _ in run)
        partly = sum(0 < int(np.sum(on)) < n for _, _, _, _, on, _, _ in run)
        print(f"E={n_envs} n={n} {ctrl} cluster {e}: above and below {both}, lockout {locked}, partly on {partly} of {ticks}")
        assert both >= need and locked >= need and partly >= need
    locks = np.array([[int(np.sum(x[3])) for x in run] for run in runs])  # [E, ticks]
    distinct = sum(len(set(locks[:, t])) == n_envs for t in range(ticks))
    print(f"lockout counts pairwise distinct on {distinct} of {ticks} ticks")
    assert distinct * 5 >= 3 * ticks


def test_numpy_order_is_deterministic_and_not_np_sum():
    differs = 0
    for n_envs, n, ticks in [(3, 129, 45), (5, 1000, 45)]:
        for T, Tm, tg, lock, on, rew, P in oracle_ticks(n, B.seeds(n_envs)[0], ticks, "bangbang"):
            terms = R.house_terms(T, Tm, tg, lock, on, rew)
            a, b = R.ordered_reduce(terms), R.ordered_reduce(terms.copy())
            assert a.tobytes() == b.tobytes()
            row = R.stats_row(T, Tm, tg, lock, on, rew, P)
            assert row[:12].tobytes() == a.tobytes() and row[12] == P and not row[13:].any()
            plain = terms.sum(axis=1)
            assert a[2] == max(0.0, terms[2].max()) and a[10] == lock.sum() and a[11] == on.sum()
            np.testing.assert_allclose(np.delete(a, 2), np.delete(plain, 2), rtol=0, atol=1e-12 * np.abs(terms).sum(axis=1).max())
            differs += int(any(a[k] != plain[k] for k in (0, 1, 3, 4, 5, 6, 7, 8)))
    assert differs > 0


def test_one_house_and_one_wave_rows():
    """One house: every sum is the house's own term.  Fewer than 128 houses: one wave, no wave sum."""
    row = R.stats_row([21.5], [20.25], [20.0], [True], [False], [-3.0], 0.0)
    assert row.tolist() == [1.5, 1.5, 1.5, 2.25, -3.0, 21.5, 1.5, 1.5, 20.25, 20.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    row = R.stats_row([19.0, 18.0], [0.0, 0.0], [20.0, 20.0], [False, False], [True, True], [0.0, 0.0], 7.0)
    assert row[0] == (19.0 - 10.0) + (18.0 - 10.0) and row[2] == 9.0 and row[6] == -3.0 and row[12] == 7.0


def test_c_abi_argument_errors_without_gpu():
    """mdr_batch_rollout_eval validates its arguments before any HIP call (absent on the parent commit)."""
    from mdr_amd import _lib

    lib = _lib.load()
    assert lib.mdr_batch_rollout_eval(None, 1, None, None, 0, 1, None, 0, None, None, None, 0, 0, None, None) == -1


def test_exported():
    import mdr_amd
    from mdr_amd import services

    assert mdr_amd.BatchRolloutStats is services.BatchRolloutStats and mdr_amd.evaluate_batch is services.evaluate_batch
    assert {"BatchRolloutStats", "evaluate_batch"} <= set(mdr_amd.__all__)


def test_python_refusals_need_no_device():
    from mdr_amd.batch import EnvBatch
    from mdr_amd.services import RETURNS_CONTROLLERS, BatchRolloutStats, evaluate_batch

    for name in ("empty_returns", "rollout_returns"):
        assert callable(getattr(EnvBatch, name))

    class NoBatch:  # (the checks below come before anything touches the batch)
        n_envs, n = 2, 50

    with pytest.raises(ValueError, match="controller must be"):
        evaluate_batch(NoBatch(), "greedy", 4)
    assert "greedy" not in RETURNS_CONTROLLERS
    with pytest.raises(ValueError, match="n_ticks"):
        evaluate_batch(NoBatch(), "bangbang", 0)
    for g in (0.0, 1.5, -1.0, float("nan"), None):
        with pytest.raises(ValueError, match="gamma"):
            evaluate_batch(NoBatch(), "bangbang", 4, gamma=g)
    with pytest.raises(ValueError, match="capacity_ticks"):
        BatchRolloutStats(NoBatch(), 0)
