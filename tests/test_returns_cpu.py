"""``rollout_returns`` without a GPU: the NumPy restatements (tests/returns_np.py), the bound the
closed-loop window form is held to — shown here on the oracle's own trajectories, so the reference
alone stays inside it —, the C entry points' MDR_EARG refusals and the Python ``ValueError``s that
need no device."""
import ctypes as C
import random

import numpy as np
import pytest

import golden_util as gu
import returns_np as RN
from bangbang_inputs import CTRLS, SEED, overrides
from oracle import env_np as O

N, TICKS = 130, 70


def test_weights_recurrence():
    w = RN.weights(0.5, 0.99, 5)
    assert w.shape == (6,) and w[0] == 0.5
    x = 0.5
    for t in range(5):
        x = x * 0.99
        assert w[t + 1] == x
    assert np.array_equal(RN.weights(1.0, 1.0, 4), np.ones(5))
    from mdr_amd.environment import discount_weights

    assert np.array_equal(discount_weights(0.5, 0.99, 70), RN.weights(0.5, 0.99, 70))


def test_window_plan_is_the_librarys():
    assert RN.window_plan(70, 32) == [24, 23, 23]
    assert RN.window_plan(37, 7) == [7, 6, 6, 6, 6, 6]
    assert RN.window_plan(5, 32) == [5] and RN.window_plan(1, 7) == [1]
    for n, win in ((70, 32), (37, 7), (64, 32), (33, 32)):
        p = RN.window_plan(n, win)
        assert sum(p) == n and max(p) <= win and len(p) == -(-n // win) and sorted(p, reverse=True) == p


def test_row_form_is_two_roundings():
    """a multiply, then an add — not an FMA: a case where the fused result differs."""
    w = np.array([1.0 + 2.0 ** -30])
    rows = np.array([[1.0 + 2.0 ** -30]])
    ret = np.array([-1.0])
    got = RN.row_form(ret, w, rows)[0]
    prod = np.float64(w[0] * rows[0, 0])       # rounded: the 2^-60 term is lost
    assert got == -1.0 + prod == 2.0 ** -29
    from fractions import Fraction

    exact = Fraction(float(w[0])) * Fraction(float(rows[0, 0])) - 1   # what an FMA would round
    assert float(exact) != got


@pytest.fixture(scope="module", params=CTRLS)
def oracle_run(request):
    """The oracle under a bang-bang controller: per tick the reward row, the raw temperature
    penalties and the signal term, formed with the oracle's own expressions."""
    ctrl = request.param
    props = gu.props_from_overrides(overrides(N))
    ora = O.OracleEnv(props, random.Random(SEED))
    hp, rp = props.cluster_prop.house_prop, props.reward_prop
    tg = ora.pop["target"]
    norm_t = O._deadband_l2_scalar(hp.target_temp, 0, hp.target_temp + 1)
    norm_s = O._deadband_l2_scalar(rp.norm_reg_sig, 0, 0.75 * rp.norm_reg_sig)
    rows, pen, sig = [], [], []
    for _ in range(TICKS):
        a = O.bangbang(ora.T, tg) if ctrl == "bangbang" else O.deadband_bangbang(ora.T, tg, hp.deadband, ora.on)
        s_prev = ora.S
        _, r = ora.step(a)
        pj = O.deadband_l2(tg, hp.deadband, ora.T)
        sj = rp.alpha_sig * ((ora.P - s_prev) / N) ** 2 / norm_s
        np.testing.assert_array_equal(-1 * (rp.alpha_temp * pj / norm_t + sj), r)  # (the pieces are the row's)
        rows.append(r), pen.append(pj), sig.append(sj)
    assert rp.alpha_temp >= 0 and rp.alpha_sig >= 0 and norm_t > 0 and norm_s > 0
    return np.array(rows), np.array(pen), np.array(sig, np.float64), rp.alpha_temp, norm_t


@pytest.mark.parametrize("gamma", [1.0, 0.99])
@pytest.mark.parametrize("win", [32, 7])
def test_window_form_within_the_bound_on_oracle_trajectories(oracle_run, win, gamma):
    rows, pen, sig, alpha_temp, norm_t = oracle_run
    w = RN.weights(1.0, gamma, TICKS)
    ret0 = np.zeros(N)
    ref = RN.row_form(ret0, w, rows)
    got = RN.window_form(ret0, w, pen, sig, win, alpha_temp, norm_t)
    assert np.all(ref < 0)  # (every house is penalised at some tick: the bound is relative)
    err = np.abs(got - ref)
    lim = RN.bound(TICKS, ref)
    print(f"win={win} gamma={gamma}: max err / bound = {np.max(err / lim):.3f}")
    assert np.all(err <= lim)
    # ... and chained calls (70 ticks, then 37 more from the same trajectory's start) stay inside it
    ref2 = RN.row_form(ref, RN.weights(w[TICKS], gamma, 37), rows[:37])
    got2 = RN.window_form(got, RN.weights(w[TICKS], gamma, 37), pen[:37], sig[:37], win, alpha_temp, norm_t)
    assert np.all(np.abs(got2 - ref2) <= RN.bound(TICKS + 37, ref2))


def test_argument_errors_without_gpu():
    """mdr_rollout_returns checks its arguments before any HIP call: MDR_EARG on a CPU box, each
    refusal naming its argument."""
    from mdr_amd import _lib

    lib = _lib.load()
    EARG = -1
    ticks = (_lib.mdr_tick * 2)()
    w = (C.c_double * 2)(1.0, 1.0)
    ret = C.c_void_p(8)  # (never dereferenced: the checks come first)
    tp, wp = C.cast(ticks, C.c_void_p), C.cast(w, C.c_void_p)

    def call(ctx=None, n=2, t=tp, action=None, mode=_lib.ACT_RANDOM, weights=wp, returns=ret):
        rc = lib.mdr_rollout_returns(ctx, n, t, action, 0, mode, weights, returns, None, None)
        return rc, lib.mdr_last_error().decode()

    for kw, word in (({"n": 0}, "n_ticks"), ({"n": -3}, "n_ticks"), ({"weights": None}, "weights"),
                     ({"returns": None}, "returns"), ({"mode": 99}, "action source"),
                     ({"mode": _lib.ACT_BUFFER}, "without actions"), ({"t": None}, "bad argument"),
                     ({}, "bad argument")):  # (the last: a null context)
        rc, msg = call(**kw)
        assert rc == EARG and "mdr_rollout_returns" in msg and word in msg, (kw, rc, msg)
    assert lib.mdr_rollout_returns_path(None, _lib.ACT_RANDOM) == EARG


class _FakeShard:
    device = "cpu"


def _bare_env(n=4):
    """An Environment object with just what rollout_returns' argument checks read (no device)."""
    from mdr_amd.environment import Environment

    env = object.__new__(Environment)
    env._comm, env._shard, env._n_local = None, _FakeShard(), n
    return env


def test_python_value_errors_without_gpu():
    import torch

    env = _bare_env()
    good = torch.zeros(4, dtype=torch.float64)
    for kw in ({"n_ticks": 0}, {"n_ticks": -1}, {"gamma": 0.0}, {"gamma": 1.5}, {"gamma": -0.5}, {"gamma": float("nan")},
               {"weight0": float("inf")}, {"weight0": float("nan")},
               {"returns": torch.zeros(4, dtype=torch.float32)}, {"returns": torch.zeros(5, dtype=torch.float64)},
               {"returns": torch.zeros((1, 4), dtype=torch.float64)}, {"returns": np.zeros(4)},
               {"returns": torch.zeros(4, dtype=torch.float64, device="meta")}):
        args = {"n_ticks": 3, "returns": good, "gamma": 1.0, "weight0": 1.0}
        args.update(kw)
        with pytest.raises(ValueError):
            env.rollout_returns(**args)
    with pytest.raises(ValueError):
        env.rollout_returns(3, good, action_mode="buffer")
    env._comm = object()
    with pytest.raises(NotImplementedError):
        env.rollout_returns(3, good)


def test_controller_returns_refuses_before_any_device_work():
    from mdr_amd import services

    with pytest.raises(ValueError):
        services.controller_returns(None, "greedy", 5)
    with pytest.raises(ValueError):
        services.controller_returns(None, "random", 0)
