"""The inputs of tests/test_env_batch_gpu.py tell the clusters of a batch apart, and the argument
errors of ``EnvBatch`` that need no device.

Under the oracle (oracle/env_np.OracleEnv), at every GPU shape with N_c >= 50 and both bang-bang
controllers: the clusters' per-tick powers are pairwise distinct on at least four fifths of the ticks
(36 of 45), so a kernel that mixed two clusters' counts or drivers could not pass the GPU test's ==;
and every cluster has "on" requests refused by the lockout, so the FSM is exercised.  Measured here with
seeds 8, 9, ...: distinct on 43-45 of 45 ticks at N_c = 50, 129, 1,000 and on 12 of 12 at 1,024; refused
requests 69-13,162 per cluster over 45 ticks.  The full block (2, 1024, 12) runs 12 ticks, 8 s past one
lockout (L = 40 s, dt = 4 s): under the bang-bang form both clusters have refusals (213, 876), under the
deadband form, which holds most houses inside the band, only one of the two (0, 3) — so there the
assertion is that the shape has refusals, not that every cluster has; the GPU test runs both forms at
that shape."""
import random

import numpy as np
import pytest

import batch_inputs as B
from bangbang_inputs import CTRLS
from oracle import env_np as O


def oracle_run(n, seed, ticks, ctrl):
    """(per-tick cluster power, refused 'on' requests) of one cluster under the oracle and the controller."""
    props = B.props(n)
    ora = O.OracleEnv(props, random.Random(seed))
    db = props.cluster_prop.house_prop.deadband
    tg = ora.pop["target"]
    P, refused = [], 0
    for _ in range(ticks):
        on0 = ora.on.copy()
        a = O.bangbang(ora.T, tg) if ctrl == "bangbang" else O.deadband_bangbang(ora.T, tg, db, ora.on)
        o, _ = ora.step(a)
        on1 = np.asarray(o["on"], bool)
        refused += int(np.sum(np.asarray(a, bool) & ~on0 & ~on1))
        P.append(float(ora.P))
    return np.array(P), refused


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("n_envs,n,ticks", [s for s in B.SHAPES if s[1] >= 50])
def test_shapes_tell_clusters_apart(n_envs, n, ticks, ctrl):
    runs = [oracle_run(n, s, ticks, ctrl) for s in B.seeds(n_envs)]
    P = np.stack([r[0] for r in runs])  # [E, ticks]
    distinct = sum(len(set(P[:, t])) == n_envs for t in range(ticks))
    refused = [r[1] for r in runs]
    print(f"E={n_envs} n={n} ticks={ticks} {ctrl}: distinct on {distinct}/{ticks}, refused {refused}")
    assert distinct * 45 >= 36 * ticks
    if ticks >= 45 or ctrl == "bangbang":
        assert all(r > 0 for r in refused)
    else:  # 12 ticks (48 s against a lockout of 40 s): the deadband form holds most houses inside the band
        assert any(r > 0 for r in refused)


def test_python_refusals_need_no_device():
    from mdr_amd.batch import EnvBatch, batch_stride, check_batch_props

    assert [batch_stride(n) for n in (1, 50, 128, 129, 1000, 1024)] == [128, 128, 128, 256, 1024, 1024]
    with pytest.raises(ValueError, match="1024"):
        EnvBatch(B.props(1025), 2)
    with pytest.raises(ValueError, match="n_envs"):
        EnvBatch(B.props(50), 0)
    for pmode in ("common_L2", "common_max_error", "mixture"):
        with pytest.raises(NotImplementedError, match="individual_L2"):
            EnvBatch(B.props(50, {"reward_prop.penalty_props.mode": pmode}), 2)
    for cmode in ("closed_groups", "random_fixed", "neighbours_2D"):
        with pytest.raises(NotImplementedError, match="neighbours"):
            EnvBatch(B.props(50, {"cluster_prop.agents_comm_prop.mode": cmode}), 2)
    with pytest.raises(NotImplementedError, match="random_sample"):
        EnvBatch(B.props(50, {"cluster_prop.agents_comm_prop.mode": "random_sample"}), 2)
    with pytest.raises(NotImplementedError, match="interpolation"):
        EnvBatch(B.props(50, {"power_grid_prop.base_power_props.mode": "interpolation"}), 2)
    with pytest.raises(NotImplementedError, match="communicator"):
        EnvBatch(B.props(50), 2, comm=object())
    with pytest.raises(NotImplementedError, match="population"):
        EnvBatch(B.props(50), 2, population="synthetic")
    with pytest.raises(ValueError, match="seeds"):
        EnvBatch(B.props(50), 3, seeds=[1, 2])
    check_batch_props(B.props(1024), 1)  # (the accepted configuration draws nothing and needs no device)


def test_exported():
    import mdr_amd

    assert "EnvBatch" in mdr_amd.__all__
    from mdr_amd.batch import EnvBatch

    assert mdr_amd.EnvBatch is EnvBatch


def test_c_abi_argument_errors_without_gpu():
    """The batch entry points validate their arguments before any HIP call."""
    from mdr_amd import _lib

    lib = _lib.load()
    assert [lib.mdr_batch_stride(n) for n in (-3, 0, 1, 128, 129, 1000, 1024)] == [0, 0, 128, 128, 256, 1024, 1024]
    assert lib.mdr_batch_set(None, 1, 1, None) == -1
    assert lib.mdr_batch_rollout(None, 1, None, None, 0, 1, None, 0, None, None) == -1
    assert lib.mdr_batch_obs(None, None, None, None, None, None) == -1
