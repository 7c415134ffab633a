"""CPU checks of the DQN layers: the mdr_actor_set_head entry point, the reference DQN fixture
(tests/golden/dqn.npz, made by tests/golden/make_golden_dqn.py from dqn.py:54-194) against
``make_qnet`` / ``dqn_update`` / the reference sampler, the replay ring's slot arithmetic, the
epsilon schedules and the NumPy restatement of the Q head's decision rule (no GPU calls)."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest

import golden_util as gu
import philox_np as PH
import qhead_np as QH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    g = gu.load("dqn.npz")
    return g, json.loads(bytes(g["meta_json"]).decode())


# ------------------------------------------------------------------------------------ C ABI
def test_set_head_declared_exported_and_bound():
    from mdr_amd import _lib

    with open(os.path.join(ROOT, "include", "mdr.h")) as f:
        src = f.read()
    assert re.search(r"^int\s+mdr_actor_set_head\s*\(mdr_ctx\* ctx, int head, float epsilon, void\* stream\);", src, re.M)
    assert re.search(r"MDR_HEAD_SOFTMAX\s*=\s*0\s*,\s*MDR_HEAD_Q\s*=\s*1", src)
    assert "dqn.py:93-105" in src and "rl_controllers.py:143-159" in src
    lib = _lib.load()
    assert hasattr(lib, "mdr_actor_set_head")
    assert _lib.SIGNATURES["mdr_actor_set_head"] == (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p])
    assert _lib.HEADS == {"softmax": 0, "q": 1}


def test_set_head_argument_errors_without_gpu():
    """Validation comes before any HIP call: MDR_EARG on a CPU box.  The bad head and the bad
    epsilons are given a non-null context pointer that is never dereferenced for them."""
    from mdr_amd import _lib

    lib = _lib.load()
    assert lib.mdr_actor_set_head(None, 1, 0.5, None) == -1
    assert b"mdr_actor_set_head" in lib.mdr_last_error()
    dummy = (C.c_char * 65536)()  # stands in for a context: the checks below fail before it is read
    ctx = C.cast(dummy, C.c_void_p)
    for head in (-1, 2, 7):
        assert lib.mdr_actor_set_head(ctx, head, 0.5, None) == -1
        assert b"head" in lib.mdr_last_error()
    for eps in (-0.1, 1.5, float("nan")):
        for head in (0, 1):
            assert lib.mdr_actor_set_head(ctx, head, eps, None) == -1
            assert b"epsilon" in lib.mdr_last_error()
        assert lib.mdr_actor_set_head(None, 1, eps, None) == -1


def test_lazy_reexports():
    import mdr_amd
    from mdr_amd import actor, dqn, replay

    assert mdr_amd.DeviceDQN is dqn.DeviceDQN and mdr_amd.DQNConfig is dqn.DQNConfig
    assert mdr_amd.ReplayStore is replay.ReplayStore and mdr_amd.make_qnet is actor.make_qnet
    with pytest.raises(AttributeError):
        mdr_amd.no_such_name


def test_device_actor_head_arguments():
    """Head and epsilon are validated before the env is touched."""
    from mdr_amd.actor import DeviceActor

    with pytest.raises(ValueError, match="head"):
        DeviceActor(None, None, head="argmax")
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            DeviceActor(None, None, head="q", epsilon=eps)


# ------------------------------------------------------------------------------------ fixture
def test_config_defaults_are_dqn_properties(gold):
    from mdr_amd.dqn import DQNConfig

    _, meta = gold
    cfg = DQNConfig()
    assert (cfg.network_layers, cfg.buffer_capacity, cfg.batch_size) == ([100, 100], 524288, 256)
    for k in ("gamma", "tau", "lr", "epsilon_decay", "min_epsilon"):
        assert getattr(cfg, k) == meta[k], k


def test_make_qnet_is_reference_init(gold):
    from mdr_amd.actor import make_qnet

    g, meta = gold
    net = make_qnet(meta["num_state"], seed=meta["seed"])
    sd = net.state_dict()
    assert sorted(sd) == sorted(k[len("init_policy_"):] for k in g.files if k.startswith("init_policy_"))
    for k, v in sd.items():
        np.testing.assert_array_equal(v.numpy(), g["init_policy_" + k])


def _memory(g, meta):
    """The reference deque after the fixture's pushes, oldest first: (s, a, r, s2) arrays."""
    T, N, cap = meta["T"], meta["N"], meta["buffer_capacity"]
    pushes = [(t, i) for t in range(T) for i in range(N)][-cap:]
    t = np.array([p[0] for p in pushes])
    i = np.array([p[1] for p in pushes])
    return (g["states"][t, i], g["actions"][t, i], g["rewards"][t, i].astype(np.float32), g["states"][t + 1, i])


def test_reference_sampler_draws_recorded_indices(gold):
    from mdr_amd.dqn import reference_sample

    g, meta = gold
    random.seed(meta["update_seed"])
    for u in range(meta["updates"]):
        assert reference_sample(meta["buffer_capacity"], meta["batch_size"]) == list(g["indices"][u])
    assert random.random() == float(g["after_replay"])


def test_dqn_update_reproduces_reference(gold):
    import torch

    from mdr_amd.actor import make_qnet
    from mdr_amd.dqn import DQNConfig, dqn_update

    g, meta = gold
    cfg = DQNConfig(batch_size=meta["batch_size"], buffer_capacity=meta["buffer_capacity"])
    torch.manual_seed(meta["seed"])
    policy = make_qnet(meta["num_state"], seed=None)
    target = make_qnet(meta["num_state"], seed=None)
    target.load_state_dict(policy.state_dict())
    opt = torch.optim.Adam(policy.parameters(), cfg.lr)
    s, a, r, s2 = (torch.from_numpy(np.ascontiguousarray(x)) for x in _memory(g, meta))
    for u in range(meta["updates"]):
        idx = torch.from_numpy(g["indices"][u])
        loss = dqn_update(policy, target, opt, s[idx], a[idx], r[idx], s2[idx], cfg)
        print(f"update {u}: loss {float(loss):.9g} (reference {float(g['losses'][u]):.9g})")
        np.testing.assert_allclose(float(loss), g["losses"][u], rtol=1e-6, atol=0)
        for name, net in (("policy", policy), ("target", target)):
            for k, v in net.state_dict().items():
                np.testing.assert_allclose(v.numpy(), g[f"u{u}_{name}_{k}"], rtol=1e-5, atol=1e-6, err_msg=f"u{u} {name} {k}")
    # the policy moved, the target followed by tau
    assert np.abs(policy.state_dict()["fc.0.weight"].numpy() - g["init_policy_fc.0.weight"]).max() > 1e-3
    assert np.abs(target.state_dict()["fc.0.weight"].numpy() - g["init_policy_fc.0.weight"]).max() < 1e-3


def test_double_dqn_target_is_elementwise():
    """double=True: r_i + gamma Q_target(s'_i, argmax_a Q_policy(s'_i, a)), a float64 restatement."""
    import torch

    from mdr_amd.actor import make_qnet
    from mdr_amd.dqn import DQNConfig, dqn_update

    cfg = DQNConfig(batch_size=8)
    torch.manual_seed(3)
    policy, target = make_qnet(6, seed=None, layers=(16, 16)), make_qnet(6, seed=None, layers=(16, 16))
    rs = np.random.RandomState(0)
    s, s2 = (torch.from_numpy(rs.normal(0, 1, (8, 6)).astype(np.float32)) for _ in range(2))
    a = torch.from_numpy(rs.randint(0, 2, 8))
    r = torch.from_numpy(rs.normal(0, 1, 8).astype(np.float32))
    with torch.no_grad():
        p64, t64 = (make_qnet(6, seed=None, layers=(16, 16)).double() for _ in range(2))
        p64.load_state_dict({k: v.double() for k, v in policy.state_dict().items()})
        t64.load_state_dict({k: v.double() for k, v in target.state_dict().items()})
        na = p64(s2.double()).argmax(1, keepdim=True)
        want = r.double() + cfg.gamma * t64(s2.double()).gather(1, na).squeeze(1)
        q = p64(s.double()).gather(1, a.view(-1, 1)).squeeze(1)
        d = (q - want).abs()
        want_loss = torch.where(d < 1, 0.5 * d * d, d - 0.5).mean()
        t_before = {k: v.clone() for k, v in target.state_dict().items()}
    loss = dqn_update(policy, target, torch.optim.Adam(policy.parameters(), cfg.lr), s, a, r, s2, cfg, double=True)
    np.testing.assert_allclose(float(loss), float(want_loss), rtol=1e-5)
    for k, v in target.state_dict().items():  # ... and the soft target update the reference's DDQN lacks
        np.testing.assert_allclose(v.numpy(), ((1 - cfg.tau) * t_before[k] + cfg.tau * policy.state_dict()[k]).numpy(),
                                   rtol=1e-6, atol=1e-8)


def test_epsilon_schedules(gold):
    from mdr_amd.dqn import DQNConfig, next_epsilon

    g, _ = gold
    cfg = DQNConfig()
    assert next_epsilon(1.0, cfg, "reference") == float(g["epsilon_final"]) == 0.99998
    assert next_epsilon(0.3, cfg, "reference") == 0.99998  # (constant after the first update: dqn.py:179-181)
    e = 1.0
    for _ in range(3):
        e = next_epsilon(e, cfg, "multiplicative")
    assert e == 1.0 * 0.99998 * 0.99998 * 0.99998
    assert next_epsilon(0.0100001, cfg, "multiplicative") == 0.01
    assert next_epsilon(1.0, DQNConfig(epsilon_decay=0.001), "reference") == 0.01
    with pytest.raises(ValueError):
        next_epsilon(1.0, cfg, "linear")


# ------------------------------------------------------------------------------------ ring
def test_tick_ring_arithmetic():
    from mdr_amd.replay import TickRing

    r = TickRing(3)
    assert (r.slots, r.head, r.count, r.valid_slots()) == (4, 0, 0, [])
    assert r.segments(2) == [(0, 2)]
    r.commit(2)  # ticks in slots 0, 1; the trailing snapshot in slot 2
    assert (r.head, r.count, r.oldest, r.valid_slots()) == (2, 2, 0, [0, 1])
    assert [r.next_slot(s) for s in r.valid_slots()] == [1, 2]
    assert r.segments(3) == [(2, 2), (0, 1)]  # a wrap in the middle of a collect: two runs
    r.commit(3)  # ticks now in slots 2, 3, 0; trailing in 1, which held the tick before the oldest kept
    assert (r.head, r.count, r.oldest) == (1, 3, 2)
    assert r.valid_slots() == [2, 3, 0]  # oldest first; slot 1 (trailing) is not a transition
    assert [r.next_slot(s) for s in r.valid_slots()] == [3, 0, 1]
    assert r.segments(1) == [(1, 1)]
    r.commit(1)  # the trailing slot moves on to 2: the oldest tick (slot 2) is dropped, like deque(maxlen)
    assert (r.head, r.count, r.valid_slots()) == (2, 3, [3, 0, 1])
    assert r.segments(2) == [(2, 2)]  # ends exactly at the ring's end: one run, the head wraps to 0
    r.commit(2)
    assert (r.head, r.valid_slots()) == (0, [1, 2, 3])
    for bad in (0, 4):
        with pytest.raises(ValueError):
            r.segments(bad)
    with pytest.raises(ValueError):
        TickRing(0)
    r.clear()
    assert (r.head, r.count) == (0, 0)


# ------------------------------------------------------------------------------------ head rule
def test_head_rule_restatement(gold):
    import torch

    # argmax rows: plain, tie, NaN in either or both places, infinities
    q = np.array([[0.0, 1.0], [1.0, 0.0], [2.0, 2.0], [np.nan, 5.0], [5.0, np.nan], [np.nan, np.nan],
                  [-np.inf, np.inf], [np.inf, np.inf], [-0.0, 0.0]], np.float32)
    want = np.array([int(torch.argmax(torch.from_numpy(row))) for row in q], np.uint8)
    np.testing.assert_array_equal(QH.greedy(q), want)
    np.testing.assert_array_equal(want, [1, 0, 0, 0, 1, 0, 1, 0, 0])
    # the fixture's recorded select_actions at epsilon 0
    g, _ = gold
    np.testing.assert_array_equal(QH.greedy(g["sel_q"]), g["sel_actions"])
    # the word: the same block as the softmax head's uniform
    gid = np.arange(5000, dtype=np.uint64) + np.uint64(12345)
    w = QH.actor_word(77, gid, 9)
    np.testing.assert_array_equal(QH.word_u01f(w), PH.u01f(77, gid, 9))
    qq = np.tile(np.array([[1.0, 0.0]], np.float32), (5000, 1))  # greedy: always 0
    np.testing.assert_array_equal(QH.decide(qq, w, 0.0), np.zeros(5000, np.uint8))
    np.testing.assert_array_equal(QH.decide(qq, w, 1.0), (w & 1).astype(np.uint8))
    ex = QH.explore(w, 0.25)
    assert abs(ex.mean() - 0.25) < 5 * np.sqrt(0.25 * 0.75 / 5000)
    a = QH.decide(qq, w, 0.25)
    np.testing.assert_array_equal(a[~ex], 0)
    np.testing.assert_array_equal(a[ex], (w[ex] & 1).astype(np.uint8))
    assert abs(a[ex].mean() - 0.5) < 5 * 0.5 / np.sqrt(ex.sum())  # bit 0 is independent of the uniform


def test_argmax_net_keeps_torch_outside_the_band():
    """tests/test_qhead_gpu.py test_greedy_vs_torch_argmax compares the kernel's greedy action with
    torch's argmax except where torch's own |q1 - q0| is below twice the Q tolerance, and caps those
    houses at 1 %.  Checked here before that test relies on it: torch fp32 alone, on the oracle's obs
    rows of the same states (the test's props, population seed and five ticks of random actions), keeps
    the x3-scaled net of seed ARGMAX_SEED inside the cap for the widest (bf16) band at every size."""
    import torch

    from mdr_amd.actor import make_qnet
    from oracle import env_np as O

    band = 2.0 * max(QH.Q_RTOL.values())
    for n in QH.ARGMAX_SIZES:
        props = gu.props_from_overrides({"cluster_prop.nb_agents": n,
                                         "power_grid_prop.signal_properties.mode": "sinusoidals"})
        env = O.OracleEnv(props, random.Random(5))
        rs = np.random.RandomState(7)
        for _ in range(5):
            env.step(rs.randint(0, 2, n).astype(np.uint8).astype(bool))
        obs = torch.from_numpy(np.asarray(env.norm_vector(), np.float32))
        net = make_qnet(obs.shape[1], 2, (100, 100), seed=QH.ARGMAX_SEED)
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(3.0)
            q = net(obs).numpy()
        gap = np.abs(q[:, 1] - q[:, 0])
        width = band * max(1.0, float(np.abs(q).max()))
        share = float((gap < width).mean())
        print(f"n={n}: max |q| {np.abs(q).max():.3g}, band {width:.3g}, smallest |q1 - q0| {gap.min():.3g}, "
              f"{100 * share:.2f} % inside")
        assert share <= 0.01, (n, share)
