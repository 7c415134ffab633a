"""The actor kernels' Q head (csrc/mdr_actor.hip actor_head; mdr_actor_set_head, DeviceActor(head="q"))
against references that do not come from the kernel:

  * the Q rows against torch on the kernel's own obs rows.  fp32 forms: the project's rule for the
    fp32 probabilities carried over to the Q-values — no further from the float64 forward than twice
    torch-fp32's own error + 2e-7 max(1, max |q|).  bf16x3 / bf16: max |q - q_torch| / max(1, max |q|)
    below Q_RTOL, which is 4x the largest value measured over this file's cases on an MI355X
    (bf16x3 measured 9.8e-5, bf16 2.67e-2, both at 4,099 houses with max |q| 14.2; the reference of
    that number is torch fp32, never the kernel);
  * the action, replayed exactly from the kernel's own Q row and the house's Philox word
    (tests/qhead_np.py: explore iff u < eps, random action = bit 0 of the word, else torch.argmax's
    rule), prob == q[i, action] bitwise;
  * at eps 0 the action against torch's argmax, except where torch's own |q1 - q0| is below twice the
    tolerance above (at most 1 % of the houses: weights x3, the net's seed chosen on the CPU so that
    torch alone stays inside that cap, tests/test_dqn_cpu.py);
  * the ON counts of the chosen actions (count_next) through step_tensor against a twin env that
    counts them with mdr_power_counts;
  * the default-layout and generic fused kernels, many tiles per wave (one block, 2,085 houses), the
    layer chain (k_actor_head), and tiles that take the fp16-split form's fp32 fallback;
  * ties and NaNs; the graph-captured rollout, epsilon changes between replays of one graph, and a
    softmax actor on the same env afterwards.
"""
import json
import random

import numpy as np
import pytest

import golden_util as gu
import qhead_np as QH

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "fp32_bf16", "bf16x3", "bf16")
FP32S = ("fp32", "fp32_bf16")
Q_RTOL = QH.Q_RTOL  # max |q - q_torch| / max(1, max |q|): 4 x the measured maxima (module docstring)
SEED = 0x5EED_0000_1234_5678
SAT = 0x3FFFFFFF  # hvac word: off, unlocked, seconds-since-off saturated (beyond the fp16 path's range)


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def q_actor(env, net, precision, eps=0.0):
    from mdr_amd.actor import DeviceActor

    if precision == "fp32_bf16":
        return DeviceActor(env, net, precision="fp32", fp32_form="bf16_split3", head="q", epsilon=eps)
    return DeviceActor(env, net, precision=precision, head="q", epsilon=eps)


def make_env(torch, n, extra=None, ticks=5, generic=False):
    from mdr_amd.environment import Environment

    ov = {"cluster_prop.nb_agents": n, "power_grid_prop.signal_properties.mode": "sinusoidals"}
    ov.update(extra or {})
    env = Environment(gu.props_from_overrides(ov), rng=random.Random(5), seed=SEED)
    rs = np.random.RandomState(7)
    for _ in range(ticks):
        env.step_tensor(torch.from_numpy(rs.randint(0, 2, n).astype(np.uint8)).to("cuda"))
    env.shard.set_option("actor_generic", int(generic))
    return env


def scaled_qnet(torch, n_in, scale=3.0, seed=3, layers=(100, 100)):
    from mdr_amd.actor import make_qnet

    net = make_qnet(n_in, 2, layers, seed=seed)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(scale)
    return net.to("cuda")


def calibrated_qnet(torch, env, seed=5):
    """A Q-net whose first layer folds the observation's normalisation in (golden_util.calibrated_actor,
    output layer x3), with the second output's bias moved so that the median of q1 - q0 over the env's
    current houses is 0: both actions occur at any cluster size, so the argmax is not trivial."""
    from mdr_amd.actor import make_qnet

    F = env.obs_spec().n_feat
    obs = env.obs_tensor()
    a = gu.calibrated_actor(F, obs.abs().amax(0).double().cpu().numpy(), seed=seed)
    net = make_qnet(F, seed=None)
    net.load_state_dict(a.state_dict())
    net = net.to("cuda")
    with torch.no_grad():
        q = net(obs)
        net.fc[-1].bias[1] -= (q[:, 1] - q[:, 0]).median()
    return net


def forward64(net, x):
    import torch

    for i, l in enumerate(net.fc):
        x = torch.nn.functional.linear(x, l.weight.double(), l.bias.double())
        if i + 1 < len(net.fc):
            x = torch.relu(x)
    return x


def select(torch, env, da, count_next=False):
    n, F = env.n_local, env.obs_spec().n_feat
    q = torch.full((n, 2), float("nan"), dtype=torch.float32, device="cuda")
    obs = torch.full((n, F), float("nan"), dtype=torch.float32, device="cuda")
    act = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    qa = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    tick = env._tick
    da.select_actions(action=act, prob=qa, probs=q, obs_out=obs, count_next=count_next)
    return q, obs, act, qa, tick


def check_q_rows(torch, net, q, obs, precision, tag):
    """The Q rows against torch on the kernel's own obs rows; returns (torch's q, the absolute tolerance)."""
    with torch.no_grad():
        tq = net(obs).cpu().numpy()
        q64 = forward64(net, obs.double()).cpu().numpy()
    qn = q.cpu().numpy()
    assert np.all(np.isfinite(qn)), tag
    scale = max(1.0, float(np.abs(tq).max()))
    err = float(np.abs(qn - tq).max())
    if precision in FP32S:
        e_ours, e_torch = float(np.abs(qn - q64).max()), float(np.abs(tq - q64).max())
        tol = 2.0 * e_torch + 2e-7 * scale
        print(f"{tag} {precision}: vs float64 ours {e_ours:.3g}, torch fp32 {e_torch:.3g}, bound {tol:.3g}; "
              f"max |q| {scale:.3g}")
        assert e_ours <= tol, (tag, e_ours, e_torch)
    else:
        tol = Q_RTOL[precision] * scale
        print(f"{tag} {precision}: max |q - q_torch| / max(1, max |q|) = {err / scale:.3g} (bound "
              f"{Q_RTOL[precision]:.3g}); max |q| {scale:.3g}")
        assert err <= tol, (tag, err / scale)
    return tq, tol


def check_actions(env, q, act, qa, tick, eps):
    """The actions replayed from the kernel's own Q rows and the Philox words, exactly; prob == q[action]."""
    qn, a, p = q.cpu().numpy(), act.cpu().numpy(), qa.cpu().numpy()
    n = qn.shape[0]
    word = QH.actor_word(SEED, int(getattr(env, "_offset", 0)) + np.arange(n, dtype=np.uint64), tick)
    np.testing.assert_array_equal(a, QH.decide(qn, word, eps))
    np.testing.assert_array_equal(p.view(np.uint32), qn[np.arange(n), a].view(np.uint32))
    return word


def check_vs_torch_argmax(tq, act, tol, tag):
    a = act.cpu().numpy()
    near = np.abs(tq[:, 1] - tq[:, 0]) < 2.0 * tol
    share = float(near.mean())
    print(f"{tag}: {int(near.sum())} of {len(a)} houses within 2 x tol of a tie ({100 * share:.2f} %)")
    np.testing.assert_array_equal(a[~near], QH.greedy(tq)[~near])
    assert share <= 0.01, (tag, share)


def check_counts(torch, env, twin, act):
    """count_next of the launch == mdr_power_counts of the same actions (the twin's step_tensor)."""
    rb = twin.step_tensor(act.clone()).clone()
    assert torch.equal(env.step_tensor(act), rb)
    for k in ("t_air", "t_mass", "hvac"):
        assert torch.equal(getattr(env.shard, k), getattr(twin.shard, k)), k


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 37, 300, 4099])
def test_q_rows_and_greedy_sizes(torch_gpu, n, precision):
    torch = torch_gpu
    env, twin = make_env(torch, n), make_env(torch, n)
    net = scaled_qnet(torch, env.obs_spec().n_feat)
    da = q_actor(env, net, precision, eps=0.0)
    assert da.fused()
    ref_obs = env.obs_tensor().clone()
    q, obs, act, qa, tick = select(torch, env, da, count_next=True)
    assert torch.equal(obs, ref_obs)
    tq, tol = check_q_rows(torch, net, q, obs, precision, f"n={n}")
    check_actions(env, q, act, qa, tick, 0.0)
    np.testing.assert_array_equal(act.cpu().numpy(), QH.greedy(q.cpu().numpy()))  # eps 0: pure greedy, every house
    check_counts(torch, env, twin, act)
    assert da.status()["range_faults"] == 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", QH.ARGMAX_SIZES)
def test_greedy_vs_torch_argmax(torch_gpu, n, precision):
    """eps 0 against torch's argmax on the kernel's obs rows, except where torch's own |q1 - q0| is
    below twice the Q tolerance; those houses must be at most 1 % (weights x3).

    The net's seed (qhead_np.ARGMAX_SEED) is chosen on the CPU so that torch alone, on the oracle's
    obs rows, stays inside that cap for the widest (bf16) band: tests/test_dqn_cpu.py asserts it.  With
    the other tests' seed 3, 9 of 37 (24.3 %) and 173 of 300 (57.7 %) houses were inside the bf16 band
    (0.214 max(1, max |q|), about the spread of q1 - q0 of that net at those sizes), measured on an
    MI355X; the band is relative, so no weight scale moves that, the net has to."""
    torch = torch_gpu
    env = make_env(torch, n)
    net = scaled_qnet(torch, env.obs_spec().n_feat, seed=QH.ARGMAX_SEED)
    da = q_actor(env, net, precision, eps=0.0)
    q, obs, act, qa, tick = select(torch, env, da)
    tq, tol = check_q_rows(torch, net, q, obs, precision, f"n={n}")
    check_actions(env, q, act, qa, tick, 0.0)
    check_vs_torch_argmax(tq, act, tol, f"n={n} {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("eps", [0.25, 1.0])
def test_epsilon_greedy_replayed(torch_gpu, eps, precision):
    torch = torch_gpu
    n = 4099
    env, twin = make_env(torch, n), make_env(torch, n)
    net = scaled_qnet(torch, env.obs_spec().n_feat)
    da = q_actor(env, net, precision, eps=eps)
    q, obs, act, qa, tick = select(torch, env, da, count_next=True)
    check_q_rows(torch, net, q, obs, precision, f"eps={eps}")
    word = check_actions(env, q, act, qa, tick, eps)
    ex = QH.explore(word, eps)
    assert abs(ex.mean() - eps) <= 5 * np.sqrt(eps * (1 - eps) / n) + 1e-12, ex.mean()
    if eps == 1.0:
        np.testing.assert_array_equal(act.cpu().numpy(), (word & 1).astype(np.uint8))
    else:  # the explored houses' actions differ from the greedy ones somewhere, and are fair coin flips
        a = act.cpu().numpy()
        assert np.any(a[ex] != QH.greedy(q.cpu().numpy())[ex])
        assert abs(a[ex].mean() - 0.5) <= 5 * 0.5 / np.sqrt(ex.sum())
    check_counts(torch, env, twin, act)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("layout", ["def", "generic"])
def test_many_tiles_per_wave(torch_gpu, layout, precision):
    """One block, 2,085 houses: every wave walks 5 to 9 tiles, so the odd tiles take their Philox words
    (uniform and action bit) from the previous tile's pass."""
    torch = torch_gpu
    n = 2085
    env, twin = (make_env(torch, n, generic=(layout == "generic")) for _ in range(2))
    try:
        net = calibrated_qnet(torch, env)
        da = q_actor(env, net, precision, eps=0.25)
        assert da.fused()
        env.shard.set_option("actor_grid", 1)
        q, obs, act, qa, tick = select(torch, env, da, count_next=True)
        assert torch.equal(obs, twin.obs_tensor())
        tq, tol = check_q_rows(torch, net, q, obs, precision, f"{layout} grid 1")
        check_actions(env, q, act, qa, tick, 0.25)
        check_counts(torch, env, twin, act)
        da.set_epsilon(0.0)
        q, obs, act, qa, tick = select(torch, env, da)
        check_actions(env, q, act, qa, tick, 0.0)
        tq, tol = check_q_rows(torch, net, q, obs, precision, f"{layout} grid 1 (tick 2)")
        a = act.cpu().numpy()
        assert 0.05 < a.mean() < 0.95  # (both actions occur: the argmax is not trivial)
        near = np.abs(tq[:, 1] - tq[:, 0]) < 2.0 * tol
        print(f"{layout} {precision}: {int(near.sum())} of {n} houses within 2 x tol of a tie")
        np.testing.assert_array_equal(a[~near], QH.greedy(tq)[~near])
    finally:
        for e in (env, twin):
            e.shard.set_option("actor_grid", 0)
            e.shard.set_option("actor_generic", 0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chain_head(torch_gpu, precision):
    """A three-hidden-layer net runs the layer chain: k_actor_head's Q head."""
    torch = torch_gpu
    n = 300
    env, twin = make_env(torch, n), make_env(torch, n)
    net = scaled_qnet(torch, env.obs_spec().n_feat, scale=2.0, layers=(64, 48, 32))
    da = q_actor(env, net, precision, eps=0.25)
    assert not da.fused()
    q, obs, act, qa, tick = select(torch, env, da, count_next=True)
    check_q_rows(torch, net, q, obs, precision, "chain")
    check_actions(env, q, act, qa, tick, 0.25)
    check_counts(torch, env, twin, act)
    da.set_epsilon(0.0)
    q, obs, act, qa, tick = select(torch, env, da)
    check_actions(env, q, act, qa, tick, 0.0)
    np.testing.assert_array_equal(act.cpu().numpy(), QH.greedy(q.cpu().numpy()))


@pytest.mark.parametrize("grid", [0, 1])
def test_fp16_split_fallback_tiles(torch_gpu, grid):
    """Houses off for ~34 years send their tiles to the fp16-split form's scalar fp32 fallback (provoked
    as tests/test_actor_gpu.py test_actor_fp16_split_range does); with one block the tiles are deferred
    inside a wave's loop and run after it with fresh Philox words.  Their Q rows and actions obey the
    same rules as every other tile's."""
    torch = torch_gpu
    n = 2085
    env, twin = make_env(torch, n), make_env(torch, n)
    try:
        for e in (env, twin):
            e.shard.hvac[100:132] = SAT
            e.shard.hvac[n - 5:n] = SAT
        absmax = env.obs_tensor().abs().amax(0).double().cpu().numpy()
        assert absmax.max() > 65504.0
        net = gu.calibrated_actor(env.obs_spec().n_feat, absmax, seed=4)
        from mdr_amd.actor import make_qnet

        qnet = make_qnet(env.obs_spec().n_feat, seed=None)
        qnet.load_state_dict(net.state_dict())
        qnet = qnet.to("cuda")
        da = q_actor(env, qnet, "fp32", eps=0.25)
        env.shard.set_option("actor_grid", grid)
        da.status()
        q, obs, act, qa, tick = select(torch, env, da, count_next=True)
        st = da.status()
        assert st["kernel_prec"] == 4 and st["exact"] >= 2 and st["range_faults"] == 0, st
        tq, tol = check_q_rows(torch, qnet, q, obs, "fp32", f"fallback grid {grid}")
        check_actions(env, q, act, qa, tick, 0.25)
        check_counts(torch, env, twin, act)
        da.set_epsilon(0.0)
        q, obs, act, qa, tick = select(torch, env, da)
        check_actions(env, q, act, qa, tick, 0.0)
        rows = np.r_[100:132, n - 5:n]
        np.testing.assert_array_equal(act.cpu().numpy()[rows], QH.greedy(q.cpu().numpy())[rows])
    finally:
        env.shard.set_option("actor_grid", 0)


@pytest.mark.parametrize("layers", [(100, 100), (64, 48, 32)])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_ties_and_nans(torch_gpu, layers, precision):
    """A zero output layer gives q0 == q1 for every house (a tie: action 0); a NaN output bias gives NaN
    Q-values: NaN counts as the maximum and the first one wins, as torch.argmax."""
    torch = torch_gpu
    n = 300
    env = make_env(torch, n)
    net = scaled_qnet(torch, env.obs_spec().n_feat, scale=1.0, layers=layers)
    da = q_actor(env, net, precision, eps=0.0)
    assert da.fused() == (len(layers) == 2)
    nan = float("nan")
    for b3, want in (((0.0, 0.0), 0), ((0.5, 0.5), 0), ((nan, 0.0), 0), ((0.0, nan), 1), ((nan, nan), 0),
                     ((0.0, 1.0), 1)):
        with torch.no_grad():
            net.fc[-1].weight.zero_()
            net.fc[-1].bias.copy_(torch.tensor(b3))
        da.load_weights()
        q, obs, act, qa, tick = select(torch, env, da)
        qn = q.cpu().numpy()
        np.testing.assert_array_equal(qn, np.tile(np.array(b3, np.float32), (n, 1)))
        assert int(torch.argmax(torch.tensor(b3))) == want
        np.testing.assert_array_equal(act.cpu().numpy(), np.full(n, want, np.uint8))
        np.testing.assert_array_equal(qa.cpu().numpy(), qn[:, want])
    da.status()  # (the fp16-split form counted the non-finite rows: cleared)


def test_graph_rollout_epsilon_and_heads(torch_gpu):
    """rollout(16) with the Q head == the select_actions -> step_tensor loop, bit for bit; epsilon
    changes between replays of the one captured graph; a softmax actor on the same env afterwards runs
    its own graph and still equals its own loop (the head is in the graph key and each actor applies
    its own head)."""
    from mdr_amd.actor import DeviceActor

    torch = torch_gpu
    n, T = 2049, 16
    env_a, env_b = make_env(torch, n, ticks=0), make_env(torch, n, ticks=0)
    net = scaled_qnet(torch, env_a.obs_spec().n_feat)
    # (every DeviceActor first: constructing one sets a context option, which drops the cached graphs)
    sa, sb = DeviceActor(env_a, net, precision="bf16x3"), DeviceActor(env_b, net, precision="bf16x3")
    da, db = q_actor(env_a, net, "bf16x3", eps=0.25), q_actor(env_b, net, "bf16x3", eps=0.25)
    rew = torch.empty((T, n), dtype=torch.float64, device="cuda")
    acts = torch.empty((T, n), dtype=torch.uint8, device="cuda")
    qas = torch.empty((T, n), dtype=torch.float32, device="cuda")
    g0 = env_a.shard.graph_info()
    explored = []
    for rep, eps in enumerate((0.25, 0.25, 1.0, 0.0)):
        da.set_epsilon(eps)
        db.set_epsilon(eps)
        tick0 = env_a._tick
        da.rollout(T, rewards=rew, actions=acts, probs=qas)
        gi = env_a.shard.graph_info()
        assert gi["actor_graphs"] == g0["actor_graphs"] + 1, (rep, gi)       # one capture, whatever epsilon
        assert gi["actor_launches"] == g0["actor_launches"] + rep + 1, (rep, gi)
        word = QH.actor_word(SEED, np.arange(n, dtype=np.uint64), tick0)
        for t in range(T):
            a, p = db.select_actions(count_next=True)
            r = env_b.step_tensor(a)
            assert torch.equal(a, acts[t]) and torch.equal(p, qas[t]) and torch.equal(r, rew[t]), (rep, t)
        a0 = acts[0].cpu().numpy()
        if eps == 1.0:
            np.testing.assert_array_equal(a0, (word & 1).astype(np.uint8))
        explored.append(float(np.mean(a0 == (word & 1))))
    assert explored[2] == 1.0 and explored[3] < 0.75  # (eps 0: the greedy action matches a coin flip about half the time)
    # a softmax actor over the same weights on the same env: its own graph, its own head
    for rep in range(2):
        sa.rollout(T, rewards=rew, actions=acts, probs=qas)
        gi = env_a.shard.graph_info()
        assert gi["actor_graphs"] == g0["actor_graphs"] + 2, gi
        for t in range(T):
            a, p = sb.select_actions(count_next=True)
            r = env_b.step_tensor(a)
            assert torch.equal(a, acts[t]) and torch.equal(p, qas[t]) and torch.equal(r, rew[t]), (rep, t)
        assert float(qas.min()) >= 0.0 and float(qas.max()) <= 1.0  # probabilities again
    # ... and back: the Q actor re-applies its head and replays its graph
    da.set_epsilon(0.25)
    db.set_epsilon(0.25)
    da.rollout(T, rewards=rew, actions=acts, probs=qas)
    assert env_a.shard.graph_info()["actor_graphs"] == g0["actor_graphs"] + 2
    for t in range(T):
        a, p = db.select_actions(count_next=True)
        r = env_b.step_tensor(a)
        assert torch.equal(a, acts[t]) and torch.equal(p, qas[t]) and torch.equal(r, rew[t]), t
    for k in ("t_air", "t_mass", "hvac"):
        assert torch.equal(getattr(env_a.shard, k), getattr(env_b.shard, k)), k


def test_set_head_errors_with_context(torch_gpu):
    """mdr_actor_set_head on a live context: bad arguments are MDR_EARG and change nothing."""
    from mdr_amd import _lib as L

    torch = torch_gpu
    env = make_env(torch, 37, ticks=0)
    sh = env.shard
    for head, eps in ((2, 0.5), (1, -0.1), (1, 1.5), (0, float("nan"))):
        assert sh.lib.mdr_actor_set_head(sh.ctx, head, eps, sh.stream()) == -1
    with pytest.raises(KeyError):
        sh.actor_set_head("argmax", 0.0)
    assert sh.actor_head == ("softmax", 0.0)


def test_golden_argmax_actions(torch_gpu):
    """The reference DQN's select_actions at epsilon 0 on the fixture's 64 recorded states
    (tests/golden/dqn.npz), at the torch level on the GPU and through the head's decision rule."""
    from mdr_amd.actor import make_qnet

    torch = torch_gpu
    g = gu.load("dqn.npz")
    meta = json.loads(bytes(g["meta_json"]).decode())
    net = make_qnet(meta["num_state"], seed=None)
    u = meta["updates"] - 1
    net.load_state_dict({k: torch.from_numpy(g[f"u{u}_policy_{k}"]) for k in net.state_dict()})
    net = net.to("cuda")
    with torch.no_grad():
        q = net(torch.from_numpy(g["sel_states"]).to("cuda")).cpu().numpy()
    np.testing.assert_allclose(q, g["sel_q"], rtol=1e-5, atol=1e-6)
    clear = np.abs(g["sel_q"][:, 1] - g["sel_q"][:, 0]) > 1e-5
    assert clear.sum() >= 60
    np.testing.assert_array_equal(QH.greedy(q)[clear], g["sel_actions"][clear])
    np.testing.assert_array_equal(q.argmax(1)[clear], g["sel_actions"][clear])
