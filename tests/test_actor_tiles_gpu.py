"""k_actor's per-wave tile loop against torch (csrc/mdr_actor.hip "the wave's tiles").

A launch has at most one block per CU, and wave v0 of the grid walks tiles v0, v0 + stride, ...: on a
full card a wave gets a second tile only above ~65,000 houses, so the other actor tests run one tile
per wave.  MDR_OPT_ACTOR_GRID ("actor_grid") caps the grid; with one block a wave of a 2,085-house
cluster carries 5 to 9 tiles and one of a 27,141-house cluster more than 64.  What the loop does from
its second tile on is pinned here against references that do not come from the kernel:

  * probabilities against torch fp32 on the kernel's own obs rows (4e-6 for the fp32 forms, 1e-4
    bf16x3, 3e-2 bf16: tests/test_actor_chain_gpu.py's tolerances), and for the fp32 forms no further
    from the float64 forward than twice torch's own fp32 error + 2e-7 (tests/test_actor_gpu.py);
  * the obs rows, bit-equal to the standalone obs kernel;
  * the sampled action, replayed exactly: action == (u01f(seed, goff + i, tick) >= probs[i, 0]) in
    float32 (tests/philox_np.py restates philox_u01f; the kernel draws two tiles' uniforms in one
    pass every other tile), and prob == probs[i, action];
  * the ON counts of the new actions (count_next) through step_tensor's reward, against a twin env
    fed the same actions through mdr_power_counts;
  * grid invariance, bit for bit (a self-comparison by design: the one-block launch is the one
    anchored to torch);
  * the fp16-split form's fp32 fallback for tiles that leave fp16's range, at any tile index of a
    wave (a wave's 65th and later out-of-range tiles used to take the previous tile's logits), at
    the range threshold (kActorF16Sso), from the hidden layer, and through a table topology's messages.
"""
import random

import numpy as np
import pytest

import golden_util as gu
import philox_np as P

pytestmark = pytest.mark.gpu

ATOL = {"fp32": 4e-6, "fp32_bf16": 4e-6, "bf16x3": 1e-4, "bf16": 3e-2}
FP32S = ("fp32", "fp32_bf16")
PRECISIONS = ("fp32", "fp32_bf16", "bf16x3", "bf16")
SEED = 0x5EED_0000_1234_5678  # (both words of the Philox key)
N_SMALL = 2085   # 65 full tiles + 5 houses: one block's waves carry 5 and 6 (12 waves) or 8 and 9 (8) tiles
N_LONG = 27141   # 848 full tiles + 5 houses: with one block of <= 12 waves, tile index >= 768 is j >= 64
SAT = 0x3FFFFFFF  # hvac word: off, unlocked, seconds-since-off saturated (2^30 - 1 s)
# every own-state feature + hvac messages: 88 features, 100 slots -> KS1 = 4 (tests/test_actor_gpu.py LAYOUTS)
KS1_4 = {"cluster_prop.message_prop.hvac": True, "state_prop.hvac": True, "state_prop.solar_gain": True,
         "state_prop.thermal": True}


def device_actor(env, actor, precision):
    """DeviceActor for a test precision: 'fp32_bf16' = precision fp32 in its three-way bf16 form."""
    from mdr_amd.actor import DeviceActor

    if precision == "fp32_bf16":
        return DeviceActor(env, actor, precision="fp32", fp32_form="bf16_split3")
    return DeviceActor(env, actor, precision=precision)


def _forward64(actor, x):
    """The actor's logits in float64 (network.py:29-33 without the softmax)."""
    import torch

    for i, l in enumerate(actor.fc):
        x = torch.nn.functional.linear(x, l.weight.double(), l.bias.double())
        if i + 1 < len(actor.fc):
            x = torch.relu(x)
    return x


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _overrides(layout, n):
    """(env overrides, actor_generic) of a layout name."""
    ov = {"cluster_prop.nb_agents": n, "power_grid_prop.signal_properties.mode": "sinusoidals"}
    if layout == "ks1_4":
        ov.update(KS1_4)
    elif layout == "closed_groups":  # the table topology of the n30_maxerr_groups_hvacmsg golden, at n houses
        _, meta = gu.traj("n30_maxerr_groups_hvacmsg")
        ov = dict(meta["overrides"])
        ov.update({"cluster_prop.nb_agents": n, "reward_prop.penalty_props.mode": "individual_L2"})
    else:
        assert layout in ("def", "generic")
    return ov, int(layout == "generic")


def _state(torch, layout, n, edit=None):
    """An env of the layout after 5 ticks of random actions (+ `edit(env)` on its state)."""
    from mdr_amd.environment import Environment

    ov, generic = _overrides(layout, n)
    env = Environment(gu.props_from_overrides(ov), rng=random.Random(5), seed=SEED)
    rs = np.random.RandomState(7)
    for _ in range(5):
        env.step_tensor(torch.from_numpy(rs.randint(0, 2, n).astype(np.uint8)).to("cuda"))
    if edit is not None:
        edit(env)
    env.shard.set_option("actor_generic", generic)
    return env


def _reset_options(*envs):
    for e in envs:
        e.shard.set_option("actor_grid", 0)
        e.shard.set_option("actor_generic", 0)


def _calibrated(env, seed):
    F = env.obs_spec().n_feat
    return gu.calibrated_actor(F, env.obs_tensor().abs().amax(0).double().cpu().numpy(), seed=seed).to("cuda")


def _select(torch, env, da, grid, count_next=False):
    """One select_actions launch at an actor_grid value: (probs, obs, action, prob) on device + status."""
    n, F = env.n_local, env.obs_spec().n_feat
    env.shard.set_option("actor_grid", grid)
    da.status()  # (clear)
    probs = torch.full((n, 2), float("nan"), dtype=torch.float32, device="cuda")
    obs = torch.full((n, F), float("nan"), dtype=torch.float32, device="cuda")
    act = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    prob = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    da.select_actions(action=act, prob=prob, probs=probs, obs_out=obs, count_next=count_next)
    return (probs, obs, act, prob), da.status()


def _check_probs(torch, actor, out, precision, rows=None, tag=""):
    """Probabilities vs torch fp32 on the kernel's own obs rows (+ the float64 bound for the fp32 forms)."""
    probs, obs = out[0], out[1]
    with torch.no_grad():
        tp = actor(obs).cpu().numpy()
    p = probs.cpu().numpy()
    assert np.all(np.isfinite(p)), tag
    sl = slice(None) if rows is None else rows
    err = float(np.abs(p[sl] - tp[sl]).max())
    print(f"{tag} {precision}: max |p - p_torch| = {err:.3g}")
    assert err < ATOL[precision], (tag, err)
    if precision in FP32S:
        with torch.no_grad():
            p64 = torch.softmax(_forward64(actor, obs.double()), 1).cpu().numpy()
        e_ours, e_torch = float(np.abs(p[sl] - p64[sl]).max()), float(np.abs(tp[sl] - p64[sl]).max())
        print(f"  vs float64: ours {e_ours:.3g}, torch fp32 {e_torch:.3g}")
        assert e_ours <= 2.0 * e_torch + 2e-7, (tag, e_ours, e_torch)
    return tp


def _check_sampling(env, out):
    """The sampled actions replayed from philox_u01f, exactly; prob == probs[action]."""
    probs, _, act, prob = (x.cpu().numpy() for x in out)
    n = probs.shape[0]
    goff = int(getattr(env, "_offset", 0))
    u = P.u01f(SEED, goff + np.arange(n, dtype=np.uint64), env._tick)
    assert u.dtype == np.float32 and probs.dtype == np.float32
    want = (u >= probs[:, 0]).astype(np.uint8)
    np.testing.assert_array_equal(act, want)
    np.testing.assert_array_equal(prob, probs[np.arange(n), act])


def _same(torch, a, b, tag):
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (tag, ("probs", "obs", "action", "prob")[k])


CASES = [(l, p) for l in ("def", "generic", "ks1_4", "closed_groups") for p in PRECISIONS
         if not (l == "ks1_4" and p == "fp32_bf16")]  # (that one runs the layer chain: no tile loop)


@pytest.mark.parametrize("layout,precision", CASES)
def test_many_tiles_per_wave_vs_torch(torch_gpu, layout, precision):
    """(a) One block, 2,085 houses: every wave walks 5 to 9 tiles, the ragged tile last after a full one."""
    torch = torch_gpu
    env = _state(torch, layout, N_SMALL)
    try:
        actor = _calibrated(env, seed=5)
        da = device_actor(env, actor, precision)
        if not (layout == "closed_groups" and precision == "fp32_bf16"):
            assert da.fused()
        ref_obs = env.obs_tensor().clone()
        out, st = _select(torch, env, da, grid=1)
        assert torch.equal(out[1], ref_obs)  # the rows the network read == the standalone obs kernel's
        tp = _check_probs(torch, actor, out, precision, tag=f"{layout} grid 1")
        _check_sampling(env, out)
        gu.assert_not_saturated(tp[:, 1], out[2].cpu().numpy())
        assert st["range_faults"] == 0, st
    finally:
        _reset_options(env)


@pytest.mark.parametrize("layout,precision", CASES)
def test_grid_invariance(torch_gpu, layout, precision):
    """(b) actor_grid 1, 3 and 0 on the same state: probabilities, obs rows, actions, chosen
    probabilities and the next tick's ON counts, bit for bit."""
    torch = torch_gpu
    grids = (1, 3, 0)
    envs = [_state(torch, layout, N_SMALL) for _ in grids]
    twin = _state(torch, layout, N_SMALL)
    try:
        actor = _calibrated(twin, seed=5)
        outs = []
        for env, grid in zip(envs, grids):
            da = device_actor(env, actor, precision)
            out, st = _select(torch, env, da, grid, count_next=True)
            assert st["range_faults"] == 0, (grid, st)
            outs.append(out)
        for out, grid in zip(outs[1:], grids[1:]):
            _same(torch, outs[0], out, f"grid {grid} vs 1")
        state0 = {k: getattr(twin.shard, k).clone() for k in ("t_air", "t_mass", "hvac")}
        tick0 = twin._tick
        rb = twin.step_tensor(outs[0][2].clone()).clone()
        assert twin._tick == tick0 + 1 and not torch.equal(twin.shard.hvac, state0["hvac"])
        for env, out, grid in zip(envs, outs, grids):
            ra = env.step_tensor(out[2])
            assert torch.equal(ra, rb), grid
            for k in state0:
                assert torch.equal(getattr(env.shard, k), getattr(twin.shard, k)), (grid, k)
    finally:
        _reset_options(twin, *envs)


def _saturate_long(env):
    """(c)'s out-of-range houses: tile 3 (j = 0), tile 769 (j >= 64 of its wave) and the ragged tile 848."""
    for a, b in ((100, 132), (24608, 24640), (N_LONG - 5, N_LONG)):
        env.shard.hvac[a:b] = SAT


SAT_ROWS = np.r_[100:132, 24608:24640, N_LONG - 5:N_LONG]


@pytest.mark.parametrize("precision", FP32S)
@pytest.mark.parametrize("layout", ["def", "generic"])
def test_out_of_range_tiles_past_64(torch_gpu, layout, precision):
    """(c) One block, 27,141 houses: more than 64 tiles per wave, houses off for ~34 years (sso ratio
    ~2.7e7, beyond fp16) in a wave's first tile, in a tile at j >= 64 and in the ragged last tile.
    Every out-of-range tile gets its logits from the fp32 fallback, whatever its index.  (With the
    deferral mask's 64-tile limit inside one launch, the fp32 cases were 0.087 (default layout) and
    0.068 (generic) from torch at houses 24,576.. — the previous tile's logits — with range_faults
    5; launch_actor now runs a launch per 64 tiles of a wave.)"""
    torch = torch_gpu
    env1, env0, twin = (_state(torch, layout, N_LONG, _saturate_long) for _ in range(3))
    try:
        actor = _calibrated(twin, seed=4)  # (on the obs absmax after saturation)
        assert float(twin.obs_tensor()[SAT_ROWS].abs().max()) > 65504.0
        da1, da0 = device_actor(env1, actor, precision), device_actor(env0, actor, precision)
        out1, st = _select(torch, env1, da1, grid=1, count_next=True)
        p = out1[0].cpu().numpy()
        with torch.no_grad():
            tp = actor(out1[1]).cpu().numpy()
        err = np.abs(p - tp).max(1)
        print(f"{layout} {precision}: max |p - p_torch| = {err.max():.3g} (saturated rows {err[SAT_ROWS].max():.3g}), {st}")
        assert np.all(np.isfinite(p)) and err.max() < 4e-6, (err.max(), np.flatnonzero(err >= 4e-6)[:8])
        assert torch.equal(out1[1], twin.obs_tensor())
        # (a stale-logit row must not pass by comparing 1.0 with 1.0)
        gu.assert_not_saturated(tp[SAT_ROWS, 1])
        gu.assert_not_saturated(tp[:, 1], out1[2].cpu().numpy())
        _check_sampling(env1, out1)
        assert st["range_faults"] == 0, st
        if precision == "fp32":
            assert st["kernel_prec"] == 4 and st["exact"] >= len(np.unique(SAT_ROWS // 32)), st
        else:
            assert st["kernel_prec"] == 6 and st["exact"] == 0, st
        out0, st0 = _select(torch, env0, da0, grid=0, count_next=True)
        assert st0["range_faults"] == 0, st0
        _same(torch, out1, out0, "grid 0 vs 1")
        rb = twin.step_tensor(out1[2].clone()).clone()
        for env, out in ((env1, out1), (env0, out0)):
            assert torch.equal(env.step_tensor(out[2]), rb)
            for k in ("t_air", "t_mass", "hvac"):
                assert torch.equal(getattr(env.shard, k), getattr(twin.shard, k)), k
    finally:
        _reset_options(env1, env0, twin)


F16_SSO = 64  # csrc/mdr_actor.h kActorF16Sso: the largest sso ratio of the fp16 path, exclusive


@pytest.mark.parametrize("ratio", [F16_SSO, 32768])
def test_fp16_range_threshold(torch_gpu, ratio):
    """(d) The fp16-split form's input threshold.  Houses 40..47 are off and unlocked with a
    seconds-since-off ratio of exactly `ratio` - 1, then houses 1,000..1,007 with `ratio`; the actor
    is calibrated on the absmax after both edits, so the sso columns' weights are 1 / ratio of the
    others' scale — the case in which the per-layer fp16 scale loses the small weights' low bits.
    Both states are within the fp32 tolerances at one block and at the default grid.  Measured with
    the bound at 2^15: a ratio of 32,767 on the fp16 path was 7e-5 from torch and from float64
    (1,023: 2.9e-6, 127: 3.7e-7, 63: 1.1e-7; the float64 bound was 3.5e-7), so the bound is now
    kActorF16Sso = 64: below it the tile stays on the fp16 MFMA path (exact == 0), from it on the
    tile takes the fp32 fallback — 32,767 and 32,768 both do."""
    torch = torch_gpu
    env = _state(torch, "def", N_SMALL)
    try:
        L_ = int(env.init_props.cluster_prop.house_prop.hvac_prop.lockout_duration)
        env.shard.hvac[40:48] = ratio * L_ - 1      # off, unlocked, int(sso / L) = ratio - 1
        below = env.shard.hvac.clone()
        env.shard.hvac[1000:1008] = ratio * L_      # ... = ratio
        above = env.shard.hvac.clone()
        absmax = env.obs_tensor().abs().amax(0)
        assert float(absmax.max()) == float(ratio)
        F = env.obs_spec().n_feat
        actor = gu.calibrated_actor(F, absmax.double().cpu().numpy(), seed=6).to("cuda")
        da = device_actor(env, actor, "fp32")
        for top, words in ((ratio - 1, below), (ratio, above)):
            env.shard.hvac.copy_(words)
            assert float(env.obs_tensor().max()) == float(top)
            outs = []
            for grid in (1, 0):
                out, st = _select(torch, env, da, grid)
                print(f"sso ratio {top} grid {grid}: {st}")
                tp = _check_probs(torch, actor, out, "fp32", tag=f"sso ratio {top} grid {grid}")
                assert st["kernel_prec"] == 4 and st["range_faults"] == 0, st
                if top < F16_SSO:
                    assert st["exact"] == 0, st
                else:
                    assert st["exact"] >= 1, st
                _check_sampling(env, out)
                gu.assert_not_saturated(tp[:, 1], out[2].cpu().numpy())
                outs.append(out)
            _same(torch, outs[0], outs[1], f"sso ratio {top}: grid 0 vs 1")
    finally:
        _reset_options(env)


def test_fp16_hidden_layer_overflow(torch_gpu):
    """(d) relu(layer 1) >= 2^15 in the layer's scaled space with every input inside the fp16 path's
    range (the maximum tracked on the MFMA results, `mbits`).  A power-of-two factor on the whole
    first layer cannot trip it: k_actor_pack's per-layer scale s1 = 2^-e (max |W1| < 2^e) cancels the
    factor exactly, and the first part asserts that with a factor of 2^17 (hidden values beyond 2^15,
    exact == 0).  What trips it is a sum of large in-range inputs under weights at the layer's maximum:
    here houses 1,000..1,031 at 40,000 K above their target (the temperature feature (T - target) / 5
    = 8,000 in the own row and the 10 ring neighbours' messages: 11 inputs of 8,000, sso ratios
    untouched) and hidden neuron 0 with the layer's largest |weight| on those 11 columns, s1 |w| in
    [0.5, 1), so s1 h1[0] is in [44,000, 88,000) >= 2^15 for the middle houses.  Layer 2's column
    of that neuron is scaled by 2^-16, so the probabilities stay unsaturated."""
    torch = torch_gpu
    env = _state(torch, "def", N_SMALL)
    try:
        F = env.obs_spec().n_feat
        # 1. an ordinary state, first layer x 2^17 and output layer x 2^-17: s1 absorbs the factor
        actor = _calibrated(env, seed=6)
        with torch.no_grad():
            actor.fc[0].weight.mul_(2.0 ** 17)
            actor.fc[0].bias.mul_(2.0 ** 17)
            actor.fc[2].weight.mul_(2.0 ** -17)
        da = device_actor(env, actor, "fp32")
        out, st = _select(torch, env, da, grid=1)
        assert float(out[1].abs().max()) < 32768.0
        with torch.no_grad():
            h1 = torch.relu(actor.fc[0](out[1]))
        assert float(h1.max()) >= 32768.0  # (the unscaled hidden layer is beyond 2^15)
        _check_probs(torch, actor, out, "fp32", tag="W1 x 2^17")
        assert st["kernel_prec"] == 4 and st["exact"] == 0 and st["range_faults"] == 0, st
        # 2. many in-range inputs under maximal weights
        env.shard.t_air[1000:1032] = env.shard.target[1000:1032] + 40000.0
        obs = env.obs_tensor()
        assert 8000.0 <= float(obs.abs().max()) < 8001.0
        cols = torch.nonzero((obs[1016] - 8000.0).abs() < 1.0).ravel()
        assert cols.numel() == 11  # own temperature difference + the 10 ring neighbours'
        actor = gu.calibrated_actor(F, obs.abs().amax(0).double().cpu().numpy(), seed=6).to("cuda")
        with torch.no_grad():
            actor.fc[0].weight[0, cols] = actor.fc[0].weight.abs().max()
            actor.fc[1].weight[:, 0].mul_(2.0 ** -16)
        da = device_actor(env, actor, "fp32")
        for grid in (1, 0):
            out, st = _select(torch, env, da, grid)
            print(f"hidden overflow grid {grid}: {st}")
            tp = _check_probs(torch, actor, out, "fp32", tag=f"hidden overflow grid {grid}")
            assert st["kernel_prec"] == 4 and st["exact"] >= 1 and st["range_faults"] == 0, st
            _check_sampling(env, out)
            gu.assert_not_saturated(tp[:, 1], out[2].cpu().numpy())
            gu.assert_not_saturated(tp[1000:1032, 1])
    finally:
        _reset_options(env)


def test_fp16_range_table_messages(torch_gpu):
    """(d) A table topology's messages: one house off for ~34 years makes every tile that holds one of
    its group neighbours out of range through the gathered message's sso ratio, although the tile's
    own rows are ordinary."""
    torch = torch_gpu
    env = _state(torch, "closed_groups", N_SMALL)
    try:
        links = np.asarray(env._obs_links)
        # a house h whose group has a member in another tile
        h = next(int(j) for i in range(32, N_SMALL) for j in links[i] if j // 32 != i // 32)
        readers = np.flatnonzero((links == h).any(1))
        tiles = np.unique(np.r_[readers // 32, h // 32])
        other = [t for t in tiles if t != h // 32]
        assert other, "the house has a group neighbour in another tile"
        F = env.obs_spec().n_feat
        before = env.shard.hvac.clone()
        env.shard.hvac[h] = SAT
        actor = _calibrated(env, seed=8)
        da = device_actor(env, actor, "fp32")
        assert da.fused()
        for grid in (1, 0):
            env.shard.hvac.copy_(before)
            out, st = _select(torch, env, da, grid)
            assert st["kernel_prec"] == 4 and st["exact"] == 0 and st["range_faults"] == 0, st
            env.shard.hvac[h] = SAT
            out, st = _select(torch, env, da, grid)
            tp = _check_probs(torch, actor, out, "fp32", tag=f"table messages grid {grid}")
            rows = np.concatenate([np.arange(32 * t, min(32 * t + 32, N_SMALL)) for t in other])
            _check_probs(torch, actor, out, "fp32", rows=rows, tag=f"  the neighbour tiles {other}")
            assert float(out[1].cpu().numpy()[rows].max()) > 65504.0  # (through the message only)
            assert st["kernel_prec"] == 4 and st["exact"] >= len(tiles) and st["range_faults"] == 0, (st, tiles)
            _check_sampling(env, out)
            gu.assert_not_saturated(tp[:, 1], out[2].cpu().numpy())
    finally:
        _reset_options(env)
