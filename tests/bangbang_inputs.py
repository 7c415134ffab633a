"""Inputs shared by tests/test_bangbang_rollout_gpu.py and tests/test_bangbang_rollout_cpu.py: the
GPU test compares rollouts of these configurations with the per-tick loop, the CPU test asserts
under the oracle that they exercise the controllers."""

SEED = 8          # random.Random(SEED): the host-drawn population and the outdoor-temperature noise
DEADBAND = 0.05   # degC (at the reference's 0.5 the deadband form switches no house back on within 65 ticks)
CTRLS = ["bangbang", "deadband_bangbang"]
# (n, ticks, window): one lane; both slots of a lane; a second tile holding one house, short windows;
# a second block; three windows with a ragged last tile
SHAPES = [(1, 5, 32), (2, 33, 32), (129, 40, 7), (513, 33, 32), (4099, 65, 32)]


def overrides(n, pmode="individual_L2", deadband=DEADBAND):
    return {"cluster_prop.nb_agents": n,
            "power_grid_prop.signal_properties.mode": "sinusoidals",
            "reward_prop.penalty_props.mode": pmode,
            "cluster_prop.house_prop.deadband": deadband}
