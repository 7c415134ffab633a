"""Inputs shared by tests/test_env_batch_gpu.py and tests/test_env_batch_cpu.py: the GPU test compares
every member of an ``EnvBatch`` with a stand-alone ``Environment`` of the same seed, the CPU test
asserts under the oracle that these inputs tell the clusters of a batch apart and exercise the lockout."""
import golden_util as gu
from bangbang_inputs import overrides

SOURCES = ["buffer", "random", "always_on", "bangbang", "deadband_bangbang"]
# (E, N_c, ticks): one house; both slots of a lane; config C1 (one ragged wave, no barrier); a second
# tile holding one house; the reference's cluster size (8 waves, ragged last tile); the full block
SHAPES = [(1, 1, 5), (3, 2, 33), (3, 50, 45), (3, 129, 45), (5, 1000, 45), (2, 1024, 12)]
OBS_SHAPES = [(3, 50), (3, 129), (2, 1000)]
ACTION_SEED = 2024  # the fixed uint8 action matrix of the buffer source


def seeds(n_envs):
    return [8 + e for e in range(n_envs)]


def props(n, extra=None):
    o = overrides(n)  # sinusoidal signal, deadband 0.05, individual_L2
    o.update(extra or {})
    return gu.props_from_overrides(o)
