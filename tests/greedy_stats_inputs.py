"""Inputs shared by tests/test_greedy_stats_gpu.py and tests/test_greedy_stats_cpu.py: the GPU test
compares ``greedy_rollout(stats=...)`` on these configurations with the per-tick loop, the CPU test
asserts under the oracle that they exercise the controller.

The populations are the device's synthetic ones (k_populate: Philox4x32-10 keyed by (seed, house),
counters (gid lo, gid hi, 0x9090, 0 | 1)); ``synthetic_pop`` restates the kernel in NumPy.  The two
agree to the rounding of log / cos / sqrt (nothing here needs more: the CPU test counts events)."""
import numpy as np

import philox_np as PH

SEED = 31  # random.Random(SEED): the outdoor-temperature noise and the signal ratio; Environment(seed=SEED)
# (houses, ticks): below one quad-block with odd n, one tick past a batch of 32; one tick; one short of
# a batch; two k_tick_stats blocks with a 2-house ragged tail, exactly one batch; three batches, odd n;
# 258 partial blocks (the finish's threads 0 and 1 add two partials each), ragged tail
SHAPES = [(17, 33), (130, 1), (130, 31), (1030, 32), (4099, 70), (263_173, 6)]
FORM_N = 4099  # the forms-and-modes cases


def overrides(n, pmode="individual_L2", signal="sinusoidals"):
    return {"cluster_prop.nb_agents": n,
            "power_grid_prop.signal_properties.mode": signal,
            "reward_prop.penalty_props.mode": pmode}


def _u01(x):
    return (x.astype(np.float64) + 0.5) * 2.3283064365386963e-10


def _triangular(u, lo, hi, mode=1.0):
    c = (mode - lo) / (hi - lo)
    flip = u > c
    u = np.where(flip, 1.0 - u, u)
    c = np.where(flip, 1.0 - c, c)
    a, b = np.where(flip, hi, lo), np.where(flip, lo, hi)
    return a + (b - a) * np.sqrt(u * c)


def synthetic_pop(props, n, seed):
    """k_populate (csrc/mdr_kernels.hip) for houses 0 .. n-1 as OracleEnv's ``population`` dict."""
    hp = props.cluster_prop.house_prop
    nz = hp.noise_prop
    gid = np.arange(n, dtype=np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    r0 = PH.philox4x32_10(gid & np.uint64(0xFFFFFFFF), gid >> np.uint64(32), 0x9090, 0, k0, k1)
    r1 = PH.philox4x32_10(gid & np.uint64(0xFFFFFFFF), gid >> np.uint64(32), 0x9090, 1, k0, k1)
    g = np.sqrt(-2.0 * np.log(_u01(r0[0]))) * np.cos(6.283185307179586 * _u01(r0[1]))
    lo, hi = nz.factor_thermo_low, nz.factor_thermo_high
    caps = np.array(list(hp.hvac_prop.noise_prop.cooling_capacity_list), np.float64)
    return {"target": hp.target_temp + np.abs(g * nz.std_target_temp),
            "Ua": _triangular(_u01(r0[2]), lo, hi),
            "Cm": hp.Cm * _triangular(_u01(r0[3]), lo, hi),
            "Ca": hp.Ca * _triangular(_u01(r1[0]), lo, hi),
            "Hm": hp.Hm * _triangular(_u01(r1[1]), lo, hi),
            "cap": caps[((r1[2].astype(np.uint64) * np.uint64(len(caps))) >> np.uint64(32)).astype(np.int64)]}
