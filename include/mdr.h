/*
 * mdr.h — C ABI of the MI355X-native vectorised environment step (libmdr_hip.so).
 *
 * Drop-in boundary for the reference's per-tick environment step, ALLabMTL/marl-demandresponse
 * v2 (file:line relative to /root/reference):
 *
 *   Environment.step               server/app/core/environment/environment.py:72-108
 *     Cluster.step (house loop)    server/app/core/environment/cluster/cluster.py:73-89
 *       HVAC.step (lockout FSM)    server/app/core/environment/cluster/hvac.py:43-64
 *       Building.update_temperature server/app/core/environment/cluster/building.py:141-222
 *       get_power_consumption      server/app/core/environment/cluster/hvac.py:101-111
 *     RewardsCalculator            server/app/core/environment/rewards_calculator.py:135-203
 *     Cluster.get_obs / messages   server/app/core/environment/cluster/cluster.py:91-121
 *   norm_state_dict (obs vector)   server/app/utils/norm.py:178-218
 *   controllers                    server/app/core/agents/controllers/bangbang_controllers.py:25-89,
 *                                  server/app/core/agents/controllers/greedy_myopic_controller.py:67-104
 *   Environment.reset / noise      server/app/core/environment/environment.py:49-70,161-194
 *   PowerInterpolator (base power) server/app/core/environment/power_grid/interpolation.py:186-264
 *
 * The reference has no FFI: its boundary is a Python object (Environment.reset/step).  The
 * Python layer mdr_amd.Environment keeps that object surface and binds these symbols with ctypes
 * (INTEGRATION.md shows the binding).  Per-tick scalar drivers (outdoor temperature, solar gain,
 * regulation signal, datetime) stay on the host in the reference's own arithmetic and RNG order
 * and are passed in as mdr_tick; everything per house runs on the GPU.
 *
 * Conventions
 *   - All device pointers are caller-owned (PyTorch tensors in mdr_amd); the library owns only
 *     small scratch (per-tick power counts, penalty partials, graph cache).
 *   - Every call is asynchronous on the caller's hipStream_t (passed as void*; NULL = legacy
 *     default stream) and returns 0 on success, a negative MDR_E* code otherwise;
 *     mdr_last_error() gives the text (thread-local).
 *   - A context maps to ONE device and ONE contiguous shard of houses [global_offset,
 *     global_offset + n_local) of a cluster of n_global houses; it is not thread-safe.
 *
 * Per-house state layout (SoA, length n_local):
 *   t_air, t_mass : double   indoor air / mass temperature (Celsius)
 *   hvac          : uint32   bits 0..29 seconds_since_off (saturating), bit 30 lockout, bit 31 on
 *   ua, ca, cm, hm, target : double  (noised per-house parameters)
 *   cap_idx       : uint8    index into the cooling-capacity table (mdr_config.cap_table)
 */
#ifndef MDR_H_
#define MDR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_ABI_VERSION 5
#define MDR_MAX_CAP 64

enum {
  MDR_OK = 0,
  MDR_EARG = -1,   /* bad argument / shape / unbound context */
  MDR_EHIP = -2,   /* HIP runtime error */
  MDR_ERCCL = -3,  /* RCCL error */
  MDR_ENOMEM = -4,
  MDR_ESTATE = -5, /* call out of order (e.g. step before bind) */
};

/* penalty modes, rewards_calculator.py:46-133 */
enum { MDR_PEN_INDIVIDUAL_L2 = 0, MDR_PEN_COMMON_L2 = 1, MDR_PEN_COMMON_MAX = 2, MDR_PEN_MIXTURE = 3 };

/* where a tick's actions come from */
enum {
  MDR_ACT_BUFFER = 0,     /* uint8 action[n_local] (non-zero = turn on), the Dict[int,bool] of step() */
  MDR_ACT_RANDOM = 1,     /* Bernoulli(0.5) from Philox4x32-10(seed, global house id, tick) */
  MDR_ACT_ALWAYS_ON = 2,  /* AlwaysOnController, bangbang_controllers.py:7-16 */
  MDR_ACT_BANGBANG = 16,  /* BangBangController on the pre-step state, bangbang_controllers.py:54-65 */
  MDR_ACT_DEADBAND_BANGBANG = 17 /* DeadbandBangBangController, bangbang_controllers.py:25-42 */
};

/* controller evaluated on the post-step state, written as the NEXT tick's action buffer
 * (MDR_CTRL_GREEDY_KEYS: no action buffer — the greedy controller's keys and key histogram of the
 * post-step state are prepared for the next mdr_ctrl_greedy, which then skips its key pass) */
enum { MDR_CTRL_NONE = 0, MDR_CTRL_BANGBANG = 1, MDR_CTRL_DEADBAND_BANGBANG = 2, MDR_CTRL_GREEDY_KEYS = 3 };

/* communication (message) topology, agent_communication_builder.py:36-203 */
enum { MDR_COMM_RING = 0, MDR_COMM_TABLE = 1 };

typedef struct mdr_config {
  int32_t abi_version;      /* = MDR_ABI_VERSION */
  int32_t device;           /* HIP device ordinal */
  int64_t n_local;          /* houses in this shard */
  int64_t global_offset;    /* global id of the shard's first house */
  int64_t n_global;         /* cluster size N (signal penalty, obs normalisation) */
  int32_t dt;               /* time_step.seconds */
  int32_t lockout_duration; /* L (hvac_prop.lockout_duration) */
  double cop;               /* hvac_prop.cop */
  double lcf;               /* hvac_prop.latent_cooling_fraction */
  double deadband;          /* house_prop.deadband */
  int32_t n_cap;            /* entries in cap_table (<= MDR_MAX_CAP) */
  int32_t penalty_mode;     /* MDR_PEN_* */
  double cap_table[MDR_MAX_CAP]; /* cooling capacities (W) the population draws from */
  double alpha_temp, alpha_sig;  /* reward_prop */
  double norm_temp, norm_sig;    /* deadbandL2 normalisers, computed by the caller */
  double alpha_ind_l2, alpha_common_l2, alpha_common_max;
  uint64_t seed;                 /* Philox key for MDR_ACT_RANDOM and synthetic populations */
} mdr_config;

typedef struct mdr_soa {
  double* t_air;
  double* t_mass;
  uint32_t* hvac;
  const double* ua;
  const double* ca;
  const double* cm;
  const double* hm;
  const double* target;
  const uint8_t* cap_idx;
} mdr_soa;

/* host-side per-tick drivers (environment.py:86-106 ordering) */
typedef struct mdr_tick {
  double t_od_prev; /* outdoor temperature BEFORE this step (used by the thermal update) */
  double solar;     /* compute_solar_gain at the NEW datetime, 0 if house_prop.solar_gain is off */
  double s_prev;    /* regulation signal before this step (the reward uses the old signal) */
  uint64_t tick;    /* tick counter (Philox stream for MDR_ACT_RANDOM) */
} mdr_tick;

typedef struct mdr_ctx mdr_ctx;

/* ---- lifecycle ------------------------------------------------------------------------- */
int mdr_abi_version(void);
/* "MDR_SRC_HASH:<16 hex>": sha256 of the sources and build flags the library was built from
 * (build_ext.py src_hash); the Python binding refuses a library whose hash differs from its tree's. */
const char* mdr_build_id(void);
/* sizeof of the ABI structs, for binding checks: out[0..8] = mdr_config, mdr_soa, mdr_tick,
 * mdr_pop_spec, mdr_obs_spec, mdr_obs_scalars, mdr_actor_spec, mdr_interp_spec, mdr_actor_net;
 * returns the number written */
int mdr_abi_sizes(int64_t* out, int n);
const char* mdr_last_error(void);
/* Graph cache diagnostics: out[0..5] = cached rollout graphs, cached actor-rollout graphs,
 * hipGraphLaunch calls of mdr_rollout, of mdr_actor_rollout, captured graphs the memset guard
 * walked (every capture fails with MDR_EHIP on a memset node), their nodes; returns the number
 * written. */
int mdr_graph_info(mdr_ctx* ctx, int64_t* out, int n);
/* The carried first-group counts of direct rollouts (MDR_OPT_ROLLOUT_CARRY): out[0..3] = calls whose
 * last launch counted the next call's first group, calls that started from such a count, counts
 * discarded unused, 1 if one is outstanding now; returns the number written. */
int mdr_rollout_carry_info(mdr_ctx* ctx, int64_t* out, int n);
/* Diagnostic (synchronises, overwrites the count slabs): captures hipMemsetAsync of the count slabs
 * to zero in this context and reports out[13] = {nodes, memset nodes, dst == the slabs, value,
 * elementSize, width, height, pitch, bytes passed, non-zero 64-bit words after replays 1..3 (slabs
 * pre-filled with 0xA5 before replays 1 and 2), non-zero words after the kernel zeroing}. */
int mdr_graph_memset_probe(mdr_ctx* ctx, int64_t* out, int n, void* stream);
int mdr_create(mdr_ctx** out, const mdr_config* cfg);
int mdr_destroy(mdr_ctx* ctx);
/* Bind the caller-owned SoA arrays (Environment.reset, environment.py:49-70). */
int mdr_bind(mdr_ctx* ctx, const mdr_soa* soa);

/* The caller rewrote ua/ca/cm/hm (or dt changed): the per-house flag that routes a house outside
 * the exact shared-reciprocal division range to the IEEE operator is recomputed before the next
 * step.  mdr_bind and mdr_populate imply it.  Also the call that announces an in-place write to
 * hvac or cap_idx between two rollouts: it discards a first-group count the previous direct rollout
 * made for the next one from the old FSM words (MDR_OPT_ROLLOUT_CARRY). */
int mdr_params_changed(mdr_ctx* ctx);

/* ---- options (no reference counterpart) ------------------------------------------------ */
/* Alternative launch forms of the same computation, for verification and measurement; every
 * option has a test that pins it against the default.  Drops cached rollout graphs.
 *   MDR_OPT_STEP_TPW        per-tick step kernel: 1/2/4/8 = k_step_pipe tiles per wave, 0 = the
 *                           one-tile k_step_t, -1 = the measured default (2 up to 1.5M houses, 4)
 *   MDR_OPT_FASTDIV         1 = shared-reciprocal exact division (default), 0 = the IEEE operator
 *                           everywhere (bit-identical results)
 *   MDR_OPT_WINDOW_PIPELINE sharded window rollouts: 1 = count + allreduce on a side stream up to
 *                           two windows ahead (default), 0 = one stream
 *   MDR_OPT_SHARDED_OVERLAP sharded one-tick rollouts: 1 = allreduce of tick t beside the step of
 *                           tick t, rewards written one launch later (default), 0 = serial
 *   MDR_OPT_GREEDY_SORT     1 = mdr_ctrl_greedy always runs the full-sort form
 *   MDR_OPT_FORCE_HALO      1 = mdr_actor_rollout_sharded exchanges the ring halo even at world 1
 *                           (send/recv to self: the one-GPU check of the multi-GPU exchange)
 *   MDR_OPT_HALO_OVERLAP    mdr_actor_rollout_sharded: 1 (default) = each tick's ring halo is packed and
 *                           exchanged on the communicator's side stream while the interior tiles'
 *                           k_actor runs, then the first and last tile; 0 = halo, then one k_actor
 *   MDR_OPT_HALO_IN_COUNTS  mdr_actor_rollout_sharded: 1 (default) = ONE collective per tick: the edge
 *                           houses' post-step message rows (the next tick's ring halo) are computed
 *                           before the step and summed into the count allreduce; 0 = a ring-halo
 *                           send/recv per tick plus the count allreduce (MDR_OPT_HALO_OVERLAP applies)
 *   MDR_OPT_GQ_BAND         mdr_ctrl_greedy: 1 (default) = k_gq_binsc cuts the window from the step
 *                           epilogue's predicted band when it holds the crossing (no bins pass) and
 *                           k_gq_finish ranks and decides; 0 = the bins pass every call (k_gq_bins,
 *                           k_gq_compact, k_gq_select: faster when the budget jumps across the cluster
 *                           every call)
 *   MDR_OPT_GQ_FUSED        mdr_greedy_rollout: 1 = the fused tick, one decision launch per tick
 *                           (k_gq_decide2: the previous step's epilogue counted the keys and the band's
 *                           houses, the step applies the decision from the pre-step keys); 0 (default)
 *                           = the mdr_ctrl_greedy + mdr_step tick (bit-identical; faster at 1M houses,
 *                           DESIGN.md §3.3)
 *   MDR_OPT_GQ_ADAPTIVE     mdr_greedy_rollout with the band form: 1 (default) = a tick whose budget change departs
 *                           from the previous change by more than four superbins' worth of power runs the
 *                           three-launch form (a band miss costs more); 0 = the band form on every tick
 *   MDR_OPT_ACTOR_GENERIC   1 = k_actor runs its generic form for the reference's default obs layout too
 *                           (0, default: that layout runs the form specialised for it, mdr_actor.hip DEF)
 *   MDR_OPT_ACTOR_GRID      v >= 1 = k_actor's grid is capped at min(v, CUs) blocks, so every wave walks more
 *                           tiles (the same outputs bit for bit: the tests' way to many tiles per wave on
 *                           a small cluster); 0 (default) = min(blocks with a tile per wave, CUs).  Every
 *                           fused-actor launch (act, the rollout graph, the sharded interior / edge
 *                           launches); the layer chain ignores it; a negative value is MDR_EARG
 *   MDR_OPT_ACTOR_FP32_FORM the fused actor's MDR_PREC_FP32 arithmetic: MDR_FP32_F16_SPLIT (default) =
 *                           fp16 hi/lo operands on the fp16 MFMA, 3 products per term, power-of-two
 *                           per-layer weight scales (activations must stay inside fp16's range:
 *                           mdr_actor_status counts the tiles that did not); MDR_FP32_BF16_SPLIT3 =
 *                           three-way bf16 operands, 6 products per term, no range limit
 *   MDR_OPT_WINDOW_THERMAL  k_step_window's per-tick thermal update: MDR_THERMAL_AFFINE (default)
 *                           = the reference's update as a per-house affine transition formed once
 *                           per window (4 FMAs per temperature per tick; ~1e-13 K per tick from the
 *                           reference order), MDR_THERMAL_EXACT = the reference's expression in its
 *                           operation order every tick (bit-identical to the one-tick kernels).
 *                           Open-loop sources only: the closed-loop windows of the bang-bang
 *                           sources (k_step_closed) always run the EXACT form and ignore it — a
 *                           decision compares T with a threshold, so a last-bit difference could
 *                           flip an action and fork the trajectory
 *   MDR_OPT_WINDOW_GROUP    directly launched window rollouts (mdr_rollout without a graph, one
 *                           GPU, individual_L2): 1..4 = that many consecutive windows per step
 *                           launch (k_step_group: state, parameters and per-window coefficients
 *                           loaded and formed once per group, one reduce launch per group; default
 *                           4), 0 = one k_step_window launch per window.  Bit-identical results
 *                           either way; graphs, sharded and common-penalty rollouts ignore it
 *   MDR_OPT_ROLLOUT_CARRY   the grouped direct sequence from a random or always_on source: 1 (default) =
 *                           a call that continues the previous one (same n, source, window and stream,
 *                           the next tick id) lets its last step launch run its FSM lookahead on over
 *                           the first group of the NEXT such call, which then starts from staged
 *                           drivers with no count kernel and no KA launch (mdr_rollout_begin for it
 *                           launches nothing); any other entry point, option or state write in between
 *                           discards that count (mdr_rollout_carry_info).  0 = every call counts its own
 *                           first window.  Bit-identical results either way.  The count runs on from the
 *                           FSM words (soa.hvac) as the previous call left them: a caller that rewrites
 *                           the bound arrays in place between two calls must say so (mdr_params_changed,
 *                           mdr_bind), as for every other derived state the library keeps; an unannounced
 *                           write to hvac would be missed by the next call's first group
 *   MDR_OPT_GROUP_LA_ORDER  k_step_group launches: which blocks run the FSM lookahead over the next group
 *                           BEFORE their ticks instead of behind them, so that part of the chip counts while
 *                           the rest writes reward rows.  MDR_LA_AFTER = none (every block counts last),
 *                           MDR_LA_ALT1 / _ALT8 / _ALT256 = blocks alternate in runs of 1 / 8 / 256,
 *                           MDR_LA_BEFORE = every block; | MDR_LA_TAIL_BEFORE = also every block past the
 *                           launch's first resident round (occupancy API x CUs); value >> 8, when non-zero,
 *                           is that threshold in blocks instead (for the tests).  Default MDR_LA_ALT8 |
 *                           MDR_LA_TAIL_BEFORE (measured).  Bit-identical results for every
 *                           value: the lookahead reads the end words and tick ids only and writes the half
 *                           of the group mask rows the launch does not read.  The AFFINE staged form
 *                           (the rollout default) has both orders; the EXACT, first-window and returns
 *                           forms keep the one order (a second position costs them a wave per SIMD) */
enum { MDR_LA_AFTER = 0, MDR_LA_ALT1 = 1, MDR_LA_ALT8 = 2, MDR_LA_ALT256 = 3, MDR_LA_BEFORE = 4,
       MDR_LA_TAIL_BEFORE = 16 };
enum { MDR_OPT_STEP_TPW = 1, MDR_OPT_FASTDIV = 2, MDR_OPT_WINDOW_PIPELINE = 3, MDR_OPT_SHARDED_OVERLAP = 4,
       MDR_OPT_GREEDY_SORT = 5, MDR_OPT_FORCE_HALO = 6, MDR_OPT_WINDOW_THERMAL = 7,
       MDR_OPT_HALO_OVERLAP = 9, MDR_OPT_ACTOR_GENERIC = 10, MDR_OPT_HALO_IN_COUNTS = 12,
       MDR_OPT_GQ_BAND = 13, MDR_OPT_ACTOR_FP32_FORM = 14, MDR_OPT_GQ_FUSED = 15, MDR_OPT_GQ_ADAPTIVE = 16,
       MDR_OPT_ACTOR_GRID = 17, MDR_OPT_WINDOW_GROUP = 18, MDR_OPT_ROLLOUT_CARRY = 19,
       MDR_OPT_GROUP_LA_ORDER = 20 };
enum { MDR_FP32_F16_SPLIT = 0, MDR_FP32_BF16_SPLIT3 = 1 };
/* (8 was MDR_OPT_ACTOR_PINGPONG, a k_actor schedule measured slower and retired in r04: rejected) */
enum { MDR_THERMAL_EXACT = 0, MDR_THERMAL_AFFINE = 1 };
int mdr_set_option(mdr_ctx* ctx, int option, int64_t value);

/* ---- launch geometry (no reference counterpart) ---------------------------------------- */
/* Bytes of the window ON-mask rows ([tiles][HPT][32] u64) that a window launch over n_local houses
 * with `waves` waves per block touches (every wave of a ragged last block stores and loads the rows
 * of its tile): the count launches use the build's kCountWaves, the step launches 4. */
size_t mdr_window_onb_bytes(int64_t n_local, int waves);
/* MDR_OK when ON-mask rows of onb_bytes and end words of wah_bytes cover every count and step
 * window launch over n_local houses; MDR_EARG otherwise.  Every k_count_window / k_step_window
 * launch checks its context's buffers with it, so a new launch geometry cannot overrun them. */
int mdr_window_geometry_check(int64_t n_local, size_t onb_bytes, size_t wah_bytes);
/* ... for a k_step_group launch: MDR_OK when group rows of onb_bytes cover `windows` (1..4) windows
 * of mask rows for every tile of the 4-wave grid over n_local houses (windows *
 * mdr_window_onb_bytes(n_local, 4)) and wah_bytes an end word per house; MDR_EARG otherwise.  Every
 * k_step_group launch checks its context's buffers with it. */
int mdr_window_group_check(int64_t n_local, int windows, size_t onb_bytes, size_t wah_bytes);
/* The group rows come in two halves (a launch reads its windows' rows from one and writes the counted
 * windows' rows to the other): bytes of one half, 4 * mdr_window_onb_bytes(n_local, 4), which is also
 * where the second half starts; and MDR_OK when group rows of onb_bytes hold both halves and wah_bytes
 * an end word per house, MDR_EARG otherwise.  Every k_step_group launch checks its buffers with it. */
size_t mdr_window_group_half_bytes(int64_t n_local);
int mdr_window_group_halves_check(int64_t n_local, size_t onb_bytes, size_t wah_bytes);
/* Bytes of the per-tick, per-wave penalty partial rows ([32][tiles_padded][2] doubles, tiles of 128
 * houses rounded up to whole 4-wave blocks) that a common-penalty window launch over n_local houses
 * writes: ceil(ceil(n_local / 128) / 4) * 4 * 32 * 2 * 8.  0 for n_local < 0. */
size_t mdr_window_pen_bytes(int64_t n_local);
/* MDR_OK when penalty partial rows of pen_bytes cover a common-penalty window launch over n_local
 * houses; MDR_EARG otherwise ("penalty partial" in mdr_last_error), also for n_local < 1.  Every
 * such launch checks its context's buffer with it first. */
int mdr_window_pen_check(int64_t n_local, size_t pen_bytes);
/* Bytes of the per-tick block partials ([32][blocks][12] doubles, a block = 4 tiles of 128 houses)
 * that a closed-loop window launch with stats rows (mdr_rollout_stats) over n_local houses writes:
 * ceil(ceil(n_local / 128) / 4) * 32 * 12 * 8.  0 for n_local < 0. */
size_t mdr_window_stats_bytes(int64_t n_local);
/* MDR_OK when stats partial rows of `bytes` cover such a launch over n_local houses; MDR_EARG
 * otherwise ("stats partial" in mdr_last_error), also for n_local < 1.  Every such launch checks
 * its context's buffer with it first. */
int mdr_window_stats_check(int64_t n_local, size_t bytes);

/* ---- population ------------------------------------------------------------------------ */
/* Synthetic population drawn on device from Philox4x32-10(seed, global house id): the reference
 * noise model (building.py:224-267, hvac.py:66-70: target = target_temp + |N(0, std_target)|,
 * Ua = Tri(lo, hi, 1) (the reference ASSIGNS the factor), Cm/Ca/Hm = cfg * Tri(lo, hi, 1), cap =
 * a uniform entry of cooling_capacity_list) with a counter-based RNG instead of MT19937, so a population is
 * identical for any sharding.  Initial state as Building.reset/HVAC.reset: T = init temps, on,
 * no lockout, sso = 0.  Writes every bound array. */
typedef struct mdr_pop_spec {
  double target_temp, std_target;   /* house_prop.target_temp, noise_prop.std_target_temp */
  double thermo_lo, thermo_hi;      /* noise_prop.factor_thermo_low / _high */
  double ca, cm, hm;                /* house_prop.Ca, Cm, Hm */
  double init_air, init_mass;       /* house_prop.init_air_temp, init_mass_temp */
  int32_t n_draw;                   /* cap drawn uniformly over n_draw list entries (random.choices
                                       of noise_prop.cooling_capacity_list, hvac.py:68-70);
                                       0 = uniform over the whole cap_table */
  uint8_t draw_idx[MDR_MAX_CAP];    /* cap_table index of each list entry */
} mdr_pop_spec;
int mdr_populate(mdr_ctx* ctx, const mdr_pop_spec* spec, void* stream);

/* ---- tick: phase 1 (cluster power) ------------------------------------------------------ */
/* Lockout FSM on the current state + this tick's actions -> ON houses per capacity class,
 * accumulated into the context's count slab for this tick (int64[kCountShards * n_cap], sharded
 * to spread atomics).  P = sum_k count_k * cap_k / cop is exact and order independent.  State
 * is not modified.  (cluster.py:82-88)  Not needed when the previous mdr_step ran with a
 * lookahead action source.  MDR_ACT_BANGBANG / _DEADBAND_BANGBANG evaluate the controller on the
 * current state (the decision mdr_step takes from the pre-step state). */
int mdr_power_counts(mdr_ctx* ctx, const uint8_t* action, int action_mode, uint64_t tick,
                     void* stream);
/* Device pointer + element count of the current tick's count slab: the buffer a multi-GPU caller
 * sum-allreduces (int64) between phase 1 and phase 2. */
int mdr_counts_buffer(mdr_ctx* ctx, int64_t** dev_ptr, int* len);

/* ---- tick: phase 2 (fused step) -------------------------------------------------------- */
/* FSM + RC thermal update + per-house reward with this tick's GLOBAL cluster power; updates the
 * state in place and writes reward[n_local] (double).
 *   action_mode : MDR_ACT_* (BUFFER reads action[]), or MDR_ACT_BANGBANG / _DEADBAND_BANGBANG to
 *                 evaluate that controller on the pre-step state (the obs the caller would act on)
 *   lookahead   : 0, or the action source of the NEXT tick (MDR_ACT_RANDOM / _ALWAYS_ON /
 *                 _BANGBANG / _DEADBAND_BANGBANG): its ON counts are accumulated here on the new
 *                 state, so the next tick needs no phase-1 launch
 *   ctrl_out    : if non-NULL, the bang-bang (ctrl = MDR_CTRL_*) decision on the new state
 *   p_out       : if non-NULL, device double receiving the tick's cluster power
 *   ctrl = MDR_CTRL_GREEDY_KEYS: the next mdr_ctrl_greedy's keys (see MDR_CTRL_*)
 * For common penalty modes reward holds the raw penalty until mdr_reward_finalize (mdr_rollout
 * finalises its rewards itself). */
int mdr_step(mdr_ctx* ctx, const uint8_t* action, int action_mode, const mdr_tick* tick,
             double* reward, int lookahead, int ctrl, uint8_t* ctrl_out, double* p_out,
             void* stream);

/* Common penalty modes (common_L2 / common_max_error / mixture): per-shard {sum pen/N, max pen}
 * into the context's partial buffer (device double[2]; sum-/max-allreduce it on multi-GPU), then
 * the rewards are finalised in place. */
int mdr_penalty_partials(mdr_ctx* ctx, void* stream);
int mdr_penalty_buffer(mdr_ctx* ctx, double** dev_ptr);
int mdr_reward_finalize(mdr_ctx* ctx, const mdr_tick* tick, double* reward, void* stream);

/* ---- several ticks in one call (single GPU) --------------------------------------------- */
/* n_ticks consecutive steps; ticks[] in host memory.  action / reward advance by act_stride /
 * rew_stride elements per tick (0 = reuse one buffer).  Where the temporally blocked paths below
 * (mdr_set_rollout_window) do not apply, with an in-kernel action source (MDR_ACT_RANDOM /
 * _ALWAYS_ON / _BANGBANG / _DEADBAND_BANGBANG) every tick is ONE launch (the first tick's counts from
 * a phase-1 launch, the counts of tick t+1 from tick t's lookahead); with MDR_ACT_BUFFER two.
 * MDR_ACT_BANGBANG / _DEADBAND_BANGBANG (bangbang_controllers.py:25-65) are closed-loop: every tick's
 * action is taken from the state the tick before left, bit for bit the loop of mdr_step(action_mode
 * = lookahead = the source).  use_graph != 0
 * captures the sequence in a hipGraph (cached per shape) and replays it.  p_out (device scalar,
 * may be NULL) receives the cluster power of the LAST tick, as mdr_step's p_out.
 * Common penalty modes (common_L2 / common_max_error / mixture): the rewards come out finalised —
 * on the temporally blocked path (below) each window's step kernel writes per-wave {sum pen/N,
 * max pen} partials every tick and two finish kernels (k_win_pen_reduce, k_win_reward_common)
 * follow it; on the one-tick path every step is followed by mdr_penalty_partials /
 * mdr_reward_finalize's kernels.  The bang-bang sources' closed-loop windows (below) form the pair
 * per tick and block in the one-tick kernels' summation order (k_step_closed<..., COMMON>), and
 * k_win_pen_reduce + k_closed_reward_common finish each window behind k_win_reduce: bit for bit the
 * one-tick path.  With rew_stride == 0 only the last tick's rewards are finalised
 * (the row every tick overwrites).  Fixed reduction order: bit-reproducible from run to run.  A
 * context with a communicator (or world > 1) returns MDR_EARG for these modes: per-step API. */
int mdr_rollout(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const uint8_t* action,
                int64_t act_stride, int action_mode, double* reward, int64_t rew_stride,
                double* p_out, int use_graph, void* stream);
/* mdr_rollout that also writes tick t's stats row — mdr_tick_stats' 16 doubles of the state after
 * its step, its rewards and P — into stats[row0 + t][16] (caller-owned device doubles; the caller
 * answers for row0 + n_ticks rows), inside the launch sequence: the baseline controllers'
 * Metrics.update (metrics_service.py:108-157) and TrainingManager.test means
 * (training_manager.py:265-295) at rollout speed.  stats == NULL is mdr_rollout, launch for launch.
 *   - closed-loop windows (MDR_ACT_BANGBANG / _DEADBAND_BANGBANG under individual_L2, <= 4 capacity
 *     classes, window > 0; under a common penalty mode a call WITH stats rows stays on the one-tick
 *     sequence below, though the same call without them runs windows): the window kernel itself
 *     forms every tick's block partials
 *     (k_step_closed<..., STATS>) and one more kernel per window (k_closed_stats) writes its rows.
 *     Slots 2, 10, 11, 12 are mdr_tick_stats' bits; the sums are formed in another fixed order, and
 *     slot 4 from sum_i pen_i and the tick's signal term: -((alpha_temp sum pen [/ norm_temp] + n sig)
 *     / N), the same with rew_stride == 0;
 *   - one launch per tick (the bang-bang sources otherwise — the common penalty modes among them —,
 *     any source with mdr_set_rollout_window(0)
 *     or > 4 capacity classes): mdr_tick_stats' two kernels behind every tick's step and finalise
 *     kernels, bit for bit mdr_tick_stats after mdr_step;
 *   - the open-loop window rollout (k_step_window) writes no rows: MDR_EARG.
 * use_graph: the graph is cached per (mdr_rollout's key, stats, row0).  MDR_EARG: row0 < 0.
 * MDR_ESTATE: a communicator or world > 1 (a row sums this shard's houses only). */
int mdr_rollout_stats(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const uint8_t* action,
                      int64_t act_stride, int action_mode, double* reward, int64_t rew_stride,
                      double* p_out, double* stats, int row0, int use_graph, void* stream);
/* Which of the three cases above mdr_rollout_stats would take for this action source on this
 * context as it stands (window, penalty mode, capacity classes); nothing is launched:
 * MDR_STATS_CLOSED_WINDOWS, MDR_STATS_PER_TICK, or the MDR_EARG / MDR_ESTATE it would return (so a
 * caller can refuse before it advances its own drivers). */
#define MDR_STATS_CLOSED_WINDOWS 1
#define MDR_STATS_PER_TICK 2
int mdr_rollout_stats_path(mdr_ctx* ctx, int action_mode);

/* mdr_rollout that writes no reward row and instead adds every house's weighted rewards to
 * returns[n_local] (device doubles, accumulated on top of their contents): the discounted return the
 * reference forms from a stored reward sequence (ppo.py:196-206) and TrainingManager.test averages
 * (training_manager.py:265-295), without a [n_ticks, N] reward matrix.
 *     returns[i] <- returns[i] + weights[0] r_i(0) + weights[1] r_i(1) + ...   (left to right)
 * weights: n_ticks host doubles (the caller's w[t + 1] = w[t] * gamma; read before the call returns).
 * r_i(t) has the bits mdr_rollout would have written to reward row t; state, FSM words, P, and p_out
 * are mdr_rollout's.  Three sequences (mdr_rollout_returns_path), never captured into a graph:
 *   - MDR_RETURNS_GROUPED: the open-loop sources under individual_L2, <= 4 capacity classes, window > 0,
 *     consecutive tick ids — k_count_window, then k_step_group_ret per group of MDR_OPT_WINDOW_GROUP
 *     windows (0: groups of one), the sum in a register across the group.  One multiply and one add per
 *     house and tick, never fused: bit for bit a NumPy loop ret = ret + w[t] * rows[t]; under
 *     MDR_THERMAL_EXACT independent of window, grouping and the per-tick sequence.
 *   - MDR_RETURNS_CLOSED_WINDOWS: the bang-bang sources where mdr_rollout runs closed-loop windows under
 *     individual_L2 — per window k_step_closed's ClosedRet form (a_i = sum_j w_j pen_i(j)), k_win_reduce and
 *     k_closed_return (S = sum_j w_j sig(j); returns[i] += -(alpha_temp a_i [/ norm_temp] + S)).  The
 *     same sum regrouped: with alpha_temp, alpha_sig >= 0, norm_* > 0 and weights of one sign it is
 *     within 2 (T + 8) 2^-53 relative of the row form after T accumulated ticks; state and P are exact;
 *     fixed order, so two runs agree bit for bit.
 *   - MDR_RETURNS_PER_TICK: everything else (window 0, > 4 classes, the common penalty modes, tick ids
 *     with gaps): mdr_rollout's one launch per tick into a context-owned row, k_return_acc behind each
 *     tick's final reward.  The row form's bits.
 * MDR_EARG: null ticks / weights / returns, n_ticks < 1, an unknown action source, MDR_ACT_BUFFER
 * without actions (all before any HIP call).  MDR_ESTATE: a context with a communicator or world > 1. */
#define MDR_RETURNS_GROUPED 0
#define MDR_RETURNS_CLOSED_WINDOWS 1
#define MDR_RETURNS_PER_TICK 2
int mdr_rollout_returns(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const uint8_t* action,
                        int64_t act_stride, int action_mode, const double* weights, double* returns,
                        double* p_out, void* stream);
/* Which sequence mdr_rollout_returns takes for this action source on this context as it stands
 * (tick ids taken as consecutive); nothing is launched. */
int mdr_rollout_returns_path(mdr_ctx* ctx, int action_mode);

/* Open-loop sources (MDR_ACT_RANDOM / _ALWAYS_ON / _BUFFER) with <= 4 capacity classes (every
 * penalty mode on an unsharded context; individual_L2 on a sharded one) run TEMPORALLY BLOCKED: windows of up to `ticks` steps per launch (k_step_window), the
 * state and parameters read and written once per window, rewards written every tick, each tick's
 * cluster power from counts the previous launch ran ahead (the FSM of an open-loop source does
 * not depend on the thermal state).  Bit-identical to the one-tick path under MDR_THERMAL_EXACT.
 * The bang-bang sources (MDR_ACT_BANGBANG / _DEADBAND_BANGBANG) run blocked too in mdr_rollout,
 * with <= 4 capacity classes: a closed-loop window (k_step_closed) keeps
 * controller, lockout FSM and thermal update in registers for its ticks, writes each tick's raw
 * temperature penalty to the reward row and counts its ON houses; k_win_reduce then forms every
 * tick's cluster power and a finish kernel (k_closed_reward) rewrites the rows in place (with
 * rew_stride == 0 only the last tick's).  Under a common penalty mode (unsharded) the window also
 * stores a {sum pen/N, max pen} pair per tick and block, added in the one-tick kernels' order, and
 * k_win_pen_reduce + k_closed_reward_common finish the rows (the uniform modes write no raw
 * penalties at all).  Always the EXACT thermal form (MDR_OPT_WINDOW_THERMAL is
 * ignored): bit-identical to the one-tick path.  What falls back to one launch per tick inside the
 * call: the bang-bang sources under a common penalty mode when stats rows are asked for
 * (mdr_rollout_stats), any source with more than 4 capacity classes, and ticks = 0.
 * mdr_rollout_sharded runs the same closed-loop windows on every rank under individual_L2 (the
 * window's state never reads the cluster power: its class totals are allreduced behind it, see
 * mdr_rollout_sharded).
 * ticks in 1..32 (default 32), 0 = one launch per tick.  Applies to mdr_rollout and
 * mdr_rollout_sharded; drops cached rollout graphs. */
int mdr_set_rollout_window(mdr_ctx* ctx, int ticks);

/* Optional, before mdr_rollout (no reference counterpart): launch the first window's lockout-FSM
 * count of an n_ticks rollout whose first tick id is tick0, and that window's cluster power — they
 * need the tick ids only, so they run while the host computes the ticks' drivers.  The next
 * mdr_rollout with the same n_ticks, action source, action buffer and first tick id (and
 * consecutive tick ids) uses them and launches the first window's step kernel with the drivers as
 * kernel arguments; any other entry point called in between discards them.  A no-op for rollouts
 * that do not take the open-loop temporally blocked path (the bang-bang sources among them: every
 * tick's ON set depends on the thermal state, so nothing can be counted ahead).  On a context with an RCCL communicator it also
 * allreduces the counts (single-window rollouts; the match is mdr_rollout_sharded). */
int mdr_rollout_begin(mdr_ctx* ctx, int n_ticks, uint64_t tick0, const uint8_t* action, int64_t act_stride,
                      int action_mode, void* stream);

/* Measurement (no reference counterpart): mdr_rollout's launch sequence issued directly (no graph)
 * with an event pair around every step-kernel launch; *ms = the summed step-kernel time,
 * *launches = step launches (windows — k_step_window or k_step_closed —, or ticks on the one-tick
 * path).  Advances the state like
 * mdr_rollout; synchronises the stream.  Every penalty mode on an unsharded context (a common
 * mode's finish kernels are outside the event pairs of a window, inside those of a one-tick group). */
int mdr_time_step_kernels(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const uint8_t* action,
                          int64_t act_stride, int action_mode, double* reward, int64_t rew_stride,
                          void* stream, float* ms, int* launches);

/* ---- observation vector (norm_state_dict, norm.py:178-218) ----------------------------- */
typedef struct mdr_obs_spec {
  int32_t n_feat;        /* features per house written (row length of obs) */
  int32_t hvac_state;    /* state_prop.hvac */
  int32_t solar_state;   /* state_prop.solar_gain */
  int32_t thermal_state; /* state_prop.thermal */
  int32_t msg_thermal;   /* message_prop.thermal */
  int32_t msg_hvac;      /* message_prop.hvac */
  int32_t n_comm;        /* messages per house (nb_comm) */
  int32_t comm_mode;     /* MDR_COMM_RING (neighbours, arithmetic) or MDR_COMM_TABLE */
  const int32_t* comm_table; /* TABLE mode: [n_local, n_comm] local house indices */
  const float* halo_msg;     /* RING mode, multi-GPU: [lo + hi][msg_w] message features of the
                                houses before / after the shard (mdr_halo_pack of the neighbours);
                                NULL = single shard, ring wraps around locally */
  double norm_reg_sig;   /* R */
  double cfg_ua, cfg_ca, cfg_cm, cfg_hm; /* house_prop (un-noised) for the thermal ratios */
  double cfg_cap;        /* hvac_prop.cooling_capacity (message hvac feature) */
  const float* msg_all;  /* TABLE mode, multi-GPU: [n_global][msg_w] message features of every house
                            (mdr_msg_pack of each shard, all-gathered); comm_table then holds GLOBAL
                            house ids; NULL = single shard (table ids are local) */
} mdr_obs_spec;

typedef struct mdr_obs_scalars {
  double p;       /* cluster power of the tick (obs cluster_hvac_power) */
  double s;       /* regulation signal after the step (obs reg_signal) */
  double solar;   /* obs solar_gain */
  double t_od;    /* obs OD_temp */
} mdr_obs_scalars;

/* message feature width for a spec (4, +4 thermal, +3 hvac) */
int mdr_msg_width(const mdr_obs_spec* spec);
/* float32 obs[n_local, n_feat].  p_dev, when non-NULL, overrides sc->p with a device scalar
 * (the value mdr_step wrote), so no host round trip is needed. */
int mdr_obs(mdr_ctx* ctx, const mdr_obs_spec* spec, const mdr_obs_scalars* sc,
            const double* p_dev, float* obs, void* stream);
/* message features of this shard's first hi and last lo houses -> out[(hi + lo) * msg_w] floats:
 * rows [0, hi) = first hi houses, rows [hi, hi + lo) = last lo houses. */
/* Message features (Building.message, building.py:79-139) of every local house: out [n_local][msg_w]
 * (sharded table comm modes all-gather these into mdr_obs_spec.msg_all). */
int mdr_msg_pack(mdr_ctx* ctx, const mdr_obs_spec* spec, float* out, void* stream);

int mdr_halo_pack(mdr_ctx* ctx, const mdr_obs_spec* spec, float* out, void* stream);

/* ---- cluster statistics for the server's Metrics / UI summary ----------- */
/* One deterministic reduction over the shard's state (+ reward, may be NULL) into out[12] (device
 * doubles): sum(T - target/N), sum|T - target/N|, max(0, max(T - target/N)), sum (T - target/N)^2,
 * sum reward/N (Metrics.update, metrics_service.py:108-157, its operator precedence kept),
 * sum T, sum (T - target), sum |T - target|, sum T_mass, sum target, #lockout, #on
 * (ClientManagerService, client_manager_service.py:62-111,177-196).  Sharded: sum-allreduce all but
 * out[2] (max-allreduce). */
int mdr_cluster_stats(mdr_ctx* ctx, const double* reward, double* out, void* stream);

/* ---- greedy-myopic controller (greedy_myopic_controller.py:67-104) --------------------- */
/* Next actions for the whole shard (single GPU: shard = cluster) from the current state: order
 * by -(T - target) ascending, then the reference's sequential take rule with budget S.  Also fills
 * the current tick's cluster-power counts with the ON houses those actions produce, so the next
 * mdr_step(action, MDR_ACT_BUFFER) needs no mdr_power_counts.  Asynchronous (no host
 * synchronisation): histogram select on device — only the houses around the budget crossing are
 * ordered; what that window cannot decide (a crossing among NaN keys or inside a bin of > 4,096
 * houses, e.g. identical keys; a walk past the window) the last kernel decides exactly itself.
 * With more than 4 capacity classes (or MDR_OPT_GREEDY_SORT) the full-sort form runs. */
int mdr_ctrl_greedy(mdr_ctx* ctx, double budget, uint8_t* action, void* stream);
/* Diagnostics (synchronises): mdr_ctrl_greedy calls decided by the exact in-kernel fallback;
 * mdr_greedy_diag: out[4] = {fallbacks, histogram-select calls, sum of their candidate-window
 * sizes, the last call's window size}. */
int mdr_greedy_fallbacks(mdr_ctx* ctx, uint64_t* count);
int mdr_greedy_diag(mdr_ctx* ctx, uint64_t* out);
/* The select state after the last stage run (synchronises): out[12] = mdr_greedy_diag's 4 values,
 * then {crossing superbin, crossing bin b*, window end bin, all taken, overflow, houses after the
 * window, window allocator count (zero again once the select has run), sharded need-fallback flag}. */
int mdr_greedy_state(mdr_ctx* ctx, uint64_t* out);
/* Config C3's loop: n ticks of {mdr_ctrl_greedy with budget ticks[t].s_prev (the
 * signal before the tick's step, the one the observation carries) into action + t * act_stride,
 * then mdr_step of those actions with MDR_CTRL_GREEDY_KEYS (reward + t * rew_stride; common
 * penalty modes: + mdr_penalty_partials / mdr_reward_finalize — closed-loop, so never the windowed
 * finish of mdr_rollout)}; strides 0 = every tick overwrites.
 * Replaces the per-tick Python loop GreedyMyopic.get_action -> Environment.step
 * (greedy_myopic_controller.py:67-104, environment.py:86-106).  Single GPU only: a sharded context
 * (world > 1) returns MDR_ESTATE (its decision needs the caller's collectives: mdr_gq_shard_*). */
int mdr_greedy_rollout(mdr_ctx* ctx, int n, const mdr_tick* ticks, uint8_t* action, int64_t act_stride,
                       double* reward, int64_t rew_stride, double* p_out, void* stream);
/* mdr_greedy_rollout that also writes tick t's stats row — mdr_tick_stats' 16 doubles of the state
 * after its step, with its final rewards (under the common penalty modes: after
 * mdr_reward_finalize) and its cluster power — into stats[row0 + t][16] (caller-owned device
 * doubles; the caller answers for row0 + n rows): Metrics.update (metrics_service.py:108-157) and
 * TrainingManager.test's means (training_manager.py:265-295) for GreedyMyopic at rollout speed.
 * Both forms of the tick (MDR_OPT_GQ_FUSED 0 and 1).  Per tick one more launch (k_tick_stats into
 * one of 32 slots of block partials in the context); one k_tick_rows_finish per 32 ticks and after
 * the last tick writes the rows, a block each, and the last tick's P to p_out (may be NULL).  The
 * rows have the bits of mdr_tick_stats called after every tick of the per-tick loop.
 * MDR_EARG: row0 < 0, stats NULL with n > 0 (no rows: mdr_greedy_rollout).  MDR_ESTATE: a
 * communicator or world > 1 (a row sums this shard's houses only).  A refused call launches
 * nothing and leaves the context as it was; n == 0 runs the checks alone (the pointers may be
 * NULL), so a caller can refuse before it advances its own drivers. */
int mdr_greedy_rollout_stats(mdr_ctx* ctx, int n, const mdr_tick* ticks, uint8_t* action, int64_t act_stride,
                             double* reward, int64_t rew_stride, double* p_out, double* stats, int row0,
                             void* stream);
/* The predicted band (synchronises): out[4] = {mdr_ctrl_greedy calls that skipped the bins pass
 * (the step epilogue's band held the crossing, or no bins were needed), histogram-select calls,
 * the first superbin of the band the next GQ step counts, the band's width in superbins}.
 * Misses = calls - skips. */
int mdr_greedy_band(mdr_ctx* ctx, uint64_t* out);
/* The fused tick's counters (synchronises): out[6] = {decisions, band hits, misses (the decision's own
 * pass over the cluster), exact decisions (gq_exact), the last decision's mode (0 window, 1 all taken,
 * 2 every house's byte), the last window's houses}. */
int mdr_greedy_fused_diag(mdr_ctx* ctx, uint64_t* out);
/* Diagnostics: on != 0 makes the following fused decisions record each block's phase clocks (the
 * 100 MHz constant clock; [kGqSelBlocks = 256][16] words, slot 10 = 1 in the deciding block); out, when
 * non-NULL, receives the current record (synchronises); on = 0 stops. */
int mdr_greedy_fused_stamps(mdr_ctx* ctx, int on, uint64_t* out);

/* Sharded greedy, histogram form (per-rank work O(N/G + window)): the same
 * select as mdr_ctrl_greedy with the caller's collectives between its stages, every rank deciding
 * the same window:
 *   mdr_gq_shard_begin      this shard's key codes, superbin histogram and (min, -max) key range
 *   [caller] sum-allreduce the superbin histogram (uint32, n_super) and min-allreduce the range (2 f64)
 *   mdr_gq_shard_bins       the crossing superbin, the next key map; this shard's bin counts
 *   [caller] sum-allreduce the bin histogram (uint32, n_bin)
 *   mdr_gq_shard_compact    this shard's actions below the crossing bin and its window houses:
 *                           window = {count, 0, 0, 0} + count 16-B entries (window_bytes in all)
 *   [caller] all-gather the ranks' windows (window_bytes each) in rank order
 *   mdr_gq_shard_select     order the gathered window, decide it, write this shard's window actions
 *   mdr_gq_shard_fallback   (synchronises) 1 = the window could not decide this call (a crossing
 *                           among NaN keys or inside one bin of > 4,096 houses, a walk past the
 *                           window): decide it with the all-gather form below instead.
 * mdr_gq_shard_buffers exposes the device buffers the collectives work on (valid after begin). */
int mdr_gq_shard_begin(mdr_ctx* ctx, void* stream);
int mdr_gq_shard_buffers(mdr_ctx* ctx, void** super_hist, int64_t* n_super, void** bin_hist, int64_t* n_bin,
                         void** range, void** window, int64_t* window_bytes);
int mdr_gq_shard_bins(mdr_ctx* ctx, double budget, void* stream);
int mdr_gq_shard_compact(mdr_ctx* ctx, double budget, uint8_t* action, void* stream);
int mdr_gq_shard_select(mdr_ctx* ctx, double budget, const void* gathered, int world, uint8_t* action, void* stream);
int mdr_gq_shard_fallback(mdr_ctx* ctx, int* need, void* stream);

/* Sharded greedy (the all-gather form): mdr_greedy_inputs writes this shard's
 * rows key = -(T - target), P = cooling capacity / cop, lockout (u8); the caller all-gathers them
 * in global house order, and every rank runs mdr_greedy_select over the n gathered rows — the same
 * sort / sequential take rule as mdr_ctrl_greedy — writing the cluster's actions (u8 [n]), of
 * which it keeps its own slice. */
int mdr_greedy_inputs(mdr_ctx* ctx, double* key, double* power, uint8_t* lock, void* stream);
int mdr_greedy_select(mdr_ctx* ctx, int64_t n, const double* key, const double* power, const uint8_t* lock,
                      double budget, uint8_t* action, void* stream);

/* ---- MA-PPO actor fused with the observation ----------------- */
/* Replaces MAPPO.select_actions (server/app/core/agents/trainables/mappo.py:83-97) over
 * norm_state_dict vectors (server/app/utils/norm.py:178-218) with Actor.forward
 * (server/app/core/agents/trainables/network.py:29-33; actor_layers = [h1, h2], default [100, 100],
 * server/app/core/agents/trainables/ppo.py:23-26): one persistent launch builds every house's obs
 * row on chip, runs both hidden layers on MFMA, softmax + Categorical sampling in fp32. */
enum { MDR_PREC_BF16 = 1,   /* bf16 products, fp32 accumulate (~4e-3 relative) */
       MDR_PREC_BF16X3 = 3, /* split-bf16 (hi*hi + hi*lo + lo*hi), fp32 accumulate (~1e-5) */
       MDR_PREC_FP32 = 6    /* fp32-faithful (~1e-7), the reference Actor's precision: fp16 hi/lo split
                               (22 significand bits, 3 products on the fp16 MFMA) or, with
                               MDR_OPT_ACTOR_FP32_FORM, three-way split-bf16 (24 bits, 6 products);
                               fp32 accumulate.  The layer chain runs the three-way split. */ };

typedef struct mdr_actor_spec {
  int32_t n_in;      /* obs features (= mdr_obs_spec.n_feat) */
  int32_t h1, h2;    /* hidden widths (actor_layers) */
  int32_t n_act;     /* actions (num_action): 2, the on/off decision */
  int32_t precision; /* MDR_PREC_* */
} mdr_actor_spec;

/* Load (or replace, after a PPO update) the actor weights.  Device fp32 tensors in nn.Linear
 * layout: w1 [h1][n_in], b1 [h1], w2 [h2][h1], b2 [h2], w3 [n_act][h2], b3 [n_act] (the
 * reference Actor's fc.0 / fc.1 / fc.2).  They are packed into MFMA fragment order on `stream`. */
int mdr_actor_load(mdr_ctx* ctx, const mdr_actor_spec* spec, const float* w1, const float* b1,
                   const float* w2, const float* b2, const float* w3, const float* b3, void* stream);
/* The general actor: any number of hidden layers (actor_layers, network.py:14-33) of any widths,
 * over any obs row.  w[l] / b[l], l = 0 .. n_hidden: device fp32 nn.Linear weights [out][in] and
 * biases of fc.l (the last one the output layer, [n_act][hidden[n_hidden-1]]).  A net of two
 * hidden layers <= 128 wide whose obs row (<= 128 feature slots) and weight planes fit a CU's LDS
 * runs the fused k_actor; any other runs the chain k_obs -> k_dense per hidden layer ->
 * k_actor_head (the same precisions and sampling stream). */
#define MDR_ACTOR_MAX_LAYERS 8
typedef struct mdr_actor_net {
  int32_t n_in, n_hidden, n_act, precision;
  int32_t hidden[MDR_ACTOR_MAX_LAYERS];
} mdr_actor_net;
int mdr_actor_load_net(mdr_ctx* ctx, const mdr_actor_net* net, const float* const* w, const float* const* b,
                       void* stream);
/* The head after the actor's output layer, for every later actor call of the context (mdr_actor_act,
 * mdr_actor_rollout[_snap|_stats], mdr_actor_rollout_sharded, mdr_actor_profile; fused kernel and
 * layer chain alike).  MDR_HEAD_SOFTMAX (the default after mdr_create): softmax + Categorical sampling,
 * MAPPO.select_actions.  MDR_HEAD_Q: the net is the reference's DQN_network (network.py:84-103, the
 * same MLP without the softmax), its two outputs are the Q-values, and the action is DQN.select_actions'
 * epsilon-greedy choice (server/app/core/agents/trainables/dqn.py:93-105): with probability epsilon a
 * uniformly random action, otherwise torch.argmax's (a tie gives 0; a NaN counts as the maximum, the
 * first one wins).  epsilon = 0 is the DQNController (server/app/core/agents/controllers/
 * rl_controllers.py:143-159).  The draws are the house's Philox word of the tick, the one the softmax
 * head samples from: explore iff its 24-bit uniform (word >> 8) < epsilon, random action = bit 0 of the
 * word.  Outputs under MDR_HEAD_Q: action = the chosen action, prob = its Q-value, probs = (Q0, Q1).
 * epsilon is written to a context-owned device float on `stream` and loaded by every actor launch:
 * captured rollout graphs follow later values, and a call that changes only epsilon keeps them.  The
 * head is part of the rollout graph keys, so a graph captured under one head is never replayed under
 * the other.  MDR_EARG, before any HIP call: ctx NULL, an unknown head, epsilon outside [0, 1] or NaN. */
enum { MDR_HEAD_SOFTMAX = 0, MDR_HEAD_Q = 1 };
int mdr_actor_set_head(mdr_ctx* ctx, int head, float epsilon, void* stream);
/* Synchronises; counts since the last call (zeroed by it).  out[0] = 32-house tiles of the fused
 * fp16-split form (MDR_PREC_FP32, MDR_FP32_F16_SPLIT) that wrote a non-finite logit (nothing else is
 * counted there), out[1] = the fused kernel's arithmetic (1 bf16, 3 bf16x3, 4 the fp16 split, 6 the
 * three-way bf16 split; 0 without an actor), out[2] = every tile of the fp16 split whose values left
 * the range that form carries (a hidden activation >= 2^15 x the layer's weight scale, or a
 * seconds-since-off ratio >= 64 in the tile's rows or messages) and whose logits were computed in
 * scalar fp32 instead, wherever the tile sits in its wave's loop. */
int mdr_actor_status(mdr_ctx* ctx, int64_t* out, int n, void* stream);  /* out[3] */
/* 1 when the loaded actor runs the fused kernel for this obs layout, 0 when it runs the chain. */
int mdr_actor_fused(mdr_ctx* ctx, const mdr_obs_spec* obs);
/* One select_actions over the shard.  Outputs (device, any may be NULL): action u8 [n_local],
 * prob f32 [n_local] (probability of the sampled action, MAPPO.last_probs), probs f32
 * [n_local][n_act], obs_out f32 [n_local][n_in].  Sampling: Philox4x32-10(seed, global house id,
 * tick).  count_next != 0 also fills the cluster-power counts the sampled actions produce, so the
 * next mdr_step(MDR_ACT_BUFFER) needs no mdr_power_counts. */
int mdr_actor_act(mdr_ctx* ctx, const mdr_obs_spec* obs, const mdr_obs_scalars* sc, const double* p_dev,
                  uint64_t tick, uint8_t* action, float* prob, float* probs, float* obs_out,
                  int count_next, void* stream);
/* n_ticks of (select_actions -> env.step) on device, hipGraph-captured when use_graph:
 *   tick t: actor on the state after tick t-1 (obs scalars obs_sc[t]: p ignored — the cluster
 *   power comes from p_dev, which each step rewrites), then the step with those actions.
 * action [n_ticks][n_local] u8 / prob [n_ticks][n_local] f32 (stride 0 = overwrite one row) and
 * reward [n_ticks][n_local] f64 (rew_stride 0 = one row).  p_dev: device double, in/out. */
int mdr_actor_rollout(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const mdr_obs_scalars* obs_sc,
                      const mdr_obs_spec* obs, uint8_t* action, int64_t act_stride, float* prob,
                      int64_t prob_stride, double* reward, int64_t rew_stride, double* p_dev,
                      int use_graph, void* stream);

/* mdr_actor_rollout over a house-sharded cluster (config C5 on N GPUs, RCCL communicator of
 * mdr_rccl_init), no graph: per tick the 'neighbours' ring obs gets the edge houses' message
 * features of ranks r-1 / r+1 (mdr_halo_pack + grouped ncclSend/ncclRecv), then the actor, a
 * sum-allreduce of the ON counts its actions produce, then the step.  obs->halo_msg is ignored
 * (the context owns the halo buffer); TABLE comm modes are single-shard only.  Bit-identical to
 * the single-shard rollout. */
int mdr_actor_rollout_sharded(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const mdr_obs_scalars* obs_sc,
                              const mdr_obs_spec* obs, uint8_t* action, int64_t act_stride, float* prob,
                              int64_t prob_stride, double* reward, int64_t rew_stride, double* p_dev,
                              void* stream);

/* ---- replay snapshots: training data from the fused rollout ------------------------------ */
/* The reference stores the normalised state of every agent every tick (training_manager.py:224-240,
 * mappo.py:105-126): n_feat float32 per house-tick.  An obs row is a function of the house's and
 * its neighbours' t_air, t_mass and hvac word, the tick's four obs scalars and parameters that are
 * fixed between resets, so a snapshot keeps 8 + 8 + 4 B per house-tick and one scalar row per tick,
 * and mdr_obs_gather rebuilds any transition's row on demand, bit-identical to mdr_obs of that tick.
 * These entry points are single shard only (a neighbour's snapshot would live on another shard): a
 * context with a communicator or world > 1 gives MDR_ESTATE.  A shard of a 'neighbours' ring cluster
 * takes the sharded forms further down (mdr_snap_halo), which keep the tick's ring halo as well. */
typedef struct mdr_snap {
  int32_t struct_bytes;   /* = sizeof(mdr_snap); anything else is MDR_EARG ("mdr_snap" in mdr_last_error) */
  int32_t cap_rows;       /* ticks the slabs hold */
  int64_t row_stride;     /* elements between rows, >= n_local */
  double* t_air;          /* [cap_rows][row_stride], caller-owned device memory */
  double* t_mass;         /* [cap_rows][row_stride] */
  uint32_t* hvac;         /* [cap_rows][row_stride] */
  double* scalars;        /* [cap_rows][4], mdr_obs_scalars rows, p filled on device */
} mdr_snap;
/* Row `row` <- the current t_air / t_mass / hvac of every local house and {p, s, solar, t_od} of
 * sc (p_dev, when non-NULL, overrides sc->p with the device scalar, as in mdr_obs).  MDR_EARG: row
 * outside [0, cap_rows), row_stride < n_local, a NULL slab. */
int mdr_snapshot(mdr_ctx* ctx, const mdr_snap* snap, int row, const mdr_obs_scalars* sc, const double* p_dev,
                 void* stream);
/* mdr_actor_rollout that also records tick t's pre-step state and obs scalars (what its actor
 * reads) into snapshot row row0 + t: one more kernel node per tick of the captured graph.
 * snap == NULL is mdr_actor_rollout.  MDR_EARG: row0 < 0 or row0 + n_ticks > cap_rows,
 * row_stride < n_local, a NULL slab. */
int mdr_actor_rollout_snap(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const mdr_obs_scalars* obs_sc,
                           const mdr_obs_spec* obs, uint8_t* action, int64_t act_stride, float* prob,
                           int64_t prob_stride, double* reward, int64_t rew_stride, double* p_dev,
                           int use_graph, const mdr_snap* snap, int row0, void* stream);
/* ---- per-tick stats rows: metrics and policy evaluation without a host round trip per tick ---- */
/* out16 (device doubles) <- one row of the shard's post-step state: [0..11] mdr_cluster_stats' twelve
 * values in its per-house expressions (Metrics.update, metrics_service.py:108-157; reward may be
 * NULL: out16[4] = 0), [12] the cluster power after the step (p_dev, when non-NULL, overrides
 * p_host with the device scalar, as in mdr_snapshot) — the post-step obs' cluster_hvac_power that
 * TrainingManager.test reads (training_manager.py:279-291) —, [13..15] = 0.  Asynchronous: two kernel
 * launches, a fixed summation order, no atomics.  Single shard: a communicator or world > 1 gives
 * MDR_ESTATE (a shard's partial row: mdr_tick_stats_sharded).  MDR_EARG: ctx or out16 NULL. */
int mdr_tick_stats(mdr_ctx* ctx, const double* reward, const double* p_dev, double p_host, double* out16,
                   void* stream);
/* mdr_actor_rollout_snap (snap may be NULL) that also writes tick t's row — the state after its
 * step, its reward row, P — into stats[stats_row0 + t][16] (caller-owned device doubles,
 * stats_rows rows), by two kernel nodes after tick t's step launch: what TrainingManager.start
 * feeds Metrics.update every tick (training_manager.py:242-245) and what TrainingManager.test
 * accumulates (training_manager.py:265-295), read by the host once per call.  stats == NULL is
 * mdr_actor_rollout_snap: same launches, same graph keys.  MDR_EARG, before anything is launched:
 * stats_row0 < 0 or stats_row0 + n_ticks > stats_rows.  MDR_ESTATE: a communicator or world > 1. */
int mdr_actor_rollout_stats(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const mdr_obs_scalars* obs_sc,
                            const mdr_obs_spec* obs, uint8_t* action, int64_t act_stride, float* prob,
                            int64_t prob_stride, double* reward, int64_t rew_stride, double* p_dev,
                            int use_graph, const mdr_snap* snap, int row0, double* stats, int64_t stats_rows,
                            int64_t stats_row0, void* stream);
/* float32 obs[m][n_feat]: row q is the obs row of house idx[q] % n_local at the tick of snapshot
 * row idx[q] / n_local (idx: device int64[m]), over the first `rows` snapshot rows.  An idx outside
 * [0, rows * n_local) is not dereferenced: its row is NaN.  MDR_EARG: rows outside [0, cap_rows],
 * m < 0, a spec with halo_msg or msg_all set, a NULL slab. */
int mdr_obs_gather(mdr_ctx* ctx, const mdr_obs_spec* spec, const mdr_snap* snap, int rows, const int64_t* idx,
                   int64_t m, float* obs, void* stream);

/* ---- replay snapshots of a house-sharded ring cluster (MA-PPO training on config C5) ----------- */
/* A 'neighbours' ring obs row of a shard reads at most lo = n_comm / 2 houses before the shard and
 * hi = (n_comm + 1) / 2 after it, and only their message features: the ring halo that the sharded
 * actor reads every tick.  Stored beside the snapshot row ((lo + hi) * msg_w floats per tick, at most
 * 440 B), it makes every local obs row rebuildable on its own rank.  The entry points above keep
 * their single-shard refusals; these are the sharded forms. */
typedef struct mdr_snap_halo {
  int32_t struct_bytes;   /* = sizeof(mdr_snap_halo); anything else is MDR_EARG ("mdr_snap_halo" in mdr_last_error) */
  int32_t cap_rows;       /* ticks the slab holds, >= the mdr_snap rows used with it */
  int64_t row_stride;     /* floats between rows, >= (lo + hi) * msg_w */
  float* rows;            /* [cap_rows][row_stride], caller-owned device memory: row t = the halo of
                           * tick t in the layout of mdr_obs_spec.halo_msg, [lo rows of the houses
                           * before the shard | hi rows of the houses after it], msg_w floats each */
} mdr_snap_halo;
/* mdr_snapshot for per-tick loops on a shard: one launch writes snapshot row `row` and copies
 * halo_src — device [lo + hi][msg_w] floats, the halo the caller's exchange produced for this tick's
 * obs (what it passes as mdr_obs_spec.halo_msg) — into row `row` of halo.  Needs `spec` for lo, hi and
 * msg_w.  halo and halo_src may both be NULL when the obs reads no halo (n_comm == 0).  MDR_ESTATE: a
 * context that is neither sharded (n_local < n_global) nor has a communicator.  MDR_EARG: mdr_snapshot's,
 * a TABLE comm mode, a row outside the halo slab, a short halo stride, a NULL slab or halo_src while
 * n_comm > 0. */
int mdr_snapshot_sharded(mdr_ctx* ctx, const mdr_obs_spec* spec, const mdr_snap* snap, const mdr_snap_halo* halo,
                         int row, const mdr_obs_scalars* sc, const double* p_dev, const float* halo_src,
                         void* stream);
/* mdr_actor_rollout_sharded that also records tick t's pre-step state, its obs scalars and the ring
 * halo its actor reads into row row0 + t of snap / halo, in all three forms of the loop (one launch
 * per tick, before the tick's step, after the halo's arrival and before the halo buffer's next reuse;
 * tick 0's halo is that of the exchange before the loop).  snap == NULL is mdr_actor_rollout_sharded,
 * launch for launch.  MDR_EARG, before anything is launched: rows outside [0, cap_rows) of either
 * struct, a short stride, a NULL slab, halo == NULL while a halo is exchanged (world > 1 or
 * MDR_OPT_FORCE_HALO, with n_comm > 0).  MDR_ESTATE: no communicator. */
int mdr_actor_rollout_sharded_snap(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const mdr_obs_scalars* obs_sc,
                                   const mdr_obs_spec* obs, uint8_t* action, int64_t act_stride, float* prob,
                                   int64_t prob_stride, double* reward, int64_t rew_stride, double* p_dev,
                                   const mdr_snap* snap, const mdr_snap_halo* halo, int row0, void* stream);
/* mdr_obs_gather on a shard: idx are local (tick * n_local + local house); the sources of a ring obs
 * outside the shard come from halo row `tick`, so the rows are bit-identical to mdr_obs /
 * mdr_actor_act on this rank at that tick.  halo may be NULL only when no halo is read (n_comm == 0,
 * or a communicator at world 1 without MDR_OPT_FORCE_HALO: the local wrap-around).  MDR_ESTATE: a
 * context that is neither sharded nor has a communicator.  MDR_EARG: mdr_obs_gather's, a spec with
 * halo_msg or msg_all set (the halo comes from the slab), a TABLE comm mode, rows > halo->cap_rows, a
 * short halo stride, a NULL slab. */
int mdr_obs_gather_sharded(mdr_ctx* ctx, const mdr_obs_spec* spec, const mdr_snap* snap, const mdr_snap_halo* halo,
                           int rows, const int64_t* idx, int64_t m, float* obs, void* stream);

/* ---- stats rows of a house-sharded cluster: one exact exchange per call -------- */
/* The single-shard entry points above (mdr_tick_stats, mdr_rollout_stats[_path], mdr_actor_rollout_stats,
 * mdr_greedy_rollout_stats) keep their MDR_ESTATE on a context with a communicator; these are the
 * sharded forms.  A row is twelve reductions over houses plus the cluster power, and nobody reads it
 * before the call returns, so the ranks' PARTIAL rows of a whole call of m ticks are combined once,
 * behind the call: rank r writes only X[r] of the context-owned exchange slab X[world][m][16] (all zero
 * between calls), ONE in-place double sum-allreduce of world * m * 16 elements assembles it — every
 * element has exactly one non-zero contributor, so the sum is exact in any order, tree or backend (a
 * -0.0 partial arrives as +0.0) — and k_stats_rows_combine forms row t in rank order (slot 2 by fmax,
 * the other eleven by +; [12] = P, global on every rank already; [13..15] = 0), writes it to the
 * caller's rows and zeroes the slab again.  The rows are bit-identical on every rank and between
 * communicators; at world 1 they are the single-shard rows; against the single process at world > 1
 * the sum slots differ by the regrouping of the same addends only. */
/* bytes of the slab of an m-row call (host only); 0: world < 1, m < 1, or overflow */
size_t mdr_stats_exchange_bytes(int world, int m);
/* World and rank of the slab on a shard WITHOUT a communicator of the library's (exchanges driven by
 * the caller, e.g. torch.distributed); a context with one answers MDR_OK for its own pair, MDR_ESTATE
 * for another.  MDR_EARG: ctx NULL, world < 1, rank outside [0, world). */
int mdr_stats_exchange_ranks(mdr_ctx* ctx, int world, int rank);
/* Reserve the slab for an m-row call and return it (*count = world * m * 16 doubles): what a caller
 * driving the exchange itself sum-allreduces between mdr_tick_stats_sharded and mdr_stats_rows_combine.
 * MDR_EARG: dev_ptr, count or ctx NULL, m < 1.  MDR_ESTATE: neither a communicator nor a shard. */
int mdr_stats_exchange_buffer(mdr_ctx* ctx, int m, double** dev_ptr, int64_t* count);
/* This rank's partial row `row` of an m-row call: mdr_tick_stats' two launches into X[rank][row]
 * ([0..11] this shard's values with N = n_global, [12] P, [13..15] 0).  MDR_EARG: row outside [0, m),
 * ctx NULL, m < 1.  MDR_ESTATE: neither a communicator nor a shard (n_local < n_global). */
int mdr_tick_stats_sharded(mdr_ctx* ctx, const double* reward, const double* p_dev, double p_host, int m, int row,
                           void* stream);
/* The combine of an m-row call of mdr_tick_stats_sharded rows, after the caller's sum-allreduce of the
 * slab: rows -> stats[stats_row0 .. stats_row0 + m][16], the slab zeroed.  MDR_EARG (the row range
 * first): stats_row0 < 0 or stats_row0 + m > stats_rows, stats or ctx NULL, m < 1. */
int mdr_stats_rows_combine(mdr_ctx* ctx, int m, double* stats, int64_t stats_rows, int64_t stats_row0, void* stream);
/* ... with the allreduce over the context's communicator (RCCL or mdr_comm_host) in front of it.
 * MDR_ESTATE: no communicator. */
int mdr_stats_rows_exchange(mdr_ctx* ctx, int m, double* stats, int64_t stats_rows, int64_t stats_row0, void* stream);
/* mdr_rollout_sharded that also writes tick t's row into stats[stats_row0 + t][16]; stats == NULL is
 * mdr_rollout_sharded launch for launch.  Bang-bang sources under individual_L2, <= 4 classes, the
 * window on: the same closed-loop window sequencers with k_step_closed<..., STATS>, and per window
 * k_closed_stats_part (this rank's raw sums, S = sum pen_i in slot 4, its ON totals per class in
 * [12..15]) behind k_win_shard_sum and before the window's allreduce rewrites those totals; the
 * combine's closed form sums the class totals (exact integers) and forms P, the signal term and slot 4
 * with k_closed_stats' expressions and N = n_global — the rows need no collective of their own per
 * window.  Window 0 or more classes: one launch per tick on one stream, every tick's P on the device
 * and mdr_tick_stats' launches behind each step (never the lagged-reward overlap form).  Either way
 * ONE exchange and combine on the caller's stream after the last finish.  MDR_EARG: the row range
 * (checked before anything is staged or launched), an open-loop window source (mdr_rollout_stats'
 * message), the common penalty modes. */
int mdr_rollout_sharded_stats(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const uint8_t* action,
                              int64_t act_stride, int action_mode, double* reward, int64_t rew_stride,
                              double* p_out, double* stats, int64_t stats_rows, int64_t stats_row0, void* stream);
/* Which of those applies, without launching: MDR_STATS_CLOSED_WINDOWS, MDR_STATS_PER_TICK, or the
 * refusal mdr_rollout_sharded_stats would give. */
int mdr_rollout_sharded_stats_path(mdr_ctx* ctx, int action_mode);
/* mdr_actor_rollout_sharded_snap (snap may be NULL) that also writes tick t's row: in all three forms
 * of the loop tick t's partial row follows its step on the compute stream, before tick t + 1's snapshot
 * and actor (and before a stride-0 reward row is overwritten); one exchange after the loop.
 * stats == NULL is the _snap call launch for launch. */
int mdr_actor_rollout_sharded_stats(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const mdr_obs_scalars* obs_sc,
                                    const mdr_obs_spec* obs, uint8_t* action, int64_t act_stride, float* prob,
                                    int64_t prob_stride, double* reward, int64_t rew_stride, double* p_dev,
                                    const mdr_snap* snap, const mdr_snap_halo* halo, int row0, double* stats,
                                    int64_t stats_rows, int64_t stats_row0, void* stream);

/* ---- interpolated base power ---------------------------------------- */
/* Replaces PowerInterpolator (server/app/core/environment/power_grid/interpolation.py:24-264) as
 * PowerGrid.power_step calls it every interp_update_period seconds (power_grid.py:149-161): the
 * host draws the sampled house ids (random.choices, interpolation.py:218-224 — the reference's RNG
 * stream) and the per-tick scalars; the per-house clip / nearest / multilinear lookup over the
 * Monte-Carlo table (interpolate_grid_fast, :137-178) reads the device state directly.
 * Axes in interp_dict_keys.csv order: Ua_ratio, Cm_ratio, Ca_ratio, Hm_ratio (nearest), air_temp,
 * mass_temp, OD_temp (linear), HVAC_power (nearest), hour, date (linear). */
#define MDR_INTERP_AXES 10
typedef struct mdr_interp_spec {
  int32_t len[MDR_INTERP_AXES]; /* grid points per axis (linear axes: >= 2, strictly ascending) */
  const double* grid;           /* host: the axis values, concatenated in axis order */
  const double* values;         /* host: the table, prod(len) doubles, C order over the axes */
  double cfg_ua, cfg_cm, cfg_ca, cfg_hm; /* house_prop Ua, Cm, Ca, Hm (the ratio denominators) */
} mdr_interp_spec;
/* Copy the grid + table to the device (synchronous); replaces a previous table. */
int mdr_interp_load(mdr_ctx* ctx, const mdr_interp_spec* spec);
/* vals[s] (device double[n]) = the interpolated power of house ids[s] (device int64 global ids)
 * at outdoor temperature od_temp and the point's hour / date (interpolation.py:204-216); houses
 * outside this shard give +0.0, so a sum-allreduce of vals assembles the cluster's values. */
int mdr_interp_values(mdr_ctx* ctx, const int64_t* ids, int n, double od_temp, double hour, double date,
                      double* vals, void* stream);
/* out[0] (device) = (sum of vals[0..n) in order) * multi_factor — the base power. */
int mdr_interp_sum(const double* vals, int n, double multi_factor, double* out, void* stream);

/* ---- multi-GPU (RCCL over xGMI) --------------------------------------------------------- */
/* ncclUniqueId is 128 bytes; rank 0 creates it, the caller broadcasts it (torch.distributed). */
int mdr_rccl_unique_id(uint8_t* id128);
int mdr_rccl_init(mdr_ctx* ctx, const uint8_t* id128, int world, int rank);
/* in-place allreduce on `stream`: dtype 0 = int64 sum, 1 = double sum, 2 = double max,
 * 3 = uint32 sum, 4 = double min */
int mdr_rccl_allreduce(mdr_ctx* ctx, void* buf, int64_t count, int dtype, void* stream);
/* Host collectives: the same sharded C loops (mdr_rollout_begin / mdr_rollout_sharded /
 * mdr_actor_rollout_sharded) with their exchanges handed to the caller instead of the library
 * RCCL communicator — e.g. torch.distributed over gloo, so several ranks can share one GPU (how the
 * world > 2 sharded paths are tested on a 1-GPU box).  Before each callback the library
 * synchronises the stream the exchange is ordered on; the callback completes the exchange on the
 * device buffers before it returns (0 = OK).  allreduce: in place, `op` = the mdr_rccl_allreduce
 * dtype codes.  sendrecv: `send_bytes` from dev_send to rank dst and `recv_bytes` from rank src
 * into dev_recv, as one paired exchange; `tag` tells the two ring directions apart (1: to the next
 * rank, 2: to the previous).  Replaces SURVEY §8(e)'s RCCL calls one for one (environment.py:72-108
 * exchange points). */
typedef int (*mdr_host_allreduce_fn)(void* user, void* dev_buf, int64_t count, int op);
typedef int (*mdr_host_sendrecv_fn)(void* user, const void* dev_send, int64_t send_bytes, int dst, void* dev_recv,
                                    int64_t recv_bytes, int src, int tag);
int mdr_comm_host(mdr_ctx* ctx, int world, int rank, mdr_host_allreduce_fn allreduce, mdr_host_sendrecv_fn sendrecv,
                  void* user);
/* all-gather of `bytes` per rank into recv (world x bytes, rank order) on `stream` */
int mdr_rccl_allgather(mdr_ctx* ctx, const void* send, void* recv, int64_t bytes, void* stream);
/* sharded multi-tick rollout, RCCL allreduce of the count slab inside the loop:
 * per tick  [phase 1 if BUFFER] -> allreduce(counts) -> phase 2 (with lookahead when possible)
 * The bang-bang sources (individual_L2, <= 4 capacity classes, the window on): per window
 * k_step_closed on this rank's houses -> k_win_shard_sum (the rank's per-tick class totals) ->
 * allreduce of the K x n_cap totals (<= 1 KiB) -> k_closed_reward_sharded (P and the signal term
 * from the cluster's totals; the rows rewritten in place; the last P to p_out) — bit for bit the
 * single-process mdr_rollout.  With a reward row per tick and MDR_OPT_WINDOW_PIPELINE (default) the
 * allreduce and the finish run on the communicator's side stream beside the next window's step
 * kernel; one shared row (rew_stride == 0) finishes the last window's last tick only, on one
 * stream.  With mdr_set_rollout_window(0) or more classes they take the per-tick loops above.
 * Refused (MDR_EARG): the common penalty modes.  Stats rows on a sharded context:
 * mdr_rollout_sharded_stats (mdr_rollout_stats keeps its MDR_ESTATE). */
int mdr_rollout_sharded(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const uint8_t* action,
                        int64_t act_stride, int action_mode, double* reward, int64_t rew_stride,
                        double* p_out, void* stream);
/* Pipelines mdr_rollout_sharded uses (MDR_OPT_WINDOW_PIPELINE / MDR_OPT_SHARDED_OVERLAP with the
 * communicator's side stream present): *window_pipeline = windows counted + allreduced on the side
 * stream ahead of the steps; *tick_overlap = one-tick rollouts with the allreduce of tick t beside
 * the step of tick t (that tick's reward written by the next launch, bit-identical). */
int mdr_rollout_sharded_mode(mdr_ctx* ctx, int* window_pipeline, int* tick_overlap);

/* ---- environment batches: many independent small clusters in one context ------------------ */
/* A batch is n_envs independent clusters of env_len <= MDR_BATCH_MAX_LEN houses each (the same
 * mdr_config: dt, lockout, capacity table, reward weights), resident in ONE context and stepped by ONE
 * launch per rollout call: a cluster fits one workgroup, so its per-tick cluster power never leaves
 * the block (k_batch_rollout).  Layout: cluster e is elements [e * S, e * S + env_len) of the bound
 * SoA arrays, S = mdr_batch_stride(env_len) = 128 * ceil(env_len / 128); the pad elements in between
 * are never read into a result, written, counted or rewarded.
 *
 * mdr_batch_set declares the segmentation of a bound context created with n_local = n_global =
 * n_envs * S and global_offset 0; seeds[e] (host) is cluster e's Philox key for MDR_ACT_RANDOM: house
 * i of cluster e draws what house i of a stand-alone context with that seed draws.  The bound arrays
 * must be 16-byte aligned.  Calling it again with the same geometry replaces the seeds.
 * MDR_EARG: n_envs < 1, env_len outside 1..MDR_BATCH_MAX_LEN, a context of another size or with a
 * global offset, a common penalty mode, a communicator or world > 1.  MDR_ESTATE: not bound.
 * After it the entry points that form a cluster-level quantity over the whole context (counts, step,
 * the rollouts, stats, greedy, actor, obs and their sharded forms) answer MDR_ESTATE: nobody gets a
 * power summed across clusters. */
#define MDR_BATCH_MAX_LEN 1024
size_t mdr_batch_stride(int64_t env_len); /* 0 for env_len < 1 */
int mdr_batch_set(mdr_ctx* ctx, int32_t n_envs, int32_t env_len, const uint64_t* seeds);
/* n_ticks steps of every cluster in one launch.  ticks: host [n_envs][n_ticks], cluster e's drivers
 * (its own outdoor temperature, solar gain, signal and tick ids), staged into a context-owned buffer.
 * action (MDR_ACT_BUFFER) / reward: rows of n_envs * S elements in the layout above, advancing by
 * act_stride / rew_stride elements per tick (rew_stride 0: one row that keeps the last tick);
 * reward 16-byte aligned, rew_stride even.  p_out: device doubles [n_envs] <- every cluster's power of
 * the last tick.  Per cluster bit for bit the loop of mdr_step(action_mode = lookahead = the source) on
 * a stand-alone context of env_len houses, with env_len in place of n_global in the signal penalty.
 * MDR_EARG (before anything is staged or launched): null ticks / reward / p_out, n_ticks < 1, an
 * unknown source, MDR_ACT_BUFFER without actions, a misaligned reward.  MDR_ESTATE: no mdr_batch_set. */
int mdr_batch_rollout(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const uint8_t* action,
                      int64_t act_stride, int action_mode, double* reward, int64_t rew_stride,
                      double* p_out, void* stream);
/* mdr_batch_rollout with stats rows and / or returns out of the same ONE launch (k_batch_eval); state,
 * FSM words, p_out and the pad elements exactly as mdr_batch_rollout leaves them.
 *   reward   device rows as in mdr_batch_rollout, or NULL: no reward row is written.
 *   weights  host [n_envs][n_ticks], staged behind the tick records in the same context-owned buffer;
 *   returns  device [n_envs * S] in the batch layout, 16-byte aligned.  Both or neither.  Per house of
 *            cluster e, for t = 0 .. n_ticks - 1: returns[i] = returns[i] + weights[e][t] * r_i(t), one
 *            multiply and one add, r_i(t) with the bits the reward row would hold; on top of the contents.
 *            reward and returns exclude each other.
 *   stats    device [n_envs][stats_cap][16], or NULL: row stats_row0 + t of cluster e is mdr_tick_stats'
 *            16 doubles of that cluster after tick t (slots 0..11 with N = env_len, slot 12 the tick's
 *            P, slots 13..15 written as 0).  Order of every sum: a lane starts every slot at 0.0 and adds
 *            house 128 w + 2 l, then 128 w + 2 l + 1 (wave w, lane l; houses >= env_len add nothing);
 *            the 64 lanes of a wave combine by the xor butterfly 32, 16, ..., 1, v = v + v[l ^ off]
 *            (slot 2: fmax, from 0.0); the waves are added in ascending w, starting from wave 0's value.
 *            stats alone (no reward, no returns) is allowed: the rows form without its reward stores.
 * At least one of reward / returns / stats.  reward alone is mdr_batch_rollout's launch.
 * MDR_EARG (before anything is staged or launched): null ticks / p_out, n_ticks < 1, an unknown source,
 * MDR_ACT_BUFFER without actions, all three outputs NULL, reward together with returns, exactly one of
 * weights / returns, stats_row0 < 0 or stats_row0 + n_ticks > stats_cap, a misaligned reward or
 * returns, an odd rew_stride.  MDR_ESTATE: no mdr_batch_set. */
int mdr_batch_rollout_eval(mdr_ctx* ctx, int n_ticks, const mdr_tick* ticks, const uint8_t* action,
                           int64_t act_stride, int action_mode, double* reward, int64_t rew_stride,
                           const double* weights, double* returns, double* stats, int stats_cap,
                           int stats_row0, double* p_out, void* stream);
/* float32 obs[n_envs][env_len][n_feat]: mdr_obs of every cluster, MDR_COMM_RING only (the ring wraps
 * inside the cluster).  sc: host [n_envs], each cluster's scalars; p_dev, when non-NULL, overrides
 * sc[e].p with the device doubles [n_envs] mdr_batch_rollout wrote.  MDR_EARG: MDR_COMM_TABLE, a
 * halo or msg_all pointer, n_feat not matching the flags.  MDR_ESTATE: no mdr_batch_set. */
int mdr_batch_obs(mdr_ctx* ctx, const mdr_obs_spec* spec, const mdr_obs_scalars* sc, const double* p_dev,
                  float* obs, void* stream);

/* ---- diagnostics ------------------------------------------------------------------------ */
/* Memory-floor probe: the loads/stores of one mdr_step over the bound arrays with no arithmetic
 * (writes the state back unchanged, garbage into reward).  Roofline calibration only. */
int mdr_probe_stream(mdr_ctx* ctx, double* reward, void* stream);
/* Exact-division self-check: counts (into *mismatches, device int64) the i where the
 * shared-reciprocal division sequence of the step kernels differs bitwise from a[i] / b[i]. */
int mdr_div_check(const double* a, const double* b, int64_t n, int64_t* mismatches, void* stream);

/* Phase profile of one mdr_actor_act launch (no outputs written): shader cycles per phase
 * averaged over the launch's blocks, cycles_out[8] (host): loop-top barrier wait, obs build,
 * prefetch + obs_out, layer 1, layer 2, -, output layer + softmax + stores (+ weight fill), tiles
 * per block.  Synchronises the stream. */
int mdr_actor_profile(mdr_ctx* ctx, const mdr_obs_spec* obs, const mdr_obs_scalars* sc, const double* p_dev,
                      double* cycles_out, void* stream);

/* ---- timing helpers for bench.py (HIP events on the given stream) ---------------------- */
int mdr_event_record(mdr_ctx* ctx, int slot, void* stream);
int mdr_event_elapsed_ms(mdr_ctx* ctx, int slot0, int slot1, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* MDR_H_ */
